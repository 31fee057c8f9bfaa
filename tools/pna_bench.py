"""PNA layers in inference on an MI355X -> profiles/pna_bench.json.

For S-fb15k237 and S-wn18rr (``data.synthetic_triples``) at B = 16, eval mode, no grad, through the PUBLIC forward only -- so the
same file runs on a commit without the native path and measures the four-call route there:
  * layer  -- one ``GeneralizedRelationalConvNBFMod(64, 64, ..., "distmult", "pna")`` forward with the sparse boundary attached
  * model  -- a 6-layer ``TransferNBFNet`` ``bellmanford``
Device events, median of 5 after 2 warm-ups.  Where the package has the native path the two kernels are also timed on their own,
next to what they replace in the same run:
  * operator  -- ``functional.pna_statistics`` against the four ``rspmm_forward`` calls (with their two squaring passes)
  * epilogue  -- ``functional.pna_combine_forward`` against ``layer._pna`` + ``layer.combine`` in ATen
with their bytes against the floors ``E (4 F 2 + 12) + 4 4 N F`` and ``4 rows 64 (5 + 1) + weight``.

    python tools/pna_bench.py [--out profiles/pna_bench.json] [--shapes S-fb15k237,S-wn18rr] [--batch 16]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, warmup=2, reps=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return sorted(times)[len(times) // 2]


def bench_shape(name, B):
    from ultra_torchdrug_amd import functional as UF, layer as UL
    from ultra_torchdrug_amd.data import synthetic_triples
    from ultra_torchdrug_amd.graph import Graph
    from ultra_torchdrug_amd.model import TransferNBFNet
    dev = torch.device("cuda:0")
    triples, n, r = synthetic_triples(name, 1024)
    torch.manual_seed(1)
    model = TransferNBFNet(input_dim=64, hidden_dims=[64] * 6, num_relation=r, message_func="distmult", aggregate_func="pna",
                           short_cut=True, layer_norm=True, project=True, mod=True).to(dev).eval()
    graph = model._undirected(Graph(torch.from_numpy(triples).to(dev), num_node=n, num_relation=r))
    gen = torch.Generator(device=dev).manual_seed(2)
    rel_repr = torch.randn(B, 2 * r, 64, device=dev, generator=gen)
    h_index = torch.randint(0, n, (B,), device=dev, generator=gen)
    r_index = torch.randint(0, 2 * r, (B,), device=dev, generator=gen)
    model.query = rel_repr
    for conv in model.layers:
        conv.relation = rel_repr

    def run_model():
        with torch.no_grad():
            return model.bellmanford(graph, h_index, r_index)["node_feature"]

    conv = UL.GeneralizedRelationalConvNBFMod(64, 64, 2 * r, 64, "distmult", "pna", layer_norm=True).to(dev).eval()
    conv.relation = rel_repr
    x = torch.randn(n, B, 64, device=dev, generator=gen)
    run_model()                                       # leaves query, boundary and its sparse form on the graph
    graph.relation_tables = None

    def run_layer():
        with torch.no_grad():
            return conv(graph, x, shortcut=True)

    csr = graph.relcsr
    E, F, rows = csr.n_edges, B * 64, n * B
    res = {"nodes": n, "edges": E, "relations": 2 * r, "B": B, "F": F, "native": bool(getattr(UL, "PNA_NATIVE", False)),
           "layer_ms": timed(run_layer), "model_6_layers_ms": timed(run_model)}
    if hasattr(UF, "pna_statistics"):
        with torch.no_grad():
            relation = conv._relation_table(graph, B).flatten(1).contiguous()
        flat, boundary = x.flatten(1), graph.boundary_sparse

        def four_calls():
            square = (boundary[0], boundary[1] * boundary[1])
            return [UF.rspmm_forward(csr, relation, flat, "add", "mul", boundary=boundary),
                    UF.rspmm_forward(csr, relation * relation, flat * flat, "add", "mul", boundary=square),
                    UF.rspmm_forward(csr, relation, flat, "max", "mul", boundary=boundary),
                    UF.rspmm_forward(csr, relation, flat, "min", "mul", boundary=boundary)]
        stats = UF.pna_statistics(csr, relation, flat, "mul", boundary=boundary)
        degree = graph.degree_out.unsqueeze(-1) + 1
        table = UF.pna_node_table(degree)
        ln = conv.layer_norm

        def aten_epilogue():
            with torch.no_grad():
                update = conv._pna(stats[0] / degree, stats[1] / degree, stats[2], stats[3], degree).view(n, B, -1)
                return conv.combine(x, update) + x
        op_floor = E * (4 * F * 2 + 12) + 4 * 4 * n * F
        ep_floor = 4 * rows * 64 * (5 + 1) + 4 * 64 * 832
        op_ms = timed(lambda: UF.pna_statistics(csr, relation, flat, "mul", boundary=boundary))
        ep_ms = timed(lambda: UF.pna_combine_forward(x, stats, table, conv.linear.weight, conv.linear.bias, ln.weight, ln.bias,
                                                     ln.eps, pna_eps=conv.eps, relu=True, shortcut=True))
        res["operator"] = {"one_walk_ms": op_ms, "four_calls_ms": timed(four_calls), "floor_bytes": op_floor,
                           "floor_tb_per_s": op_floor / (op_ms * 1e-3) / 1e12}
        res["epilogue"] = {"fused_ms": ep_ms, "aten_ms": timed(aten_epilogue), "floor_bytes": ep_floor,
                           "floor_tb_per_s": ep_floor / (ep_ms * 1e-3) / 1e12,
                           "tflops": 2.0 * rows * 64 * 832 / (ep_ms * 1e-3) / 1e12}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pna_bench.json"))
    ap.add_argument("--shapes", default="S-fb15k237,S-wn18rr")
    ap.add_argument("--batch", type=int, default=16)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "pna_bench needs an MI355X"
    import ultra_torchdrug_amd as U
    U.require_library()
    out = {"device": torch.cuda.get_device_name(0), "timing": "device events, median of 5 after 2 warm-ups",
           "shapes": {name: bench_shape(name, args.batch) for name in args.shapes.split(",")}}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()

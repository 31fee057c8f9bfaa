"""NeuralBellmanFordNetwork on an MI355X -> profiles/nbfnet_bench.json.

S-fb15k237 (14 541 nodes, 272 115 triples, 237 relations: 474 with inverses), 6 x 64 d, DistMult / sum, shortcut, LayerNorm,
dependent=True.  Device events, medians of 5 after 2 warm-ups (min and max beside them), the two legs of a comparison
alternating in one run:

  (A) tables     the per-query relation tables of all six layers, forward and backward, as ONE launch / ONE call each
                 (functional.query_tables) against the per-layer ATen route, at 32 and 64 queries.  The ATen leg is
                 functional.dense_query_tables -- F.linear, view, transpose and a copy per layer, and their autograd: the
                 operations a layer issues under ULTRA_QUERY_TABLES=0 -- called in THIS process, so that the two legs alternate
                 on the same operands; the switch itself is read at import and is exercised by the child process of (C)
  (B) predict    task.predict of a B = 16 evaluation batch (32 queries) through the fused sequence against the layer-by-layer
                 route (functional.FAST_INFERENCE off: what ULTRA_FAST_INFERENCE=0 selects)
  (C) train      an eager and a captured training step (engine.train_step / engine.GraphedTrainStep) at B = 64 with 128
                 negatives; the same two in a child process with ULTRA_QUERY_TABLES=0

No time is fixed in advance: nobody has measured these before.

    python tools/nbfnet_bench.py [--out profiles/nbfnet_bench.json]
"""
import argparse
import json
import os
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPE, LAYERS, DIM = "S-fb15k237", 6, 64


def one(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def alternate(legs, warmup=2, reps=5):
    """``{name: [median, min, max]}`` of the legs ``{name: fn}``, run in turn ``reps`` times after ``warmup`` rounds."""
    for _ in range(warmup):
        for fn in legs.values():
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name in legs}
    for _ in range(reps):
        for name, fn in legs.items():
            times[name].append(one(fn))
    return {name: [sorted(t)[len(t) // 2], min(t), max(t)] for name, t in times.items()}


def build(dev, seed=1024):
    from ultra_torchdrug_amd import data
    from ultra_torchdrug_amd.task import build_nbfnet
    graph = data.synthetic_kg(SHAPE, device="cpu")
    torch.manual_seed(seed)
    task = build_nbfnet(graph.num_relation, DIM, (DIM,) * LAYERS, num_negative=128)
    task.preprocess(graph)
    return task.to(dev)


def bench_tables(task, dev):
    from ultra_torchdrug_amd import functional as UF
    convs = list(task.model.layers)
    n_rel = convs[0].num_relation
    weights = [c.relation_linear.weight for c in convs]
    biases = [c.relation_linear.bias for c in convs]
    res = {}
    for batch in (32, 64):
        gen = torch.Generator(device=dev).manual_seed(batch)
        query = torch.randn(batch, DIM, device=dev, generator=gen).requires_grad_()
        upstream = [torch.randn(n_rel, batch * DIM, device=dev, generator=gen) for _ in convs]
        state = {}

        def forward(fn, key):
            def run():
                state[key] = fn(query, weights, biases, n_rel)
            return run

        def backward(key):
            def run():
                torch.autograd.grad(state[key], [query] + weights + biases, upstream, retain_graph=True)
            return run
        fwd = alternate({"one_launch": forward(UF.query_tables, "ours"), "aten_per_layer": forward(UF.dense_query_tables, "aten")})
        bwd = alternate({"one_call": backward("ours"), "aten_per_layer": backward("aten")})
        moved = sum(w.numel() + b.numel() + n_rel * batch * DIM for w, b in zip(weights, biases)) * 4
        res["aten_leg"] = "functional.dense_query_tables in the same process (the operations of ULTRA_QUERY_TABLES=0)"
        res["batch_%d" % batch] = {"forward_ms": fwd, "backward_ms": bwd, "forward_bytes": moved,
                                   "forward_gb_per_s_one_launch": moved / fwd["one_launch"][0] / 1e6,
                                   "forward_gflop": 2.0 * sum(w.numel() for w in weights) * batch / 1e9}
    return res


def bench_predict(task, dev):
    from ultra_torchdrug_amd import functional as UF
    task.eval()
    gen = torch.Generator(device=dev).manual_seed(3)
    edges = task.fact_graph.edge_list
    batch = edges[torch.randperm(len(edges), device=dev, generator=gen)[:16]].contiguous()

    def leg(fast):
        def run():
            UF.FAST_INFERENCE = fast
            try:
                with torch.no_grad():
                    return task.predict(batch)
            finally:
                UF.FAST_INFERENCE = True
        return run
    times = alternate({"fused_sequence": leg(True), "layer_by_layer": leg(False)})
    return {"batch": 16, "predict_ms": times, "equal_bits": bool(torch.equal(leg(True)(), leg(False)()))}


def bench_train(task, dev):
    from ultra_torchdrug_amd import engine
    task.train()
    edges = task.fact_graph.edge_list
    gen = torch.Generator(device=dev).manual_seed(5)
    batch = edges[torch.randperm(len(edges), device=dev, generator=gen)[:64]].contiguous()
    optimizer = torch.optim.AdamW(task.parameters(), lr=1e-4)
    eager = alternate({"eager_step": lambda: engine.train_step(task, optimizer, batch)})
    step = engine.GraphedTrainStep(task, optimizer, batch)
    captured = alternate({"captured_step": lambda: step(batch)})
    return {"batch": 64, "negatives": 128, "step_ms": dict(eager, **captured)}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nbfnet_bench.json"))
    ap.add_argument("--train-only", action="store_true", help="(the child process) print the training leg's json and stop")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("nbfnet_bench: no MI355X visible (nothing is timed on the host)")
    dev = torch.device("cuda:0")
    from ultra_torchdrug_amd import functional as UF
    task = build(dev)
    if args.train_only:
        print("TRAIN " + json.dumps(dict(query_tables=UF.QUERY_TABLES, **bench_train(task, dev))), flush=True)
        return
    out = {"device": torch.cuda.get_device_name(0), "shape": SHAPE, "layers": LAYERS, "dim": DIM,
           "timing": "[median, min, max] of 5 after 2 warm-ups, ms, device events; legs alternate"}
    out["tables"] = bench_tables(task, dev)
    out["predict"] = bench_predict(task, dev)
    out["train"] = bench_train(task, dev)
    child = subprocess.run([sys.executable, os.path.abspath(__file__), "--train-only"], env=dict(os.environ, ULTRA_QUERY_TABLES="0"),
                           capture_output=True, text=True)
    lines = [l for l in child.stdout.splitlines() if l.startswith("TRAIN ")]
    out["train_per_layer_tables"] = json.loads(lines[-1][6:]) if lines else {"error": (child.stdout + child.stderr)[-2000:]}
    print(json.dumps(out), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()

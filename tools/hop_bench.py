"""Hop distances on an MI355X -> profiles/hop_bench.json.

For S-fb15k237, its twin with uniformly drawn triples (S-fb15k237-uniform: the same sizes without hub rows, to show what the Zipf
hubs cost a level) and S-stress, each with inverse edges (the graph that carries the messages), for 64 and 512 sources, in the
matrix form (int32 (N, B)) and the targets form (8 targets per source):
  * call_ms        -- functional.hop_distance as a user calls it (num_iters = 100, polled: a source block ends at the first level
                      that adds nothing; one 4-byte host read per level)
  * fixed_ms       -- the same result with poll=False and num_iters = depth (the largest finite distance + 1): exactly
                      blocks * depth levels are enqueued and nothing is read
  * level_us       -- fixed_ms / (blocks * depth): one level of one block of 64 sources, with its share of the clear / seed /
                      fill launches and, in the targets form, of the per-level pair kernel
  * floor_us, fraction_of_8TBs -- the bytes one level must move, E * (4 + 8 [+ 4 with weights]) + 3 * 8 * N per source block
                      (src index, one gathered 8-byte frontier word per edge, the visited / frontier / next words), at 8 TB/s, and
                      floor_us / level_us
(median of 5 after 2 warm-ups, device events).  In the same run, on S-fb15k237 with 64 sources, the time per iteration of the
ATen loop that restates the reference routine on the device (``ultra/model.py:302-314``: gather (E, B), + 1, scatter amin, gather
twice, minimum, scatter) and the ratio aten_iteration_ms / level_ms.  The polled result, the fixed result and -- on S-fb15k237 -- the
ATen loop's table are compared.

    python tools/hop_bench.py [--out profiles/hop_bench.json] [--shapes S-fb15k237,S-fb15k237-uniform,S-stress]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_BYTES_PER_S = 8e12


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


def aten_iteration(dist, node_in, node_out, index):
    """One round of the reference routine: every edge offers dist[node_in] + 1 to node_out, the minimum is kept."""
    message = dist[node_in] + 1
    update = torch.full_like(dist, torch.iinfo(torch.int32).max).scatter_reduce(0, index, message, "amin", include_self=True)
    dist[node_out] = torch.minimum(dist[node_out], update[node_out])
    return dist


def aten_loop(graph, sources, num_iters):
    n = graph.num_node
    node_in, node_out = graph.edge_list[:, 0].contiguous(), graph.edge_list[:, 1].contiguous()
    index = node_out[:, None].expand(-1, len(sources))
    dist = torch.full((n, len(sources)), n, dtype=torch.int32, device=graph.device)
    dist[sources, torch.arange(len(sources), device=graph.device)] = 0
    for _ in range(num_iters):
        dist = aten_iteration(dist, node_in, node_out, index)
    return dist, (node_in, node_out, index)


def bench_shape(name):
    from ultra_torchdrug_amd import functional as UF
    from ultra_torchdrug_amd.data import SHAPES, synthetic_kg
    from ultra_torchdrug_amd.graph import Graph
    dev = torch.device("cuda:0")
    label, uniform = name, name.endswith("-uniform")         # the same sizes with uniformly drawn triples: no hub rows
    name = name[:-len("-uniform")] if uniform else name
    n, n_triple, n_rel = SHAPES[name]
    gen = torch.Generator(device=dev).manual_seed(1024)
    if name == "S-stress":                                   # built on the device, as data.stress_task does
        cols = [torch.randint(0, m, (n_triple,), device=dev, generator=gen) for m in (n, n, n_rel)]
        fact = Graph(torch.stack(cols, dim=1), None, n, n_rel)
        del cols
    else:
        fact = synthetic_kg(name, device=dev, alpha=0.0 if uniform else None)
    graph = fact.undirected(add_inverse=True)
    csr = graph.relcsr
    row_ptr, src, _, w = csr.csr_arrays
    n_edges = int(src.numel())
    floor_bytes = n_edges * (4 + 8 + (4 if w is not None else 0)) + 3 * 8 * n
    res = {"nodes": n, "coalesced_edges": n_edges, "largest_in_degree": int(torch.diff(row_ptr).max()), "weights_read": w is not None, "lanes_per_row": 64 if n_edges // n >= 48 else
           32 if n_edges // n >= 24 else 16, "floor_bytes_per_level": floor_bytes, "floor_us": floor_bytes / HBM_BYTES_PER_S * 1e6,
           "runs": {}}
    for n_source in (64, 512):
        sources = torch.randint(0, n, (n_source,), device=dev, generator=gen)
        targets = torch.randint(0, n, (n_source, 8), device=dev, generator=gen)
        blocks = (n_source + 63) // 64
        for form, tgt in (("matrix", None), ("targets", targets)):
            polled = UF.hop_distance(csr, sources, 100, tgt)
            if tgt is None:                                      # (the matrix form runs first)
                depth = int(torch.where(polled == n, -1, polled).max()) + 1
            fixed = UF.hop_distance(csr, sources, depth, tgt, poll=False)
            same = bool(torch.equal(polled, fixed))
            del polled, fixed
            call_ms = timed(lambda: UF.hop_distance(csr, sources, 100, tgt))
            fixed_ms = timed(lambda: UF.hop_distance(csr, sources, depth, tgt, poll=False))
            level_us = fixed_ms * 1e3 / (blocks * depth)
            res["runs"]["%s_b%d" % (form, n_source)] = {
                "sources": n_source, "source_blocks": blocks, "depth": depth, "call_ms": call_ms, "fixed_ms": fixed_ms,
                "level_us": level_us, "fraction_of_8TBs": res["floor_us"] / level_us, "polled_equals_fixed": same}
            print(label, form, n_source, json.dumps(res["runs"]["%s_b%d" % (form, n_source)]), flush=True)
            torch.cuda.empty_cache()
        if name == "S-fb15k237" and not uniform and n_source == 64:
            # the ATen loop: timed per iteration in its steady state (the table keeps changing for the first `depth` rounds only;
            # every round moves the same bytes)
            dist, (node_in, node_out, index) = aten_loop(graph, sources, depth)
            ours = UF.hop_distance(csr, sources, depth)
            iteration_ms = timed(lambda: aten_iteration(dist, node_in, node_out, index))
            level_ms = res["runs"]["matrix_b64"]["level_us"] / 1e3
            res["aten_loop_b64"] = {"iteration_ms": iteration_ms, "equals_hop_distance": bool(torch.equal(dist, ours)),
                                    "bytes_per_iteration_at_least": 4 * n_edges * 64 * 4, "level_ms": level_ms,
                                    "aten_iteration_over_level": iteration_ms / level_ms,
                                    "call_100_iterations_ms_extrapolated": 100 * iteration_ms,
                                    "hop_distance_call_ms": res["runs"]["matrix_b64"]["call_ms"]}
            del dist, ours, node_in, node_out, index
            torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hop_bench.json"))
    ap.add_argument("--shapes", default="S-fb15k237,S-fb15k237-uniform,S-stress")
    args = ap.parse_args()
    out = {"device": torch.cuda.get_device_name(0), "timing": "median of 5 after 2 warm-ups, device events", "shapes": {}}
    for name in args.shapes.split(","):
        out["shapes"][name] = bench_shape(name)
        print(name, json.dumps(out["shapes"][name]), flush=True)
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()

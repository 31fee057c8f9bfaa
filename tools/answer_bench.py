"""Top-K answers on an MI355X -> profiles/answer_bench.json.

For S-fb15k237 (Q = 32 queries) and S-stress (Q = 8 queries over 10 M candidates), K = 10 and K = 128, on two score tensors --
normal draws, and rows of ASCENDING scores (every candidate beats the running threshold: the selection's worst case) -- the time
(median of 5 after 2 warm-ups, device events) of
  * topk_keys            -- functional.topk_keys (ultra_topk_keys: the filter looked up in the graph's sorted completion keys)
  * masked_torch_topk    -- what a user does without it: a dense (Q, N) bool mask cleared at the known completions (found in the
                            same sorted keys: the cheapest way to build it), masked_fill with -inf, torch.topk; mask building
                            included
  * filtered_rank_keys   -- ultra_filtered_rank_keys on the same scores (target = entity 0): it reads the same bytes once
and the two ratios topk_keys / masked_torch_topk and topk_keys / filtered_rank_keys.  The two top-K routes are compared on
their values and indices (torch.topk breaks ties its own way: equal indices are expected on rows without tied answers).

    python tools/answer_bench.py [--out profiles/answer_bench.json] [--shapes S-fb15k237,S-stress]
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


def masked_topk(scores, k, keys, anchor, rel, n_rel):
    """torch.topk behind a dense filter mask built from the sorted completion keys."""
    rows, n = scores.shape
    base = (anchor * n_rel + rel) * n
    first, last = torch.searchsorted(keys, base), torch.searchsorted(keys, base + n)
    count = last - first
    row = torch.repeat_interleave(torch.arange(rows, device=scores.device), count)
    at = torch.arange(row.numel(), device=scores.device) - torch.repeat_interleave(count.cumsum(0) - count, count) + first[row]
    mask = torch.ones(rows, n, dtype=torch.bool, device=scores.device)
    mask[row, keys[at] - base[row]] = False
    return torch.topk(scores.masked_fill(~mask, -float("inf")), k, dim=1)


def bench_shape(name, n_query):
    from ultra_torchdrug_amd import functional as UF
    from ultra_torchdrug_amd.data import SHAPES, synthetic_kg
    from ultra_torchdrug_amd.graph import Graph
    dev = torch.device("cuda:0")
    n, n_triple, n_rel = SHAPES[name]
    gen = torch.Generator(device=dev).manual_seed(1024)
    if name == "S-stress":                                   # built on the device, as data.stress_task does
        cols = [torch.randint(0, m, (n_triple,), device=dev, generator=gen) for m in (n, n, n_rel)]
        graph = Graph(torch.stack(cols, dim=1), None, n, n_rel)
        del cols
    else:
        graph = synthetic_kg(name, device=dev)
    keys = graph.completion_keys(0)
    anchor, rel = graph.edge_list[:n_query, 0].contiguous(), graph.edge_list[:n_query, 2].contiguous()
    target = torch.zeros(n_query, dtype=torch.int64, device=dev)
    res = {"nodes": n, "queries": n_query, "completion_keys": int(keys.numel()), "score_bytes": n_query * n * 4, "runs": {}}
    rows = {"normal": torch.randn(n_query, n, device=dev, generator=gen),
            "ascending": torch.arange(n, device=dev, dtype=torch.float32).repeat(n_query, 1)}
    for what, scores in rows.items():
        rank_ms = timed(lambda: UF.filtered_rank_keys(scores, target, keys, anchor, rel, n_rel, n))
        for k in (10, 128):
            ours = timed(lambda: UF.topk_keys(scores, k, keys, anchor, rel, n_rel, n))
            dense = timed(lambda: masked_topk(scores, k, keys, anchor, rel, n_rel))
            value, index = UF.topk_keys(scores, k, keys, anchor, rel, n_rel, n)
            want = masked_topk(scores, k, keys, anchor, rel, n_rel)
            res["runs"]["%s_k%d" % (what, k)] = {
                "topk_keys_ms": ours, "masked_torch_topk_ms": dense, "filtered_rank_keys_ms": rank_ms,
                "topk_keys_over_masked_torch_topk": ours / dense, "topk_keys_over_filtered_rank_keys": ours / rank_ms,
                "values_equal_torch_topk": bool(torch.equal(value, want.values)),
                "indices_equal_torch_topk": bool(torch.equal(index, want.indices))}
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "answer_bench.json"))
    ap.add_argument("--shapes", default="S-fb15k237,S-stress")
    args = ap.parse_args()
    out = {"device": torch.cuda.get_device_name(0), "timing": "median of 5 after 2 warm-ups, device events, ms", "shapes": {}}
    for name in args.shapes.split(","):
        out["shapes"][name] = bench_shape(name, 8 if name == "S-stress" else 32)
        print(name, json.dumps(out["shapes"][name]), flush=True)
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()

"""Relation prediction on an MI355X -> profiles/relation_bench.json.

For S-fb15k237 (R = 237, every forward relation a candidate) and S-stress (10 M nodes; 8 candidate relations of its 500 in
batches of 2 columns, so that a run fits the device and stays in seconds), with the relation cache built first:
  * relation_scores        -- task.relation_scores for ONE pair, and for 64 pairs over 16 heads (4 tails each): wall time per
                              call behind a device synchronisation, per pair and per query column (#heads x C columns);
  * relation_select        -- functional.relation_select alone at (P, C) = (256, 474) on normal scores, filtered by the graph's
                              two completion-key arrays, with a target: all five outputs, k = 10 (device events);
  * dense_relation_select  -- the dense torch twin of the same definition on the same device tensors;
and whether the two agree.  Medians of 5 after 2 warm-ups (S-stress scores: the slower of 2 after 1).

    python tools/relation_bench.py [--out profiles/relation_bench.json] [--shapes S-fb15k237,S-stress]
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, warmup=2, reps=5, wall=False):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        if wall:
            start = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times.append((time.perf_counter() - start) * 1e3)
        else:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            times.append(a.elapsed_time(b))
    return sorted(times)[len(times) // 2]


def build_task(name, dev):
    from ultra_torchdrug_amd.data import SHAPES, stress_task, synthetic_kg
    from ultra_torchdrug_amd.task import build_ultra
    if name == "S-stress":
        return stress_task(dev)[0]
    torch.manual_seed(1024)
    task = build_ultra(SHAPES[name][2], full_batch_eval=True).to(dev).eval()
    task.preprocess(synthetic_kg(name, device=dev))
    return task


def bench_shape(name):
    from ultra_torchdrug_amd import functional as UF
    dev = torch.device("cuda:0")
    task = build_task(name, dev).eval()
    n, n_rel = task.num_entity, task.num_relation
    stress = name == "S-stress"
    cand = torch.arange(8 if stress else n_rel, device=dev)
    batch_size = 2 if stress else 16                        # (16 columns of 10 M nodes x 64 floats do not fit beside the graph)
    task.cache_relation_representations()
    edges = task.graph.edge_list
    heads = torch.unique(edges[:200_000, 0])[:16]
    gen = torch.Generator(device=dev).manual_seed(7)
    tails = torch.randint(0, n, (16, 4), device=dev, generator=gen)
    res = {"nodes": n, "relations": n_rel, "candidates": int(cand.numel()), "batch_size": batch_size, "relation_scores": {}}
    reps = dict(warmup=1, reps=2) if stress else dict(warmup=2, reps=5)
    for what, (h, t) in (("1_pair_1_head", (heads[:1], tails[0, :1])),
                         ("64_pairs_16_heads", (heads.repeat_interleave(4), tails.reshape(-1)))):
        ms = timed(lambda: task.relation_scores(h, t, candidates=cand, batch_size=batch_size), wall=True, **reps)
        columns = int(torch.unique(h).numel()) * int(cand.numel())
        res["relation_scores"][what] = {"ms": ms, "pairs": int(h.numel()), "ms_per_pair": ms / h.numel(), "query_columns": columns,
                                        "ms_per_column": ms / columns}
    # the selection alone
    n_pair, n_cand, k = 256, 474, 10
    assert n_cand <= 2 * n_rel
    keys = task.graph.completion_keys(0), task.graph.completion_keys(1)
    rows = edges[torch.randint(0, len(edges), (n_pair,), device=dev, generator=gen)]
    h, t, target = rows[:, 0].contiguous(), rows[:, 1].contiguous(), rows[:, 2].contiguous()
    score = torch.randn(n_pair, n_cand, device=dev, generator=gen)
    ids = torch.arange(n_cand, device=dev)
    ours = timed(lambda: UF.relation_select(score, None, keys[0], keys[1], h, t, target, n_rel, n, k))
    dense = timed(lambda: UF.dense_relation_select(score, ids, keys[0], keys[1], h, t, target, n_rel, n, k))
    got = UF.relation_select(score, None, keys[0], keys[1], h, t, target, n_rel, n, k)
    want = UF.dense_relation_select(score, ids, keys[0], keys[1], h, t, target, n_rel, n, k)
    res["selection"] = {"pairs": n_pair, "candidates": n_cand, "k": k, "completion_keys": [int(x.numel()) for x in keys],
                        "relation_select_ms": ours, "dense_relation_select_ms": dense, "relation_select_over_dense": ours / dense,
                        "known_pairs": int(got.known.sum()),
                        "equal": all(bool(torch.equal(a, b)) for a, b in zip(got, want))}
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "relation_bench.json"))
    ap.add_argument("--shapes", default="S-fb15k237,S-stress")
    args = ap.parse_args()
    out = {"device": torch.cuda.get_device_name(0),
           "timing": "medians, ms: relation_scores wall time behind a synchronisation, the selection device events", "shapes": {}}
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

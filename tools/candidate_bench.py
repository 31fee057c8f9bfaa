"""Candidate sets on an MI355X -> profiles/candidate_bench.json.

Two shapes, Q = 16 queries and k = 10 each, normal scores, a target per query, all five outputs:
  * S-fb15k237  -- the 2R = 474 sets of data.relation_candidates over the graph's own triples; every query is the (h, r, ?) of
                   a triple and takes the set of its relation, filtered by the graph's completion keys;
  * synthetic   -- N = 10^7 entities, ONE list of 10^6 candidates for all 16 queries (the two-launch form: 31 slices), 1000
                   known completions per query.
Timed in the same run, each the median of 5 after 2 warm-ups with device events:
  * candidate_select        -- functional.candidate_select (ultra_candidate_select_f32);
  * dense_candidate_select  -- the torch twin of the same definition on the same device tensors (dense (Q, N) masks);
  * topk_keys               -- functional.topk_keys on the same scores: the K best of ALL entities, no rank, no counts;
and whether the first two agree.  No ratio is fixed in advance.

    python tools/candidate_bench.py [--out profiles/candidate_bench.json] [--shapes S-fb15k237,synthetic]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

Q, K = 16, 10


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


def inputs(name, dev):
    """``(pred, sets, set_of, keys, anchor, rel, n_rel, target, max_len)`` of a shape."""
    from ultra_torchdrug_amd import data
    gen = torch.Generator(device=dev).manual_seed(7)
    if name == "synthetic":
        n, n_list, n_rel = 10_000_000, 1_000_000, 1
        items = torch.randperm(n, device=dev, generator=gen)[:n_list].sort().values
        sets = data.CandidateSets(torch.tensor([0, n_list], device=dev), items.to(torch.int32), n)
        anchor = torch.arange(Q, device=dev) * 1000
        rel = torch.zeros(Q, dtype=torch.int64, device=dev)
        known = items[torch.randint(0, n_list, (Q, 1000), device=dev, generator=gen)]
        keys = torch.unique(anchor[:, None] * n + known)
        set_of = torch.zeros(Q, dtype=torch.int64, device=dev)
        target = items[torch.randint(0, n_list, (Q,), device=dev, generator=gen)]
    else:
        graph = data.synthetic_kg(name, device=dev)
        n, n_rel = graph.num_node, graph.num_relation
        sets = data.relation_candidates(graph.edge_list, n, n_rel)
        rows = graph.edge_list[torch.randint(0, len(graph.edge_list), (Q,), device=dev, generator=gen)]
        anchor, target, rel = rows[:, 0].contiguous(), rows[:, 1].contiguous(), rows[:, 2].contiguous()
        keys, set_of = graph.completion_keys(0), rel
    pred = torch.randn(Q, n, device=dev, generator=gen)
    return pred, sets, set_of, keys, anchor, rel, n_rel, target, sets.max_len


def bench_shape(name):
    from ultra_torchdrug_amd import functional as UF
    dev = torch.device("cuda:0")
    pred, sets, set_of, keys, anchor, rel, n_rel, target, max_len = inputs(name, dev)
    n = pred.shape[1]
    ours = lambda: UF.candidate_select(pred, sets, set_of, K, keys, anchor, rel, n_rel, target, max_len=max_len)
    dense = lambda: UF.dense_candidate_select(pred, sets, set_of, K, keys, anchor, rel, n_rel, target, max_len=max_len)
    every = lambda: UF.topk_keys(pred, K, keys, anchor, rel, n_rel, n)
    res = {"nodes": n, "queries": Q, "k": K, "sets": sets.num_sets, "max_len": max_len, "completion_keys": int(keys.numel()),
           "slices": (max_len + UF.CANDIDATE_SLICE - 1) // UF.CANDIDATE_SLICE if max_len > UF.CANDIDATE_SLICE else 0,
           "candidate_select_ms": timed(ours), "dense_candidate_select_ms": timed(dense), "topk_keys_ms": timed(every)}
    got, want = ours(), dense()
    res["mean_candidates"] = float(got.n_free.double().mean())
    res["candidate_select_over_dense"] = res["candidate_select_ms"] / res["dense_candidate_select_ms"]
    res["candidate_select_over_topk_keys"] = res["candidate_select_ms"] / res["topk_keys_ms"]
    res["equal"] = all(bool(torch.equal(a, b)) for a, b in zip(got, want))
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "candidate_bench.json"))
    ap.add_argument("--shapes", default="S-fb15k237,synthetic")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("candidate_bench: no MI355X visible (nothing is timed on the host)")
    out = {"device": torch.cuda.get_device_name(0), "timing": "medians of 5 after 2 warm-ups, ms, device events", "shapes": {}}
    for name in args.shapes.split(","):
        out["shapes"][name] = bench_shape(name)
        print(name, json.dumps(out["shapes"][name]), flush=True)
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()

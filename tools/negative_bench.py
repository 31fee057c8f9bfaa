"""Type-constrained strict negatives on an MI355X -> profiles/negative_bench.json.

S-fb15k237, the 2R = 474 sets of data.relation_candidates over the graph's own (training) triples, B = 64 triples with 128
negatives each.  Timed, the median of 5 runs after 2 warm-ups, from device events: the two sampling launches a training step
would make (tail half: set r minus completion_keys(0); head half: set r + R minus completion_keys(1)) through
functional.constrained_negatives, next to functional.strict_negatives (ultra_strict_negative) on the same rows and the same
uniform numbers.  No time is fixed in advance.  (The task does not draw through the operator yet -- DESIGN.md section 22 -- so
there is no captured training step to time with sets.)

    python tools/negative_bench.py [--out profiles/negative_bench.json]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPE, BATCH, NEGATIVES = "S-fb15k237", 64, 128


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


def bench():
    from ultra_torchdrug_amd import data, functional as UF
    dev = torch.device("cuda:0")
    graph = data.synthetic_kg(SHAPE, device=dev)
    gen = torch.Generator(device=dev).manual_seed(7)
    batch = graph.edge_list[torch.randperm(graph.num_edge, device=dev, generator=gen)[:BATCH]].contiguous()
    sets = data.relation_candidates(graph.edge_list, graph.num_node, graph.num_relation)
    h, t, r = batch.t()
    half, n, n_rel = BATCH // 2, graph.num_node, graph.num_relation
    keys = graph.completion_keys(0), graph.completion_keys(1)
    rand = torch.rand(2, half, NEGATIVES, device=dev, generator=gen)
    # sets R .. 2R - 1 as sets 0 .. R - 1 of a view (ptr holds offsets into the shared items): the relation column is the set id
    # on both halves, and anchor / rel / set_of keep the stride of batch.t()
    domains = data.CandidateSets(sets.ptr[n_rel:], sets.items, n, sets.max_len, validate=False)

    def constrained():
        return (UF.constrained_negatives(keys[0], h[:half], r[:half], n_rel, n, rand[0], sets, r[:half], return_free=True),
                UF.constrained_negatives(keys[1], t[half:], r[half:], n_rel, n, rand[1], domains, r[half:], return_free=True))

    def strict():
        return (UF.strict_negatives(keys[0], h[:half], r[:half], n_rel, n, rand[0]),
                UF.strict_negatives(keys[1], t[half:], r[half:], n_rel, n, rand[1]))

    res = {"shape": SHAPE, "batch": BATCH, "negatives": NEGATIVES, "nodes": n, "n_sets": sets.num_sets, "max_len": sets.max_len,
           "timing": "medians of 5 after 2 warm-ups, ms, device events; two launches each",
           "constrained_draw_ms": timed(constrained), "strict_draw_ms": timed(strict)}
    got = constrained()
    free = torch.cat([got[0][1], got[1][1]])
    every = torch.cat([UF.filter_counts(keys[0], h[:half].contiguous(), r[:half].contiguous(), n_rel, n),
                       UF.filter_counts(keys[1], t[half:].contiguous(), r[half:].contiguous(), n_rel, n)])
    res["mean_free"], res["min_free"], res["rows_fallen_back"] = float(free.double().mean()), int(free.min()), int((free < 1).sum())
    res["mean_unconstrained_free"] = float(every.double().mean())
    want = (UF.dense_constrained_negatives(keys[0], h[:half], r[:half], n_rel, n, rand[0], sets, r[:half]),
            UF.dense_constrained_negatives(keys[1], t[half:], r[half:], n_rel, n, rand[1], sets, r[half:] + n_rel))
    res["equal_to_dense_twin"] = bool(torch.equal(got[0][0], want[0])) and bool(torch.equal(got[1][0], want[1]))
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "negative_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("negative_bench: no MI355X visible (nothing is timed on the host)")
    out = dict(device=torch.cuda.get_device_name(0), **bench())
    print(json.dumps(out), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()

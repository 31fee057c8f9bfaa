"""Exact answer sets and query evaluation on an MI355X -> profiles/query_eval_bench.json.

On S-fb15k237 (a tenth of the triples held out of the fact graph) with the shipped 6 x 64d architecture (seeded random weights),
the time (median of 5 after 2 warm-ups, device events) of
  (i)   project_sets_exact -- functional.project_sets_exact (ultra_sets_project) at Q = 16 and 64 over the filter graph with
                              inverse edges, against functional.dense_project_sets_exact, its dense torch twin, on the device in
                              the same run; sets of 32 random members.  "entry_alone": the C entry on preallocated buffers,
                              without the range checks of the Python call (two host reads)
  (ii)  set_ranks          -- functional.set_ranks (ultra_sets_rank) at Q = 16 and 64 with 32 targets per query and a tenth of the
                              entities excluded, against functional.dense_set_ranks
  (iii) evaluate_queries   -- engine.evaluate_queries of 64 sampled queries per structure (data.sample_queries on the filter graph)
No threshold is set on any of these numbers.

    python tools/query_eval_bench.py [--out profiles/query_eval_bench.json]
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


def build_task(dev, held_out=0.1):
    from ultra_torchdrug_amd.data import SHAPES, synthetic_kg
    from ultra_torchdrug_amd.task import build_ultra
    torch.manual_seed(1024)
    task = build_ultra(SHAPES["S-fb15k237"][2], full_batch_eval=True).to(dev).eval()
    graph = synthetic_kg("S-fb15k237", device=dev)
    fact_mask = torch.rand(graph.num_edge, generator=torch.Generator().manual_seed(3)) >= held_out
    task.preprocess(graph, fact_mask.to(dev))
    return task


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "query_eval_bench.json"))
    args = ap.parse_args()
    from ultra_torchdrug_amd import _lib, data, engine
    from ultra_torchdrug_amd import functional as UF
    from ultra_torchdrug_amd.task import QUERY_STRUCTURES
    dev = torch.device("cuda:0")
    task = build_task(dev)
    n, n_rel2 = task.num_entity, 2 * task.num_relation
    filter_graph = task.model._undirected(task.graph)
    csr = filter_graph.relcsr
    csr.csr_arrays
    gen = torch.Generator(device=dev).manual_seed(7)
    out = {"device": torch.cuda.get_device_name(0), "timing": "median of 5 after 2 warm-ups, device events, ms",
           "shape": "S-fb15k237", "nodes": n, "edges_with_inverses": csr.n_edges, "project_sets_exact": {}, "set_ranks": {},
           "evaluate_queries": {}}
    for n_query in (16, 64):
        member = torch.zeros(n_query, n, dtype=torch.bool, device=dev)
        member.scatter_(1, torch.randint(0, n, (n_query, 32), device=dev, generator=gen), True)
        bits = UF.pack_sets(member)
        relation = torch.randint(0, n_rel2, (n_query,), device=dev, generator=gen)
        ours = timed(lambda: UF.project_sets_exact(csr, bits, relation))
        dense = timed(lambda: UF.dense_project_sets_exact(csr, bits, relation))
        same = bool(torch.equal(UF.project_sets_exact(csr, bits, relation), UF.dense_project_sets_exact(csr, bits, relation)))
        row_ptr, src, rel, w = csr.csr_arrays
        result = torch.empty_like(bits)
        ws_bytes = int(_lib.load().ultra_sets_project_workspace(n_rel2, n_query))
        ws = torch.empty(ws_bytes // 8, dtype=torch.int64, device=dev)
        entry = timed(lambda: _lib.launch(dev, "ultra_sets_project", row_ptr, src, rel, w, n, csr.n_edges, n_rel2, bits, relation,
                                          n_query, result, ws, ws_bytes))
        out["project_sets_exact"][str(n_query)] = {"project_sets_exact_ms": ours, "entry_alone_ms": entry,
                                                   "dense_torch_twin_ms": dense, "ours_over_twin": ours / dense, "equal_twin": same}
        pred = torch.randn(n_query, n, device=dev, generator=gen)
        excluded = UF.pack_sets(torch.rand(n_query, n, device=dev, generator=gen) < 0.1)
        ptr = torch.arange(n_query + 1, device=dev) * 32
        entity = torch.randint(0, n, (n_query * 32,), device=dev, generator=gen)
        ours = timed(lambda: UF.set_ranks(pred, excluded, ptr, entity))
        dense = timed(lambda: UF.dense_set_ranks(pred, excluded, ptr, entity))
        same = bool(torch.equal(UF.set_ranks(pred, excluded, ptr, entity), UF.dense_set_ranks(pred, excluded, ptr, entity)))
        rank = torch.empty_like(entity)
        entry = timed(lambda: _lib.launch(dev, "ultra_sets_rank", pred, n_query, n, n, excluded, ptr, entity, n_query * 32, rank))
        out["set_ranks"][str(n_query)] = {"targets": n_query * 32, "set_ranks_ms": ours, "entry_alone_ms": entry,
                                          "dense_torch_twin_ms": dense,
                                          "ours_over_twin": ours / dense, "equal_twin": same}
        print(n_query, json.dumps(out["project_sets_exact"][str(n_query)]), json.dumps(out["set_ranks"][str(n_query)]), flush=True)
    host_graph = filter_graph.cpu()
    for k, name in enumerate(QUERY_STRUCTURES):
        anchors, relations, _ = data.sample_queries(host_graph, name, 64, torch.Generator().manual_seed(100 + k))
        anchors, relations = anchors.to(dev), relations.to(dev)
        ms = timed(lambda: engine.evaluate_queries(task, name, anchors, relations))
        metrics = engine.evaluate_queries(task, name, anchors, relations)
        out["evaluate_queries"][name] = {"queries": 64, "evaluate_queries_ms": ms, "num_evaluated": metrics["num_evaluated"],
                                         "num_hard_answers": metrics["num_hard_answers"]}
        print(name, json.dumps(out["evaluate_queries"][name]), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()

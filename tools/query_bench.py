"""Logical queries on an MI355X -> profiles/query_bench.json.

On S-fb15k237 (Q = 16 queries) and S-stress (Q = 2 queries over 10 M entities), with the shipped 6 x 64d architecture (seeded
random weights), the time (median of 5 after 2 warm-ups, device events) of
  (i)   set_boundary          -- functional.set_boundary (ultra_set_boundary_f32) against the torch expression it replaces, built
                                 here: compare, where, transposing copy, broadcast multiply; ms and GB/s against the byte floor
                                 4 * (Q * N + N * Q * D); on a set cut to 32 members per row and on uncut uniform memberships
  (ii)  project               -- TransferNBFNet.project over a 32-member set against score_all_entities for the same Q: the price
                                 of the dense boundary (no sparse first layer, no frontier, no fused layers)
  (iii) whole queries         -- task.answer_query for 2p, 3p and 2i, k = 10, max_sources = 32

    python tools/query_bench.py [--out profiles/query_bench.json] [--shapes S-fb15k237,S-stress]
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


def torch_boundary(member, query, floor):
    """The route named in the issue: a compare, a ``where``, a transposing copy and a broadcast multiply."""
    keep = (member > 0) & (member >= floor.unsqueeze(-1))
    kept = torch.where(keep, member, torch.zeros_like(member))
    return kept.t().contiguous().unsqueeze(-1) * query.unsqueeze(0)


def build_task(name, dev):
    from ultra_torchdrug_amd.data import SHAPES, stress_task, synthetic_kg
    from ultra_torchdrug_amd.task import build_ultra
    if name == "S-stress":
        return stress_task(dev)[0]
    torch.manual_seed(1024)
    task = build_ultra(SHAPES[name][2], full_batch_eval=True).to(dev).eval()
    task.preprocess(synthetic_kg(name, device=dev))
    return task


def bench_shape(name, n_query):
    from ultra_torchdrug_amd import functional as UF
    dev = torch.device("cuda:0")
    task = build_task(name, dev)
    n, n_rel, dim = task.num_entity, task.num_relation, 64
    gen = torch.Generator(device=dev).manual_seed(7)
    res = {"nodes": n, "queries": n_query, "dim": dim, "byte_floor": 4 * (n_query * n + n * n_query * dim)}

    # (i) the boundary alone
    query = torch.randn(n_query, dim, device=dev, generator=gen)
    member = torch.rand(n_query, n, device=dev, generator=gen)
    zero = torch.zeros(n_query, dtype=torch.int64, device=dev)
    floors = {"cut_to_32": UF.topk_keys(member, 32, None, zero, zero, 1)[0][:, -1].contiguous(),
              "uncut": torch.zeros(n_query, device=dev)}
    res["set_boundary"] = {}
    for what, floor in floors.items():
        ours = timed(lambda: UF.set_boundary(member, query, floor, with_count=True))
        dense = timed(lambda: torch_boundary(member, query, floor))
        got, count = UF.set_boundary(member, query, floor, with_count=True)
        same = bool(torch.equal(got, torch_boundary(member, query, floor)))
        res["set_boundary"][what] = {
            "kept_per_row": count.tolist(), "set_boundary_ms": ours, "torch_expression_ms": dense,
            "set_boundary_over_torch_expression": ours / dense, "set_boundary_gb_per_s": res["byte_floor"] / ours / 1e6,
            "torch_expression_gb_per_s": res["byte_floor"] / dense / 1e6, "equal_torch_expression": same}
        del got
    del member
    torch.cuda.empty_cache()

    # (ii) one projection of a 32-member set against the single-source pass
    with torch.no_grad():
        anchor = torch.randint(0, n, (n_query,), device=dev, generator=gen)
        rel = torch.randint(0, 2 * n_rel, (n_query,), device=dev, generator=gen)
        rel_rep = task.relation_representations(rel % n_rel)
        sources = torch.randint(0, n, (n_query, 32), device=dev, generator=gen)
        member = torch.zeros(n_query, n, device=dev)
        member.scatter_(1, sources, torch.rand(n_query, 32, device=dev, generator=gen) * 0.5 + 0.5)
        single = timed(lambda: task.model.score_all_entities(task.fact_graph, rel_rep, anchor, rel))
        proj = timed(lambda: task.model.project(task.fact_graph, rel_rep, member, rel))
        res["project"] = {"members": 32, "project_ms": proj, "score_all_entities_ms": single,
                          "project_over_score_all_entities": proj / single}
        del member
        torch.cuda.empty_cache()

        # (iii) whole queries
        res["queries_ms"] = {}
        for structure, (n_anchor, n_relation) in (("2p", (1, 2)), ("3p", (1, 3)), ("2i", (2, 2))):
            anchors = torch.randint(0, n, (n_query, n_anchor), device=dev, generator=gen)
            relations = torch.randint(0, 2 * n_rel, (n_query, n_relation), device=dev, generator=gen)
            res["queries_ms"][structure] = timed(lambda: task.answer_query(structure, anchors, relations, k=10, max_sources=32))
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "query_bench.json"))
    ap.add_argument("--shapes", default="S-fb15k237,S-stress")
    args = ap.parse_args()
    out = {"device": torch.cuda.get_device_name(0), "timing": "median of 5 after 2 warm-ups, device events, ms", "shapes": {}}
    for name in args.shapes.split(","):
        out["shapes"][name] = bench_shape(name, 2 if name == "S-stress" else 16)
        print(name, json.dumps(out["shapes"][name]), flush=True)
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()

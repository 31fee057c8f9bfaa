"""Training through logical queries on an MI355X -> profiles/query_train_bench.json.

At the shapes of S-fb15k237 with Q = 16 and of S-stress with Q = 2, 64 columns, seeded random values:
  (A) set_boundary_backward -- functional.set_boundary_backward (ultra_set_boundary_backward_f32) against the backward of the
                               torch expression (functional.dense_set_boundary on the device; its graph is built outside the
                               timed region), half of the entities kept; achieved bytes per second against the byte floor
                               4 * (N Q D + 2 Q N)
  (B) score_backward        -- functional.score_all_backward (ultra_score_backward_f32) against the ATen backward of the
                               materialised head (cat, two F.linear, relu; graph built outside the timed region), with each
                               side's peak memory over forward and backward; the FLOP rate of the three 64 x 128 products a row
                               (49 152 FLOP) against the 157 TF f32 matrix peak
  (C) train_query_step      -- engine.train_query_step for 2p and 2i with the shipped 6 x 64d architecture (seeded random weights)
                               on S-fb15k237 (16 grounded queries, 32 negatives each); --stress-step adds S-stress at Q = 2
Device events, the median of 5 after 2 warm-ups; three such runs alternating the two sides in one session, reported as
median [min, max].  No ratio is fixed in advance; the requirement is that each native band lies at or below the ATen band.

    python tools/query_train_bench.py [--out profiles/query_train_bench.json] [--stress-step] [--skip-stress]
"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MATRIX_PEAK_F32 = 157.3e12
ROW_FLOP = 3 * 2 * 64 * 128


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


def band(values):
    values = sorted(values)
    return {"median_ms": values[len(values) // 2], "min_ms": values[0], "max_ms": values[-1]}


def alternate(ours, theirs, runs=3):
    """``runs`` rounds of (ours, theirs), each the median of 5 after 2 warm-ups."""
    a, b = [], []
    for _ in range(runs):
        a.append(timed(ours))
        b.append(timed(theirs))
    return band(a), band(b)


def peak_of(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    before = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - before


def bench_set_boundary(n_node, n_query, dev, gen):
    from ultra_torchdrug_amd import functional as UF
    dim = 64
    member = torch.rand(n_query, n_node, device=dev, generator=gen)
    query = torch.randn(n_query, dim, device=dev, generator=gen)
    floor = torch.full((n_query,), 0.5, device=dev)
    d_boundary = torch.randn(n_node, n_query, dim, device=dev, generator=gen)
    m, q = member.clone().requires_grad_(), query.clone().requires_grad_()
    boundary = UF.dense_set_boundary(m, q, floor)
    ours, aten = alternate(lambda: UF.set_boundary_backward(d_boundary, member, query, floor),
                           lambda: torch.autograd.grad(boundary, [m, q], d_boundary, retain_graph=True))
    mine = UF.set_boundary_backward(d_boundary, member, query, floor)
    ref = torch.autograd.grad(boundary, [m, q], d_boundary, retain_graph=True)
    floor_bytes = 4 * (n_node * n_query * dim + 2 * n_query * n_node)
    return {"nodes": n_node, "queries": n_query, "dim": dim, "kept_share": float(((member >= 0.5).float().mean())),
            "native": ours, "aten_backward_of_the_torch_expression": aten,
            "native_over_aten": ours["median_ms"] / aten["median_ms"], "byte_floor": floor_bytes,
            "native_bytes_per_second_of_the_floor": floor_bytes / (ours["median_ms"] * 1e-3),
            "max_abs_difference_d_member": float((mine[0] - ref[0]).abs().max()),
            "max_abs_difference_d_query_relative": float((mine[1] - ref[1]).abs().max() / ref[1].abs().max())}


def bench_score(n_node, batch, dev, gen):
    from ultra_torchdrug_amd import functional as UF
    hidden = torch.randn(n_node, batch, 64, device=dev, generator=gen)
    query = torch.randn(batch, 64, device=dev, generator=gen)
    w1 = torch.randn(128, 128, device=dev, generator=gen) / 11.3
    b1 = torch.randn(128, device=dev, generator=gen) / 11.3
    w2 = torch.randn(128, device=dev, generator=gen) / 11.3
    b2 = torch.zeros(1, device=dev)
    grad = torch.randn(batch, n_node, device=dev, generator=gen)

    def aten_forward():
        leaves = [t.detach().clone().requires_grad_() for t in (hidden, query, w1, b1, w2, b2)]
        x = torch.cat([leaves[0], leaves[1].unsqueeze(0).expand(n_node, -1, -1)], dim=-1)
        score = F.linear(F.relu(F.linear(x, leaves[2], leaves[3])), leaves[4].view(1, 128), leaves[5]).squeeze(-1).t()
        return score, leaves

    def native_whole():
        leaves = [t.detach().requires_grad_() for t in (hidden, query, w1, b1, w2.view(1, 128), b2)]
        torch.autograd.grad(UF.score_all_entities(*leaves), leaves, grad)

    def aten_whole():
        score, leaves = aten_forward()
        torch.autograd.grad(score, leaves, grad)

    peak_native, peak_aten = peak_of(native_whole), peak_of(aten_whole)
    score, leaves = aten_forward()
    ours, aten = alternate(lambda: UF.score_all_backward(hidden, query, w1, b1, w2, grad),
                           lambda: torch.autograd.grad(score, leaves, grad, retain_graph=True))
    whole_native, whole_aten = alternate(native_whole, aten_whole)
    mine = UF.score_all_backward(hidden, query, w1, b1, w2, grad)
    ref = torch.autograd.grad(score, leaves, grad, retain_graph=True)
    rows = n_node * batch
    # where the two fp32 sides differ most in d_hidden: both against the fp64 definition on the 32 entities around that row (a
    # pre-activation within rounding of zero may lie on either side of the ReLU in either fp32 run)
    worst = int((mine[0] - ref[0]).abs().amax(dim=(1, 2)).argmax())
    lo = max(0, min(worst - 16, n_node - 32))
    hi = min(n_node, lo + 32)
    x = torch.cat([hidden[lo:hi].double(), query.double().unsqueeze(0).expand(hi - lo, -1, -1)], dim=-1)
    pre = x @ w1.double().t() + b1.double()
    d_pre = torch.where(pre > 0, grad[:, lo:hi].t().double().unsqueeze(-1) * w2.double(), torch.zeros((), dtype=torch.float64, device=dev))
    d_hidden64 = (d_pre @ w1.double())[..., :64]
    spot = {"entities": [lo, hi], "scale": float(d_hidden64.abs().max()),
            "native_from_fp64": float((mine[0][lo:hi].double() - d_hidden64).abs().max()),
            "aten_from_fp64": float((ref[0][lo:hi].double() - d_hidden64).abs().max()),
            "smallest_abs_preactivation_fp64": float(pre.abs().min())}
    # the sums over all rows, both sides against the fp64 definition evaluated in chunks of entities
    w1d, b1d, w2d, qd = w1.double(), b1.double(), w2.double(), query.double()
    d_b1_64 = torch.zeros(128, dtype=torch.float64, device=dev)
    d_w1_64 = torch.zeros(128, 128, dtype=torch.float64, device=dev)
    for c0 in range(0, n_node, 1 << 18):
        c1 = min(n_node, c0 + (1 << 18))
        xc = torch.cat([hidden[c0:c1].double(), qd.unsqueeze(0).expand(c1 - c0, -1, -1)], dim=-1).reshape(-1, 128)
        dp = torch.where(xc @ w1d.t() + b1d > 0, grad[:, c0:c1].t().double().reshape(-1, 1) * w2d,
                         torch.zeros((), dtype=torch.float64, device=dev))
        d_b1_64 += dp.sum(dim=0)
        d_w1_64 += dp.t() @ xc
        del xc, dp
    sums = {name: {"native_from_fp64_relative": float((m.double() - t).abs().max() / t.abs().max()),
                   "aten_from_fp64_relative": float((r.double() - t).abs().max() / t.abs().max())}
            for name, m, r, t in (("d_w1", mine[2], ref[2], d_w1_64), ("d_b1", mine[3], ref[3], d_b1_64))}
    return {"nodes": n_node, "queries": batch, "rows": rows, "native_backward": ours, "aten_backward": aten,
            "d_hidden_where_the_fp32_sides_differ_most": spot, "row_sums_against_fp64": sums,
            "native_over_aten": ours["median_ms"] / aten["median_ms"],
            "native_forward_and_backward": whole_native, "aten_forward_and_backward": whole_aten,
            "peak_bytes_native_forward_and_backward": peak_native, "peak_bytes_aten_forward_and_backward": peak_aten,
            "activation_bytes_never_stored": rows * 128 * 4,
            "flop_per_row_executed": ROW_FLOP, "native_flop_per_second": rows * ROW_FLOP / (ours["median_ms"] * 1e-3),
            "share_of_the_f32_matrix_peak": rows * ROW_FLOP / (ours["median_ms"] * 1e-3) / MATRIX_PEAK_F32,
            "relative_differences": {name: float((m.reshape(-1) - r.reshape(-1)).abs().max() / r.abs().max())
                                     for name, m, r in zip(("d_hidden", "d_query", "d_w1", "d_b1", "d_w2", "d_b2"), mine, ref)}}


def bench_steps(task, n_query, n_negative, dev, host_graph=None):
    from ultra_torchdrug_amd import data, engine
    task.train()
    optimizer = torch.optim.Adam(task.parameters(), lr=5e-4)
    out = {}
    for k, name in enumerate(("2p", "2i")):
        g = torch.Generator().manual_seed(200 + k)
        if host_graph is not None:
            anchors, relations, targets = data.sample_queries(host_graph, name, n_query, g)
        else:                                   # (a graph too large for the host-side sampler: seeded random ids)
            from ultra_torchdrug_amd.task import parse_query_structure
            _, n_anchor, n_relation = parse_query_structure(name)
            anchors = torch.randint(0, task.num_entity, (n_query, n_anchor), generator=g)
            relations = torch.randint(0, 2 * task.num_relation, (n_query, n_relation), generator=g)
            targets = torch.randint(0, task.num_entity, (n_query,), generator=g)
        anchors, relations, targets = anchors.to(dev), relations.to(dev), targets.to(dev)
        answers = task.query_answers(name, anchors, relations, graph="filter")
        negatives = data.sample_query_negatives(answers, n_negative, g)
        del answers
        values = [timed(lambda: engine.train_query_step(task, optimizer, name, anchors, relations, targets, negatives))
                  for _ in range(3)]
        out[name] = dict(band(values), queries=n_query, negatives=n_negative)
        print(name, json.dumps(out[name]), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "query_train_bench.json"))
    ap.add_argument("--stress-step", action="store_true", help="also time train_query_step on S-stress (builds the 100 M edge plans)")
    ap.add_argument("--skip-stress", action="store_true", help="S-fb15k237 only")
    args = ap.parse_args()
    from ultra_torchdrug_amd.data import SHAPES, stress_task, synthetic_kg
    from ultra_torchdrug_amd.task import build_ultra
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(7)
    out = {"device": torch.cuda.get_device_name(0),
           "timing": "device events, median of 5 after 2 warm-ups; three runs alternating the two sides: median [min, max], ms",
           "set_boundary_backward": {}, "score_backward": {}, "train_query_step": {}}
    shapes = [("S-fb15k237", SHAPES["S-fb15k237"][0], 16)] + ([] if args.skip_stress else [("S-stress", SHAPES["S-stress"][0], 2)])
    for name, n_node, n_query in shapes:
        out["set_boundary_backward"][name] = bench_set_boundary(n_node, n_query, dev, gen)
        print(name, "A", json.dumps(out["set_boundary_backward"][name]), flush=True)
        out["score_backward"][name] = bench_score(n_node, n_query, dev, gen)
        print(name, "B", json.dumps(out["score_backward"][name]), flush=True)
        torch.cuda.empty_cache()
    torch.manual_seed(1024)
    task = build_ultra(SHAPES["S-fb15k237"][2], full_batch_eval=True).to(dev)
    graph = synthetic_kg("S-fb15k237", device=dev)
    task.preprocess(graph)
    out["train_query_step"]["S-fb15k237"] = bench_steps(task, 16, 32, dev, host_graph=task.message_graph().cpu())
    del task, graph
    torch.cuda.empty_cache()
    if args.stress_step and not args.skip_stress:
        task, _ = stress_task(dev)
        out["train_query_step"]["S-stress"] = bench_steps(task, 2, 32, dev)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()

"""Explaining one prediction (``TransferNBFNet.visualize``) at B = 1 on S-fb15k237 and S-stress (GPU only).

    python tools/explain_bench.py [--workloads S-fb15k237,S-stress] [--messages distmult] [--materialised S-fb15k237]
                                  [--reps 3] [--beams 10] [--json PATH]

Per workload and message function (``--messages distmult,rotate``): the shipped 6 x 64d entity stack (sum, LayerNorm, shortcut,
projected relations; seeded random init and random relation representations -- the relation stack is not part of an
explanation), the graph with inverse edges and its plans built first.  ``--materialised WORKLOADS``: on these workloads a second
leg (``route: materialised``) with every layer on the materialised ``message()`` + ``aggregate()`` route -- for rotate messages
what ``visualize`` ran before the native rotate edge gradient existed; never ask for it on S-stress, where ONE ``(E, D)``
tensor is 25.6 GB.  Reported:
  * ``gradient_ms``: the per-layer edge gradients (``edge_gradients``: forward with leaf weights + ``autograd.grad``);
  * ``search_ms``: the beam search over all layers plus the path assembly (``visualize`` minus the gradient part);
  * ``peak_extra_bytes``: ``max_memory_allocated`` during one ``visualize`` above the allocation before it, and ``E * 64 * 4``, the
    size of ONE materialised (E, D) message tensor, beside it;
  * ``beam_kernel``: the ``ultra_beam_search_step_f32`` launch alone (device events around the C ABI call, median of ``--reps``
    per layer, on that layer's real inputs) against its byte floor ``E (8 + 4 + 4K) + 4 (N + 1) + 12 N K``;
  * ``weight_grad_kernel`` (rotate legs): the ``ultra_rspmm_rotate_backward_weight_f32`` launch alone (sum, F = 64, random
    rows) against its byte floor: three rows of ``F`` floats (input, relation, output gradient), the three index words and the
    ``d_weight`` word per edge, ``E (12 F + 16)``.
Prints one JSON object; a workload that fails records the error instead of a result.

    python tools/explain_bench.py --batch [B] [--workloads S-fb15k237] [--messages distmult] [--beams 10] [--json PATH]

``--batch`` (``B`` = 16 when not given): the batched explanation instead of the above.  Per workload and message function, in ONE
run and alternating (three alternations of the two legs; each figure the median of 5 calls after 2 warm-up calls of its own, device
events around the call, which ends in a synchronise):
  * ``looped``: ``B`` ``visualize`` calls, one per triple;  ``batched``: ONE ``visualize_batch`` of the same ``B`` triples;
  * per leg ``ms_per_triple`` and its split: ``gradient_ms_per_triple`` (``edge_gradients`` x B / ``edge_gradients_batch``) and
    ``search_ms_per_triple`` (the rest: beam search, path assembly, host sort);
  * ``ratio``: batched over looped time per triple (below 1: the batch is faster), per alternation and of the medians;
  * ``batched_peak_extra_bytes`` beside ``B * E * 64 * 4``, one batched message tensor;  ``same_paths``: how many of the ``B``
    results name the same paths as their single-triple call (the batched score head may differ from it in the last bits).
Written to ``profiles/explain_batch_bench.json`` unless ``--json`` names another file.  Activation memory grows with ``B``: on
S-stress use ``--batch 2`` or leave the workload out.
"""
import argparse
import ctypes
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

HBM_PEAK = 8.0e12      # bytes / s (MI355X_MICROARCH.md)


def build(workload, dev, message="distmult", seed=1024):
    from ultra_torchdrug_amd.data import SHAPES, synthetic_kg
    from ultra_torchdrug_amd.graph import Graph
    from ultra_torchdrug_amd.model import TransferNBFNet
    if workload == "S-stress":
        n_node, n_triple, n_rel = SHAPES["S-stress"]
        gen = torch.Generator(device=dev).manual_seed(seed)
        triples = torch.stack([torch.randint(0, n, (n_triple,), device=dev, generator=gen) for n in (n_node, n_node, n_rel)], 1)
        graph = Graph(triples, None, n_node, n_rel)
    else:
        graph = synthetic_kg(workload, device=dev)
    torch.manual_seed(seed)
    model = TransferNBFNet(input_dim=64, hidden_dims=[64] * 6, num_relation=graph.num_relation, message_func=message,
                           aggregate_func="sum", short_cut=True, layer_norm=True, project=True, mod=True).to(dev)
    rel = torch.randn(1, 2 * graph.num_relation, 64, device=dev, generator=torch.Generator(device=dev).manual_seed(seed))
    return graph, model, rel


def kernel_ms(row_ptr, src, grad, beams, tail, reps):
    from ultra_torchdrug_amd import _lib
    lib = _lib.load()
    n, K = beams.shape
    out = torch.empty_like(beams)
    be = torch.empty(n, K, dtype=torch.int32, device=beams.device)
    br = torch.empty_like(be)
    stream = torch.cuda.current_stream()
    times = []
    for _ in range(reps + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        _lib.check(lib.ultra_beam_search_step_f32(row_ptr.data_ptr(), src.data_ptr(), grad.data_ptr(), beams.data_ptr(), n,
                                                  src.numel(), tail, K, out.data_ptr(), be.data_ptr(), br.data_ptr(),
                                                  ctypes.c_void_p(stream.cuda_stream)))
        b.record(stream)
        b.synchronize()
        times.append(a.elapsed_time(b))
    times = sorted(times[1:])
    return times[len(times) // 2], out


def weight_grad_kernel_ms(csr, n_rel, dev, reps):
    """The rotate d_weight launch alone on the graph's forward plan (F = block = 64, sum): median ms of ``reps`` launches."""
    from ultra_torchdrug_amd import _lib
    lib = _lib.load()
    gen = torch.Generator(device=dev).manual_seed(7)
    x, grad = (torch.randn(csr.shape[0], 64, device=dev, generator=gen) for _ in range(2))
    relation = torch.randn(n_rel, 64, device=dev, generator=gen)
    d_w = torch.empty(csr.n_edges, dtype=torch.float32, device=dev)
    plan = csr.fwd
    stream = torch.cuda.current_stream()
    times = []
    for _ in range(reps + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        _lib.check(lib.ultra_rspmm_rotate_backward_weight_f32(plan.pointer, relation.data_ptr(), x.data_ptr(), None, grad.data_ptr(),
                                                              d_w.data_ptr(), n_rel, 64, 64, 0,
                                                              ctypes.c_void_p(stream.cuda_stream)))
        b.record(stream)
        b.synchronize()
        times.append(a.elapsed_time(b))
    times = sorted(times[1:])
    return times[len(times) // 2]


def run(workload, dev, reps, beams_k, message="distmult", materialised=False):
    from ultra_torchdrug_amd import functional
    rec = {"workload": workload, "message": message, "route": "materialised" if materialised else "native", "B": 1,
           "num_beam": beams_k}
    t0 = time.perf_counter()
    graph, model, rel = build(workload, dev, message)
    model.num_beam, model.path_topk = beams_k, 10
    und = model._undirected(graph)
    csr = und.relcsr
    _ = csr.csr_arrays, csr.fwd, csr.by_src, csr.by_rel
    torch.cuda.synchronize()
    rec["build_s"] = time.perf_counter() - t0
    n, E = und.num_node, csr.n_edges
    rec["N"], rec["E"] = n, E
    h, t, r = (int(x) for x in graph.edge_list[0])
    rec["triple"] = [h, t, r]
    model.visualize(graph, [rel], [h], [t], [r])            # warm-up: lazily built indices, code objects
    torch.cuda.synchronize()
    grad_ms, total_ms = [], []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        grads = model.edge_gradients(graph, [rel], [h], [t], [r])
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        del grads
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        paths, weights = model.visualize(graph, [rel], [h], [t], [r])
        torch.cuda.synchronize()
        t3 = time.perf_counter()
        peak = torch.cuda.max_memory_allocated() - base
        grad_ms.append(1e3 * (t1 - t0))
        total_ms.append(1e3 * (t3 - t2))
    rec["gradient_ms"] = sorted(grad_ms)[len(grad_ms) // 2]
    rec["visualize_ms"] = sorted(total_ms)[len(total_ms) // 2]
    rec["search_ms"] = rec["visualize_ms"] - rec["gradient_ms"]
    rec["peak_extra_bytes"] = int(peak)
    rec["one_message_tensor_bytes"] = E * 64 * 4
    rec["n_paths"] = len(paths)
    rec["top_path"] = [list(e) for e in paths[0]] if paths else None
    rec["top_weight"] = weights[0] if weights else None
    if materialised:                 # the comparison leg: times and memory of the route, no kernel figures
        return rec
    if message == "rotate":
        floor_w = E * (12 * 64 + 16)
        ms = weight_grad_kernel_ms(csr, csr.shape[2], dev, max(reps, 5))
        rec["weight_grad_kernel"] = {"byte_floor": floor_w, "ms": ms, "GB_per_s_of_floor": floor_w / ms / 1e6,
                                     "fraction_of_hbm_peak": floor_w / (ms * 1e-3) / HBM_PEAK}
    # the beam kernel alone, per layer, on that layer's real inputs
    grads = model.edge_gradients(graph, [rel], [h], [t], [r])
    row_ptr, src, _, _ = csr.csr_arrays
    beams = torch.full((n, beams_k), float("-inf"), device=dev)
    beams[h, 0] = 0
    floor = E * (8 + 4 + 4 * beams_k) + 4 * (n + 1) + 12 * n * beams_k
    layers = []
    for g in grads:
        g = g.contiguous()
        ms, out = kernel_ms(row_ptr, src, g, beams, t, reps)
        want = functional.beam_search_step(row_ptr, src, g, beams, t)[0]
        assert torch.equal(out, want)
        layers.append({"ms": ms, "GB_per_s_of_floor": floor / ms / 1e6, "fraction_of_hbm_peak": floor / (ms * 1e-3) / HBM_PEAK})
        beams = want
    rec["beam_kernel"] = {"byte_floor_per_layer": floor, "layers": layers}
    return rec


def _event_ms(fn):
    """Device time of ``fn()`` between two events; the call is followed by a synchronise."""
    stream = torch.cuda.current_stream()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record(stream)
    out = fn()
    b.record(stream)
    b.synchronize()
    return a.elapsed_time(b), out


def _median_ms(fn, reps=5, warmup=2):
    for _ in range(warmup):
        _event_ms(fn)
    times = sorted(_event_ms(fn)[0] for _ in range(reps))
    return times[len(times) // 2]


def run_batch(workload, dev, n_query, beams_k, message="distmult", alternations=3):
    rec = {"workload": workload, "message": message, "B": n_query, "num_beam": beams_k, "timing": "device events; median of 5 "
           "after 2 warm-ups per figure; %d alternations of the two legs in one run" % alternations}
    graph, model, _ = build(workload, dev, message)
    model.num_beam, model.path_topk = beams_k, 10
    csr = model._undirected(graph).relcsr
    _ = csr.csr_arrays, csr.fwd, csr.by_src, csr.by_rel
    rec["N"], rec["E"] = graph.num_node, csr.n_edges
    rel = torch.randn(n_query, 2 * graph.num_relation, 64, device=dev, generator=torch.Generator(device=dev).manual_seed(1))
    rows = torch.arange(n_query, device=dev) * (len(graph.edge_list) // n_query)         # spread over the edge list
    h, t, r = (graph.edge_list[rows, c] for c in range(3))
    rec["triples"] = torch.stack([h, t, r], 1).tolist()
    one = lambda b: ([rel[b:b + 1]], h[b:b + 1], t[b:b + 1], r[b:b + 1])
    legs = {
        "looped": (lambda: [model.edge_gradients(graph, *one(b)) for b in range(n_query)],
                   lambda: [model.visualize(graph, *one(b)) for b in range(n_query)]),
        "batched": (lambda: model.edge_gradients_batch(graph, [rel], h, t, r),
                    lambda: model.visualize_batch(graph, [rel], h, t, r)),
    }
    rounds = []
    for _ in range(alternations):
        entry = {}
        for name, (gradients, whole) in legs.items():
            g_ms, v_ms = _median_ms(gradients), _median_ms(whole)
            entry[name] = {"ms_per_triple": v_ms / n_query, "gradient_ms_per_triple": g_ms / n_query,
                           "search_ms_per_triple": (v_ms - g_ms) / n_query}
        entry["ratio"] = entry["batched"]["ms_per_triple"] / entry["looped"]["ms_per_triple"]
        rounds.append(entry)
    rec["alternations"] = rounds
    median = lambda xs: sorted(xs)[len(xs) // 2]
    for name in legs:
        rec[name] = {key: median([e[name][key] for e in rounds]) for key in rounds[0][name]}
    rec["ratio"] = rec["batched"]["ms_per_triple"] / rec["looped"]["ms_per_triple"]
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    batched = legs["batched"][1]()
    torch.cuda.synchronize()
    rec["batched_peak_extra_bytes"] = int(torch.cuda.max_memory_allocated() - base)
    rec["one_batched_message_tensor_bytes"] = n_query * csr.n_edges * 64 * 4
    looped = legs["looped"][1]()
    rec["same_paths"] = sum(int(a[0] == b[0]) for a, b in zip(batched, looped))
    rec["n_paths"] = [len(p) for p, _ in batched]
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="S-fb15k237,S-stress")
    ap.add_argument("--messages", default="distmult", help="message functions, e.g. distmult,rotate")
    ap.add_argument("--materialised", default="", help="workloads that also get a leg on the materialised route")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--beams", type=int, default=10)
    ap.add_argument("--json", default=None)
    ap.add_argument("--batch", type=int, nargs="?", const=16, default=None,
                    help="time B looped visualize calls against one visualize_batch (B = 16 when no value is given)")
    args = ap.parse_args()
    if args.batch is not None and args.batch < 1:
        raise SystemExit("--batch needs a positive number of triples")
    import ultra_torchdrug_amd as U
    U.require_library()
    if not torch.cuda.is_available():
        raise SystemExit("explain_bench.py measures on an MI355X; no GPU is visible")
    dev = torch.device("cuda:0")
    out = {"device": torch.cuda.get_device_name(0), "results": []}
    from ultra_torchdrug_amd.layer import _RelationalConvBase
    if args.batch is not None:
        out["batch"] = args.batch
        for workload in args.workloads.split(","):
            for message in args.messages.split(","):
                try:
                    out["results"].append(run_batch(workload, dev, args.batch, args.beams, message))
                except Exception as err:        # (out of memory: activation memory grows with B): recorded, not hidden
                    out["results"].append({"workload": workload, "message": message, "B": args.batch,
                                           "error": "%s: %s" % (type(err).__name__, err)})
                torch.cuda.empty_cache()
                print(json.dumps(out["results"][-1]), file=sys.stderr, flush=True)
        text = json.dumps(out, indent=1)
        print(text)
        path = args.json or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                         "explain_batch_bench.json")
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            f.write(text + "\n")
        return
    legs = [(w, m, False) for w in args.workloads.split(",") for m in args.messages.split(",")]
    legs += [(w, m, True) for w in args.materialised.split(",") if w for m in args.messages.split(",")]
    native_edge_grad = _RelationalConvBase.native_edge_grad
    for workload, message, materialised in legs:
        if materialised:            # every layer declines its native edge gradient: model._edge_grad_graph clones the graph
            _RelationalConvBase.native_edge_grad = lambda self, *args: False
        try:
            out["results"].append(run(workload, dev, args.reps, args.beams, message, materialised))
        except Exception as err:            # (out of memory on a smaller device, ...): recorded, not hidden
            out["results"].append({"workload": workload, "message": message, "error": "%s: %s" % (type(err).__name__, err)})
        finally:
            _RelationalConvBase.native_edge_grad = native_edge_grad
        torch.cuda.empty_cache()
        print(json.dumps(out["results"][-1]), file=sys.stderr, flush=True)
    text = json.dumps(out, indent=1)
    print(text)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()

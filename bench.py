"""bench.py -- edges aggregated / second of the rspmm Bellman-Ford hot path on MI355X.

Contract (driver): ``python bench.py --gpus N --steps K --warmup W``; for N > 1 it is launched by
``python -m torch.distributed.run --nproc-per-node N ...`` (one rank per GPU, RCCL).  Rank 0 prints ONE JSON line.
``--gpus N`` WITHOUT a launcher (no WORLD_SIZE in the environment) starts the N ranks itself: the parent makes no GPU call,
spawns ``python -m torch.distributed.run --nproc-per-node N bench.py ...`` as a child, relays rank 0's line and exits with
the children's code; fewer than N visible devices (or a WORLD_SIZE that contradicts ``--gpus``) is a non-zero exit, never
an ``n_gpus: 1`` line.  With ``--full``, at N > 1 every rank also runs BASELINE config 4 -- the pretrain_3g-shaped step, B = 64 per rank, with
the bucketed RCCL gradient all-reduce (``engine.GradientReducer``; ranks draw their graphs with seed + rank,
/root/reference/script/run_full.py:102-107) -- timed as max over ranks, next to the same steps without the collectives.

Workload (BASELINE.json metric: "edges aggregated/sec ... FB15k237 6L x 64d rspmm"): S-fb15k237 -- a seeded
synthetic KG of FB15k237's size (N=14 541, 272 115 triples, 237 relations => E=544 230, R=474 after inverse
edges), seeded random-init Ultra weights (6 x 64d entity stack + 6 x 64d relation stack).
One STEP = one evaluation batch of B=16 test triples through ``predict`` (/root/reference/ultra/task.py:228-263):
relation-graph Bellman-Ford (6 rspmm) + tail pass + head pass over all N candidates (the reference: 2 x 6 rspmm +
epilogues + score MLP = 18 rspmm calls; here the tail and head queries share ONE 2B-wide Bellman-Ford, every score
bit-identical: tests/test_model_gpu.py), replayed as one hipGraph.  All inputs are resident in HBM before the timed
region.  Multi-GPU: every rank holds the graph and evaluates its own query batch (query sharding, no data-path
collective) => weak scaling; ``value`` = units of all ranks / max-over-ranks time.

A plain run does only what the headline needs: set-up, ``--warmup`` steps, the ``--steps`` timed steps, the result line
(``metric``, ``value``, ``unit``, ``higher_is_better``, ``dtype``, ``ms_per_step`` = milliseconds of one timed step, and the
spread of the blocks inside the timed region).  Everything else below -- the per-kernel and composition timings after the
timed region, the per-config timings (``config.configs``), S-stress (``roofline``), MRR with the CPU-oracle check, the
fine-tuning run, ``cpu_baseline`` -- runs with ``--full`` only.  ``--dump-outputs DIR`` writes what the timed path returned in
its last step (rank 0): ``DIR/scores.npy``, the float32 (B, 2, N) scores of ``predict``; the inputs are seeded, so two builds
run with the same arguments can be compared output for output.

What ``value`` counts (round 3).  Unit of work = one edge message = one ENTITY-graph edge x one
query x 64 fp32 lanes that a kernel actually VISITS.  Per step: layers 2-6 walk all E edges for 2B queries
(10 * E * B messages) and layer 1 -- whose input is the boundary, zero outside one row per query -- visits only the
out-edges of the boundary nodes (the frontier kernel; ``config.frontier_edges_per_step``, counted exactly).  The
relation-graph stack (a complete 474-node graph under the SURVEY 8d generator, LDS-resident, not a sparse-gather
workload) is part of the step's TIME but not of ``value``; its rate is ``config.relation_graph_edges_per_s``.  The
figure round 2 printed (all 12 * E * B + 6 * E_rel * B messages, visited or not) is ``config.value_r2_definition``.

Driver-kept keys (the driver keeps metric / value / ... / config / roofline / cpu_baseline and only the NAMES of the
rest), so everything a reader needs to check the headline sits in those three objects:
* ``config``       -- workload, what ``value`` counts, per-rank times, and ``config.configs``: one timing per BASELINE
                      config measured in THIS run (1: inductive v1 shape on the CPU kernels; 2: S-codexs inference;
                      3: S-wn18rr operator fwd+bwd and fine-tune step, median + spread; 4: pretrain_3g-shaped B = 64
                      step; 5: S-stress).
* ``roofline``     -- SURVEY 8d's line: S-stress (10 M nodes / 100 M edges / 1 k relations, B = 1) AT SIZE, algorithmic
                      bytes / HIP-event kernel time against the 8 TB/s HBM peak.  ``roofline.l2`` is the dominant kernel
                      of the HEADLINE workload, whose gathered matrix (119 MB) is cache-resident: priced against the
                      XCD-L2 peak, never against HBM (its algorithmic rate exceeds 8 TB/s).
* ``cpu_baseline`` -- the CPU restatement (oracle row loop, rebuilt -O3 -march=native here, OpenMP, kind "port") on all
                      host cores, one rspmm call of the headline graph at the GPU kernel's width F = 2 * B * 64.
"""
import argparse
import ctypes
import glob
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np
import torch
import torch.distributed as dist

# MI355X_MICROARCH.md: chip-level parameters / L2 (per XCD) / Indexed rows: gather into LDS
HBM_PEAK_GBS = 8000.0
L2_PEAK_GBS = 34500.0
L2_GATHER_CEILING_GBS = (16800.0, 18800.0)

# FB15k237Inductive v1 (GraIL split) sizes [ULTRA paper's dataset table; the files are fetched at run time by the
# reference, /root/reference/ultra/dataset.py:450-460]: relations, (entities, triples) of the training graph,
# (entities, fact triples, valid, test) of the inference graph
FB_V1 = dict(n_rel=180, train=(1594, 4245), inference=(1093, 1993, 206, 205))
PRETRAIN_3G = ("S-fb15k237", "S-wn18rr", "S-codexm")


class HipEvents:
    """hipEvent_t pairs created through the library (same HIP runtime as the kernels); the C ABI's profile hook
    records them on the kernel's own stream."""

    def __init__(self, lib):
        self.lib = lib
        self.pairs = []

    def new_pair(self):
        a, b = ctypes.c_void_p(), ctypes.c_void_p()
        assert self.lib.ultra_rspmm_event_create(ctypes.byref(a)) == 0
        assert self.lib.ultra_rspmm_event_create(ctypes.byref(b)) == 0
        self.pairs.append((a, b))
        return a, b

    def elapsed_ms(self):
        out = []
        for a, b in self.pairs:
            ms = ctypes.c_float()
            rc = self.lib.ultra_rspmm_event_elapsed_ms(a, b, ctypes.byref(ms))
            assert rc == 0, "event_elapsed_ms failed: %d (hip %d)" % (rc, self.lib.ultra_rspmm_last_hip_error())
            out.append(ms.value)
        return out


def bytes_algo(E, N, R, F):
    """every edge gathers one F-wide fp32 source row and a 12-byte (src, rel, w) triple; every
    destination row is written once; relation table and row pointers are read once."""
    return E * (4 * F + 12) + 4 * N * F + 4 * R * F + 4 * (N + 1)


def bytes_min(E, N, R, F):
    """SURVEY.md 8d, compulsory bytes (perfect reuse): input read once, output written once, indices, relation table."""
    return 8 * N * F + 4 * R * F + 12 * E + 4 * (N + 1)


def timed_kernel(lib, events, fn, n):
    """Average duration (ms) of the main rspmm kernel inside `fn`, from HIP events recorded by the library around it."""
    first = len(events.pairs)
    for _ in range(n):
        a, b = events.new_pair()
        lib.ultra_rspmm_profile_next(a, b)
        fn()
    torch.cuda.synchronize()
    ms = events.elapsed_ms()[first:]
    return float(np.mean(ms)), len(ms)


def wall_ms(fn, n, warm=0):
    """Host-clock time per call of ``fn(i)`` over n calls between two device synchronisations."""
    for i in range(warm):
        fn(i)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(n):
        fn(i)
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / max(n, 1)


def spread(samples):
    """Median and spread of per-step times (ms): the fine-tune step moved between 7.9 and 11 ms over round 2's records."""
    s = np.sort(np.asarray(samples, dtype=np.float64))
    return {"n": int(len(s)), "median_ms": float(np.median(s)), "min_ms": float(s[0]), "max_ms": float(s[-1]),
            "p10_ms": float(s[int(0.1 * (len(s) - 1))]), "p90_ms": float(s[int(round(0.9 * (len(s) - 1)))])}


def host_cores():
    """Cores in this process's affinity mask, capped by the cgroup's CPU quota where one is set."""
    n = len(os.sched_getaffinity(0))
    try:
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
        if quota != "max":
            n = max(1, min(n, int(int(quota) / int(period))))
    except (OSError, ValueError):
        pass
    return n


def cpu_baseline(graph_np, n_node, n_rel, F, budget_s=24.0):
    """The oracle's CSR row loop (OpenMP; rebuilt here with -O3 -march=native -ffp-contract=off) on ONE rspmm call of
    the bench graph at the width of the GPU's launch; rank 0, N=1 only.  A GPU box's affinity mask may list more cores
    than its share of the host grants, so a few OpenMP team sizes are timed and the FASTEST is reported with the thread
    count it used (``cores``); every team size's median is in ``threads_tried``."""
    from oracle import oracle as O
    cores = host_cores()
    os.environ["OMP_NUM_THREADS"] = str(cores)
    O.build()
    try:
        forward, build = O.native_forward_fn(), "gcc -O3 -march=native -ffp-contract=off -fopenmp (built on this host)"
    except Exception as err:                         # no compiler on the box: the committed portable build
        forward, build = O.rspmm_forward, "oracle/Makefile build (-O3, portable); native rebuild failed: %s" % err
    rng = np.random.default_rng(1024)
    csr = O.coalesce_csr(graph_np["dst"], graph_np["src"], graph_np["rel"], None, n_node, n_node, n_rel)
    relation = rng.standard_normal((n_rel, F)).astype(np.float32)
    x = rng.standard_normal((n_node, F)).astype(np.float32)
    forced = int(os.environ.get("ULTRA_BENCH_CPU_THREADS", "0"))
    sizes = [forced] if forced else sorted({cores, min(cores, 128), min(cores, 64), min(cores, 32), min(cores, 16)}, reverse=True)
    set_threads = getattr(forward, "set_threads", None)
    if set_threads is None:
        sizes = sizes[:1]
    tried, best = {}, None
    t_all = time.perf_counter()
    for n_thr in sizes:
        if set_threads is not None:
            set_threads(n_thr)
        forward(csr, relation, x, "add", "mul")                    # warm-up (page-in, thread pool)
        times = []
        t_start = time.perf_counter()
        while len(times) < 10 and (time.perf_counter() - t_start) < budget_s / len(sizes):
            t0 = time.perf_counter()
            forward(csr, relation, x, "add", "mul")
            times.append(time.perf_counter() - t0)
        tried[str(n_thr)] = float(np.median(times))
        if best is None or tried[str(n_thr)] < best[1]:
            best = (n_thr, tried[str(n_thr)], len(times))
    cpu_wall = time.perf_counter() - t_all
    threads, med, n_calls = best
    # second CPU number: the reference's own O(E) formulation (ultra/layer.py:249-255,275-276) in PyTorch
    torch.set_num_threads(threads)
    ti = torch.from_numpy(csr.col.astype(np.int64)); tr = torch.from_numpy(csr.rel.astype(np.int64))
    td = torch.from_numpy(csr.row.astype(np.int64))
    Fm = min(F, 1024)                                          # (E, F) fp32 temporaries: 2.2 GB each at F = 1 024
    tx, trel = torch.from_numpy(x[:, :Fm].copy()), torch.from_numpy(relation[:, :Fm].copy())
    t0 = time.perf_counter()
    torch.zeros(n_node, Fm).index_add_(0, td, trel[tr] * tx[ti])
    t_torch = time.perf_counter() - t0
    algo = bytes_algo(csr.n_edges, n_node, n_rel, F)
    return {"value": csr.n_edges * (F // 64) / med, "unit": "edges aggregated/s", "cores": threads,
            "kind": "port", "algorithmic_GBps": algo / med / 1e9, "seconds_per_call": med, "F": F,
            "threads_tried": tried, "affinity_cores": len(os.sched_getaffinity(0)),
            "torch_materialised_value": csr.n_edges * (Fm // 64) / t_torch, "build": build,
            "sample": "%d x one rspmm forward (add,mul) on S-fb15k237, E=%d, F=%d (the GPU launch's width: tail and head "
                      "queries of B=%d) with %d OpenMP threads (fastest of the team sizes %s); median %.4f s; %.1f s of CPU-leg "
                      "wall time in all; oracle/rspmm_oracle.c row loop (64-column x equal-edge row-range tasks), restatement of "
                      "the torchdrug CPU algorithm" % (n_calls, csr.n_edges, F, F // 128, threads, sorted(int(k) for k in tried),
                                                       med, cpu_wall)}


def latest_profile(pattern):
    """Newest committed PMC summary of a kind (profiles/rNN_<pattern>): measured in separate rocprofv3 --pmc passes of the
    same kernel and workload, never in this run."""
    paths = sorted(glob.glob(os.path.join(ROOT, "profiles", "r[0-9][0-9]_" + pattern)))
    if not paths:
        return None, None
    try:
        with open(paths[-1]) as f:
            return json.load(f), "profiles/%s (rocprofv3 --pmc passes, not this run)" % os.path.basename(paths[-1])
    except (OSError, ValueError):
        return None, None


def stress_roofline(dev, lib, n_node=10_000_000, n_triple=50_000_000, n_base_rel=500, cpu_leg=True):
    """Config 5 at size: S-stress -- uniform triples + inverse edges => E = 100 M, R = 1 000, 64d.
    (i) the operator at B = 1 (the gathered matrix, 2.56 GB, cannot live in any cache: the HBM roofline of the path) and at
    B = 4 (`b4`: 1-KiB gathers, 64 lanes per row); (ii) what BASELINE calls this config -- INFERENCE: the whole `predict` of the
    shipped 6 x 64d model (relation stack, 6 entity layers with their epilogues, score head) + the filtered rank, at B = 1 and
    B = 4 triples (2 B queries), with one middle layer kernel by kernel; (iii) the CPU restatement on the same graph (`cpu`)."""
    from ultra_torchdrug_amd import functional as UF
    from ultra_torchdrug_amd.data import stress_task
    t0 = time.perf_counter()
    task, gen = stress_task(dev, n_node, n_triple, n_base_rel)
    torch.cuda.synchronize()
    task_s = time.perf_counter() - t0
    t0 = time.perf_counter()
    und = task.model._undirected(task.fact_graph)
    csr = und.relcsr
    plan = csr.fwd
    _ = csr.frontier_index
    _ = task.rel_graphs[0].relcsr.fwd
    torch.cuda.synchronize()
    build_s = time.perf_counter() - t0
    R = 2 * n_base_rel
    E = csr.n_edges
    events = HipEvents(lib)

    def operator(F, reps):
        x = torch.randn(n_node, F, device=dev, generator=gen)
        relation = torch.randn(R, F, device=dev, generator=gen)
        for _ in range(3):
            UF.rspmm_forward(csr, relation, x, "add", "mul")
        ms, n = timed_kernel(lib, events, lambda: UF.rspmm_forward(csr, relation, x, "add", "mul"), reps)
        return x, relation, ms, n

    x, relation, ms, n = operator(64, 12)
    # the chunked kernel the plan would run without the row-per-group kernel (A/B of the same launch)
    lib.ultra_rspmm_force_general_path(8)
    try:
        for _ in range(2):
            UF.rspmm_forward(csr, relation, x, "add", "mul")
        ms_chunked, _ = timed_kernel(lib, events, lambda: UF.rspmm_forward(csr, relation, x, "add", "mul"), 6)
    finally:
        lib.ultra_rspmm_force_general_path(0)
    algo = bytes_algo(E, n_node, R, 64)
    kernel = "rowgroup_kernel<add,mul,unit_w,624 of 1000 relation rows from LDS>" if plan.row_ptr is not None and plan.n_pieces == 0 \
        else "packed_kernel<FWD,add,mul,unit_w,VAR 2>"
    tj, tsrc = latest_profile("traffic_stress.json")
    achieved = algo / (ms * 1e-3) / 1e9
    cal = box_calibration(dev, lib, x, plan.node_a[:E])
    del x, relation
    _, _, ms4, n4 = operator(256, 6)
    torch.cuda.empty_cache()
    algo4 = bytes_algo(E, n_node, R, 256)
    b4 = {"bound": "hbm", "achieved": algo4 / (ms4 * 1e-3) / 1e9, "peak": HBM_PEAK_GBS, "unit": "GB/s",
          "frac": algo4 / (ms4 * 1e-3) / 1e9 / HBM_PEAK_GBS, "kernel_ms": ms4, "algorithmic_bytes": algo4, "launches_timed": n4,
          "workload": "S-stress B=4 F=256 (input %.2f GB; one 1-KiB gather per edge, 64 lanes per row)" % (n_node * 256 * 4 / 1e9),
          "edges_per_s": 4 * E / (ms4 * 1e-3)}
    inference = stress_inference(task, csr, gen, n_node, n_base_rel)
    inference["task_build_s"] = task_s
    # (the CPU leg: rank 0 at N = 1 only, as the contract's cpu_baseline)
    cpu = stress_cpu_baseline(csr, plan, n_node, R) if cpu_leg else {"skipped": "N > 1 or --no-cpu-baseline"}
    # the keys the driver's record keeps come first: the contract's six, then what THIS box delivers ("confirm on the
    # box with a copy / gather calibration, report both") -- `frac` moves 0.65 <-> 0.70 with the box, `frac_of_gather` says how much
    # of that is the box and how much the kernel
    return {"bound": "hbm", "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": achieved / HBM_PEAK_GBS,
            "traffic": tj.get("hbm_bytes_per_launch") if tj else None,
            "copy_GBps": cal["copy_GBps"], "gather_GBps": cal["gather_GBps"], "frac_of_gather": achieved / cal["gather_GBps"],
            "frac_of_copy": achieved / cal["copy_GBps"],
            "kernel_ms": ms, "algorithmic_bytes": algo, "bytes_per_unit": algo / E, "launches_timed": n,
            "workload": "S-stress N=%d E=%d R=%d B=1 F=64 (input %.2f GB)" % (n_node, E, R, n_node * 64 * 4 / 1e9),
            "kernel": kernel, "edges_per_s": E / (ms * 1e-3), "chunked_kernel_ms": ms_chunked, "plan_build_s": build_s,
            "traffic_source": tsrc, "calibration": cal["note"],
            "timed": "HIP events recorded by the library around the kernel, on the kernel's stream, %d launches" % n,
            "b4": b4, "inference": inference, "cpu": cpu}


def stress_inference(task, csr, gen, n_node, n_base_rel):
    """BASELINE config 5 as INFERENCE (/root/reference/ultra/task.py:228-263, ultra/model.py:101-143,182-194): `predict` + filtered
    rank on S-stress, eager (every kernel runs for milliseconds: nothing to gain from a hipGraph), B = 1 and B = 4 triples; and
    the sequence `TransferNBFNet.score_both_sides` runs, op by op between stream events, at B = 1."""
    from ultra_torchdrug_amd import backend
    dev = csr.device
    ops = backend.get()
    E, R = csr.n_edges, 2 * n_base_rel
    out = {}

    def draw(B):
        return torch.stack([torch.randint(0, n_node, (B,), device=dev, generator=gen),
                            torch.randint(0, n_node, (B,), device=dev, generator=gen),
                            torch.randint(0, n_base_rel, (B,), device=dev, generator=gen)], dim=1)

    with torch.no_grad():
        for B in (1, 4):
            batch = draw(B)
            pred = task.predict(batch)
            ranks = task.rank_batch(batch, pred)
            torch.cuda.synchronize()
            p_ms, r_ms = [], []
            for _ in range(3):
                t0 = time.perf_counter()
                pred = task.predict(batch)
                torch.cuda.synchronize()
                t1 = time.perf_counter()
                task.rank_batch(batch, pred)
                torch.cuda.synchronize()
                p_ms.append(1e3 * (t1 - t0)); r_ms.append(1e3 * (time.perf_counter() - t1))
            tag = "b%d" % B
            out[tag] = {"triples": B, "queries": 2 * B, "F": 128 * B, "predict_ms": float(np.median(p_ms)),
                        "filtered_rank_ms": float(np.median(r_ms)), "ranks_first": ranks[0].tolist(),
                        "scores_finite": bool(torch.isfinite(pred).all()),
                        "entity_edge_messages_per_s": 5 * E * 2 * B / (float(np.median(p_ms)) * 1e-3),
                        "counts": "5 full entity layers x E x 2B queries (the first layer visits the boundary nodes' out-edges "
                                  "only) over the whole predict: relation stack, epilogues and score head are in the time"}
            del pred
        torch.cuda.empty_cache()
        # ---- B = 1, op by op (what score_both_sides runs)
        model = task.model
        batch = draw(1)
        rel_rep = task.relation_representations(batch[:, 2])[0]
        stack = model._fast_stack()
        anchor, anchor32, relation, query = ops.prepare_queries(batch, rel_rep, n_base_rel)
        tables = ops.relation_project(rel_rep, [entry["project"] for entry in stack], repeat=2)
        boundary = (anchor32, query)
        marks = []

        def mark(name):
            e = torch.cuda.Event(enable_timing=True)
            e.record()
            marks.append((name, e))

        forms_equal = None
        for rep in range(2):                                           # the second pass is the measured one
            marks.clear()
            mark("start")
            w, b, g, beta, eps, relu = stack[0]["combine"]
            first_out = ops.first_layer_forward(csr, tables[0], boundary, w, b, g, beta, eps, relu, model.short_cut, want_list=True)
            hidden, listed = (None, None) if first_out is None else (first_out[0], first_out[1:])
            if hidden is None:
                update = ops.rspmm_frontier(csr, tables[0], boundary).view(n_node, 2, 64)
                hidden = ops.combine_forward(None, update, w, b, g, beta, eps, relu, model.short_cut, reuse_update=True,
                                             input_boundary=boundary)
            mark("first_layer")
            for i in range(1, len(stack)):
                w, b, g, beta, eps, relu = stack[i]["combine"]
                if i == 1:
                    # layer 2 three ways on the same input: the TWO launches the fused kernel replaces (A/B), the fused launch, and
                    # the fused launch with the constant-row sources predict uses after a sparse first layer -- equal bits required
                    update = ops.rspmm_forward(csr, tables[i], hidden.flatten(1), "add", "mul", boundary=boundary)
                    mark("rspmm_%d" % (i + 1))
                    split = ops.combine_forward(hidden, update.view(n_node, 2, 64), w, b, g, beta, eps, relu, model.short_cut,
                                                reuse_update=True)
                    mark("epilogue_%d" % (i + 1))
                    fused = ops.layer_forward(csr, tables[i], hidden, boundary, w, b, g, beta, eps, relu, model.short_cut)
                    mark("layer_%d" % (i + 1))
                    again = None
                    if fused is not None:
                        sources = ops.second_layer_sources(csr, listed[0], listed[1], 2) if listed is not None else None
                        mark("second_layer_sources")
                        if sources is not None:
                            again = ops.layer_forward(csr, tables[i], hidden, boundary, w, b, g, beta, eps, relu, model.short_cut,
                                                      sources=sources)
                            mark("layer_2_constant_sources")
                        forms_equal = bool(torch.equal(fused, split)) and (again is None or bool(torch.equal(again, split)))
                    del fused, again
                    hidden = split
                    del update, split
                    mark("(comparisons)")
                    continue
                if i == len(stack) - 1:                                # the last layer with the score head inside, as predict runs it
                    first, second = model.mlp.layers
                    score = ops.layer_score_forward(csr, tables[i], hidden, boundary, w, b, g, beta, eps, relu, model.short_cut, query,
                                                    first.weight, first.bias, second.weight, second.bias)
                    if score is not None:
                        mark("last_layer_with_score_head")
                        hidden = None
                        break
                fused = ops.layer_forward(csr, tables[i], hidden, boundary, w, b, g, beta, eps, relu, model.short_cut)
                if fused is not None:
                    hidden = fused
                    mark("layer_%d" % (i + 1))
                    continue
                update = ops.rspmm_forward(csr, tables[i], hidden.flatten(1), "add", "mul", boundary=boundary)
                mark("rspmm_%d" % (i + 1))
                hidden = ops.combine_forward(hidden, update.view(n_node, 2, 64), w, b, g, beta, eps, relu, model.short_cut,
                                             reuse_update=True)
                mark("epilogue_%d" % (i + 1))
            if hidden is not None:
                first, second = model.mlp.layers
                ops.score_all_entities(hidden, query, first.weight, first.bias, second.weight, second.bias)
                mark("score_head")
            torch.cuda.synchronize()
        steps = {name: marks[k - 1][1].elapsed_time(e) for k, (name, e) in enumerate(marks) if k > 0}
        rspmm = float(np.median([v for k, v in steps.items() if k.startswith("rspmm_")]))
        epi = float(np.median([v for k, v in steps.items() if k.startswith("epilogue_")]))
        fused_ms = [v for k, v in steps.items() if k.startswith("layer_") and not k.startswith("layer_2")]
        F = 128
        split_bytes = bytes_algo(E, n_node, R, F) + 3 * n_node * F * 4
        fused_bytes = bytes_algo(E, n_node, R, F) + 1 * n_node * F * 4            # the `update` rows neither written nor read
        layer_ms = float(np.median(fused_ms)) if fused_ms else rspmm + epi
        layer_bytes = fused_bytes if fused_ms else split_bytes
        tlj, tlsrc = latest_profile("traffic_layer_fused.json")
        out["layer_b1"] = {"first_layer_ms": steps["first_layer"], "layer_ms": layer_ms,
                           "traffic": (tlj.get("hbm_bytes_per_launch") if fused_ms else tlj.get("two_launch_hbm_bytes_per_layer")) if tlj else None,
                           "traffic_source": tlsrc,
                           "layer_kernel": "rowgroup_layer_kernel (rspmm + epilogue in one launch, csrc/layer_fused.hip)" if fused_ms
                                           else "rowgroup_kernel + combine_kernel",
                           "two_launch_rspmm_ms": rspmm, "two_launch_epilogue_ms": epi, "two_launch_layer_ms": rspmm + epi,
                           "second_layer_constant_sources_ms": steps.get("layer_2_constant_sources"),
                           "second_layer_sources_build_ms": steps.get("second_layer_sources"),
                           "layer_2_forms_bit_identical": forms_equal,
                           "score_head_ms": steps.get("score_head"),
                           "last_layer_with_score_head_ms": steps.get("last_layer_with_score_head"), "steps_ms": steps,
                           "layer_algorithmic_bytes": layer_bytes, "two_launch_layer_algorithmic_bytes": split_bytes,
                           "frac_of_hbm_peak_whole_layer": layer_bytes / (layer_ms * 1e-3) / 1e9 / HBM_PEAK_GBS,
                           "frac_of_hbm_peak_two_launch_layer": split_bytes / ((rspmm + epi) * 1e-3) / 1e9 / HBM_PEAK_GBS,
                           "frac_of_hbm_peak_rspmm": bytes_algo(E, n_node, R, F) / (rspmm * 1e-3) / 1e9 / HBM_PEAK_GBS,
                           "bytes": "one layer = rspmm's algorithmic bytes at F = 128 (E (4F + 12) + 4NF + 4RF + 4(N + 1)) + the epilogue's "
                                    "own streams: the rows' input segments in (N F 4; the output rows are the rspmm's) when fused, input + "
                                    "update in and output out (3 N F 4) as two launches; stream events on the launch stream between eager "
                                    "calls; layer 2 runs three ways on the same input (two launches, fused, fused with the constant-row sources predict uses: "
                                    "`layer_2_forms_bit_identical`), layers 3-5 fused (median), the last layer with the score head"}
    return out


def stress_cpu_baseline(csr, plan, n_node, n_rel, budget_s=20.0):
    """SURVEY 8d's second CPU leg: the restatement of the torchdrug CPU algorithm (oracle/rspmm_oracle.c) on S-stress, B = 1,
    on this host's cores -- only when the host has the memory for it (the operands are ~8 GB).  The coalesced CSR comes from the
    device's plan (sorting 100 M keys on the host is not what is timed)."""
    try:
        avail = next(int(l.split()[1]) for l in open("/proc/meminfo") if l.startswith("MemAvailable")) / 1e6
    except (OSError, StopIteration, ValueError):
        avail = 0.0
    if avail < 24.0:
        return {"skipped": "host reports %.1f GB available (< 24 GB)" % avail}
    from oracle import oracle as O
    cores = host_cores()
    os.environ["OMP_NUM_THREADS"] = str(cores)
    O.build()
    try:
        forward = O.native_forward_fn()
    except Exception:
        forward = O.rspmm_forward
    E = csr.n_edges
    row_ptr = plan.row_ptr if plan.row_ptr is not None else torch.searchsorted(plan.row[:E], torch.arange(n_node + 1, dtype=torch.int32, device=plan.row.device))
    host = O.CSR(row_ptr.cpu().numpy().astype(np.int64), plan.node_a[:E].cpu().numpy().astype(np.int64),
                 plan.rel[:E].cpu().numpy().astype(np.int64), np.ones(E, dtype=np.float32), n_node, n_node, n_rel)
    rng = np.random.default_rng(1024)
    x = rng.standard_normal((n_node, 64), dtype=np.float32)
    relation = rng.standard_normal((n_rel, 64), dtype=np.float32)
    if getattr(forward, "set_threads", None) is not None:
        forward.set_threads(cores)
    forward(host, relation, x, "add", "mul")
    times, t_start = [], time.perf_counter()
    while len(times) < 5 and time.perf_counter() - t_start < budget_s:
        t0 = time.perf_counter()
        forward(host, relation, x, "add", "mul")
        times.append(time.perf_counter() - t0)
    med = float(np.median(times))
    return {"value": E / med, "unit": "edges aggregated/s", "cores": cores, "kind": "port", "seconds_per_call": med,
            "algorithmic_GBps": bytes_algo(E, n_node, n_rel, 64) / med / 1e9, "host_available_GB": avail,
            "sample": "%d x one rspmm forward (add,mul) on S-stress, E=%d, F=64 (B=1), %d OpenMP threads; oracle/rspmm_oracle.c"
                      % (len(times), E, cores)}


def box_calibration(dev, lib, table, index):
    """What this box's memory system delivers, measured in the same run on the S-stress operands: a
    device-to-device copy of the gathered matrix (read + write bytes / time) and the BARE gather of its rows in the plan's
    own source order (ultra_calibrate_gather_f32: 256-byte rows, four per wave-instruction, eight instructions in flight, no
    relation operand, no row structure, no output rows) -- the ceiling of the rowgroup kernel's dominant stream."""
    n_rows = table.shape[0]
    other = torch.empty_like(table)
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    other.copy_(table)
    torch.cuda.synchronize()
    reps = 5
    start.record()
    for _ in range(reps):
        other.copy_(table)
    stop.record()
    torch.cuda.synchronize()
    copy_ms = start.elapsed_time(stop) / reps
    del other
    n_waves = ctypes.c_int64(0)
    index = index.contiguous()
    stream = torch.cuda.current_stream().cuda_stream
    assert lib.ultra_calibrate_gather_f32(table.data_ptr(), n_rows, index.data_ptr(), index.numel(), None, ctypes.byref(n_waves), stream) == 0
    out = torch.empty(int(n_waves.value) * 64, dtype=torch.float32, device=dev)
    call = lambda: lib.ultra_calibrate_gather_f32(table.data_ptr(), n_rows, index.data_ptr(), index.numel(), out.data_ptr(),
                                                  ctypes.byref(n_waves), stream)
    assert call() == 0
    torch.cuda.synchronize()
    start.record()
    for _ in range(reps):
        call()
    stop.record()
    torch.cuda.synchronize()
    gather_ms = start.elapsed_time(stop) / reps
    rows = int(n_waves.value) * 2048
    return {"copy_GBps": 2 * table.numel() * 4 / (copy_ms * 1e-3) / 1e9, "gather_GBps": rows * 256 / (gather_ms * 1e-3) / 1e9,
            "note": "same run, same operands: D2D copy of the %.2f GB gathered matrix %.3f ms (read + write bytes); bare gather of "
                    "%d random 256-B rows in the plan's source order %.3f ms (torch events over %d launches each)"
                    % (table.numel() * 4 / 1e9, copy_ms, rows, gather_ms, reps)}


# ------------------------------------------------------------------------------------------------ tasks of a shape
def transductive_task(workload, dev, n_test, seed):
    """Fact graph of exactly the shape's triples + ``n_test`` held-out DISTINCT triples of the same distribution (never
    edges of the message-passing graph, but part of ``graph``, which the ranking is filtered against: the transductive
    protocol, task.py:31-63); seeded random-init weights."""
    from ultra_torchdrug_amd.data import SHAPES, synthetic_triples
    from ultra_torchdrug_amd.graph import Graph
    from ultra_torchdrug_amd.task import build_ultra
    n_node, n_fact, n_rel = SHAPES[workload]
    triples, _, _ = synthetic_triples((n_node, n_fact + n_test, n_rel), seed, alpha=0.0 if workload == "S-stress" else 1.0)
    fact_mask = np.zeros(len(triples), dtype=bool)
    fact_mask[:n_fact] = True
    torch.manual_seed(seed)
    task = build_ultra(n_rel)
    task.preprocess(Graph(torch.from_numpy(triples), num_node=n_node, num_relation=n_rel), torch.from_numpy(fact_mask))
    task.to(dev).eval()
    return task, triples, fact_mask, n_fact


def prepare_plans(task):
    """Everything that is built once per graph, before any timed region."""
    und = task.model._undirected(task.fact_graph)
    for g in (und, task.rel_graphs[0]):
        _ = g.relcsr.fwd
        _ = g.relcsr.frontier_index
    for g in (task.graph, task.fact_graph):
        g.completion_keys(0), g.completion_keys(1)
    return und


def make_optimizer(task):
    """AdamW 5e-4 (the reference's fine-tuning / pre-training optimizer, config/transductive/pretrain_3g.yaml:41-43) in torch's
    single-launch form: the default multi-tensor form is 12 launches per step behind the replayed graph."""
    return torch.optim.AdamW(task.parameters(), lr=5e-4, fused=os.environ.get("ULTRA_BENCH_FUSED_ADAMW", "1") != "0")


def finetune_samples(task, facts, B, n_steps, seed, reducer=None):
    """Per-step wall times (ms, device-synchronised) of the fine-tuning step replayed as one hipGraph
    (engine.GraphedTrainStep): strict negatives, edge removal, forward, backward (+ the captured bucket all-reduces when a
    reducer is given), AdamW.  The batches are drawn before the clock starts."""
    from ultra_torchdrug_amd import engine
    task.train()
    opt = make_optimizer(task)
    pick = np.random.default_rng(seed)
    torch.manual_seed(seed)
    n_fact = len(facts)
    idx = torch.from_numpy(pick.choice(n_fact, B, replace=False)).to(facts.device)
    step = engine.GraphedTrainStep(task, opt, facts[idx], reducer=reducer)
    batches = [facts[torch.from_numpy(pick.choice(n_fact, B, replace=False)).to(facts.device)] for _ in range(n_steps + 2)]
    out = []
    for i, batch in enumerate(batches):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        step(batch)
        torch.cuda.synchronize()
        if i >= 2:
            out.append(1e3 * (time.perf_counter() - t0))
    in_graph = step.reduce_in_graph
    del step
    task.eval()
    return out, in_graph


def config_timings(dev, lib, seed, B, quick):
    """One timing per BASELINE.json config, measured in this run (rank 0, one GPU): the rows that were builder-run only."""
    import ultra_torchdrug_amd as U
    from ultra_torchdrug_amd import engine, functional as UF
    from ultra_torchdrug_amd.data import synthetic_kg, synthetic_triples
    from ultra_torchdrug_amd.engine import GraphedPredict
    from ultra_torchdrug_amd.graph import Graph
    from ultra_torchdrug_amd.task import build_ultra
    out = []
    events = HipEvents(lib)

    # ---- config 1: FB15k237Inductive-v1-shaped zero-shot inference on the CPU kernels (--gpus null)
    r = FB_V1["n_rel"]
    n_inf, t_fact, t_valid, t_test = FB_V1["inference"]
    train, _, _ = synthetic_triples((FB_V1["train"][0], FB_V1["train"][1], r), seed)
    inf, _, _ = synthetic_triples((n_inf, t_fact + t_valid + t_test, r), seed + 1)
    torch.manual_seed(seed)
    cpu_task = build_ultra(r)
    g_train = Graph(torch.from_numpy(train), num_node=FB_V1["train"][0], num_relation=r)
    cpu_task.preprocess_inductive(g_train, g_train, Graph(torch.from_numpy(inf[:t_fact]), num_node=n_inf, num_relation=r),
                                  graph=g_train, inductive_graph=Graph(torch.from_numpy(inf), num_node=n_inf, num_relation=r))
    cpu_task.eval().use("test")
    test = torch.from_numpy(inf[t_fact + t_valid:])
    torch.set_num_threads(host_cores())
    with torch.no_grad():
        cpu_task.rank_batch(test[:B])
        t0 = time.perf_counter()
        n_b = 0
        for i in range(0, len(test) - B + 1, B):
            cpu_task.rank_batch(test[i:i + B])
            n_b += 1
        cpu_ms = 1e3 * (time.perf_counter() - t0) / max(n_b, 1)
    e_inf = 2 * t_fact
    out.append({"config": 1, "name": "FB15k237Inductive v1-shaped zero-shot inference on CPU (--gpus null)",
                "shape": "inference graph N=%d, %d fact triples (E=%d), R=%d; %d test triples, B=%d" % (n_inf, t_fact, e_inf, 2 * r, t_test, B),
                "device": "cpu, %d torch threads; rspmm = CPU kernels of torch.ops.ultra_mi (csrc/torch_ext.cpp)" % torch.get_num_threads(),
                "predict_plus_rank_ms_per_batch": cpu_ms,
                "entity_edges_per_s": 12 * e_inf * B / (cpu_ms * 1e-3)})
    del cpu_task

    # ---- config 2: CoDExSmall-shaped transductive zero-shot inference, B = 16
    task, triples, _, n_fact = transductive_task("S-codexs", dev, 512, seed)
    und = prepare_plans(task)
    test = torch.from_numpy(triples[n_fact:]).to(dev)
    E, R2, N = und.relcsr.n_edges, und.num_relation, und.num_node
    with torch.no_grad():
        task.predict(test[:B])
        replay = GraphedPredict(task, test[:B], warmup=0)
        n_b = len(test) // B
        step_ms = wall_ms(lambda i: replay(test[(i % n_b) * B:(i % n_b) * B + B]), 20 if quick else 100, warm=5)
        gen = torch.Generator(device=dev).manual_seed(seed)
        xk, rk = torch.randn(N, 2 * B * 64, device=dev, generator=gen), torch.randn(R2, 2 * B * 64, device=dev, generator=gen)
        for _ in range(3):
            UF.rspmm_forward(und.relcsr, rk, xk, "add", "mul")
        k_ms, _ = timed_kernel(lib, events, lambda: UF.rspmm_forward(und.relcsr, rk, xk, "add", "mul"), 20)
        # the same operator at ONE side's width (F = B * 64: what the reference launches per side, and the shape round 2's
        # 39.3 us was measured at)
        xh, rh = xk[:, :B * 64].contiguous(), rk[:, :B * 64].contiguous()
        for _ in range(3):
            UF.rspmm_forward(und.relcsr, rh, xh, "add", "mul")
        k1_ms, _ = timed_kernel(lib, events, lambda: UF.rspmm_forward(und.relcsr, rh, xh, "add", "mul"), 20)
    algo = bytes_algo(E, N, R2, 2 * B * 64)
    out.append({"config": 2, "name": "CoDExSmall-shaped transductive zero-shot inference (rspmm fwd only)",
                "shape": "S-codexs N=%d E=%d R=%d B=%d" % (N, E, R2, B),
                "predict_ms_per_batch": step_ms, "entity_edges_visited_per_s": 10 * E * B / (step_ms * 1e-3),
                "entity_fwd_kernel_us": 1e3 * k_ms, "entity_fwd_kernel_us_one_side_width": 1e3 * k1_ms,
                "entity_fwd_kernel_algorithmic_GBps": algo / (k_ms * 1e-3) / 1e9,
                "entity_fwd_kernel_frac_of_l2_peak": algo / (k_ms * 1e-3) / 1e9 / L2_PEAK_GBS})
    del task, replay, xk, rk
    torch.cuda.empty_cache()

    # ---- config 3: WN18RR-shaped fine-tuning, fp32, B = 16 (rspmm fwd + bwd through autograd, DistMult messages)
    task, triples, _, n_fact = transductive_task("S-wn18rr", dev, 512, seed)
    und = prepare_plans(task)
    E, R2, N = und.relcsr.n_edges, und.num_relation, und.num_node
    F = B * 64
    gen = torch.Generator(device=dev).manual_seed(seed)
    xk, rk, gk = (torch.randn(N, F, device=dev, generator=gen), torch.randn(R2, F, device=dev, generator=gen),
                  torch.randn(N, F, device=dev, generator=gen))
    for _ in range(3):
        UF.rspmm_forward(und.relcsr, rk, xk, "add", "mul")
        UF.rspmm_backward(und.relcsr, rk, xk, None, gk, "add", "mul")
    fwd_ms, _ = timed_kernel(lib, events, lambda: UF.rspmm_forward(und.relcsr, rk, xk, "add", "mul"), 20)
    bwd_ms = wall_ms(lambda i: UF.rspmm_backward(und.relcsr, rk, xk, None, gk, "add", "mul"), 20, warm=3)
    del xk, rk, gk
    facts = torch.from_numpy(triples[:n_fact]).to(dev)
    samples, _ = finetune_samples(task, facts, B, 10 if quick else 30, seed)
    out.append({"config": 3, "name": "WN18RR-shaped fine-tuning fp32 (rspmm fwd+bwd autograd, DistMult message)",
                "shape": "S-wn18rr N=%d E=%d R=%d B=%d, 128 strict negatives, AdamW" % (N, E, R2, B),
                "operator_fwd_us": 1e3 * fwd_ms, "operator_bwd_us": 1e3 * bwd_ms,
                "operator_fwd_bwd_edges_per_s": 3 * E * B / ((fwd_ms + bwd_ms) * 1e-3),
                "finetune_step": spread(samples),
                "finetune_launch": "one hipGraph replay per step (engine.GraphedTrainStep) + AdamW"})
    del task, facts
    torch.cuda.empty_cache()

    # ---- config 4: pretrain_3g-shaped multi-graph step, B = 64 per GPU (ultra/engine.py:23-34, pretrain_3g.yaml:36-56)
    out.append(pretrain_timing(dev, seed, 0, 1, RankReduce(1, dev, False), quick))
    return out


def self_launch(args):
    """``--gpus N`` (N > 1) without a launcher: start the N ranks as children of a parent that has made NO GPU call
    (``torch.cuda.device_count()`` does not initialise the device on this image), relay their output and exit with their
    code.  The reference is started the same way (/root/reference/README.md:139-149: ``python -m torch.distributed.launch
    --nproc_per_node=N script/run_full.py ...``)."""
    import socket
    import subprocess
    n_dev = torch.cuda.device_count()
    share = os.environ.get("ULTRA_BENCH_SHARE_GPU") == "1"
    if n_dev < args.gpus and not share:
        print("bench.py --gpus %d: only %d MI355X visible on this node; refusing to print a %d-GPU line from fewer devices"
              % (args.gpus, n_dev, args.gpus), file=sys.stderr)
        return 2
    with socket.socket() as sock:
        sock.bind(("127.0.0.1", 0))
        port = sock.getsockname()[1]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(args.gpus),
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    proc = subprocess.Popen(cmd, stdout=subprocess.PIPE, text=True, env=env)
    lines = 0
    for line in proc.stdout:                         # rank 0's JSON line (and anything else the ranks print) goes through
        sys.stdout.write(line)
        sys.stdout.flush()
        lines += line.lstrip().startswith("{")
    rc = proc.wait()
    if rc == 0 and lines == 0:
        print("bench.py --gpus %d: the ranks exited cleanly without a result line" % args.gpus, file=sys.stderr)
        return 3
    return rc


def flat_config_keys(configs):
    """The per-config timings once more as SCALAR keys of ``config`` (the driver's record keeps scalars of ``config`` and drops
    the nested ``configs`` list: round 3's configs 1-4 survived only in its stdout tail)."""
    by = {c["config"]: c for c in configs}
    flat = {}

    def put(key, cfg, *path):
        node = by.get(cfg)
        for name in path:
            node = node.get(name) if isinstance(node, dict) else None
        if node is not None:
            flat[key] = node

    put("cfg1_cpu_ms_per_batch", 1, "predict_plus_rank_ms_per_batch")
    put("cfg2_predict_ms", 2, "predict_ms_per_batch")
    put("cfg2_fwd_us", 2, "entity_fwd_kernel_us")
    put("cfg2_fwd_us_one_side_width", 2, "entity_fwd_kernel_us_one_side_width")
    put("cfg3_fwd_us", 3, "operator_fwd_us")
    put("cfg3_bwd_us", 3, "operator_bwd_us")
    put("cfg3_step_median_ms", 3, "finetune_step", "median_ms")
    put("cfg4_n_gpus", 4, "n_gpus")
    put("cfg4_step_median_ms", 4, "step", "median_ms")
    put("cfg4_step_ms_max_over_ranks", 4, "step_ms_max_over_ranks")
    put("cfg4_edge_messages_per_s_nominal", 4, "entity_edge_messages_per_s_nominal")
    put("cfg4_allreduce_exposed_ms_per_step", 4, "allreduce_exposed_ms_per_step")
    put("cfg4_collective_backend", 4, "collective_backend")
    put("cfg4_step_mode", 4, "step_mode")
    put("cfg4_step_modes_agree", 4, "step_modes_agree")
    put("cfg4_step_ms_16_cus_reserved", 4, "step_ms_max_over_ranks_16_cus_reserved")
    put("cfg4_allreduce_exposed_ms_16_cus_reserved", 4, "allreduce_exposed_ms_per_step_16_cus_reserved")
    put("cfg4_eager_step_ms", 4, "eager_step_ms")
    put("cfg5_frac", 5, "frac_of_hbm_peak")
    put("cfg5_fwd_ms", 5, "operator_fwd_ms")
    put("cfg5_predict_ms", 5, "predict_ms")
    put("cfg5_predict_ms_b4", 5, "predict_ms_b4")
    put("cfg5_whole_layer_frac", 5, "frac_of_hbm_peak_whole_layer")
    put("cfg5_b4_frac", 5, "operator_b4_frac")
    put("cfg5_n_gpus", 5, "all_ranks", "n_gpus")
    put("cfg5_triples_per_s_all_ranks", 5, "all_ranks", "triples_per_s_all_ranks")
    put("cfg5_ms_per_triple_max_over_ranks", 5, "all_ranks", "predict_plus_rank_ms_per_triple_max_over_ranks")
    return flat


class RankReduce:
    """max / sum / gather of a few host floats over the ranks (device tensors under RCCL, host tensors under the
    development switch's gloo group)."""

    def __init__(self, world, dev, share):
        self.world, self.dev = world, ("cpu" if share else dev)

    def _t(self, values):
        return torch.tensor([float(v) for v in values], dtype=torch.float64, device=self.dev)

    def max(self, values):
        t = self._t(values)
        if self.world > 1:
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
        return [float(v) for v in t.tolist()]

    def sum(self, values):
        t = self._t(values)
        if self.world > 1:
            dist.all_reduce(t, op=dist.ReduceOp.SUM)
        return [float(v) for v in t.tolist()]

    def gather(self, value):
        t = self._t([value])
        parts = [t.clone() for _ in range(self.world)]
        if self.world > 1:
            dist.all_gather(parts, t)
        return [float(x.item()) for x in parts]

    def barrier(self):
        torch.cuda.synchronize()
        if self.world > 1:
            dist.barrier()
        torch.cuda.synchronize()


def stress_inference_ranks(dev, rank, world, ranks, shape):
    """BASELINE config 5 "on 1 and 8 MI355X": the path shards over QUERIES only -- every rank holds the whole graph
    (100 M edges: 3.6 GB of plans) and answers its own triples; no collective in the data path.  EVERY rank calls this at the
    same point: the same S-stress graph (same seed), three triples per rank drawn with seed + rank, `predict` + filtered rank
    one triple at a time; time = max-over-ranks wall time between two barriers."""
    from ultra_torchdrug_amd.data import stress_task
    n_node, n_triple, n_rel = shape
    task, _ = stress_task(dev, n_node, n_triple, n_rel)
    und = task.model._undirected(task.fact_graph)
    E = und.relcsr.n_edges
    _ = und.relcsr.fwd, und.relcsr.frontier_index
    gen = torch.Generator(device=dev).manual_seed(2000 + rank)
    batches = [torch.stack([torch.randint(0, n_node, (1,), device=dev, generator=gen), torch.randint(0, n_node, (1,), device=dev, generator=gen),
                            torch.randint(0, n_rel, (1,), device=dev, generator=gen)], dim=1) for _ in range(4)]
    with torch.no_grad():
        task.rank_batch(batches[0], task.predict(batches[0]))                    # warm-up: plans, allocator, kernels' attributes
        ranks.barrier()
        t0 = time.perf_counter()
        for b in batches[1:]:
            task.rank_batch(b, task.predict(b))
        torch.cuda.synchronize()
        mine = time.perf_counter() - t0
        ranks.barrier()
    total = ranks.max([mine])[0]
    n = len(batches) - 1
    out = {"n_gpus": world, "triples_per_rank": n, "shape": "N=%d E=%d R=%d" % (n_node, E, 2 * n_rel),
           "predict_plus_rank_ms_per_triple_max_over_ranks": 1e3 * total / n,
           "per_rank_ms_per_triple": [1e3 * v / n for v in ranks.gather(mine)],
           "triples_per_s_all_ranks": n * world / total,
           "entity_edge_messages_per_s_all_ranks": 5.0 * E * 2 * n * world / total,
           "scaling": "weak: every rank answers its own queries on its own replica of the graph; no collective in the data path"}
    del task
    torch.cuda.empty_cache()
    return out


def pretrain_timing(dev, seed, rank, world, ranks, quick):
    """BASELINE config 4: the pretrain_3g-shaped multi-graph step (FB15k237 + WN18RR + CoDEx-M shapes under one set of
    weights, B = 64 per rank, 128 strict negatives, AdamW; pretrain_3g.yaml:36-56), one hipGraph replay per step
    (engine.GraphedMultiGraphTrainStep, every graph captured in the constructor).  EVERY rank calls this at the same point.
    World 1: per-step spread + the eager step.  World N: every rank draws its own graphs (seed + rank, engine.py:23-34 /
    run_full.py:102-107) and the gradients go through engine.GradientReducer over RCCL (bucket all-reduces on a side stream
    after each replay + the packed metric reduce); step time = max-over-ranks wall time of K un-synchronised steps between
    two barriers.  What the collectives cost is measured on a sequence in which ALL ranks draw the SAME graphs (no straggler
    wait inside the difference): the same K steps with and without any cross-rank traffic."""
    from ultra_torchdrug_amd import engine
    from ultra_torchdrug_amd.data import synthetic_kg
    from ultra_torchdrug_amd.task import build_ultra
    B = 64
    torch.manual_seed(seed)                          # the same weights on every rank
    task = build_ultra(237)
    for i, name in enumerate(PRETRAIN_3G):
        task.add_context(str(i), synthetic_kg(name))
    task.to(dev).train()
    opt = make_optimizer(task)
    reducer = engine.GradientReducer(task, overlap=True) if world > 1 else None
    graphed = engine.GraphedMultiGraphTrainStep(task, opt, B, reducer=reducer)
    edges = {name: 2 * ctx["fact_graph"].num_edge for name, ctx in task.contexts.items()}      # with inverse edges
    n_steps = 9 if quick else 18

    def draw(gen, n):
        out = []
        for _ in range(n):
            batch, gid = engine.sample_edges_from_graph(task, B, gen)
            out.append((batch.to(dev), gid))
        return out

    def loop(batches, communicate, per_step=False):
        """Wall time of the steps between two barriers: (max over ranks, this rank's own, per-step times if synchronised)."""
        graphed.communicate = communicate
        ranks.barrier()
        t0 = time.perf_counter()
        each = []
        for batch in batches:
            t1 = time.perf_counter()
            graphed(batch)
            if per_step:
                torch.cuda.synchronize()
                each.append(1e3 * (time.perf_counter() - t1))
        torch.cuda.synchronize()
        mine = time.perf_counter() - t0
        ranks.barrier()
        graphed.communicate = True
        return ranks.max([mine])[0], mine, each

    own = torch.Generator().manual_seed(seed + rank)
    loop(draw(own, 3), True)                                         # every graph's replay once more before the clock
    batches = draw(own, n_steps)
    _, _, per_step = loop(batches, True, per_step=True)
    total, mine, _ = loop(batches, True)
    drawn = "".join(g for _, g in batches)
    messages = ranks.sum([sum(18 * edges[g] * B for _, g in batches)])[0]      # nominal: 6 layers x (fwd + d_input + d_relation)
    out = {"config": 4, "name": "pretrain_3g-shaped multi-graph step (FB15k237 + WN18RR + CoDEx-M shapes, one set of weights)",
           "shape": "B=64 per GPU, 128 strict negatives, AdamW 5e-4; graph drawn per step and rank with p ~ #fact edges",
           "n_gpus": world, "steps": n_steps,
           "step": spread(per_step), "graphs_drawn_rank0": drawn,
           "step_ms_max_over_ranks": 1e3 * total / n_steps,
           "per_rank_step_ms": [1e3 * v / n_steps for v in ranks.gather(mine)],
           "entity_edge_messages_per_s_nominal": messages / total,
           "edge_message_count": "nominal: 6 layers x (forward + d_input + d_relation) x E(graph drawn) x B, all ranks",
           "launch": "one hipGraph replay per step, one captured step per graph (engine.GraphedMultiGraphTrainStep; all graphs "
                     "captured in the constructor, reducer paused) + AdamW"}
    if world > 1:
        shared = torch.Generator().manual_seed(seed)                 # the same draws on every rank
        same = draw(shared, n_steps)
        loop(same[:3], True)
        with_comm, mine_with, _ = loop(same, True)
        without, mine_without, _ = loop(same, False)                 # LAST: the ranks' weights drift apart from here on
        modes = graphed.modes
        mode = "/".join(sorted(set(modes.values())))
        # every rank and context should be in the same mode (a capture whose phased backward does not verify drops to
        # "after" with a warning, possibly on one rank only: the collectives still match, the overlap is lost there)
        code = float(sum({"phased": 0, "after": 1, "in_graph": 2, "single": 3}.get(m, 4) * 10 ** i for i, m in enumerate(modes[k] for k in sorted(modes))))
        agree = ranks.max([code])[0] == -ranks.max([-code])[0] and len(set(modes.values())) == 1
        names = ("phased", "after", "in_graph", "single", "?")
        per_rank_modes = ["/".join(names[int(c) // 10 ** i % 10] for i in range(len(modes))) for c in ranks.gather(code)]
        per_rank_exposed = [1e3 * v / n_steps for v in ranks.gather(mine_with - mine_without)]
        out.update({"step_modes": modes, "step_modes_agree": bool(agree), "collective_backend": dist.get_backend(),
                    "gradient_allreduce": "engine.GradientReducer: %d buckets in %d groups (one all-reduce per group), %d fp32 "
                                          "parameters, %s, side stream; step mode `%s` (phased: 3 captured phases, each phase's group "
                                          "all-reduced while the next phase replays; after: one graph, the groups after the replay); "
                                          "+ 1 packed metric all-reduce"
                                          % (len(reducer.buckets), len(reducer.groups), sum(b["numel"] for b in reducer.buckets),
                                             dist.get_backend(), mode),
                    "step_mode": mode,
                    "same_graphs_step_ms_with_allreduce": 1e3 * with_comm / n_steps,
                    "same_graphs_step_ms_without_allreduce": 1e3 * without / n_steps,
                    "allreduce_exposed_ms_per_step": 1e3 * (with_comm - without) / n_steps,
                    "allreduce_exposed_is": "max-over-ranks wall time of the same K steps with the collectives minus without them "
                                            "(all ranks on the same graphs: no straggler wait inside the difference)",
                    "allreduce_exposed_ms_per_step_per_rank": per_rank_exposed,
                    "step_modes_per_rank": per_rank_modes,
                    "step_modes_per_rank_order": "contexts %s" % ",".join(sorted(modes))})
        reducer.remove_hooks()
    else:
        eager = []
        for s, batch in enumerate(draw(own, 4)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            engine.train_step(task, opt, batch)
            torch.cuda.synchronize()
            if s >= 1:
                eager.append(1e3 * (time.perf_counter() - t0))
        out["eager_step_ms"] = float(np.median(eager))
        out["note"] = "1 GPU: run `bench.py --gpus N` for the N-rank form of this config (RCCL gradient all-reduce)"
    del graphed, task, opt
    torch.cuda.empty_cache()
    return out


def real_data_metrics(data_dir, ckpt, dev, B):
    """``--data DIR [--ckpt PATH]``: a real transductive split (train / valid / test.txt of h<TAB>r<TAB>t lines,
    /root/reference/ultra/dataset.py:33-96) and, when given, a reference checkpoint (td_ultra_3g / 4g.pth layout,
    /root/reference/ultra/util.py:233-276) through engine.evaluate on the test split: MR / MRR / Hits@k as the reference
    reports them (ultra/task.py:317-351).  Nothing of this exists on the build machines (no network, the checkpoints in the
    reference tree are missing blobs); the switch is the hook that produces the numbers the moment the files do."""
    from ultra_torchdrug_amd import engine
    from ultra_torchdrug_amd.data import task_from_split_dir
    task, splits = task_from_split_dir(data_dir, checkpoint=ckpt, device=dev)
    test = splits["test"].to(dev)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    metric, ranking = engine.evaluate(task, test, batch_size=B)
    torch.cuda.synchronize()
    seconds = time.perf_counter() - t0
    missing, unexpected = task.checkpoint_keys
    und = task.model._undirected(task.fact_graph)
    return {"data": os.path.abspath(data_dir), "checkpoint": os.path.abspath(ckpt) if ckpt else "seeded random init",
            "checkpoint_missing_keys": missing, "checkpoint_unexpected_keys": unexpected,
            "entities": task.num_entity, "relations": task.num_relation, "edges_with_inverses": und.relcsr.n_edges,
            "test_triples": int(len(test)), "evaluate_seconds": seconds,
            # two queries per test triple, layers 2-6 over all E edges each (the first layer's frontier edges not counted)
            "entity_edge_messages_per_s": 2 * 5 * und.relcsr.n_edges * len(test) / seconds if seconds > 0 else None,
            "metrics": {k: float(v) for k, v in metric.items()}}


class Phases:
    """World > 1 only (the first real N-GPU run must not hang silently): every rank names the phase it
    enters on stderr, and a phase that overruns its limit makes the rank EXIT non-zero (a plain exit from a timer thread --
    never a re-exec of a process that has touched the GPU), so the launcher tears the job down and the driver sees which
    phase and which rank stopped."""

    def __init__(self, rank, world, limit_s=600.0):
        self.rank, self.on, self.limit, self.timer, self.t0 = rank, world > 1, limit_s, None, time.perf_counter()
        self.fallback = None

    def enter(self, name, limit_s=None):
        if not self.on:
            return
        import threading
        self.done()
        limit = float(limit_s or self.limit)
        print("[bench rank %d +%.1fs] %s (limit %.0f s)" % (self.rank, time.perf_counter() - self.t0, name, limit), file=sys.stderr, flush=True)
        self.timer = threading.Timer(limit, self._expire, args=(name, limit))
        self.timer.daemon = True
        self.timer.start()

    def _expire(self, name, limit):
        print("[bench rank %d] phase `%s` exceeded %.0f s: exiting with code 3" % (self.rank, name, limit), file=sys.stderr, flush=True)
        if self.rank == 0 and self.fallback is not None:
            # the timed region is over and reduced: the headline goes out even when a LATER leg (config 4 over RCCL, config 5 on
            # every rank: never run on N > 1 real GPUs) hangs -- marked as partial, exit code still 3
            line = dict(self.fallback)
            line["partial"] = "phase `%s` exceeded %.0f s; only the headline of the timed region is reported" % (name, limit)
            print(json.dumps(line), flush=True)
        os._exit(3)

    def done(self):
        if self.timer is not None:
            self.timer.cancel()
            self.timer = None


def distinct_devices(dev, world, share):
    """How many DIFFERENT GPUs the ranks of this job run on (all-gathered PCI ids): the driver's record must be able to tell an
    N-GPU RCCL run from N ranks on one device."""
    props = torch.cuda.get_device_properties(dev)
    ident = (int(getattr(props, "pci_domain_id", 0)) << 32) | (int(getattr(props, "pci_bus_id", 0)) << 16) | \
        int(getattr(props, "pci_device_id", dev.index or 0))
    mine = torch.tensor([ident], dtype=torch.int64, device="cpu" if share else dev)
    parts = [mine.clone() for _ in range(world)]
    if world > 1:
        dist.all_gather(parts, mine)
    return len({int(t.item()) for t in parts})


def dump_outputs(out_dir, arrays, cap_bytes=64_000_000):
    """``--dump-outputs DIR``: each array as ``DIR/<name>.npy`` in float32.  Arrays larger together than ``cap_bytes`` are
    cut to the same seeded sample of their flattened elements (sorted positions) in every run, so dumps stay comparable."""
    os.makedirs(out_dir, exist_ok=True)
    total = sum(4 * a.numel() for a in arrays.values())
    for name, a in arrays.items():
        a = a.detach().float()
        if total > cap_bytes:
            pos = np.unique(np.random.default_rng(0).integers(0, a.numel(), max(1, a.numel() * cap_bytes // total)))
            a = a.reshape(-1)[torch.from_numpy(pos).to(a.device)]
        np.save(os.path.join(out_dir, name + ".npy"), a.cpu().numpy())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--batch", type=int, default=16, help="queries per step (reference inference batch: 16)")
    ap.add_argument("--workload", default="S-fb15k237")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-stress", dest="stress", action="store_false",
                    help="skip config 5 at size (S-stress: 10 M nodes / 100 M edges, ~15 s); `roofline` is then the L2 line")
    ap.add_argument("--stress-shape", default=None, help="nodes,triples,relations of the config-5 graph (default: S-stress, "
                                                         "10000000,50000000,500); a development aid for the N-rank launch test")
    ap.add_argument("--no-configs", dest="configs", action="store_false", help="skip the per-config timings (config.configs)")
    ap.add_argument("--eager", action="store_true", help="issue every launch from Python instead of replaying a hipGraph")
    ap.add_argument("--mrr-queries", type=int, default=500,
                    help="seeded test triples ranked after the timed region (500 = the reference's fast_test, pretrain_3g.yaml:56)")
    ap.add_argument("--finetune-steps", type=int, default=50, help="seeded fine-tuning steps before the second MRR")
    ap.add_argument("--data", default=None, help="directory with train.txt / valid.txt / test.txt (h<TAB>r<TAB>t lines): also "
                                                 "evaluate the test split of this REAL dataset (result key `real_data`)")
    ap.add_argument("--ckpt", default=None, help="reference checkpoint (td_ultra_3g.pth / td_ultra_4g.pth layout) for --data")
    ap.add_argument("--full", action="store_true",
                    help="after the headline, every other measurement: per-kernel and composition timings, per-config timings, "
                         "S-stress roofline, MRR with the CPU-oracle check, fine-tuning, cpu_baseline (shaped by --no-stress, "
                         "--no-configs, --no-cpu-baseline, --stress-shape, --mrr-queries, --finetune-steps)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the scores the last timed step returned (rank 0) as DIR/scores.npy, float32 (B, 2, N)")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        raise SystemExit("bench.py: --steps must be >= 1 and --warmup >= 0")
    if args.gpus < 1:
        raise SystemExit("bench.py: --gpus must be >= 1 (the headline is the HIP path; config 1's CPU run is inside the N=1 line)")
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        raise SystemExit(self_launch(args))

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    # ULTRA_BENCH_SHARE_GPU=1 (development only): all ranks on the visible GPU(s), gloo instead of RCCL -- lets the
    # multi-rank code path (sharding, barriers, max-over-ranks timing) run on a one-GPU box
    share = os.environ.get("ULTRA_BENCH_SHARE_GPU") == "1"
    n_dev = torch.cuda.device_count()              # (does not initialise the GPU)
    if n_dev == 0:
        raise SystemExit("bench.py needs an MI355X: the headline is the HIP path")
    if world != args.gpus:                           # never a line whose n_gpus is not what was asked for
        raise SystemExit("bench.py: --gpus %d but WORLD_SIZE=%d" % (args.gpus, world))
    if world > 1 and not share and local_rank >= n_dev:
        raise SystemExit("bench.py: rank %d has no device (%d visible)" % (local_rank, n_dev))
    if share:
        local_rank %= n_dev
    phases = Phases(rank, world)
    phases.enter("init_process_group (%s)" % ("gloo, shared GPU" if share else "nccl = RCCL"), 300)
    # the process group comes first: RCCL is initialised before this process makes any other GPU call
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        torch.cuda.set_device(local_rank)
        if share:
            dist.init_process_group("gloo")
        else:
            dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank))
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)

    import ultra_torchdrug_amd as U
    from ultra_torchdrug_amd import layer as UL
    from ultra_torchdrug_amd.data import DEFAULT_SEED
    from ultra_torchdrug_amd.graph import Graph
    from ultra_torchdrug_amd.task import build_ultra
    lib = U.require_library()
    torch.backends.cuda.matmul.allow_tf32 = False          # script/run_full.py:19-20
    torch.backends.cudnn.allow_tf32 = False

    # ---------------- graph, split, model (identical on every rank) ----------------
    phases.enter("graph, plans, model")
    from ultra_torchdrug_amd.data import SHAPES
    n_node, n_fact_shape, n_rel = SHAPES[args.workload]
    n_test = min(2048, n_fact_shape // 20)
    task, triples, fact_mask, n_fact = transductive_task(args.workload, dev, n_test, DEFAULT_SEED)
    test_idx = np.arange(n_fact, n_fact + n_test)
    und = task.model._undirected(task.fact_graph)
    _ = und.relcsr.fwd                  # coalesce + sort + chunk schedule: once per graph (torchdrug: every rspmm call)
    if args.full:
        torch.cuda.synchronize()
        t_plan = time.perf_counter()        # steady-state cost of that build (the first one above also warms rocPRIM up)
        _ = U.RelCSR.from_edge_list(und.edge_list, und.edge_weight, und.num_node, und.num_relation).fwd
        torch.cuda.synchronize()
        plan_build_ms = 1e3 * (time.perf_counter() - t_plan)
    prepare_plans(task)
    E, R2 = und.relcsr.n_edges, und.num_relation
    E_rel = task.rel_graphs[0].relcsr.n_edges
    B = args.batch
    F = B * 64
    # predict() scores tails and heads in ONE Bellman-Ford over 2B queries (task.fuse_sides): 6 entity launches of
    # width 2F per step instead of 12 of width F -- the same edge messages
    Fk = 2 * F
    full_layers_edges = 10 * E * B                       # layers 2..6: every edge, 2B queries
    rel_edges_per_step = 6 * E_rel * B                   # round 2's count for the relation-graph stack (all six layers)

    # each rank evaluates its own strided shard of the seeded test triples (DistributedSampler-style)
    test = torch.from_numpy(triples[test_idx]).to(dev)
    shard = test[rank::world]
    n_batches = max(len(shard) // B, 1)
    # layer 1 visits the out-edges of the boundary nodes only: counted exactly, per batch of the shard
    deg_out = torch.bincount(und.relcsr.src, minlength=n_node)

    def frontier_edges(batch):
        h, t = batch[:, 0], batch[:, 1]
        return int(deg_out[h].sum() + deg_out[t].sum())        # tail queries start at h, head queries (tail form) at t

    frontier_per_batch = [frontier_edges(shard[b * B:b * B + B]) for b in range(n_batches)]

    # profile hook: HIP events around the entity-graph forward kernel (the dominant kernel), recorded by the library
    # on the kernel's own stream.  --eager: one pair per launch of the timed region.  Default (hipGraph replay): event
    # records cannot be captured with the HIP runtime PyTorch bundles, so the same kernel is launched eagerly, with the
    # step's own shapes and fused boundary epilogue, right after the timed region and timed there.
    events = HipEvents(lib)
    from ultra_torchdrug_amd import functional as UF
    real_forward = UF.rspmm_forward
    state = {"on": False}

    def timed_forward(csr, relation, input, sum="add", mul="mul", add_rows=None, boundary=None):
        if state["on"] and csr is und.relcsr:
            a, b = events.new_pair()
            lib.ultra_rspmm_profile_next(a, b)
        return real_forward(csr, relation, input, sum, mul, add_rows, boundary)

    if args.full:
        UF.rspmm_forward = timed_forward

    # the evaluation batch is replayed as one hipGraph (engine.GraphedPredict); --eager times the un-captured path
    from ultra_torchdrug_amd.engine import GraphedPredict

    def capture():
        with torch.no_grad():
            task.predict(shard[:B])                 # plans, kernel attributes, allocator: before the capture
        try:
            return GraphedPredict(task, shard[:B], warmup=0)
        except Exception as err:                    # capture refused (driver / runtime): time the eager path
            print("bench: hipGraph capture failed (%s); falling back to eager launches" % err, file=sys.stderr)
            torch.cuda.synchronize()
            return None

    phases.enter("capture of the evaluation step")
    graphed = None if args.eager else capture()

    def step(i, g=None):
        g = graphed if g is None else g
        batch = shard[(i % n_batches) * B:(i % n_batches) * B + B]
        return task.predict(batch) if g is None else g(batch)

    def replays_equal_eager(g, n=3):
        """Replays of the captured step on batches OTHER than the captured one give the scores of eager launches (a
        graph node replayed out of order shows here, not on the captured batch)."""
        if g is None:
            return None
        same = True
        for i in range(1, n + 1):
            batch = shard[(i % n_batches) * B:(i % n_batches) * B + B]
            got = g(batch).clone()
            same = same and bool(torch.equal(got, task.predict(batch)))
        return same

    phases.enter("warm-up, barrier, timed region")
    with torch.no_grad():
        for i in range(args.warmup):
            step(i)
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()
        state["on"] = graphed is None
        # the K steps are ONE timed region (contract); stream events at block boundaries (no host synchronisation, recorded
        # on the stream the replays run on) give the spread of the headline inside it: median / min / max over ~10 blocks
        n_blocks = max(1, min(10, args.steps))
        edges_at = [round(b * args.steps / n_blocks) for b in range(n_blocks + 1)]
        marks = [torch.cuda.Event(enable_timing=True) for _ in edges_at]
        t0 = time.perf_counter()
        marks[0].record()
        nxt = 1
        for i in range(args.steps):
            last = step(args.warmup + i)
            if i + 1 == edges_at[nxt]:
                marks[nxt].record()
                nxt += 1
        torch.cuda.synchronize()
        my_elapsed = time.perf_counter() - t0
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()
        elapsed = time.perf_counter() - t0
        state["on"] = False
        frontier_visited = sum(frontier_per_batch[(args.warmup + i) % n_batches] for i in range(args.steps))

        if args.dump_outputs and rank == 0:        # what a caller of the timed path received from its last step
            dump_outputs(args.dump_outputs, {"scores": last})

        if args.full:
            # ---- after the timed region: the dominant kernel alone, and the other per-step numbers
            phases.enter("per-kernel timings after the timed region")
            gen = torch.Generator(device=dev).manual_seed(DEFAULT_SEED)
            xk = torch.randn(n_node, Fk, device=dev, generator=gen)
            rk = torch.randn(R2, Fk, device=dev, generator=gen)
            # the layer's sparse boundary: the heads and tails of a REAL batch (Zipf hubs: a uniformly drawn boundary would
            # flatter the first-layer frontier kernel by an order of magnitude)
            bk = (torch.cat([shard[:B, 0], shard[:B, 1]])[:Fk // 64].to(torch.int32).contiguous(),
                  torch.randn(Fk // 64, 64, device=dev, generator=gen))
            if graphed is not None:
                for _ in range(4):
                    real_forward(und.relcsr, rk, xk, "add", "mul", None, bk)
                state["on"] = True
                for _ in range(48):
                    timed_forward(und.relcsr, rk, xk, "add", "mul", None, bk)
                state["on"] = False
                torch.cuda.synchronize()
            kernel_ms = events.elapsed_ms()
            n_side = min(args.steps, 50)
            eager_ms = wall_ms(lambda i: task.predict(shard[:B]), 5) if graphed is not None else 1e3 * elapsed / args.steps
            # predict + filtered ranking (what engine.evaluate does per batch): the ranks come from the sorted completion keys
            # on the device, nothing but (B, 2) int64 leaves it
            rank_ms = wall_ms(lambda i: task.rank_batch(shard[:B], pred=step(i)), n_side)
            # the same step without the first-layer frontier shortcut (every layer walks all E edges)
            UL.FRONTIER_FIRST_LAYER = False
            try:
                plain = None if args.eager else capture()
                no_frontier_ms = wall_ms(lambda i: step(i, plain), n_side, warm=5)
            finally:
                UL.FRONTIER_FIRST_LAYER = True
            frontier_ms, _ = timed_kernel(lib, events, lambda: UF.rspmm_frontier(und.relcsr, rk, bk), 10)
            # the same step with the first layer's epilogue over ALL rows (round 3's form; round 4 runs it on the rows the frontier
            # reaches and broadcasts one constant row everywhere else: ultra_first_layer_sparse_f32)
            UF.SPARSE_FIRST_LAYER = False
            try:
                dense_first = None if args.eager else capture()
                dense_first_ms = wall_ms(lambda i: step(i, dense_first), n_side, warm=5)
            finally:
                UF.SPARSE_FIRST_LAYER = True
            # the same step with the relation representations of all R relations computed once per evaluation run
            # (task.cache_relation_representations, what engine.evaluate does): identical scores, the relation stack leaves
            # the per-batch path.
            torch.cuda.synchronize()
            t_c = time.perf_counter()
            task.cache_relation_representations(B)
            torch.cuda.synchronize()
            cache_build_ms = 1e3 * (time.perf_counter() - t_c)
            try:
                cached = None if args.eager else capture()
                cached_ms = wall_ms(lambda i: step(i, cached), n_side, warm=5)
                replay_same_cached = replays_equal_eager(cached)
            finally:
                task.clear_relation_cache()
            replay_same = replays_equal_eager(graphed)
            # the same replays once the process has kept the GPU busy for seconds: the clocks settle ~2 % below the first second's
            # (tools/debug/capture_order_probe.py: the FIRST 300 replays of a process 2.00 ms, every later 300 -- same graph -- 2.04)
            sustained_ms = wall_ms(lambda i: step(i), 300, warm=20) if graphed is not None else None
            # the relation-graph stack alone (what the step spends outside the entity graph and the score head)
            rel_ms = wall_ms(lambda i: task.relation_representations(shard[:B, 2]), 20, warm=3)
    UF.rspmm_forward = real_forward

    # per-rank times (the driver computes scaling efficiency from `value`; this shows which rank set the max)
    t_mine = torch.tensor([my_elapsed], dtype=torch.float64, device="cpu" if share else dev)
    per_rank = [t_mine.clone() for _ in range(world)]
    if world > 1:
        dist.all_gather(per_rank, t_mine)
    per_rank_ms = [1e3 * float(t.item()) / args.steps for t in per_rank]
    t = torch.tensor([elapsed, float(frontier_visited)], dtype=torch.float64, device="cpu" if share else dev)
    if world > 1:
        tmax = t.clone()
        dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
        tsum = t.clone()
        dist.all_reduce(tsum, op=dist.ReduceOp.SUM)
        elapsed, frontier_all = float(tmax[0].item()), float(tsum[1].item())
    else:
        frontier_all = float(frontier_visited)

    block_ms = [marks[b].elapsed_time(marks[b + 1]) / max(edges_at[b + 1] - edges_at[b], 1) for b in range(n_blocks)]
    headline_blocks = dict(spread(block_ms), blocks=n_blocks, timed="stream events at block boundaries inside the one timed region")

    phases.fallback = {
        "metric": "edges aggregated/sec, FB15k237-shaped 6L x 64d rspmm Bellman-Ford (predict: the reference's 18 rspmm layers per batch as 6 relation-graph + 6 entity-graph launches, tails and heads in one pass)",
        "value": (full_layers_edges * args.steps * world + frontier_all) / elapsed, "unit": "edges aggregated/s",
        "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": 1e3 * elapsed / args.steps,
        "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f32", "data": "synthetic",
        "config": {"workload": args.workload, "global_batch": B * world, "per_rank_ms_per_step": per_rank_ms}}
    ranks = RankReduce(world, dev, share)
    devices = distinct_devices(dev, world, share)          # a collective: every rank
    pretrain_n = None
    if world > 1 and args.full and args.configs:     # config 4 with the RCCL gradient all-reduce: every rank takes part
        del xk, rk
        torch.cuda.empty_cache()
        phases.enter("config 4: capture of three graphs + steps with the gradient all-reduce", 900)
        pretrain_n = pretrain_timing(dev, DEFAULT_SEED, rank, world, ranks, quick=args.steps < 100)
        if not share:
            # the same steps with 16 compute units left free for RCCL's kernels (ultra_rspmm_reserve_cus): persistent
            # 256-workgroup grids may starve a collective that overlaps them -- an A/B the first N-GPU run records
            phases.enter("config 4 again with 16 compute units reserved for the collectives", 900)
            lib.ultra_rspmm_reserve_cus(16)
            try:
                reserved = pretrain_timing(dev, DEFAULT_SEED, rank, world, ranks, quick=True)
            finally:
                lib.ultra_rspmm_reserve_cus(0)
            for key in ("step_ms_max_over_ranks", "same_graphs_step_ms_with_allreduce", "allreduce_exposed_ms_per_step"):
                pretrain_n[key + "_16_cus_reserved"] = reserved.get(key)
        xk = rk = None
    stress_shape = tuple(int(v) for v in args.stress_shape.split(",")) if args.stress_shape else (10_000_000, 50_000_000, 500)
    stress_n = None
    if world > 1 and args.full and args.stress:      # config 5 at N GPUs: every rank takes part
        torch.cuda.empty_cache()
        phases.enter("config 5 on every rank: S-stress replicas, each rank its own triples", 900)
        stress_n = stress_inference_ranks(dev, rank, world, ranks, stress_shape)
    phases.enter("MRR, evaluation runs, configs (rank 0), final barrier" if args.full else "result line, final barrier", 1800)

    # ---------------- MRR (after the timed region): HIP path, and HIP vs CPU-oracle path on the same weights --------
    def mrr_of(t, queries):
        with torch.no_grad():
            rk = torch.cat([t.rank_batch(queries[i:i + B]) for i in range(0, len(queries), B)])
        return rk

    def oracle_check(label):
        """First batch once more with the CPU oracle in place of every HIP kernel (checker, never the product; the gated
        form of this check is tests/test_baseline_configs_gpu.py)."""
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        from oracle_ops import oracle_rspmm
        cpu_task = build_ultra(n_rel)
        cpu_task.load_state_dict({k: v.cpu() for k, v in task.state_dict().items()})
        cpu_task.preprocess(Graph(torch.from_numpy(triples), num_node=n_node, num_relation=n_rel),
                            torch.from_numpy(fact_mask)).eval()
        batch_cpu = shard[:B].cpu()
        with torch.no_grad(), oracle_rspmm(None):
            pred_cpu = cpu_task.predict(batch_cpu)
            ranks_cpu = cpu_task.get_ranking(pred_cpu, cpu_task.target(batch_cpu))
        with torch.no_grad():
            pred_gpu = task.predict(shard[:B])
            ranks_gpu = task.rank_batch(shard[:B], pred=pred_gpu).cpu()
        return {"weights": label, "queries": int(B), "mrr_hip": float((1.0 / ranks_gpu.float()).mean()),
                "mrr_cpu_oracle": float((1.0 / ranks_cpu.float()).mean()),
                "ranks_identical": int((ranks_gpu == ranks_cpu).sum()), "ranks_total": int(ranks_cpu.numel()),
                "max_abs_score_diff": float((pred_gpu.cpu() - pred_cpu).abs().max())}

    def metrics_of(ranks):
        """MR / MRR / Hits@k of filtered ranks (ultra/task.py:317-351), tails and heads together."""
        r = ranks.float().flatten()
        return {"queries": int(ranks.shape[0]), "mr": float(r.mean()), "mrr": float((1.0 / r).mean()),
                "hits@1": float((r <= 1).float().mean()), "hits@3": float((r <= 3).float().mean()),
                "hits@10": float((r <= 10).float().mean())}

    # ---------------- whole evaluation runs over the seeded test triples (engine.evaluate), three ways, same ranks ----
    eval_runs = None
    if args.full and rank == 0 and world == 1 and args.mrr_queries > 0:
        from ultra_torchdrug_amd import engine
        eval_runs = {"triples": int(len(test))}
        checks = []
        for name, kw in (("reference_loop", dict(cache_relations=False, unique_queries=False)),
                         ("cached_relations", dict(cache_relations=True, unique_queries=False)),
                         ("cached_relations_unique_queries", dict(cache_relations=True, unique_queries=True))):
            engine.evaluate(task, test[:4 * B], batch_size=B, **kw)        # first-use costs (code object loads) stay outside
            torch.cuda.synchronize()
            t_e = time.perf_counter()
            _, ranking = engine.evaluate(task, test, batch_size=B, **kw)
            torch.cuda.synchronize()
            eval_runs[name + "_ms"] = 1e3 * (time.perf_counter() - t_e)
            checks.append(ranking)
        eval_runs["ranks_identical"] = bool(all(torch.equal(checks[0], c) for c in checks[1:]))

    mrr = mrr_tuned = None
    metrics = metrics_tuned = None
    mrr_check = []
    train = None
    if args.full and args.mrr_queries > 0:
        # the seeded test triples are strided over the ranks; one all_gather of (n, 2) int64 ranks
        nq = min(-(-args.mrr_queries // world), len(test) // world)       # the same count on every rank

        def gathered(ranks):
            if world == 1:
                return ranks
            ranks = ranks.cpu() if share else ranks            # (development switch: gloo works on host tensors)
            parts = [torch.empty_like(ranks) for _ in range(world)]
            dist.all_gather(parts, ranks)
            return torch.cat(parts)

        metrics = metrics_of(gathered(mrr_of(task, shard[:nq])))
        mrr = metrics["mrr"]
        check = rank == 0 and world == 1 and not args.no_cpu_baseline
        if check:
            mrr_check.append(oracle_check("seeded random init (td_ultra_3g/4g.pth are missing blobs)"))
        if rank == 0 and world == 1 and args.finetune_steps > 0:
            # a short seeded fine-tuning run (config 3's step on this graph: rspmm fwd+bwd, AdamW 5e-4, 128 strict
            # negatives) so that the parity check also sees trained weights and an MRR that is not the random-init one
            facts = torch.from_numpy(triples[:n_fact]).to(dev)
            samples, _ = finetune_samples(task, facts, B, args.finetune_steps, DEFAULT_SEED)
            train = spread(samples)
            metrics_tuned = metrics_of(gathered(mrr_of(task, shard[:nq])))
            mrr_tuned = metrics_tuned["mrr"]
            if check:
                mrr_check.append(oracle_check("after %d seeded fine-tuning steps on the HIP path" % args.finetune_steps))

    if rank == 0:
        ms_per_step = 1e3 * elapsed / args.steps
        visited = full_layers_edges * args.steps * world + frontier_all        # entity-graph messages visited, all ranks
        if args.full:
            k_avg_ms = float(np.mean(kernel_ms)) if kernel_ms else float("nan")
            algo = bytes_algo(E, n_node, R2, Fk)
            compulsory = bytes_min(E, n_node, R2, Fk)
            achieved = algo / (k_avg_ms * 1e-3) / 1e9
            tj, traffic_source = latest_profile("traffic_fwd_fb15k237.json")
            traffic = tj.get("hbm_bytes_per_launch") if (tj and tj.get("F") == Fk and args.workload == "S-fb15k237") else None
            l2_line = {"bound": "l2-gather", "kernel": "quad_kernel<FWD,add,mul,unit_w,8>", "workload": args.workload,
                       "achieved": achieved, "peak": L2_PEAK_GBS, "unit": "GB/s", "frac": achieved / L2_PEAK_GBS,
                       "algorithmic_bytes": algo, "kernel_ms": k_avg_ms, "launches_timed": len(kernel_ms),
                       "l2_gather_ceiling": list(L2_GATHER_CEILING_GBS),
                       "frac_of_l2_gather_ceiling": achieved / L2_GATHER_CEILING_GBS[1],
                       "hbm_compulsory_bytes": compulsory,
                       "hbm_frac_on_compulsory_bytes": compulsory / (k_avg_ms * 1e-3) / 1e9 / HBM_PEAK_GBS,
                       "traffic": traffic, "traffic_source": traffic_source if traffic else None,
                       "note": "the gathered matrix (%.0f MB) is L2 / Infinity-Cache resident: its algorithmic rate exceeds the "
                               "HBM peak (%.1f TB/s), so it is priced against the XCD-L2 peak (MI355X_MICROARCH.md: 34.5 TB/s; "
                               "measured ceiling for rows gathered from L2: 16.8-18.8 TB/s); not an HBM-roofline workload "
                               "(SURVEY 8d)" % (n_node * Fk * 4 / 1e6, achieved / 1e3)}
            configs = []
            roofline = dict(l2_line)
            xk = rk = None
            torch.cuda.empty_cache()
            if world == 1 and args.configs:
                configs = config_timings(dev, lib, DEFAULT_SEED, B, quick=args.steps < 100)
            if pretrain_n is not None:
                configs.append(pretrain_n)
            if args.stress:                             # rank 0 of any world: the other ranks wait at the final barrier
                roofline = stress_roofline(dev, lib, n_node=stress_shape[0], n_triple=stress_shape[1], n_base_rel=stress_shape[2],
                                           cpu_leg=(world == 1 and not args.no_cpu_baseline))
                roofline["l2"] = l2_line
                inf = roofline["inference"]
                configs.append({"config": 5, "name": "Synthetic KG 10M nodes / 100M edges / 1k relations, 64d inference (HBM-roofline stress)",
                                "shape": roofline["workload"], "operator_fwd_ms": roofline["kernel_ms"],
                                "edges_per_s": roofline["edges_per_s"], "frac_of_hbm_peak": roofline["frac"],
                                "plan_build_s": roofline["plan_build_s"],
                                "predict_ms": inf["b1"]["predict_ms"], "predict_ms_b4": inf["b4"]["predict_ms"],
                                "filtered_rank_ms": inf["b1"]["filtered_rank_ms"],
                                "end_to_end_edges_per_s": inf["b1"]["entity_edge_messages_per_s"],
                                "end_to_end_edges_per_s_b4": inf["b4"]["entity_edge_messages_per_s"],
                                "layer_breakdown_b1": inf["layer_b1"],
                                "frac_of_hbm_peak_whole_layer": inf["layer_b1"]["frac_of_hbm_peak_whole_layer"],
                                "operator_b4_ms": roofline["b4"]["kernel_ms"], "operator_b4_frac": roofline["b4"]["frac"],
                                "all_ranks": stress_n})
            flat = flat_config_keys(configs)
            first = mrr_check[0] if mrr_check else {}
        # ---- `config`: the driver's record keeps about twenty scalars of it, in order, strings cut at ~128 characters (VERDICT r4
        # weak 8: the MRR half of the metric and configs 3-5 fell off the end) -- so the ones a reader needs come first
        config = {
            "workload": "%s N=%d E=%d R=%d B=%d F=%d, 6+6 layers x 64d, predict() tail+head over all entities"
                        % (args.workload, n_node, E, R2, B, F),
            "launch": "eager" if graphed is None else "hipGraph replay per step (engine.GraphedPredict)",
        }
        if args.full:
            config.update({
                "ms_per_step_sustained": sustained_ms,
                "mrr_hip": mrr,                                             # filtered MRR, HIP path, `mrr_queries` seeded test triples
                "mrr_hip_first_batch": first.get("mrr_hip"),                # the same B triples on both paths:
                "mrr_cpu_oracle_first_batch": first.get("mrr_cpu_oracle"),
                "ranks_identical": "%d/%d" % (first["ranks_identical"], first["ranks_total"]) if first else None,
                "max_abs_score_diff": first.get("max_abs_score_diff"),
                "cfg1_cpu_ms_per_batch": flat.get("cfg1_cpu_ms_per_batch"),
                "cfg2_predict_ms": flat.get("cfg2_predict_ms"),
                "cfg3_step_median_ms": flat.get("cfg3_step_median_ms"),
                "cfg3_fwd_us": flat.get("cfg3_fwd_us"),
                "cfg3_bwd_us": flat.get("cfg3_bwd_us"),
                "cfg4_step_median_ms": flat.get("cfg4_step_median_ms"),
                "cfg4_step_ms_max_over_ranks": flat.get("cfg4_step_ms_max_over_ranks"),
                "cfg4_allreduce_exposed_ms_per_step": flat.get("cfg4_allreduce_exposed_ms_per_step"),
                "cfg5_frac": flat.get("cfg5_frac"),
                "cfg5_fwd_ms": flat.get("cfg5_fwd_ms"),
                "cfg5_predict_ms": flat.get("cfg5_predict_ms"),
                "cfg5_whole_layer_frac": flat.get("cfg5_whole_layer_frac"),
            })
        config.update({
            "collective_backend": (dist.get_backend() if world > 1 else "none (one rank)"),
            "ranks_distinct_devices": devices,
            "ms_per_step_block_median": headline_blocks["median_ms"],
            "ms_per_step_block_min": headline_blocks["min_ms"], "ms_per_step_block_max": headline_blocks["max_ms"],
            "global_batch": B * world, "parallelism": "query-sharded replicas x%d" % world,
            "entity_edges_visited_per_step": visited / (args.steps * world),
            "frontier_edges_per_step": frontier_all / (args.steps * world),
            "device": "%s, %d CUs" % (torch.cuda.get_device_name(dev), torch.cuda.get_device_properties(dev).multi_processor_count),
            "E_rel": E_rel,
            "value_counts": "ENTITY-graph edge messages the kernels visit: 10*E*B per step (layers 2-6, 2B queries) "
                            "+ the boundary nodes' out-edges in layer 1 (frontier kernel), over the WHOLE step time "
                            "(relation stack and score head included in the time, not in the count)",
            "value_block_median": (visited / (args.steps * world)) * world / (headline_blocks["median_ms"] * 1e-3),
            "per_rank_ms_per_step": per_rank_ms,
            "per_rank_value": [(full_layers_edges + frontier_all / (args.steps * world)) / (m * 1e-3) for m in per_rank_ms],
        })
        result = {
            "metric": "edges aggregated/sec, FB15k237-shaped 6L x 64d rspmm Bellman-Ford (predict: the reference's 18 rspmm layers per batch as 6 relation-graph + 6 entity-graph launches, tails and heads in one pass)",
            "value": visited / elapsed,
            "unit": "edges aggregated/s",
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": ms_per_step,
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": "f32", "data": "synthetic",
            "config": config,
        }
        if args.full:
            config.update({
                "relation_stack_ms_per_step": rel_ms,
                "relation_graph_edges_per_step": rel_edges_per_step,
                "relation_graph_edges_per_s": rel_edges_per_step / (rel_ms * 1e-3),
                "value_r2_definition": (12 * E * B + rel_edges_per_step) * args.steps * world / elapsed,
            })
            config.update({k: v for k, v in flat.items() if k not in config})
            config["configs"] = configs
            result.update({
                "roofline": roofline,
                "composition": {
                    "ms_per_step_without_first_layer_frontier": no_frontier_ms,
                    "value_all_layers_full_kernel": 12 * E * B * world / (no_frontier_ms * 1e-3),
                    "first_layer_frontier_kernel_ms": frontier_ms,
                    "ms_per_step_with_dense_first_layer_epilogue": dense_first_ms,
                    "ms_per_step_with_cached_relation_representations": cached_ms,
                    "value_with_cached_relation_representations":
                        (visited / (args.steps * world)) / (cached_ms * 1e-3) if cached_ms else None,
                    "relation_cache_build_ms": cache_build_ms,
                    "evaluate_test_set": eval_runs,
                    "graph_replays_identical_to_eager": {"per_batch_relations": replay_same, "cached_relations": replay_same_cached},
                    "relation_graph_note": "E_rel = %d over %d relation nodes and 4 edge types: with independently drawn Zipf "
                                           "heads / tails / relations (SURVEY 8d generator) every pair of relations co-occurs, "
                                           "so the relation graph is complete -- LDS-resident, not a sparse-gather workload"
                                           % (E_rel, R2),
                    "predict_plus_filtered_rank_ms_per_step": rank_ms,
                    "finetune_step": train,
                    "finetune_note": "config 3's step on this graph (B = %d, 128 strict negatives, AdamW): negatives, edge removal, "
                                     "forward and backward replayed as one hipGraph (engine.GraphedTrainStep); per-step wall "
                                     "times, device-synchronised" % B,
                },
                "plan_build_ms": plan_build_ms,
                "eager_ms_per_step": eager_ms,
                "rspmm_kernel_only": {"kernel": "quad_kernel<FWD,add,mul,unit_w> (entity graph, F = %d: tail and head queries of the batch in one launch)" % Fk,
                                      "launches_timed": len(kernel_ms), "avg_ms": k_avg_ms,
                                      "timed": "every launch of the timed region" if graphed is None else
                                               "%d eager launches of the same kernel/shapes right after the timed region "
                                               "(event records cannot be captured into the hipGraph with this HIP runtime)" % len(kernel_ms),
                                      "edges_per_s": E * (Fk // 64) / (k_avg_ms * 1e-3) if kernel_ms else None},
                "mrr_hip": mrr,
                "mrr_hip_after_finetune": mrr_tuned,
                "metrics_hip": metrics,
                "metrics_hip_after_finetune": metrics_tuned,
                "mrr_check": mrr_check,
            })
        result["headline_blocks"] = headline_blocks
        if args.data and world == 1:
            result["real_data"] = real_data_metrics(args.data, args.ckpt, dev, B)
            result["config"]["real_data_mrr"] = result["real_data"]["metrics"].get("mrr")
        if args.full and world == 1 and not args.no_cpu_baseline:
            und_np = {"dst": und.edge_list[:, 1].cpu().numpy(), "src": und.edge_list[:, 0].cpu().numpy(),
                      "rel": und.edge_list[:, 2].cpu().numpy()}
            result["cpu_baseline"] = cpu_baseline(und_np, n_node, R2, Fk)
            if args.stress and isinstance(roofline.get("cpu"), dict):
                result["cpu_baseline"]["stress"] = roofline.pop("cpu")
        print(json.dumps(result))
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()
    phases.done()


if __name__ == "__main__":
    main()

"""Test infrastructure for the 4 GiB dispatch limits (importable without a GPU): which rows a case at size touches, the banded
rectangular graphs whose large-side endpoints are those rows, the case tables shared by ``test_address_width_cpu.py`` and
``test_address_width_gpu.py``, the ``plan_path`` program both ask for a case's kernel family, and the device-side fill / expected
output helpers (torch is imported inside them).

The fastest kernels address memory through buffer descriptors with 32-bit byte offsets; host comparisons (csrc/plan_path.h and
the launchers) decide where they may run.  A case sits on the last shape a comparison admits, on the first it refuses, or past
2^32 bytes, with ONE large operand: plans are rectangular, the other side has ``N_SMALL`` rows.  Only rows next to a byte offset
where 32-bit arithmetic can go wrong carry edges (``boundary_rows``), so the fp64 definition (``exact_grid.definition``) runs on a
few dozen re-labelled rows and the comparison is exact.
"""
import os
import shutil
import subprocess

import numpy as np

import exact_grid as XG

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ultra_torchdrug_amd", "csrc")

GIB = 1 << 30
CAP_BYTES = 48 * GIB                          # no test may pass this (torch.cuda.max_memory_allocated)
BYTE_LIMITS = (1 << 31, 0xffff0000, 1 << 32)  # sign bit of an int offset, the descriptors' admitted size, a wrapped uint32
FLT_MAX = XG.FLT_MAX
IDENTITY = {"add": 0.0, "min": FLT_MAX, "max": -FLT_MAX}

FWD, DX, DREL = 0, 1, 2
SUM_OPS = {"add": 0, "min": 1, "max": 2}
MUL_OPS = {"mul": 0, "add": 1}
FAM_DENSE, FAM_ROWGROUP, FAM_QUAD, FAM_PACKED, FAM_GENERAL = 0, 1, 2, 3, 4

# ---- rspmm cases: F = 1024, a row is 4096 B, 0xffff0000 = 4096 * 1 048 560
F_RSPMM = 1024
N_REL = 16                       # <= 16 relations: a 2^20-node plan still fits the packed word (8 + 4 + 20 bits)
N_SMALL = 128                    # rows of the side that is not under test
LAST_ADMITTED = 1_048_559        # n * 4096 <  0xffff0000
FIRST_REFUSED = 1_048_560        # n * 4096 == 0xffff0000
PAST_4GIB = 1_048_640            # n * 4096 >  2^32
CHUNK_EDGES, PIECE_LEN = 32, 128  # every plan of these cases: a hub row of HUB_EDGES edges is split into two pieces
HUB_EDGES = 160

# ---- row epilogues: dim = 64, a row is 256 B, 2^24 rows are 4 GiB
EPILOGUE_ROWS = ((1 << 24) - 64, (1 << 24) - 63, (1 << 24) - 1, 1 << 24)
SLICE_ROWS = 1 << 22             # the same entry on consecutive slices of 1 GiB is the whole-output reference


def boundary_rows(n_rows, row_bytes, k=4, cuts=()):
    """The rows a case touches, ascending: the first ``k`` and the last ``k``; the ``k`` rows on each side of every byte offset
    of ``BYTE_LIMITS`` the operand reaches (``n_rows * row_bytes >= limit``); the ``k`` rows on each side of every row index in
    ``cuts`` (where a splitting kernel cuts the operand into parts)."""
    rows = set(range(min(k, n_rows))) | set(range(max(0, n_rows - k), n_rows))
    edges = [limit // row_bytes for limit in BYTE_LIMITS if n_rows * row_bytes >= limit]
    for first_after in edges + [int(c) for c in cuts]:
        rows |= set(range(max(0, first_after - k), min(n_rows, first_after + k)))
    return np.array(sorted(rows), dtype=np.int64)


def part_cuts(n_rows, split):
    """First rows of parts 1 .. split - 1 of rowgroup_kernel (``rows_per_part = ceil(n_rows / split)``, rowgroup.inc)."""
    per = (n_rows + split - 1) // split
    return [p * per for p in range(1, split) if p * per < n_rows]


def banded_graph(n_large, large, rows, seed, hub=True, weighted=False, n_small=N_SMALL, n_rel=N_REL, per_row=6, n_empty=12):
    """A few hundred distinct edges of a rectangular adjacency whose endpoints on the ``large`` side (``"dst"`` or ``"src"``, that
    side has ``n_large`` rows) are ``rows`` only; every third of them, from the second, at most a dozen, is left with NO edge: 12
    of the 36 boundary rows of an operand past 2^32 bytes, 5 of the 16 rows of one that only passes 2^31 (they still lie at the
    start, on both sides of 2^31 and at the end).  ``hub``: one destination row of ``HUB_EDGES`` edges -- more than a piece --
    which is the last live large row (``large="dst"``) or small row 1 with sources among the live rows (``large="src"``).
    Weights ``None`` or ``exact_grid.grid_weights``.
    Returns a dict: ``dst src rel w n_dst n_src n_rel rows live empty``."""
    rng = np.random.default_rng(seed)
    rows = np.asarray(rows, dtype=np.int64)
    empty = rows[1::3][:n_empty]
    live = np.setdiff1d(rows, empty)
    triples = set()
    for v in live:
        while sum(1 for t in triples if t[0] == v) < per_row:
            triples.add((int(v), int(rng.integers(0, n_small)), int(rng.integers(0, n_rel))))
    big = np.array([t[0] for t in sorted(triples)], dtype=np.int64)
    small = np.array([t[1] for t in sorted(triples)], dtype=np.int64)
    rel = np.array([t[2] for t in sorted(triples)], dtype=np.int64)
    if large == "dst":
        dst, src = big, small
        if hub:
            pairs = rng.permutation(n_small * n_rel)[:HUB_EDGES]
            dst = np.concatenate([dst, np.full(HUB_EDGES, live[-1])])
            src, rel = np.concatenate([src, pairs // n_rel]), np.concatenate([rel, pairs % n_rel])
        n_dst, n_src = n_large, n_small
    else:
        dst, src = small, big
        if hub:
            assert len(live) * n_rel >= HUB_EDGES
            pairs = rng.permutation(len(live) * n_rel)[:HUB_EDGES]
            dst = np.concatenate([dst, np.full(HUB_EDGES, 1)])
            src, rel = np.concatenate([src, live[pairs // n_rel]]), np.concatenate([rel, pairs % n_rel])
        n_dst, n_src = n_small, n_large
    dst, src, rel, _ = XG.coalesce(dst, src, rel, None, n_src, n_rel)          # distinct triples in forward-plan order
    w = XG.grid_weights(np.random.default_rng(seed + 1), len(dst)) if weighted else None
    return dict(dst=dst, src=src, rel=rel, w=w, n_dst=n_dst, n_src=n_src, n_rel=n_rel, rows=rows, live=live, empty=empty,
                large=large)


def relabel(graph):
    """The graph with its large side re-labelled to positions in ``graph["rows"]``: ``(dst, src, n_dst, n_src)``."""
    rows = graph["rows"]
    if graph["large"] == "dst":
        return np.searchsorted(rows, graph["dst"]), graph["src"], len(rows), graph["n_src"]
    return graph["dst"], np.searchsorted(rows, graph["src"]), graph["n_dst"], len(rows)


def worst_case_is_exact(graph, message="mul", block=None):
    """``exact_grid.assert_all_exact`` on the re-labelled subgraph with EVERY operand entry at the grid's largest magnitude (2):
    an upper bound of the sums of |terms| of any grid fill, so it holds for what the device generator draws."""
    dst, src, n_dst, n_src = relabel(graph)
    F = 8                                      # every column carries the same bound
    full = lambda n: np.full((n, F), 2.0, dtype=np.float32)
    XG.assert_all_exact(dst, src, graph["rel"], graph["w"], full(graph["n_rel"]), full(n_src), full(n_dst), n_dst, message, block)


# ------------------------------------------------------------------------------------------------ the plan_path program
def build_plan_program(directory):
    """tests/plan_path_main.cpp compiled with the host compiler (a stand-alone program over csrc/plan_path.h); returns
    ``decide(list of input dicts) -> list of output dicts`` and the input field names."""
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++") or shutil.which("clang++")
    assert cxx is not None, "no host C++ compiler"
    exe = os.path.join(str(directory), "plan_path_main")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", CSRC, "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "plan_path_main.cpp"), "-o", exe])
    fields = subprocess.run([exe, "--fields"], check=True, capture_output=True, text=True).stdout.splitlines()

    def decide(inputs):
        lines = "".join(" ".join(str(int(inp[f])) for f in fields[0].split()) + "\n" for inp in inputs)
        done = subprocess.run([exe], input=lines, check=True, capture_output=True, text=True)
        rows = [dict(zip(fields[1].split(), map(int, line.split()))) for line in done.stdout.splitlines()]
        assert len(rows) == len(inputs)
        return rows

    return decide


PLAN_BASE = dict(kind=FWD, sum_op=0, mul_op=0, F=F_RSPMM, n_rel=N_REL, gather_rows=N_SMALL, gather2_rows=0, has_weight=0, has_node_b=0,
                 has_row_ptr=0, has_packed=1, has_packed_dead=0, has_dense=0, packed_src_shift=12, n_rows=N_SMALL, n_edges=400,
                 n_long_rows=0, n_pieces=0, n_hot=0, dense_rows=0, dense_cols=0, has_add_rows=0, has_bnode=0, bdim=0, has_act_bits=0,
                 has_act_node=0, act_words=0, has_workspace=0, workspace_bytes=0, aligned=127, knobs=0, n_cu=256, gfx950=1,
                 forced_conc=0, has_min_rows=0, min_rows=0)


def word_shift(n_node_a, n_rel, relation_plan=False, wide_ids=False):
    """``packed_src_shift`` of a plan (csrc/relcsr_build.hip): 8 + the relation field's bits while the node id fits the 32-bit word
    beside them, else 32 (node ids in ``node_a``; never for the relation-major plan)."""
    bits_rel = 0 if relation_plan else max((max(n_rel, 2) - 1).bit_length(), 1)
    bits_a = max((max(n_node_a, 2) - 1).bit_length(), 1)
    fits = 8 + bits_rel + bits_a <= 32
    return 32 if ((not fits or wide_ids) and not relation_plan) else 8 + bits_rel


def plan_input(kind, n_dst, n_src, sum="add", mul="mul", weighted=False, long_rows=0, wide_ids=False, knobs=0, n_edges=400,
               add_rows=False, bnode=False, n_cu=256, n_rel=N_REL, F=F_RSPMM):
    """What run_plan knows about a call over the plan of ``kind`` of an ``(n_dst, n_src, n_rel)`` adjacency (csrc/plan_path.h
    PlanInput): forward plans have destination rows and gather ``input``; d_input plans source rows and gather ``output_grad``;
    the relation-major plan gathers both."""
    rows, gather, gather2, node_a = {FWD: (n_dst, n_src, 0, n_src), DX: (n_src, n_dst, 0, n_dst),
                                     DREL: (n_rel, n_src, n_dst, n_src)}[kind]
    shift = word_shift(node_a, n_rel, kind == DREL, wide_ids)
    return dict(PLAN_BASE, kind=kind, sum_op=SUM_OPS[sum], mul_op=MUL_OPS[mul], F=F, n_rel=n_rel, gather_rows=gather,
                gather2_rows=gather2, has_weight=int(weighted), has_node_b=int(kind == DREL), has_row_ptr=int(shift == 32),
                packed_src_shift=shift, n_rows=rows, n_edges=n_edges, n_long_rows=long_rows, n_pieces=2 * long_rows,
                has_workspace=int(long_rows > 0), workspace_bytes=2 * long_rows * F * 4, has_add_rows=int(add_rows),
                has_bnode=int(bnode), bdim=64 if bnode else 0, knobs=knobs, n_cu=n_cu)


def rowgroup_split_sizes(decide, F=F_RSPMM, doublings=2):
    """``[(last n_rows before the doubling, its split, first n_rows after it, its split), ...]`` for the first ``doublings``
    doublings of rowgroup_tiling's ``split`` on a wide-id forward plan -- bisected through the program, i.e. taken from
    ``rowgroup_tiling`` itself."""
    ask = lambda n: decide([plan_input(FWD, n, N_SMALL, wide_ids=True, F=F)])[0]["split"]
    found, lo = [], 1
    for _ in range(doublings):
        base = ask(lo)
        hi = lo
        while ask(hi) == base:
            hi *= 2
        while hi - lo > 1:                  # ask(lo) == base < ask(hi)
            mid = (lo + hi) // 2
            lo, hi = (mid, hi) if ask(mid) == base else (lo, mid)
        found.append((lo, base, hi, ask(hi)))
        lo = hi
    return found


# ------------------------------------------------------------------------------------------------ the rspmm case tables
def _fwd(name, large, n, family, ops, knob=0, weighted=False, epilogue=None):
    return dict(name=name, kind=FWD, large=large, n=n, family=family, ops=ops, knob=knob, weighted=weighted, epilogue=epilogue,
                hub=True, wide_ids=False)


FORWARD_CASES = []
for _tag, _n, _fam in (("last_admitted", LAST_ADMITTED, FAM_QUAD), ("first_refused", FIRST_REFUSED, FAM_PACKED),
                       ("past_4gib", PAST_4GIB, FAM_PACKED)):
    FORWARD_CASES += [
        _fwd("out_%s" % _tag, "dst", _n, _fam, [("add", "mul"), ("max", "add")], weighted=True),
        _fwd("out_%s_add_rows" % _tag, "dst", _n, _fam, [("add", "mul")], epilogue="add_rows"),
        _fwd("out_%s_boundary" % _tag, "dst", _n, _fam, [("add", "mul")], epilogue="boundary"),
    ]
for _tag, _n, _fam in (("last_admitted", LAST_ADMITTED, FAM_QUAD), ("first_refused", FIRST_REFUSED, FAM_GENERAL),
                       ("past_4gib", PAST_4GIB, FAM_GENERAL)):
    FORWARD_CASES += [
        _fwd("input_%s_weighted" % _tag, "src", _n, _fam, [("add", "mul"), ("min", "mul")], weighted=True),
        _fwd("input_%s_unit" % _tag, "src", _n, _fam, [("add", "mul"), ("min", "mul")]),
    ]
FORWARD_CASES.append(_fwd("input_last_admitted_knob4", "src", LAST_ADMITTED, FAM_PACKED, [("add", "mul"), ("min", "mul")], knob=4,
                          weighted=True))
FORWARD_CASES.append(dict(_fwd("input_past_4gib_wide_ids", "src", PAST_4GIB, FAM_ROWGROUP, [("add", "mul")]), hub=False,
                          wide_ids=True))

# sum backward: d_input gathers output_grad rows (n_dst) and stores d_input rows (n_src); d_relation gathers both
BACKWARD_CASES = []
for _tag, _n in (("last_admitted", LAST_ADMITTED), ("first_refused", FIRST_REFUSED), ("past_4gib", PAST_4GIB)):
    # output_grad large: the d_input plan's rows are the small side, so it has no split row; past 2^20 nodes its ids are wide
    BACKWARD_CASES.append(dict(name="dx_output_grad_%s" % _tag, kind=DX, large="dst", n=_n,
                               family={LAST_ADMITTED: FAM_QUAD, FIRST_REFUSED: FAM_GENERAL, PAST_4GIB: FAM_ROWGROUP}[_n]))
    BACKWARD_CASES.append(dict(name="dx_d_input_%s" % _tag, kind=DX, large="src", n=_n,
                               family=FAM_QUAD if _n == LAST_ADMITTED else FAM_PACKED))
for _tag, _n, _fam in (("last_admitted", LAST_ADMITTED, FAM_QUAD), ("first_refused", FIRST_REFUSED, FAM_GENERAL)):
    BACKWARD_CASES.append(dict(name="drel_input_%s" % _tag, kind=DREL, large="src", n=_n, family=_fam))
    BACKWARD_CASES.append(dict(name="drel_output_grad_%s" % _tag, kind=DREL, large="dst", n=_n, family=_fam))


# edge kernels (weight gradients) and the rotate kernels do all their arithmetic in `long long`: no guard, one case on each
# side of the limits per large operand
OPERATOR_CASES = [dict(name="%s_%s" % (operand, tag), kind=FWD, large=large, n=n, hub=True, weighted=True)
                  for operand, large in (("out", "dst"), ("input", "src"))
                  for tag, n in (("last_admitted", LAST_ADMITTED), ("past_4gib", PAST_4GIB))]

# d_relation's second gather multiplies a node id with __umul24: gather2_rows < 2^24.  F = 4 (16-byte rows): 256 MiB
F_SMALL = 4
GATHER2_CASES = [dict(name="drel_gather2_rows_%s" % tag, kind=DREL, large="dst", n=n, family=family, F=F_SMALL, hub=True)
                 for tag, n, family in (("last_admitted", (1 << 24) - 1, FAM_QUAD), ("first_refused", 1 << 24, FAM_PACKED))]

# pna_statistics: (4, n_dst, F) with n_dst * F * 4 just past 2^31: planes 1 to 3 start past 2^31, 2^32 and 6 GiB
PNA_CASE = dict(name="pna_planes", kind=FWD, large="dst", n=(1 << 31) // (F_RSPMM * 4) + 1, hub=True, weighted=True)
# heads over (rows, 64) tensors past 4 GiB: the score head's hidden (N, 64 queries, 64), the PNA epilogue's rows of 16 queries
SCORE_SHAPE = (262_145, 64)
PNA_COMBINE_SHAPE = (1_048_577, 16)

# set_boundary: (N, Q, D) fp32 past 2^32 bytes
SET_BOUNDARY_SHAPE = (PAST_4GIB, 16, 64)


def case_graph(case, cuts=()):
    """The banded graph of a case (seeded by its name)."""
    import zlib
    rows = boundary_rows(case["n"], case.get("F", F_RSPMM) * 4, cuts=cuts)
    return banded_graph(case["n"], case["large"], rows, zlib.crc32(case["name"].encode()) % 100000, hub=case.get("hub", True),
                        weighted=case.get("weighted", False))


def long_rows_of(graph, kind):
    """Rows of the plan of ``kind`` with more than ``PIECE_LEN`` edges."""
    key = {FWD: graph["dst"], DX: graph["src"], DREL: graph["rel"]}[kind]
    return int((np.bincount(key) > PIECE_LEN).sum())


def case_plan_input(case, graph, sum="add", mul="mul", n_cu=256):
    n_dst, n_src = graph["n_dst"], graph["n_src"]
    return plan_input(case["kind"], n_dst, n_src, sum, mul, weighted=graph["w"] is not None,
                      long_rows=long_rows_of(graph, case["kind"]), wide_ids=case.get("wide_ids", False), knobs=case.get("knob", 0),
                      n_edges=len(graph["dst"]), add_rows=case.get("epilogue") == "add_rows",
                      bnode=case.get("epilogue") == "boundary", n_cu=n_cu, F=case.get("F", F_RSPMM))


def case_bytes(case, n=None):
    """Stated device memory need of an rspmm case: the large tensors (forward over a large output: result and expected result,
    ``add_rows`` one more; d_input over large sources: input, d_input and its expected value; else the one gathered operand)
    and 1 GiB for everything small."""
    n = case["n"] if n is None else n
    one = n * case.get("F", F_RSPMM) * 4
    if case.get("operator"):                 # OPERATOR_CASES: up to three large tensors (operand, result / output, expected)
        return 3 * one + GIB
    if case["kind"] == FWD:
        copies = (2 + (1 if case.get("epilogue") == "add_rows" else 0)) if case["large"] == "dst" else 1
    else:
        copies = 3 if (case["kind"] == DX and case["large"] == "src") else 1
    return one * copies + GIB


def epilogue_bytes(rows, backward=False):
    """Stated need of an epilogue case, in whole ``(rows, 64)`` tensors: forward -- input, update, the slice runs' result and
    the whole result (4); training -- input, update, grad_out, the forward's result, d_input, d_update, d_z and one more for
    the parameter partials and autograd's temporaries (8); plus 2 GiB for the 1 GiB slices and their results."""
    return rows * 256 * (8 if backward else 4) + 2 * GIB


# ------------------------------------------------------------------------------------------------ device helpers
def fill_grid(t, seed, step_rows=1 << 16):
    """Fill the 2-D tensor ``t`` on its device, in slices, from a seeded device generator, with exact-grid values ``k / 4``,
    ``|k| <= 8`` (no full-size integer temporary)."""
    import torch
    gen = torch.Generator(device=t.device).manual_seed(seed)
    step = max(1, (step_rows * 1024) // t.shape[1])
    for r0 in range(0, t.shape[0], step):
        part = t[r0:r0 + step]
        k = torch.randint(-8, 9, part.shape, generator=gen, device=t.device, dtype=torch.int32)
        torch.mul(k, 0.25, out=part)
    return t


def large_operand(n_rows, F, live, seed):
    """``(n_rows, F)`` fp32 on the device: NaN everywhere except the ``live`` rows, which hold distinct seeded grid rows -- a
    gather that lands on any row no edge may read shows as NaN.  Returns the tensor and the live rows' values on the host."""
    import torch
    dev = torch.device("cuda:0")
    t = torch.full((n_rows, F), float("nan"), dtype=torch.float32, device=dev)
    values = fill_grid(torch.empty(len(live), F, dtype=torch.float32, device=dev), seed)
    t[torch.from_numpy(np.asarray(live)).to(dev)] = values
    return t, values.cpu().numpy()


def expected_rows(n_rows, F, fill, rows, values):
    """The expected full output, built on the device: ``fill`` (a number or an ``(n_rows, F)`` tensor, which is consumed)
    everywhere, ``values`` (host, fp64 or fp32) scattered into ``rows``."""
    import torch
    dev = torch.device("cuda:0")
    out = fill if torch.is_tensor(fill) else torch.full((n_rows, F), float(fill), dtype=torch.float32, device=dev)
    as_f32 = np.ascontiguousarray(values, dtype=np.float32)
    assert np.array_equal(as_f32.astype(np.float64), np.asarray(values, dtype=np.float64)), "the reference is not fp32-exact"
    out[torch.from_numpy(np.asarray(rows)).to(dev)] = torch.from_numpy(as_f32).to(dev)
    return out

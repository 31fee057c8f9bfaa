"""Which kernel every rspmm plan run launches on the MI355X, and that it computes the definition.

``run_plan`` (csrc/rspmm_kernels.hip) decides by ``plan_path()`` (pinned without a GPU by tests/test_plan_path_cpu.py), switches on the
family and hands the decision's integers to the launchers, which turn them into template arguments.  The library records, at the
leaf of every launcher and from the template arguments instantiated there, what it launched (csrc/launch_record.h,
``ultra_rspmm_launch_records``).  Each row of ``ROWS`` below is one graph and one structural class of plan: for every call of the
row the test clears the ring, calls the DIRECT entry (``functional.rspmm_forward`` / ``rspmm_backward`` / the rotate equivalents) on
its own thread -- the record is thread-local and the autograd engine runs backward on threads of its own, so nothing here goes
through autograd --, reads the records back and asserts (i) their number is the number of plans the call runs, (ii) ``seq``
advanced, (iii) every expected field, and (iv) that every output EQUALS the fp64 definition of tests/exact_grid.py
(``np.array_equal`` on exact-grid operands: every summation order is exact, so there is no tolerance; the reference is the
definition, never another kernel).

The expected fields were worked out by hand from plan_path.h and from the launchers as written, and are literals of the table
(helpers ``Q`` / ``P`` / ``G`` / ``RG`` / ``R`` only name the fields).  Device-dependent are only ``blocks_per_label = ceil(n_cu / 8)``,
``grid = 8 * blocks_per_label`` and quad_kernel's concurrent tiles (``_concurrent``), restated below.  The fix-up pass of a row that
is not about the fix-up follows from the plan's shape (``_fixup_rule``: plain below 128 pieces per split row or for min / max, many
otherwise); the rows ABOUT the fix-up (``hub``, ``hub_rel``) state it as literals and assert the plan's shape first.

LEAVES -- every template instantiation the launchers of the parent commit could produce, enumerated by hand from their ``if
constexpr`` structure:

  launch_general   58 = 3 kinds x 6 operator pairs x UNIT_W x REL_LDS (72) - REL_LDS of d_relation (12) - of d_input add/add (2)
                        [forward 24, d_input 22, d_relation 12]
  launch_packed    84 = forward 6 pairs x UNIT_W x 5 VAR (60) + d_input 2 pairs x UNIT_W x 5 VAR (20) + d_relation 2 x UNIT_W (4)
  launch_quad      48 = forward 25 (add/mul: plain 2, X_LDS 2, DEAD 1; the five other pairs 4 each) + d_input 9 (add/mul 5,
                        add/add 4) + d_relation 14 (add/mul: plain 2, X_LDS 2, bits 2, node 2, DEAD 1, DEAD + bits 1; add/add: plain
                        2, bits 2)
  launch_rowgroup 132 = forward 6 pairs x UNIT_W x 3 REL x 3 G (108) + backward mul 2 x 3 x 3 (18) + backward add, L2 only, 2 x 3 (6)
  launch_fixup      4 = add with 64-piece strides ("many"), add, min, max
  launch_rotate_w  30 = forward / d_input 3 sums x UNIT_W x REL_LDS (24) + d_relation 3 sums x UNIT_W (6)

356 in all.  ``test_table_names_every_reachable_leaf`` holds the table to LEAVES - UNREACHABLE exactly; UNREACHABLE holds the two
leaves no ``PlanInput`` reaches (the launcher now refuses them).  Graphs, operands and definitions are built once per module
(the memo of tests/test_exact_grid_gpu.py, whose helpers this file uses) and never modified.
"""
import math

import numpy as np
import pytest
import torch

import exact_grid as XG
import test_exact_grid_gpu as EG
from graphs import ROTATE_VARIANTS

pytestmark = pytest.mark.gpu

FWD, DX, DREL = 0, 1, 2
ADD, MIN, MAX = 0, 1, 2
MUL, ADDM = 0, 1
DENSE, ROWGROUP, QUAD, PACKED, GENERAL, ROTATE = 0, 1, 2, 3, 4, 5
REL_L2, REL_LDS, REL_PART = 0, 1, 2
SUM_ID = {"add": ADD, "min": MIN, "max": MAX}
MUL_ID = {"mul": MUL, "add": ADDM}
PAIRS = [(s, m) for s in ("add", "min", "max") for m in ("mul", "add")]
HDR = 16                    # bytes of every launch's LDS header
LDS_ROOM = 156 * 1024       # kMaxLdsBytes: 624 relation rows of a 64-column tile


# ------------------------------------------------------------------------------------------------ the leaves
def _general_leaves():
    return {("general", k, s, m, uw, rl) for k in (FWD, DX, DREL) for s in (ADD, MIN, MAX) for m in (MUL, ADDM) for uw in (0, 1)
            for rl in (0, 1) if not (rl and (k == DREL or (k == DX and s == ADD and m == ADDM)))}


def _packed_leaves():
    out = {("packed", FWD, s, m, uw, v) for s in (ADD, MIN, MAX) for m in (MUL, ADDM) for uw in (0, 1) for v in range(5)}
    out |= {("packed", DX, ADD, m, uw, v) for m in (MUL, ADDM) for uw in (0, 1) for v in range(5)}
    out |= {("packed", DREL, ADD, m, uw, 0) for m in (MUL, ADDM) for uw in (0, 1)}
    return out


def _quad_leaves():
    """(kind, sum, mul, UNIT_W, X_LDS, U, ACT, DEAD): U is 8 on unit weights (kQuadU, kQuadUX) and 6 with a weight per edge."""
    out = set()
    for kind in (FWD, DX, DREL):
        for s, m in ([(s, m) for s in (ADD, MIN, MAX) for m in (MUL, ADDM)] if kind == FWD else [(ADD, MUL), (ADD, ADDM)]):
            forms = [(1, 0, 8, 0, 0), (0, 0, 6, 0, 0)]
            if kind != DREL or m == MUL:
                forms += [(1, 1, 8, 0, 0), (0, 1, 6, 0, 0)]
            if s == ADD and m == MUL:
                forms += [(1, 0, 8, 0, 1)] + ([(1, 0, 8, 2, 1)] if kind == DREL else [])
            if kind == DREL:
                forms += [(1, 0, 8, 2, 0), (0, 0, 6, 2, 0)] + ([(1, 0, 8, 3, 0), (0, 0, 6, 3, 0)] if m == MUL else [])
            out |= {("quad", kind, s, m) + f for f in forms}
    return out


def _rowgroup_leaves():
    """(sum, mul, UNIT_W, REL, NEEDS_REL, BACKWARD, G)"""
    out = {("rowgroup", s, m, uw, rel, 1, 0, g) for s in (ADD, MIN, MAX) for m in (MUL, ADDM) for uw in (0, 1) for rel in (0, 1, 2)
           for g in (16, 32, 64)}
    out |= {("rowgroup", ADD, MUL, uw, rel, 1, 1, g) for uw in (0, 1) for rel in (0, 1, 2) for g in (16, 32, 64)}
    out |= {("rowgroup", ADD, ADDM, uw, REL_L2, 0, 1, g) for uw in (0, 1) for g in (16, 32, 64)}
    return out


def _fixup_leaves():
    return {("fixup", ADD, True), ("fixup", ADD, False), ("fixup", MIN, False), ("fixup", MAX, False)}


def _rotate_leaves():
    return {("rotate", k, s, uw, rl) for k in (FWD, DX, DREL) for s in (ADD, MIN, MAX) for uw in (0, 1) for rl in (0, 1)
            if not (rl and k == DREL)}


LEAVES = _general_leaves() | _packed_leaves() | _quad_leaves() | _rowgroup_leaves() | _fixup_leaves() | _rotate_leaves()
# leaves no PlanInput reaches, each with its argument from plan_path.h; the launcher refuses them (ULTRA_ERR_BAD_OP)
UNREACHABLE = {
    ("packed", DX, ADD, ADDM, uw, 2): "d_input of mul = add has no relation operand (needs_rel false), so a wide-id plan gets var = 3"
    for uw in (0, 1)
}


def _leaf(rec):
    """The launcher leaf an expected record names."""
    f = rec["family"]
    if f == GENERAL:
        return ("general", rec["kind"], rec["sum"], rec["mul"], rec["unit_w"], rec["rel_lds"])
    if f == PACKED:
        return ("packed", rec["kind"], rec["sum"], rec["mul"], rec["unit_w"], rec["var"])
    if f == QUAD:
        return ("quad", rec["kind"], rec["sum"], rec["mul"], rec["unit_w"], rec["x_lds"], rec["unroll"], rec["act"], rec["dead"])
    if f == ROWGROUP:
        return ("rowgroup", rec["sum"], rec["mul"], rec["unit_w"], rec["rel_mode"], rec["needs_rel"], rec["backward"], rec["group"])
    if f == ROTATE:
        return ("rotate", rec["kind"], rec["sum"], rec["unit_w"], rec["rel_lds"])
    assert f == DENSE
    return None


# ------------------------------------------------------------------------------------------------ expected records, by name
def _ops(s, m):
    return SUM_ID[s] if isinstance(s, str) else s, MUL_ID[m] if isinstance(m, str) else m


def Q(kind, s, m, uw, xl, act=0, dead=0, **more):
    """quad_kernel<kind, s, m, UNIT_W, X_LDS, U, ACT, DEAD>; fields of the other families stay -1."""
    s, m = _ops(s, m)
    return dict(family=QUAD, kind=kind, sum=s, mul=m, unit_w=uw, x_lds=xl, unroll=8 if uw else 6, act=act, dead=dead, block=1024,
                var=-1, rel_lds=-1, group=-1, rel_mode=-1, status=0, **more)


def P(kind, s, m, uw, var, **more):
    """packed_kernel<kind, s, m, UNIT_W, VAR, 8>"""
    s, m = _ops(s, m)
    return dict(family=PACKED, kind=kind, sum=s, mul=m, unit_w=uw, var=var, unroll=8, block=1024, x_lds=-1, act=-1, dead=-1,
                concurrent=-1, rel_lds=-1, group=-1, status=0, **more)


def G(kind, s, m, uw, rl, **more):
    """segment_kernel<kind, s, m, UNIT_W, REL_LDS>"""
    s, m = _ops(s, m)
    return dict(family=GENERAL, kind=kind, sum=s, mul=m, unit_w=uw, rel_lds=rl, block=1024, var=-1, x_lds=-1, unroll=-1, act=-1,
                dead=-1, concurrent=-1, group=-1, status=0, **more)


def RG(s, m, uw, rel, needs_rel, backward, group, **more):
    """rowgroup_kernel<s, m, UNIT_W, REL, NEEDS_REL, BACKWARD, G>"""
    s, m = _ops(s, m)
    return dict(family=ROWGROUP, kind=DX if backward else FWD, sum=s, mul=m, unit_w=uw, rel_mode=rel, needs_rel=needs_rel,
                backward=backward, group=group, block=512, var=-1, x_lds=-1, act=-1, dead=-1, concurrent=-1, rel_lds=-1, fixup=0,
                status=0, **more)


def R(kind, s, uw, rl, **more):
    """rotate_segment_kernel<kind, s, UNIT_W, REL_LDS>"""
    s, _ = _ops(s, MUL)
    return dict(family=ROTATE, kind=kind, sum=s, mul=-1, unit_w=uw, rel_lds=rl, block=1024, var=-1, x_lds=-1, act=-1, dead=-1,
                concurrent=-1, group=-1, status=0, **more)


def D(kind, **more):
    return dict(family=DENSE, kind=kind, sum=ADD, mul=MUL, status=0, fixup=0, **more)


# ------------------------------------------------------------------------------------------------ graphs of this file
# (graph kwargs, nodes, relations, F, grid weights?) as in test_exact_grid_gpu.GRAPHS, whose memo and helpers build them
_FIRST_LAYER = EG.GRAPHS["first_layer"][0]
EG.GRAPHS.update({
    "lp_w": (dict(n_edge=2500), 200, 7, 128, True),                      # 200 gathered rows: the matrix fits LDS next to 7 relations
    "lp_u": (dict(n_edge=2500, unique=True), 200, 7, 128, False),
    "lp_rel700_w": (dict(n_edge=3000), 300, 700, 64, True),              # relation tile beyond LDS (624 rows)
    "lp_rel700_u": (dict(n_edge=3000, unique=True), 300, 700, 64, False),
    "lp_F66": (dict(n_edge=1500, unique=True), 150, 5, 66, False),       # F % 4 != 0
    "lp_F96": (dict(n_edge=1500, unique=True), 150, 5, 96, False),       # F % 64 != 0: no activity mask
    "lp_hot_w": (dict(n_edge=8000, skew=True), 800, 20, 64, True),       # 800 rows do not fit LDS: a hot-row cache is built
    "lp_hot_u": (dict(n_edge=8000, skew=True, unique=True), 800, 20, 64, False),
    "lp_conc_1024": (dict(n_edge=600, unique=True), 64, 5, 1024, False),
    "lp_conc_2048": (dict(n_edge=600, unique=True), 64, 5, 2048, False),
    "lp_conc_4096": (dict(n_edge=600, unique=True), 64, 5, 4096, False),
    "lp_act_u": (dict(_FIRST_LAYER, unique=True), 300, 9, 192, False),
    "lp_hub_rel": (dict(n_edge=2600, unique=True), 120, 2, 64, False),   # two relation rows of > 1 024 edges each
    "lp_hub": (None, 322, 8, 64, True),                                  # built by _hub_graph
    "rotate_lp_unit_beyond": (dict(n_edge=4000, unique=True, weights=False), 120, 320, 128, False),
})
# rowgroup: (relations, F) -> the relation-row mode follows from the relation count and the tile width alone
RG_SHAPES = [(12, 256), (700, 256), (2500, 64), (12, 128), (700, 128), (1300, 128), (400, 256), (12, 384)]
for _r, _F in RG_SHAPES:
    EG.GRAPHS["lp_rg_%d_%d_w" % (_r, _F)] = (dict(n_edge=2000), 300, _r, _F, True)
    EG.GRAPHS["lp_rg_%d_%d_u" % (_r, _F)] = (dict(n_edge=2000, unique=True), 300, _r, _F, False)
ROTATE_BLOCK = dict({"rotate_" + k: v[4] for k, v in ROTATE_VARIANTS.items()}, rotate_lp_unit_beyond=64)


def _hub_graph():
    """One destination row (node 0) with 160 x 8 = 1 280 in-edges and one source (node 1) with 1 280 out-edges; every other row
    of the forward and of the by-source plan has exactly 8 edges.  With pieces of 8 edges both hubs are the only split rows of
    their plans and have 160 pieces each (>= 128: the strided fix-up); the 8 relation rows have 320 edges = 40 pieces each."""
    key = ("graph", "lp_hub")
    if key not in EG._memo:
        feeders, sinks, rels = np.arange(2, 162), np.arange(162, 322), np.arange(8)
        dst = np.concatenate([np.zeros(1280, dtype=np.int64), np.repeat(sinks, 8)])
        src = np.concatenate([np.repeat(feeders, 8), np.ones(1280, dtype=np.int64)])
        rel = np.concatenate([np.tile(rels, 160), np.tile(rels, 160)])
        w = XG.grid_weights(np.random.default_rng(11), len(dst))
        EG._memo[key] = dict(dst=dst, src=src, rel=rel, w=w)
    return EG._memo[key]


def _removed_csr():
    """The unit-weight graph of EG._removed_case with the step's triples removed (``with_removed_edges``: marked words)."""
    from ultra_torchdrug_amd import RelCSR
    key = ("lp_removed_csr",)
    if key not in EG._memo:
        dst, src, rel, w, (h, t, q), *_ = EG._removed_case()
        base = RelCSR(EG._t(dst), EG._t(src), EG._t(rel), None, 300, 300, 6)
        assert base.unit_weight
        cut = base.with_removed_edges(EG._t(h), EG._t(t), EG._t(q), 3)
        assert np.array_equal(cut.weight.cpu().numpy(), w)
        EG._memo[key] = cut
    return EG._memo[key]


def _csr(row):
    if row["graph"] == "removed":
        return _removed_csr()
    if row["graph"] == "lp_hub":
        _hub_graph()
    return EG._csr(row["graph"], **row.get("opts", {}))


# ------------------------------------------------------------------------------------------------ the table
def fwd(s, m, *expect, **how):
    return dict(entry="fwd", sum=s, mul=m, expect=list(expect), **how)


def bwd(s, m, *expect, **how):
    return dict(entry="bwd", sum=s, mul=m, expect=list(expect), **how)


def _tbl(n_rel, rows=0):
    """LDS bytes: the launch header, a 64-column tile of `n_rel` relation rows and of `rows` gathered rows."""
    return HDR + 256 * n_rel + 256 * rows


def _quad_rows():
    rows = []
    for name, uw in (("lp_w", 0), ("lp_u", 1)):
        n, r = 200, 7
        # the gathered matrix in LDS (var 1); d_relation of mul = add reads no input row and keeps the plain form
        calls = [fwd(s, m, Q(FWD, s, m, uw, 1, lds=_tbl(r, n))) for s, m in PAIRS]
        calls += [bwd("add", "mul", Q(DX, ADD, MUL, uw, 1, lds=_tbl(r, n)), Q(DREL, ADD, MUL, uw, 1, lds=_tbl(0, n))),
                  bwd("add", "add", Q(DX, ADD, ADDM, uw, 1, lds=_tbl(0, n)), Q(DREL, ADD, ADDM, uw, 0, lds=HDR))]
        rows.append(dict(id="quad_x_lds_" + name, graph=name, knob=0, calls=calls, shape="narrow"))
        calls = [fwd(s, m, Q(FWD, s, m, uw, 0, lds=_tbl(r))) for s, m in PAIRS]
        calls += [bwd("add", "mul", Q(DX, ADD, MUL, uw, 0, lds=_tbl(r)), Q(DREL, ADD, MUL, uw, 0, lds=HDR)),
                  bwd("add", "add", Q(DX, ADD, ADDM, uw, 0, lds=HDR), Q(DREL, ADD, ADDM, uw, 0, lds=HDR))]
        rows.append(dict(id="quad_plain_" + name, graph=name, knob=2, calls=calls, shape="narrow"))
    # split rows: 160 pieces per hub row -> the strided fix-up for sums, the plain one for min / max; 40 per relation row -> plain
    many = dict(fixup=2, fixup_sum=ADD, fixup_grid=1)
    calls = [fwd("add", m, Q(FWD, ADD, m, 0, 1, **many)) for m in ("mul", "add")]
    calls += [fwd(s, m, Q(FWD, s, m, 0, 1, fixup=1, fixup_sum=SUM_ID[s], fixup_grid=1)) for s in ("min", "max") for m in ("mul", "add")]
    calls += [bwd("add", "mul", Q(DX, ADD, MUL, 0, 1, **many), Q(DREL, ADD, MUL, 0, 1, fixup=1, fixup_sum=ADD, fixup_grid=2)),
              bwd("add", "add", Q(DX, ADD, ADDM, 0, 1, **many), Q(DREL, ADD, ADDM, 0, 0, fixup=1, fixup_sum=ADD, fixup_grid=2))]
    rows.append(dict(id="hub", graph="lp_hub", opts=dict(piece_len=8), knob=0, calls=calls, shape="hub"))
    calls = [bwd("add", "mul", Q(DREL, ADD, MUL, 1, 1, **many), need_input=False)]
    rows.append(dict(id="hub_rel", graph="lp_hub_rel", opts=dict(piece_len=8), knob=0, calls=calls, shape="hub_rel"))
    return rows


def _concurrent_rows():
    """`concurrent` is asserted for every quad record by the rule (_concurrent); these rows are the shapes where it exceeds 1."""
    rows = []
    for F in (1024, 2048, 4096):
        name = "lp_conc_%d" % F
        calls = [fwd("add", "mul", Q(FWD, ADD, MUL, 1, 1, n_tiles=F // 64, split=1, n_slots=F // 64)),
                 bwd("add", "mul", Q(DX, ADD, MUL, 1, 1, n_tiles=F // 64), Q(DREL, ADD, MUL, 1, 1, n_tiles=F // 64))]
        rows.append(dict(id="concurrent_%d" % F, graph=name, knob=0, calls=calls, shape="narrow", conc_256={1024: 2, 2048: 4, 4096: 8}[F]))
    calls = [fwd("add", "mul", Q(FWD, ADD, MUL, 1, 1, concurrent=1)),
             bwd("add", "mul", Q(DX, ADD, MUL, 1, 1, concurrent=1), Q(DREL, ADD, MUL, 1, 1, concurrent=1))]
    rows.append(dict(id="concurrent_4096_knob32", graph="lp_conc_4096", knob=32, calls=calls, shape="narrow"))
    rows.append(dict(id="concurrent_4096_reserved", graph="lp_conc_4096", knob=0, reserve=8, calls=calls, shape="narrow", conc_256=1))
    return rows


def _mask_rows():
    rows = []
    words = (300 + 31) // 32         # bitmap words per 64-column tile
    for name, uw in (("first_layer", 0), ("lp_act_u", 1)):
        # knob 2: the gathered matrix (300 rows) stays out of LDS, so the masks are dispatched
        calls = [bwd("add", m, Q(DX, ADD, m, uw, 0), Q(DREL, ADD, m, uw, 0, act=2, lds=HDR + 4 * words), active="dst")
                 for m in ("mul", "add")]
        calls += [bwd("add", "mul", Q(DREL, ADD, MUL, uw, 0, act=3, lds=HDR), active="src", need_input=False)]
        rows.append(dict(id="masks_" + name, graph=name, knob=2, calls=calls, shape="narrow"))
        # without the knob the input rows come from LDS and mul = mul takes no mask; mul = add has no input rows to stage
        calls = [bwd("add", "mul", Q(DX, ADD, MUL, uw, 1), Q(DREL, ADD, MUL, uw, 1, act=0), active="dst"),
                 bwd("add", "add", Q(DX, ADD, ADDM, uw, 1), Q(DREL, ADD, ADDM, uw, 0, act=2), active="dst")]
        rows.append(dict(id="masks_x_lds_" + name, graph=name, knob=0, calls=calls, shape="narrow"))
    calls = [bwd("add", "mul", Q(DX, ADD, MUL, 1, 0), Q(DREL, ADD, MUL, 1, 0, act=0, lds=HDR), active="dst_any")]
    rows.append(dict(id="masks_F96", graph="lp_F96", knob=2, calls=calls, shape="narrow"))
    return rows


def _dead_rows():
    """``with_removed_edges`` on the unit-weight graph of test_exact_grid_gpu._removed_case (300 nodes, 6 relations, F = 128)."""
    words = (300 + 31) // 32
    marked = [fwd("add", "mul", Q(FWD, ADD, MUL, 1, 0, dead=1, lds=_tbl(6))),
              fwd("add", "add", Q(FWD, ADD, ADDM, 0, 0, dead=0)),
              fwd("max", "mul", Q(FWD, MAX, MUL, 0, 0, dead=0)),                      # refused under sum = max
              bwd("add", "mul", Q(DX, ADD, MUL, 1, 0, dead=1), Q(DREL, ADD, MUL, 1, 0, act=0, dead=1, lds=HDR)),
              bwd("add", "add", Q(DX, ADD, ADDM, 0, 0, dead=0), Q(DREL, ADD, ADDM, 0, 0, dead=0)),
              bwd("add", "mul", Q(DX, ADD, MUL, 1, 0, dead=1), Q(DREL, ADD, MUL, 1, 0, act=2, dead=1, lds=HDR + 4 * words), active="dst"),
              # a marked plan under the node mask keeps the weighted kernel
              bwd("add", "mul", Q(DREL, ADD, MUL, 0, 0, act=3, dead=0), active="src", need_input=False)]
    weighted = [fwd("add", "mul", Q(FWD, ADD, MUL, 0, 0, dead=0)),
                bwd("add", "mul", Q(DX, ADD, MUL, 0, 0, dead=0), Q(DREL, ADD, MUL, 0, 0, dead=0))]
    staged = [fwd("add", "mul", Q(FWD, ADD, MUL, 0, 1, dead=0)),
              bwd("add", "mul", Q(DX, ADD, MUL, 0, 1, dead=0), Q(DREL, ADD, MUL, 0, 1, dead=0))]
    return [dict(id="dead_words", graph="removed", knob=2, calls=marked, shape="removed"),
            dict(id="dead_words_knob128", graph="removed", knob=2 | 128, calls=weighted, shape="removed"),
            dict(id="dead_words_x_lds", graph="removed", knob=0, calls=staged, shape="removed")]


def _packed_rows():
    rows = []
    for name, uw in (("lp_w", 0), ("lp_u", 1)):
        n, r = 200, 7
        for knob, var in ((4, 1), (6, 0)):
            x = n if var == 1 else 0
            calls = [fwd(s, m, P(FWD, s, m, uw, var, lds=_tbl(r, x))) for s, m in PAIRS]
            calls += [bwd("add", "mul", P(DX, ADD, MUL, uw, var, lds=_tbl(r, x)), P(DREL, ADD, MUL, uw, 0, lds=HDR)),
                      bwd("add", "add", P(DX, ADD, ADDM, uw, var, lds=_tbl(0, x)), P(DREL, ADD, ADDM, uw, 0, lds=HDR))]
            rows.append(dict(id="packed_var%d_%s" % (var, name), graph=name, knob=knob, calls=calls, shape="narrow"))
        # wide ids on the chunked kernels (bit 3): the relation tile in LDS.  (The by-relation plan of a wide-id graph keeps its
        # source ids in the word -- its rows are relations -- and runs quad_kernel as on any graph.)
        calls = [fwd(s, m, P(FWD, s, m, uw, 3, lds=_tbl(r))) for s, m in PAIRS]
        calls += [bwd("add", "mul", P(DX, ADD, MUL, uw, 3, lds=_tbl(r)), Q(DREL, ADD, MUL, uw, 1, lds=_tbl(0, n))),
                  bwd("add", "add", P(DX, ADD, ADDM, uw, 3, lds=HDR), Q(DREL, ADD, ADDM, uw, 0, lds=HDR))]
        rows.append(dict(id="packed_var3_" + name, graph=name, opts=dict(wide_ids=True), knob=8, calls=calls, shape="wide"))
    for name, uw in (("lp_rel700_w", 0), ("lp_rel700_u", 1)):
        # 700 relations: no tile in LDS (var 2) wherever a relation operand exists; d_input of mul = add has none (var 3)
        calls = [fwd(s, m, P(FWD, s, m, uw, 2, lds=HDR)) for s, m in PAIRS]
        calls += [bwd("add", "mul", P(DX, ADD, MUL, uw, 2, lds=HDR), Q(DREL, ADD, MUL, uw, 1, lds=_tbl(0, 300))),
                  bwd("add", "add", P(DX, ADD, ADDM, uw, 3, lds=HDR), Q(DREL, ADD, ADDM, uw, 0, lds=HDR))]
        rows.append(dict(id="packed_var2_" + name, graph=name, opts=dict(wide_ids=True), knob=8, calls=calls, shape="wide"))
    for name, uw in (("lp_hot_w", 0), ("lp_hot_u", 1)):
        # hot-row cache on the forward and the by-source plan; the by-relation plan has none and 800 rows do not fit LDS
        calls = [fwd(s, m, P(FWD, s, m, uw, 4, lds=("hot", 20))) for s, m in PAIRS]
        calls += [bwd("add", "mul", P(DX, ADD, MUL, uw, 4, lds=("hot", 20)), Q(DREL, ADD, MUL, uw, 0, lds=HDR)),
                  bwd("add", "add", P(DX, ADD, ADDM, uw, 4, lds=("hot", 0)), Q(DREL, ADD, ADDM, uw, 0, lds=HDR))]
        rows.append(dict(id="packed_var4_" + name, graph=name, opts=dict(hot_cache=True), knob=0, calls=calls, shape="hot"))
    # rows of 66 floats are no multiple of 16 bytes: quad_kernel refused, two column tiles
    n, r = 150, 5
    geo = dict(n_tiles=2, split=4, n_slots=8)
    calls = [fwd(s, m, P(FWD, s, m, 1, 1, lds=_tbl(r, n), **geo)) for s, m in PAIRS]
    calls += [bwd("add", "mul", P(DX, ADD, MUL, 1, 1, lds=_tbl(r, n), **geo), P(DREL, ADD, MUL, 1, 0, lds=HDR, **geo)),
              bwd("add", "add", P(DX, ADD, ADDM, 1, 1, lds=_tbl(0, n), **geo), P(DREL, ADD, ADDM, 1, 0, lds=HDR, **geo))]
    rows.append(dict(id="packed_F66", graph="lp_F66", knob=0, calls=calls, shape="narrow"))
    return rows


def _alignment_rows():
    """A pointer 4 bytes into a 16-byte line sends the call to packed_kernel exactly where quad_kernel / rowgroup_kernel would
    load 16 bytes through it (the table of test_plan_path_cpu.py: packed_*_unaligned, quad_relation_unaligned,
    packed_d_input_input_unaligned, rowgroup_relation_unaligned)."""
    uw, n, r = 0, 200, 7
    quad_f, packed_f = Q(FWD, ADD, MUL, uw, 1), P(FWD, ADD, MUL, uw, 1)
    calls = [
        fwd("add", "mul", packed_f, unaligned="input"),
        fwd("add", "mul", quad_f, unaligned="relation"),
        fwd("add", "mul", quad_f, add_rows=True),
        fwd("add", "mul", packed_f, add_rows=True, unaligned="add_rows"),
        fwd("add", "mul", quad_f, boundary=True),
        fwd("add", "mul", packed_f, boundary=True, unaligned="boundary"),
        bwd("add", "mul", P(DX, ADD, MUL, uw, 1), P(DREL, ADD, MUL, uw, 0), unaligned="grad"),
        # d_input gathers output_grad, not input: still quad; d_relation gathers both
        bwd("add", "mul", Q(DX, ADD, MUL, uw, 1), P(DREL, ADD, MUL, uw, 0), unaligned="input"),
        bwd("add", "mul", Q(DX, ADD, MUL, uw, 1), Q(DREL, ADD, MUL, uw, 1), unaligned="relation"),
        bwd("add", "mul", Q(DX, ADD, MUL, uw, 1), d_input_add=True, need_relation=False),
        bwd("add", "mul", P(DX, ADD, MUL, uw, 1), d_input_add=True, need_relation=False, unaligned="d_input_add"),
    ]
    rows = [dict(id="alignment", graph="lp_w", knob=0, calls=calls, shape="narrow")]
    calls = [fwd("add", "mul", RG(ADD, MUL, 1, REL_LDS, 1, 0, 16)),
             fwd("add", "mul", P(FWD, ADD, MUL, 1, 3, lds=_tbl(r)), unaligned="relation")]
    rows.append(dict(id="alignment_wide", graph="lp_u", opts=dict(wide_ids=True), knob=0, calls=calls, shape="wide"))
    return rows


def _rowgroup_rows():
    rows = []
    # (relations, F, knob) -> (lanes per row, relation-row mode): tiles of 4 * group columns hold 624 / 312 / 156 relation rows,
    # four times as many in the partial mode
    modes = [(12, 256, 0, 16, REL_LDS), (700, 256, 0, 16, REL_PART), (2500, 64, 0, 16, REL_L2),
             (12, 128, 16, 32, REL_LDS), (700, 128, 16, 32, REL_PART), (1300, 128, 16, 32, REL_L2),
             (12, 256, 16, 64, REL_LDS), (400, 256, 16, 64, REL_PART), (700, 256, 16, 64, REL_L2),
             (12, 384, 16, 32, REL_LDS)]
    for r, F, knob, group, mode in modes:
        width = 4 * group
        n_tiles = -(-F // width)
        split = 8 // math.gcd(n_tiles, 8)
        fit = LDS_ROOM // (4 * width)
        held = {REL_LDS: r, REL_PART: fit, REL_L2: 0}[mode]
        geo = dict(n_tiles=n_tiles, split=split, n_slots=n_tiles * split)
        with_rel = dict(geo, n_rel_lds=held, lds=HDR + 4 * width * held)
        for tag, uw in (("w", 0), ("u", 1)):
            calls = [fwd(s, m, RG(s, m, uw, mode, 1, 0, group, **with_rel)) for s, m in PAIRS]
            # (d_relation: the by-relation plan is never wide -- quad_kernel with the 300 input rows in LDS for mul = mul)
            calls += [bwd("add", "mul", RG(ADD, MUL, uw, mode, 1, 1, group, **with_rel), Q(DREL, ADD, MUL, uw, 1, lds=_tbl(0, 300))),
                      bwd("add", "add", RG(ADD, ADDM, uw, REL_L2, 0, 1, group, n_rel_lds=0, lds=HDR, **geo), Q(DREL, ADD, ADDM, uw, 0, lds=HDR))]
            if F == 384:
                if uw == 0:
                    continue
                calls = calls[:1]           # three tiles of 128 columns: the geometry is what this row adds
            rows.append(dict(id="rowgroup_g%d_%s_r%d_F%d_%s" % (group, ("l2", "lds", "part")[mode], r, F, tag),
                             graph="lp_rg_%d_%d_%s" % (r, F, tag), opts=dict(wide_ids=True), knob=knob, calls=calls, shape="rowgroup"))
    return rows


def _general_rows():
    rows = []
    for name, uw, r, rl in (("lp_w", 0, 7, 1), ("lp_u", 1, 7, 1), ("lp_rel700_w", 0, 700, 0), ("lp_rel700_u", 1, 700, 0)):
        lds = _tbl(r) if rl else HDR
        calls = [fwd(s, m, G(FWD, s, m, uw, rl, lds=lds)) for s, m in PAIRS]
        # d_relation never keeps a relation tile; d_input of add / add reads no relation operand
        calls += [bwd(s, m, G(DX, s, m, uw, 0 if (s, m) == ("add", "add") else rl, lds=HDR if (s, m) == ("add", "add") else lds),
                      G(DREL, s, m, uw, 0, lds=HDR)) for s, m in PAIRS]
        rows.append(dict(id="general_" + name, graph=name, knob=1, calls=calls, shape="narrow"))
    # min / max have no packed backward: general without a knob
    calls = [bwd(s, m, G(DX, s, m, 0, 1, lds=_tbl(7)), G(DREL, s, m, 0, 0, lds=HDR)) for s in ("min", "max") for m in ("mul", "add")]
    rows.append(dict(id="general_min_max_backward", graph="lp_w", knob=0, calls=calls, shape="narrow"))
    return rows


def _dense_rows():
    n, r = 120, 4
    dense = [fwd("add", "mul", D(FWD)), bwd("add", "mul", D(DX), D(DREL))]
    walk = [fwd("add", "mul", Q(FWD, ADD, MUL, 1, 1, lds=_tbl(r, n))),
            bwd("add", "mul", Q(DX, ADD, MUL, 1, 1, lds=_tbl(r, n)), Q(DREL, ADD, MUL, 1, 1, lds=_tbl(0, n)))]
    return [dict(id="dense", graph="dense_64", knob=0, calls=dense, shape="dense"),
            dict(id="dense_knob64", graph="dense_64", knob=64, calls=walk, shape="dense")]


def _rotate_rows():
    rows = []
    # a pair tile of relation rows is 512 B: 312 relations fit LDS, 320 do not; d_relation never stages them
    for name, uw, r, rl in (("rotate_straddle_hub", 0, 5, 1), ("rotate_unit_weights", 1, 7, 1), ("rotate_beyond_lds", 0, 320, 0),
                            ("rotate_lp_unit_beyond", 1, 320, 0)):
        F = EG.GRAPHS[name][3]
        n_tiles = -(-(F // 2) // 64)
        geo = dict(n_tiles=n_tiles, split=8 // math.gcd(n_tiles, 8))
        lds = HDR + 512 * r * rl
        calls = [dict(entry="rot_fwd", sum=s, mul="rotate", expect=[R(FWD, s, uw, rl, lds=lds, **geo)]) for s in ("add", "min", "max")]
        calls += [dict(entry="rot_bwd", sum=s, mul="rotate", expect=[R(DX, s, uw, rl, lds=lds, **geo), R(DREL, s, uw, 0, lds=HDR, **geo)])
                  for s in ("add", "min", "max")]
        rows.append(dict(id=name, graph=name, opts=dict(piece_len=64), knob=0, calls=calls, shape="rotate"))
    # the rotate fix-up is the plain one whatever the piece count: a literal for the row with a hub
    rows[0]["calls"][0]["expect"][0].update(fixup=1, fixup_sum=ADD)
    rows[0]["calls"][1]["expect"][0].update(fixup=1, fixup_sum=MIN)
    return rows


ROWS = (_quad_rows() + _concurrent_rows() + _mask_rows() + _dead_rows() + _packed_rows() + _alignment_rows() + _rowgroup_rows() +
        _general_rows() + _dense_rows() + _rotate_rows())


def _table_leaves():
    named = set()
    for row in ROWS:
        for call in row["calls"]:
            for rec in call["expect"]:
                leaf = _leaf(rec)
                if leaf is not None:
                    named.add(leaf)
                if rec.get("fixup", 0) and "fixup_sum" in rec:
                    named.add(("fixup", rec["fixup_sum"], rec["fixup"] == 2))
    return named


def test_table_names_every_reachable_leaf():
    """The coverage contract: the expected records of ROWS name exactly LEAVES - UNREACHABLE (every call of every row is run and
    matched by test_launch_path below), the counts are the launchers', and every leaf in UNREACHABLE carries its reason."""
    count = lambda family: sum(1 for leaf in LEAVES if leaf[0] == family)
    assert [count(f) for f in ("general", "packed", "quad", "rowgroup", "fixup", "rotate")] == [58, 84, 48, 132, 4, 30]
    assert len(LEAVES) == 356
    assert set(UNREACHABLE) <= LEAVES and all(len(reason) > 20 for reason in UNREACHABLE.values())
    named = _table_leaves()
    assert named - LEAVES == set(), "the table expects a kernel no launcher instantiates"
    assert not (named & set(UNREACHABLE)), "a leaf listed as unreachable is reached"
    missing = LEAVES - set(UNREACHABLE) - named
    assert missing == set(), sorted(missing, key=str)
    assert len({row["id"] for row in ROWS}) == len(ROWS)


# ------------------------------------------------------------------------------------------------ device-dependent rules
def _concurrent(n_cu, n_slots, knob):
    """quad_kernel's tiles side by side (plan_path.h): doubled while a label has that many tile slots and every team of
    workgroups keeps at least 4, by a divisor of the label's workgroups; bit 5 switches it off."""
    bpl, per_label = -(-n_cu // 8), -(-n_slots // 8)
    c = 1
    while not (knob & 32) and 2 * c <= per_label and bpl % (2 * c) == 0 and bpl // (2 * c) >= 4:
        c *= 2
    return c


def _fixup_rule(seg, red_add, rotate):
    """0 none / 1 plain / 2 many: strided over the pieces only for sums with >= 128 pieces per split row on average."""
    n_long = int(seg.long_rows.shape[0])
    if n_long == 0:
        return 0
    return 2 if (red_add and not rotate and seg.n_pieces >= 128 * n_long) else 1


# ------------------------------------------------------------------------------------------------ running a row
_state = {"seq": 0}


def _unaligned(array):
    """The values of `array` in a contiguous tensor that starts 4 bytes into a 16-byte line."""
    t = EG._t(array)
    buf = torch.empty(t.numel() + 8, dtype=t.dtype, device=t.device)
    view = buf[1:1 + t.numel()].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    return view


def _removed(tag):
    """Operands and fp64 definitions on the graph of EG._removed_case: ``full`` -- its own; ``candidates`` -- the gradient zero
    outside 40 rows per 64-column block; ``boundary`` -- the input zero outside one row per block."""
    key = ("lp_removed", tag)
    if key not in EG._memo:
        n, F = 300, 128
        dst, src, rel, w, _, relation, x, grad, _ = EG._removed_case()
        rng = np.random.default_rng(21)
        extra = ()
        if tag == "candidates":
            t_index = rng.integers(0, n, (F // 64, 40))
            member = np.zeros((n, F // 64), dtype=bool)
            member[t_index, np.arange(F // 64)[:, None]] = True
            grad = (grad.reshape(n, F // 64, 64) * member[:, :, None]).reshape(n, F)
            extra = (t_index,)
        elif tag == "boundary":
            node = np.array([int(np.bincount(src, minlength=n).argmax()), 7], dtype=np.int32)
            keep = np.zeros((n, F // 64), dtype=bool)
            keep[node, np.arange(F // 64)] = True
            x = (x.reshape(n, F // 64, 64) * keep[:, :, None]).reshape(n, F)
            extra = (node,)
        wants = {}
        for s, m in (("add", "mul"), ("add", "add"), ("max", "mul")):
            wants[(s, m)] = XG.definition(dst, src, rel, w, relation, x, grad, n, s, m)
        EG._memo[key] = (relation, x, grad, wants) + extra
    return EG._memo[key]


def _case_data(row, call):
    """``(relation, x, grad, definition, extra)`` of a call."""
    active = call.get("active")
    tag = {"dst": "candidates", "src": "boundary"}.get(active, "boundary" if call.get("boundary") else "full")
    if row["graph"] == "removed":
        relation, x, grad, wants, *extra = _removed(tag)
        return relation, x, grad, wants[(call["sum"], call["mul"])], extra
    name = row["graph"]
    relation, x, grad, *extra = EG._inputs(name, tag)
    want = EG._definition(name, call["sum"], call["mul"], tag, block=ROTATE_BLOCK.get(name), ties=False)
    return relation, x, grad, want, extra


def _check_shape(row, csr):
    """The plan is the one the row was written for -- read from the RelCSR, asserted before anything runs."""
    kind = row["shape"]
    plans = (csr.fwd, csr.by_src, csr.by_rel)
    if kind in ("narrow", "hub", "hub_rel", "hot", "dense", "removed", "rotate"):
        assert all(p.packed is not None and p.packed_src_shift < 32 for p in plans), "ids inside the packed word expected"
    if kind in ("wide", "rowgroup"):
        assert csr.fwd.packed_src_shift == 32 and csr.by_src.packed_src_shift == 32 and csr.fwd.row_ptr is not None
        assert csr.by_rel.packed_src_shift == 8, "a by-relation plan keeps the source ids in its words"
    if kind == "rowgroup":
        assert csr.fwd.long_rows.shape[0] == 0 and csr.by_src.long_rows.shape[0] == 0, "rowgroup_kernel needs plans without split rows"
    if kind != "hot":
        assert csr.fwd.n_hot == 0 and csr.by_src.n_hot == 0
    else:
        assert csr.fwd.n_hot >= 16 and csr.by_src.n_hot >= 16 and csr.by_rel.n_hot == 0
    if kind == "dense":
        assert all(p.dense is not None for p in plans) and csr.unit_weight
    else:
        assert all(p.dense is None for p in plans)
    if kind == "removed":
        assert all(p.packed_dead is not None and p.weight is not None for p in plans)
    else:
        assert all(getattr(p, "packed_dead", None) is None for p in plans)
    if kind == "hub":
        assert (csr.fwd.long_rows.shape[0], csr.fwd.n_pieces) == (1, 160) and (csr.by_src.long_rows.shape[0], csr.by_src.n_pieces) == (1, 160)
        assert (csr.by_rel.long_rows.shape[0], csr.by_rel.n_pieces) == (8, 320)
    if kind == "hub_rel":
        assert csr.by_rel.long_rows.shape[0] == 2 and csr.by_rel.n_pieces >= 256
    if row["id"] == "rotate_straddle_hub":
        assert csr.fwd.long_rows.shape[0] > 0


def _resolve(rec, row, call, csr, n_cu, F):
    """The expected record with its device-dependent and plan-shape-dependent fields filled in."""
    want = dict(rec)
    family, kind = want["family"], want["kind"]
    seg = (csr.fwd, csr.by_src, csr.by_rel)[kind]
    if isinstance(want.get("lds"), tuple):              # ("hot", relations): the relation tile and the plan's cached rows
        want["lds"] = HDR + 256 * want["lds"][1] + 256 * seg.n_hot
    if family == DENSE:
        return want
    bpl = -(-n_cu // 8)
    want.update(blocks_per_label=bpl, grid=8 * bpl)
    columns, width = (F // 2, 64) if family == ROTATE else (F, 4 * want["group"] if family == ROWGROUP else 64)
    n_tiles = -(-columns // width)
    split = 8 // math.gcd(n_tiles, 8)
    assert want.setdefault("n_tiles", n_tiles) == n_tiles and want.setdefault("split", split) == split, "the row's own geometry"
    want.setdefault("n_slots", n_tiles * split)
    if family == QUAD:
        conc = _concurrent(n_cu, want["n_slots"], row["knob"])
        if "conc_256" in row and n_cu == (248 if row.get("reserve") else 256):
            assert conc == row["conc_256"]
        assert want.setdefault("concurrent", conc) == conc
    if "fixup" not in want:
        red_add = kind != FWD or want["sum"] == ADD
        want["fixup"] = _fixup_rule(seg, red_add, family == ROTATE)
        if want["fixup"]:
            want["fixup_sum"] = want["sum"] if kind == FWD else ADD
    if want["fixup"]:
        want.setdefault("fixup_grid", (int(seg.long_rows.shape[0]) * -(-F // 64) + 3) // 4)
    else:
        want.update(fixup_sum=-1, fixup_grid=-1)
    return want


def _run_call(row, call, csr, n_cu):
    from ultra_torchdrug_amd import _lib, functional as UF
    relation, x, grad, want, extra = _case_data(row, call)
    n, F = x.shape
    which = call.get("unaligned")
    place = lambda name, a: _unaligned(a) if which == name else EG._t(a)
    rel_t, x_t, grad_t = place("relation", relation), place("input", x), place("grad", grad)
    s, m, entry = call["sum"], call["mul"], call["entry"]
    out_t = None if s == "add" else EG._t(want[0].astype(np.float32))       # min / max backward: the forward result (exact)
    how, outputs = {}, []
    if call.get("add_rows"):
        base = XG.grid(np.random.default_rng(31), (n, F))
        how["add_rows"] = place("add_rows", base)
        outputs.append(("forward + add_rows", want[0] + base.astype(np.float64)))
    elif call.get("boundary"):
        node, value = extra
        how["boundary"] = (EG._t(node), place("boundary", value))
        outputs.append(("forward + boundary", want[0] + x.astype(np.float64)))
    elif entry in ("fwd", "rot_fwd"):
        outputs.append(("forward", want[0]))
    add_base = None
    if call.get("d_input_add"):
        add_base = XG.grid(np.random.default_rng(32), (n, F))
        how["d_input_add"] = place("d_input_add", add_base)
    if call.get("active") == "dst":
        how["active_dst"] = UF.candidate_rows(EG._t(extra[-1]), n)
        assert how["active_dst"] is not None
    elif call.get("active") == "dst_any":               # F % 64 != 0: the entry takes no mask, whatever the caller passes
        how["active_dst"] = UF.candidate_rows(EG._t(np.zeros((1, 4), dtype=np.int64)), n)
    elif call.get("active") == "src":
        how["active_src"] = EG._t(np.asarray(extra[0], dtype=np.int32))
    for key in ("need_input", "need_relation"):
        if key in call:
            how[key] = call[key]
    for name_, tensor in (("relation", rel_t), ("input", x_t), ("grad", grad_t), ("add_rows", how.get("add_rows")),
                          ("boundary", how.get("boundary", (None, None))[1]), ("d_input_add", how.get("d_input_add"))):
        if which == name_:
            assert tensor.data_ptr() % 16 == 4, "the case needs a pointer that is NOT 16-byte aligned"

    _lib.launch_records_clear()
    if entry == "fwd":
        got = [UF.rspmm_forward(csr, rel_t, x_t, s, m, **how)]
    elif entry == "bwd":
        d_x, d_r = UF.rspmm_backward(csr, rel_t, x_t, out_t, grad_t, s, m, **how)
        got = []
        if d_x is not None:
            outputs.append(("d_input", want[1] if add_base is None else want[1] + add_base.astype(np.float64)))
            got.append(d_x)
        if d_r is not None:
            outputs.append(("d_relation", want[2]))
            got.append(d_r)
    elif entry == "rot_fwd":
        got = [UF.rotate_rspmm_forward(csr, rel_t, x_t, s, ROTATE_BLOCK[row["graph"]])]
    else:
        d_x, d_r = UF.rotate_rspmm_backward(csr, rel_t, x_t, out_t, grad_t, s, ROTATE_BLOCK[row["graph"]])
        outputs += [("d_input", want[1]), ("d_relation", want[2])]
        got = [d_x, d_r]
    count, records = _lib.launch_records()

    label = (row["id"], entry, s, m, {k: v for k, v in call.items() if k not in ("entry", "sum", "mul", "expect")})
    assert count == len(call["expect"]) == len(records), (label, count, records)
    seqs = [rec["seq"] for rec in records]
    assert seqs[0] > _state["seq"] and seqs == list(range(seqs[0], seqs[0] + len(seqs))), (label, seqs, _state["seq"])
    _state["seq"] = seqs[-1]
    for rec, expected in zip(records, call["expect"]):
        expected = _resolve(expected, row, call, csr, n_cu, F)
        assert {k: rec[k] for k in expected} == expected, (label, rec)
    assert len(got) == len(outputs)
    for tensor, (what, value) in zip(got, outputs):
        assert EG._same(tensor, value), (label, what)
    return got, records         # (tests/test_cu_count_gpu.py compares both across compute-unit counts)


@pytest.mark.parametrize("row", ROWS, ids=[row["id"] for row in ROWS])
def test_launch_path(row):
    """Every call of the row launches the kernel the table names and computes the definition (module docstring)."""
    from ultra_torchdrug_amd import _lib
    lib = _lib.load()
    csr = _csr(row)
    _check_shape(row, csr)
    with EG._knob(row["knob"]):
        try:
            if row.get("reserve"):
                assert lib.ultra_rspmm_reserve_cus(row["reserve"]) == 0
            # (ultra_rspmm_device_info reports the device's compute units; the grids are sized for those not reserved)
            n_cu = max(8, _lib.device_info(0)["n_cu"] - row.get("reserve", 0))
            for call in row["calls"]:
                _run_call(row, call, csr, n_cu)
        finally:
            if row.get("reserve"):
                lib.ultra_rspmm_reserve_cus(0)

"""Exact-grid parity on the MI355X (``tests/exact_grid.py``): every path of the HIP library that evaluates an rspmm sum
against the plain fp64 definition, on inputs where fp32 arithmetic is exact.  The bar is ``np.array_equal`` on every entry
of forward, ``d_input``, ``d_relation`` and ``d_weight`` -- no tolerance, nothing masked -- whatever the summation order
(pieces, quad / packed / general / rowgroup kernels, the dense matrix-core form, the frontier and boundary entries, the
skipped-gather forms, rotate messages).  On these inputs min / max tie in 5 - 30 % of the cells (zeros of either sign, zero
weights, equal products, merged duplicates), so the backward kernels' equality mask is held to the convention that EVERY tied
edge receives the gradient in full; each min / max case asserts that share and a non-zero gradient on the tied cells.

Graphs, operands and definitions are built once per module and never modified."""
import zlib

import numpy as np
import pytest
import torch

import exact_grid as XG
from graphs import ROTATE_VARIANTS, random_graph

pytestmark = pytest.mark.gpu

SUMS = ["add", "min", "max"]
MULS = ["mul", "add"]

# name: (graph kwargs, nodes, relations, F, grid weights?) -- the smallest shapes that reach each plan kernel
# (tests/test_rspmm_gpu.py CASES); without grid weights the triples are distinct and the plans carry no weight array
GRAPHS = {
    "weights_dups": (dict(n_edge=3000, skew=True), 200, 7, 128, True),                  # merged duplicates, split rows
    "ragged_isolated": (dict(n_edge=2000, isolated=150, unique=True), 400, 5, 100, False),
    "narrow_F": (dict(n_edge=500), 64, 3, 1, True),
    "many_relations": (dict(n_edge=6000, skew=True, unique=True), 300, 700, 64, False),  # relation table beyond LDS
    # a hub row of 3 000 drawn edges (1 528 distinct triples: the zipf sources repeat)
    "hub": (dict(n_edge=20000, skew=True, hub_row=5, hub_edges=3000), 500, 30, 192, True),
    "hot": (dict(n_edge=40000, skew=True), 3000, 40, 128, True),
    "first_layer": (dict(n_edge=9000, skew=True, hub_row=2, hub_edges=1000, isolated=20), 300, 9, 192, True),
    "first_layer_2": (dict(n_edge=9000, skew=True, hub_row=2, hub_edges=1000, isolated=20), 300, 9, 128, True),
    "dense_64": (dict(n_edge=40000, unique=True), 120, 4, 64, False),
    "dense_1024": (dict(n_edge=40000, unique=True), 120, 4, 1024, False),
    "dense_sparse": (dict(n_edge=9500, unique=True), 150, 4, 192, False),                # 10 % of the cells: the threshold is 8 %
}
for _name, (_kw, _n, _r, _F, _block) in ROTATE_VARIANTS.items():
    GRAPHS["rotate_" + _name] = (dict(_kw, weights=False), _n, _r, _F, bool(_kw.get("weights")))
PLAN_OPTS = {"hub_split": dict(piece_len=32, chunk_edges=8)}

_memo = {}


def _dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


def _seed(name):
    return zlib.crc32(name.encode()) % 100000


def _graph(name):
    key = ("graph", name)
    if key not in _memo:
        kw, n, r, F, weighted = GRAPHS[name]
        g = random_graph(seed=_seed(name), n_node=n, n_rel=r, **kw)
        g["w"] = XG.grid_weights(np.random.default_rng(_seed(name) + 1), len(g["dst"])) if weighted else None
        _memo[key] = g
    return _memo[key]


def _inputs(name, tag="full"):
    """``(relation, x, grad)`` float32 grid arrays of a graph.  ``tag``: ``full``, or ``boundary`` -- ``x`` zero outside row
    ``node[b]`` of 64-column block ``b`` (the first Bellman-Ford layer's input) -- or ``candidates`` -- ``grad`` zero outside a
    few rows per 64-column block (the last layer's output gradient); both also return their index arrays."""
    key = ("inputs", name, tag)
    if key not in _memo:
        _, n, r, F, _ = GRAPHS[name]
        rng = np.random.default_rng(_seed(name) + 2)
        # rotate: a message is a difference of two products and ties less often than one product (4 - 8 % of the cells with
        # |k| <= 8, 11 - 17 % with |k| <= 4)
        lim = 4 if name.startswith("rotate_") else 8
        relation, x, grad = XG.grid(rng, (r, F), lim=lim), XG.grid(rng, (n, F), lim=lim), XG.grid(rng, (n, F), zero=0.0)
        extra = ()
        if tag == "boundary":
            B = F // 64
            g = _graph(name)
            node = np.array([2, 7, n - 1][:B], dtype=np.int32)          # the hub row's node, a plain one, an isolated one
            value = XG.grid(rng, (B, 64))
            x = np.zeros((n, B, 64), dtype=np.float32)
            x[node, np.arange(B)] = value
            x = x.reshape(n, F)
            assert (np.bincount(g["src"], minlength=n)[node] > 0).all()
            extra = (node, value)
        elif tag == "candidates":
            B = F // 64
            t_index = rng.integers(0, n, (B, 40))
            t_index[:, 0] = 2                                             # the hub among the candidates
            member = np.zeros((n, B), dtype=bool)
            member[t_index, np.arange(B)[:, None]] = True
            grad = (grad.reshape(n, B, 64) * member[:, :, None]).reshape(n, F)
            extra = (t_index,)
        _memo[key] = (relation, x, grad) + extra
    return _memo[key]


def _definition(name, sum, message, tag="full", block=None, ties=True):
    """The fp64 definition of a case, computed once; asserts the exactness precondition (once per operand set) and, for min /
    max, that ties are frequent and carry gradient."""
    key = ("def", name, sum, message, tag, block)
    if key not in _memo:
        g = _graph(name)
        n = GRAPHS[name][1]
        relation, x, grad = _inputs(name, tag)[:3]
        pre = ("exact", name, message, tag, block)
        if pre not in _memo:
            XG.assert_all_exact(g["dst"], g["src"], g["rel"], g["w"], relation, x, grad, n, message, block)
            _memo[pre] = True
        want = XG.definition(g["dst"], g["src"], g["rel"], g["w"], relation, x, grad, n, sum, message, block)
        if sum != "add" and ties:
            XG.assert_ties_matter(want[4], g["dst"], n, grad)
        _memo[key] = want
    return _memo[key]


def _csr(name, plan=None, **opts):
    """Device RelCSR of a graph (cached per option set)."""
    from ultra_torchdrug_amd import RelCSR
    opts = dict(PLAN_OPTS.get(plan, {}), **opts)
    key = ("csr", name, tuple(sorted(opts.items())))
    if key not in _memo:
        g = _graph(name)
        _, n, r, _, _ = GRAPHS[name]
        _memo[key] = RelCSR(_t(g["dst"]), _t(g["src"]), _t(g["rel"]), None if g["w"] is None else _t(g["w"]), n, n, r, **opts)
    return _memo[key]


def _same(got, want):
    """Every entry equal as numbers (+0 == -0), after the cast to fp64."""
    return np.array_equal(got.detach().cpu().numpy().astype(np.float64), want)


def _knob(value):
    """Context manager: ``ultra_rspmm_force_general_path(value)``, reset on exit."""
    import contextlib
    import ultra_torchdrug_amd as U

    @contextlib.contextmanager
    def manager():
        lib = U.require_library()
        lib.ultra_rspmm_force_general_path(value)
        try:
            yield
        finally:
            lib.ultra_rspmm_force_general_path(0)
    return manager()


def _check_operator(csr, name, sum, mul, tag="full", launched=None):
    """Forward and both gradients through autograd against the definition.  ``launched``: fields of the library's launch record
    (``_lib.launch_records``) the FORWARD must show -- the record is thread-local and autograd runs the backward on a thread of
    its own, so only the forward is held to it here (tests/test_launch_paths_gpu.py holds the direct backward entries)."""
    from ultra_torchdrug_amd import _lib, functional as UF
    relation, x, grad = _inputs(name, tag)[:3]
    out_w, d_x_w, d_r_w, _, _ = _definition(name, sum, mul, tag)
    rel_t, x_t = _t(relation).requires_grad_(), _t(x).requires_grad_()
    _lib.launch_records_clear()
    out = UF.generalized_rspmm(csr, rel_t, x_t, sum=sum, mul=mul)
    if launched is not None:
        count, records = _lib.launch_records()
        want = dict(launched, kind=0, sum=SUMS.index(sum), mul=MULS.index(mul), status=0)
        assert count == 1 and {k: records[0][k] for k in want} == want, (want, records)
    out.backward(_t(grad))
    assert _same(out, out_w), "forward"
    assert _same(x_t.grad, d_x_w), "d_input"
    assert _same(rel_t.grad, d_r_w), "d_relation"


# ------------------------------------------------------------------------------------------------ plan kernels
PLAN_CASES = [("weights_dups", None), ("ragged_isolated", None), ("narrow_F", None), ("many_relations", None), ("hub", None),
              ("hub", "hub_split")]


@pytest.mark.parametrize("name,plan", PLAN_CASES, ids=[p or n for n, p in PLAN_CASES])
@pytest.mark.parametrize("sum", SUMS)
@pytest.mark.parametrize("mul", MULS)
def test_plan_kernels_equal_the_definition(name, plan, sum, mul):
    csr = _csr(name, plan)
    assert csr.unit_weight == (not GRAPHS[name][4])
    if name == "hub":
        deg = int(torch.bincount(csr.dst).max())
        assert deg >= 1500 and csr.fwd.n_pieces > 0
        if plan == "hub_split":
            assert csr.piece_len == 32 and csr.fwd.n_pieces > 100 and csr.by_src.n_pieces > 100 and csr.by_rel.n_pieces > 100
    _check_operator(csr, name, sum, mul)


@pytest.mark.parametrize("name,plan", [("weights_dups", None), ("hub", None), ("hub", "hub_split")],
                         ids=["weights_dups", "hub", "hub_split"])
@pytest.mark.parametrize("knob", [0, 1, 2, 4, 6, 32])
def test_every_forward_and_sum_backward_variant_equals_the_definition(name, plan, knob):
    """General / packed / quad kernels, gathered matrix from L2 or LDS, column tiles one after the other."""
    from ultra_torchdrug_amd import functional as UF
    csr = _csr(name, plan)
    relation, x, grad = _inputs(name)
    with _knob(knob):
        outs = {(s, m): UF.rspmm_forward(csr, _t(relation), _t(x), s, m) for s in SUMS for m in MULS}
        grads = {m: UF.rspmm_backward(csr, _t(relation), _t(x), None, _t(grad), "add", m) for m in MULS}
    for (s, m), out in outs.items():
        assert _same(out, _definition(name, s, m)[0]), (s, m)
    for m, (d_x, d_r) in grads.items():
        want = _definition(name, "add", m)
        assert _same(d_x, want[1]) and _same(d_r, want[2]), m


# ------------------------------------------------------------------------------------------------ big-graph layout
@pytest.mark.parametrize("name", ["weights_dups", "ragged_isolated", "many_relations"])
@pytest.mark.parametrize("knob", [0, 8, 16])
def test_wide_id_plans_equal_the_definition(name, knob):
    """Node ids outside the packed word: one row per 16-lane group (rowgroup kernel: F % 4 == 0, no split rows), the chunked
    kernels instead (bit 3) and the wide-group forms (bit 4); ``many_relations`` has rows beyond the 512-edge pieces of these
    plans and a relation table beyond LDS, so it stays on the chunked kernels."""
    csr = _csr(name, wide_ids=True)
    assert csr.fwd.packed_src_shift == 32 and csr.by_src.packed_src_shift == 32 and GRAPHS[name][3] % 4 == 0
    assert (csr.fwd.n_pieces == 0 and csr.by_src.n_pieces == 0) == (name != "many_relations")
    # the forward's kernel (launch record; family 1 = rowgroup_kernel, 3 = packed_kernel): 16 lanes per row, 32 under bit 4 where
    # F % 128 == 0 (weights_dups: F = 128; ragged_isolated: F = 100), the relation rows (7 / 5) in LDS; packed_kernel's wide-id
    # forms under bit 3 (var 3: relation tile in LDS) and for many_relations whatever the knob (var 2: 700 rows do not fit)
    unit_w = int(not GRAPHS[name][4])
    if name == "many_relations":
        launched = dict(family=3, var=2, unit_w=unit_w)
    elif knob == 8:
        launched = dict(family=3, var=3, unit_w=unit_w)
    else:
        launched = dict(family=1, group=32 if (knob == 16 and name == "weights_dups") else 16, rel_mode=1, unit_w=unit_w, backward=0)
    with _knob(knob):
        for s in SUMS:
            for m in MULS:
                _check_operator(csr, name, s, m, launched=launched)


@pytest.mark.parametrize("sum", SUMS)
def test_hot_row_cache_plans_equal_the_definition(sum):
    csr = _csr("hot", hot_cache=True)
    assert csr.fwd.n_hot >= 16 and csr.by_src.n_hot >= 16
    for m in MULS:
        _check_operator(csr, "hot", sum, m, launched=dict(family=3, var=4, unit_w=0))       # packed_kernel, hot-row cache form


# ------------------------------------------------------------------------------------------------ dense relation-graph form
@pytest.mark.parametrize("name", ["dense_64", "dense_1024", "dense_sparse"])
@pytest.mark.parametrize("knob", [0, 64])
def test_dense_form_equals_the_definition(name, knob):
    """4 relation types, unit weights, distinct triples: the sums on the matrix cores (d_relation in its own documented order)
    and, under bit 6, along the edge list -- both exact here."""
    from ultra_torchdrug_amd import functional as UF
    csr = _csr(name)
    F = GRAPHS[name][3]
    assert csr.dense_form and csr.fwd.dense is not None and csr.kernel_order("add", "mul", F) == (0, True)
    if name == "dense_sparse":
        assert csr.n_edges < 0.11 * 150 * 150 * 4
    relation, x, grad = _inputs(name)
    with _knob(knob):
        out = UF.rspmm_forward(csr, _t(relation), _t(x), "add", "mul")
        d_x, d_r = UF.rspmm_backward(csr, _t(relation), _t(x), None, _t(grad), "add", "mul")
    want = _definition(name, "add", "mul")
    assert _same(out, want[0]), "forward"
    assert _same(d_x, want[1]), "d_input"
    assert _same(d_r, want[2]), "d_relation"


@pytest.mark.parametrize("sum", SUMS)
@pytest.mark.parametrize("mul", MULS)
def test_operators_on_a_dense_form_graph_equal_the_definition(sum, mul):
    """The other operators on a graph that carries the dense form (TransE sums: d_relation along the edge list; min / max)."""
    _check_operator(_csr("dense_64"), "dense_64", sum, mul)


# ------------------------------------------------------------------------------------------------ first layer, raw CSR
@pytest.mark.parametrize("name", ["first_layer_2", "first_layer"])
def test_first_layer_entries_equal_the_definition(name):
    """The input is a boundary -- zero outside one row per 64-column query block (2 and 3 blocks): the frontier kernel, the
    sparse boundary epilogue of every operator, the boundary rows of d_input and d_relation from the boundary nodes' out-edges."""
    from ultra_torchdrug_amd import functional as UF
    csr = _csr(name)
    _, n, r, F, _ = GRAPHS[name]
    relation, x, grad, node, value = _inputs(name, "boundary")
    assert csr.fwd.n_pieces > 0
    dense = x.astype(np.float64)                         # the boundary as a dense (n, F) tensor: the input itself
    boundary = (_t(node), _t(value))
    want_add = _definition(name, "add", "mul", "boundary")
    for knob in (0, 1):                                  # bit 0: the L2-row form of the frontier kernel
        with _knob(knob):
            assert _same(UF.rspmm_frontier(csr, _t(relation), boundary), want_add[0] + dense), knob
    epilogue = {"add": np.add, "min": np.minimum, "max": np.maximum}
    for s in SUMS:
        for m in MULS:
            want = _definition(name, s, m, "boundary", ties=False)[0]
            got = UF.rspmm_forward(csr, _t(relation), _t(x), s, m, boundary=boundary)
            assert _same(got, epilogue[s](want, dense)), (s, m)
            got = UF.rspmm_forward(csr, _t(relation), _t(x), s, m, add_rows=_t(x))
            assert _same(got, epilogue[s](want, dense)), (s, m)
    # d_input at the rows autograd consumes, added in place; every other element keeps what it held
    rng = np.random.default_rng(5)
    base = XG.grid(rng, (n, F))
    blocks = np.zeros((n, F // 64), dtype=bool)
    blocks[node, np.arange(F // 64)] = True
    at_rows = np.repeat(blocks, 64, axis=1)
    for m in MULS:
        d_x_w = _definition(name, "add", m, "boundary")[1]
        got = UF.rspmm_backward_boundary_rows(csr, _t(relation), _t(grad), _t(node), _t(base.copy()), m)
        assert _same(got, base.astype(np.float64) + np.where(at_rows, d_x_w, 0.0)), m
    assert _same(UF.rspmm_drelation_boundary(csr, _t(x), _t(grad), _t(node)), want_add[2])
    _, d_r = UF.rspmm_backward(csr, _t(relation), _t(x), None, _t(grad), "add", "mul", need_input=False, active_src=_t(node))
    assert _same(d_r, want_add[2])


@pytest.mark.parametrize("name", ["weights_dups", "many_relations"])
def test_raw_csr_entry_equals_the_definition(name):
    """``ultra_rspmm_fwd_f32``: no plan, every row sequentially; weighted and unit-weight."""
    from ultra_torchdrug_amd import functional as UF
    csr = _csr(name)
    row_ptr, src, rel, w = csr.csr_arrays
    assert (w is None) == (not GRAPHS[name][4])
    relation, x, _ = _inputs(name)
    for s in SUMS:
        for m in MULS:
            got = UF.rspmm_forward_csr(row_ptr, src, rel, w, _t(relation), _t(x), s, m)
            assert _same(got, _definition(name, s, m)[0]), (s, m)


# ------------------------------------------------------------------------------------------------ skipped-gather forms
@pytest.mark.parametrize("plan", [None, "hub_split"])
@pytest.mark.parametrize("mul", MULS)
def test_backward_with_candidate_bitmaps_equals_the_definition(plan, mul):
    """``ultra_rspmm_backward_active_f32``: an edge whose gradient row is zero by the caller's word skips its gathers and must
    contribute exactly what the definition's zero row contributes."""
    from ultra_torchdrug_amd import functional as UF
    name = "first_layer"
    csr = _csr(name, plan)
    _, n, r, F, _ = GRAPHS[name]
    relation, x, grad, t_index = _inputs(name, "candidates")
    assert (grad.reshape(n, F // 64, 64) != 0).any(axis=2).sum() < 0.5 * n * (F // 64)
    bits = UF.candidate_rows(_t(t_index), n)
    assert bits is not None
    want = _definition(name, "add", mul, "candidates")
    d_x, d_r = UF.rspmm_backward(csr, _t(relation), _t(x), None, _t(grad), "add", mul, active_dst=bits)
    assert _same(d_x, want[1]), "d_input"
    assert _same(d_r, want[2]), "d_relation"
    base = XG.grid(np.random.default_rng(6), (n, F))
    acc, _ = UF.rspmm_backward(csr, _t(relation), _t(x), None, _t(grad), "add", mul, need_relation=False,
                               d_input_add=_t(base.copy()), active_dst=bits)
    assert _same(acc, base.astype(np.float64) + want[1]), "d_input accumulated"


def _removed_case():
    """A unit-weight graph with inverse edges, the triples a training step removes from it and the definition in which those
    edges (and their inverses) carry weight 0: ``(dst, src, rel, w, (h, t, q), relation, x, grad, wants)``."""
    key = ("removed",)
    if key not in _memo:
        n, r, F = 300, 6, 128
        g = random_graph(seed=3, n_node=n, n_edge=2500, n_rel=r // 2, unique=True)
        dst, src, rel = np.concatenate([g["dst"], g["src"]]), np.concatenate([g["src"], g["dst"]]), \
            np.concatenate([g["rel"], g["rel"] + r // 2])
        dst, src, rel, _ = XG.coalesce(dst, src, rel, None, n, r)
        rng = np.random.default_rng(4)
        base_edges = np.flatnonzero(rel < r // 2)
        row = np.bincount(dst, minlength=n).argmax()
        pick = np.unique(np.concatenate([rng.choice(base_edges, 60, replace=False),
                                         base_edges[dst[base_edges] == row]]))       # every base edge into the heaviest row
        removed = set(zip(src[pick], dst[pick], rel[pick])) | set(zip(dst[pick], src[pick], rel[pick] + r // 2))
        w = np.array([0.0 if e in removed else 1.0 for e in zip(src, dst, rel)], dtype=np.float32)
        assert (w == 0).sum() >= 2 * len(pick) - 2
        # the removed triples listed with repeats, and three that are no edges
        edges = set(zip(src, dst, rel))
        loops = [a for a in range(n) if (a, a, 0) not in edges][:3]
        h = np.concatenate([src[pick], src[pick][:5], loops])
        t = np.concatenate([dst[pick], dst[pick][:5], loops])
        q = np.concatenate([rel[pick], rel[pick][:5], [0, 0, 0]])
        relation, x, grad = XG.grid(rng, (r, F)), XG.grid(rng, (n, F)), XG.grid(rng, (n, F), zero=0.0)
        for m in MULS:
            XG.assert_all_exact(dst, src, rel, w, relation, x, grad, n, m)
        wants = {m: XG.definition(dst, src, rel, w, relation, x, grad, n, "add", m) for m in MULS}
        _memo[key] = (dst, src, rel, w, (h, t, q), relation, x, grad, wants)
    return _memo[key]


@pytest.mark.parametrize("knob", [0, 128])
def test_removed_edges_equal_the_definition_with_zero_weights(knob):
    """``with_removed_edges`` on a unit-weight graph with inverse edges: marked words (and, under bit 7, the weighted kernels)
    against the definition in which the removed edges carry weight 0."""
    from ultra_torchdrug_amd import RelCSR, functional as UF
    n, r = 300, 6
    dst, src, rel, w, (h, t, q), relation, x, grad, wants = _removed_case()
    csr = RelCSR(_t(dst), _t(src), _t(rel), None, n, n, r)
    assert csr.unit_weight and csr.n_edges == len(dst)
    cut = csr.with_removed_edges(_t(h), _t(t), _t(q), r // 2)
    assert cut.fwd.packed_dead is not None and np.array_equal(cut.weight.cpu().numpy(), w)
    with _knob(knob):
        for m in MULS:
            out = UF.rspmm_forward(cut, _t(relation), _t(x), "add", m)
            d_x, d_r = UF.rspmm_backward(cut, _t(relation), _t(x), None, _t(grad), "add", m)
            assert _same(out, wants[m][0]) and _same(d_x, wants[m][1]) and _same(d_r, wants[m][2]), m


# ------------------------------------------------------------------------------------------------ rotate messages
@pytest.mark.parametrize("variant", list(ROTATE_VARIANTS))
@pytest.mark.parametrize("sum", SUMS)
def test_rotate_kernels_equal_the_definition(variant, sum):
    """The six launch variants of csrc/rotate.inc: forward, d_input, d_relation and the edge-weight gradient; split rows of
    all three plans where the variant has a hub (pieces of 64)."""
    from ultra_torchdrug_amd import functional as UF, rotate_rspmm
    name = "rotate_" + variant
    block = ROTATE_VARIANTS[variant][4]
    csr = _csr(name, piece_len=64)
    assert csr.unit_weight == (variant == "unit_weights")
    relation, x, grad = _inputs(name)
    out_w, d_x_w, d_r_w, d_w_w, _ = _definition(name, sum, "rotate", block=block)
    rel_t, x_t = _t(relation).requires_grad_(), _t(x).requires_grad_()
    out = rotate_rspmm(csr, rel_t, x_t, sum=sum, block=block)
    out.backward(_t(grad))
    assert _same(out, out_w), "forward"
    assert _same(x_t.grad, d_x_w), "d_input"
    assert _same(rel_t.grad, d_r_w), "d_relation"
    d_w = UF.rotate_rspmm_backward_weight(csr, _t(relation), _t(x), out.detach(), _t(grad), sum, block)
    assert _same(d_w, d_w_w), "d_weight"


# ------------------------------------------------------------------------------------------------ d_weight
@pytest.mark.parametrize("name", ["weights_dups", "ragged_isolated"])
@pytest.mark.parametrize("sum", SUMS)
@pytest.mark.parametrize("mul", MULS)
def test_weight_gradient_equals_the_definition(name, sum, mul):
    """``ultra_rspmm_backward_weight_f32`` on a weighted and a unit-weight plan: the unweighted message under the mask of the
    weighted one."""
    from ultra_torchdrug_amd import functional as UF
    csr = _csr(name)
    relation, x, grad = _inputs(name)
    want = _definition(name, sum, mul)
    out = UF.rspmm_forward(csr, _t(relation), _t(x), sum, mul)
    assert _same(out, want[0])
    d_w = UF.rspmm_backward_weight(csr, _t(relation), _t(x), out, _t(grad), sum, mul)
    assert d_w.shape == (csr.n_edges,) and _same(d_w, want[3])


def test_sparse_tensor_values_receive_the_definitions_weight_gradient():
    """Through ``torch.sparse_coo_tensor`` values that require grad: duplicates of one triple all receive its gradient."""
    from ultra_torchdrug_amd import functional as UF
    name = "weights_dups"
    g = _graph(name)
    _, n, r, F, _ = GRAPHS[name]
    relation, x, grad = _inputs(name)
    want = _definition(name, "max", "mul")
    values = _t(g["w"]).requires_grad_()
    sparse = torch.sparse_coo_tensor(_t(np.stack([g["dst"], g["src"], g["rel"]])), values, (n, n, r))
    out = UF.generalized_rspmm(sparse, _t(relation), _t(x), sum="max", mul="mul")
    out.backward(_t(grad))
    key = (g["dst"] * n + g["src"]) * r + g["rel"]
    position = np.searchsorted(np.unique(key), key)
    assert len(np.unique(key)) < len(key)
    assert _same(out, want[0]) and _same(values.grad, want[3][position])

"""Every grid that is sized from the compute-unit count, held to its results at 8, 24 and 240 compute units.

Almost every launcher of csrc/ sizes its grid from ``DeviceInfo::n_cu`` and lets the kernel loop over what the grid does not
cover; at the device's 256 compute units the small per-kernel tests never reach a wave's second tile or a workgroup's second
ticket.  ``ultra_rspmm_reserve_cus`` (tests/cu_count.py: ``compute_units(n)``) makes that axis cheap: at 8 compute units a
6 149-row input is several tiles per wave on the full grid with a 5-row tail, and every plan family runs with ONE workgroup per
XCD label.  24 gives three workgroups per label (odd: quad_kernel cannot split them into teams), 240 is what bench.py leaves its
multi-GPU legs (30 per label, two concurrent tiles where 256 give eight).

What is asserted, per entry:

  dense forwards (8 CUs)   the int32 bits of the same call at the default count, on every row, AND the oracle / definition the
                           entry's own test uses, with no tolerance: their summation order is per row.
  block-partial reducers   row outputs (d_input, d_update, d_hidden, d_relation rows): the default run's bits.  Reduced outputs
                           (parameter gradients) depend on the number of partials, so (a) on exact-grid operands without LayerNorm
                           every count gives the fp64 definition under ``np.array_equal`` -- the test first proves on the host that
                           every sum of |terms| stays below 2^24 units of the grid -- and (b) on seeded normals with LayerNorm
                           they stay within ``4 * ref_dev + floor * scale`` of the fp64 ATen chain, ``ref_dev`` being the fp32
                           ATen chain's own deviation and ``floor`` the one the entry's existing test uses.
  guard bands              the reducers at 8 CUs between poisoned, banded allocations (ctypes binding), and again at the default
                           count after the context has exited: Python-sized partial buffers and C-side wave counts must agree
                           whenever the setting changes between calls.
  plan families            rows of tests/test_launch_paths_gpu.py, every call of each at 8, 24 and 240: the exact-grid definition,
                           the default run's bits, and from the launch record the family, ``blocks_per_label``, ``grid`` and
                           ``concurrent`` that were asked for.  ``pna_statistics``, ``layer_forward``, ``layer_score_forward`` and
                           ``rspmm_forward_csr`` push no launch record: for them the only evidence that the geometry ran is that
                           ``ultra_rspmm_reserve_cus`` returned 0 in the same process in which the recorded families show it.

Row counts come from the launchers' own rules (kCbWaves = 4 waves of 32-row tiles per workgroup):
  6 149 = 32 * 8 * 8 * 3 + 5   combine_kernel's 2 * n_cu workgroups: three tiles per wave and a tail; six for the grids capped at n_cu
  4 064 / 4 097                127 and 129 tiles: either side of ``prefetch = n_tiles >= n_cu * 4 * 4`` at 8 compute units
  8 160 / 8 193, 12 293        the PF = true forms further in: eight and twelve tiles per wave
"""

import numpy as np
import pytest
import torch

import exact_grid as XG
import test_combine_paired_gpu as CP
import test_exact_grid_gpu as EG
import test_launch_paths_gpu as LP
import test_memory_bounds_gpu as MB
import test_pna_gpu as PG
import test_query_train_gpu as QT
import test_row_per_lane_gpu as RPL
from cu_count import CU_COUNTS, compute_units, expected_geometry, total_compute_units
from graphs import random_graph
from oracle_ops import OracleFunctional
from query_grad_definition import score_backward_numpy

pytestmark = pytest.mark.gpu

SMALL = 8
ROWS = 32 * 8 * 8 * 3 + 5
COMBINE_ROWS = [ROWS, 32 * 127, 32 * 128 + 1, 32 * 255, 32 * 256 + 1, 12293]
_memo = {}


def _dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


def _same_bits(got, want, what):
    got, want = MB._flat(got), MB._flat(want)
    assert len(got) == len(want), what
    for k, (g, w) in enumerate(zip(got, want)):
        assert g.shape == w.shape and g.dtype == w.dtype, (what, k)
        same = MB._bits(g) == MB._bits(w)
        assert bool(same.all()), "%s: output %d differs from the default-count run in %d of %d elements" % (what, k, int((~same).sum()), same.numel())


def _at_both(fn, what, n_cu=SMALL):
    """``fn()`` at the default count and at ``n_cu``: the same bits in every output; returns the result at ``n_cu``."""
    default = fn()
    torch.cuda.synchronize()
    with compute_units(n_cu):
        small = fn()
        torch.cuda.synchronize()
    _same_bits(small, default, what)
    return small


def _divisor(n, lo, hi):
    """The smallest divisor of ``n`` in [lo, hi]."""
    for d in range(lo, hi + 1):
        if n % d == 0:
            return d
    raise AssertionError((n, lo, hi))


# ==================================================================================================== dense forwards at 8 CUs
@pytest.mark.parametrize("alias", [False, True], ids=["separate_out", "out_is_update"])
@pytest.mark.parametrize("knob", [0, 256, 512, 512 | 2048])
@pytest.mark.parametrize("rows", COMBINE_ROWS)
def test_combine_forward(rows, knob, alias):
    """The plain epilogue in each of its kernels: as dispatched, the one-wave kernel (PF false below 128 tiles at 8 compute units,
    true from there), the paired row-per-lane form and its column-per-lane form."""
    from ultra_torchdrug_amd import _lib
    ops = CP._on_device(rows, "normal")
    forms = []

    def run():
        out = CP._run(knob, *ops, True, True, True, alias)
        forms.append(_lib.combine_forward_last_form())
        return out

    got = _at_both(run, "combine_forward rows %d knob %d" % (rows, knob))
    prefetch = -(-rows // 32) >= SMALL * 4 * 4
    if knob & 256 or not (prefetch or knob & 512):
        want_form = "combine_kernel"
    else:
        want_form = "combine_paired_kernel_lds" if knob & 2048 else "combine_paired_kernel"
    assert forms[1] == want_form, forms
    assert np.array_equal(got.cpu().numpy(), CP._oracle(rows, "normal", True, True, True).numpy())


@pytest.mark.parametrize("rows", [ROWS, 32 * 127, 32 * 128 + 1, 12293])
def test_combine_forward_with_z_out_and_with_a_boundary_input(rows):
    """``combine_kernel<PF, 0, true>`` (the training forward that keeps the Linear's output) and the boundary forms
    ``<PF, 1>`` (up to 128 queries: node and value in LDS) and ``<PF, 2>``, PF false at 4 064 rows and true at the others."""
    from ultra_torchdrug_amd import _lib, functional as UF
    x, u, w, b, gamma, beta = CP._on_device(rows, "normal")
    x_h, u_h, w_h, b_h, gamma_h, beta_h = CP._operands(rows, "normal")

    def run_z():
        z = torch.empty_like(x)
        out = UF.combine_forward(x, u, w, b, gamma, beta, 1e-5, True, True, z_out=z)
        assert _lib.combine_forward_last_form() == "combine_kernel"
        return [out, z]

    out, z = _at_both(run_z, "combine_forward z_out rows %d" % rows)
    assert np.array_equal(out.cpu().numpy(), CP._oracle(rows, "normal", True, True, True).numpy())
    assert np.array_equal(z.cpu().numpy(), CP._oracle(rows, "normal", False, False, False).numpy()), "z is the Linear in the kernel's order"
    for n_query in (_divisor(rows, 2, 128), _divisor(rows, 129, rows)):
        n_node = rows // n_query
        node = ((torch.arange(n_query) * 7) % n_node).to(torch.int32)
        value = x_h[:n_query].contiguous()
        boundary = (node.to(_dev()), value.to(_dev()))
        update = u.view(n_node, n_query, 64)

        def run_b():
            out = UF.combine_forward(None, update, w, b, gamma, beta, 1e-5, True, True, input_boundary=boundary)
            assert _lib.combine_forward_last_form() == "combine_kernel"
            return out

        got = _at_both(run_b, "combine_forward boundary rows %d queries %d" % (rows, n_query))
        dense = torch.zeros(n_node, n_query, 64)
        dense[node.long(), torch.arange(n_query)] = value
        with torch.no_grad():
            want = OracleFunctional(None).combine(dense.view(rows, 64), u_h, w_h, b_h, gamma_h, beta_h, 1e-5, True, True)
        assert np.array_equal(got.view(rows, 64).cpu().numpy(), want.numpy()), n_query


@pytest.mark.parametrize("k,relu", [(64, True), (128, False)], ids=["64_to_64", "128_to_128"])
def test_linear_forward(oracle, k, relu):
    """``linear_kernel<64>`` and ``<128>``: at most n_cu workgroups, six tiles per wave and a tail."""
    from ultra_torchdrug_amd import functional as UF
    gen = torch.Generator().manual_seed(ROWS + k)
    x, w, b = torch.randn(ROWS, k, generator=gen), torch.randn(k, k, generator=gen) / k ** 0.5, torch.randn(k, generator=gen)
    ops = [t.to(_dev()) for t in (x, w, b)]
    got = _at_both(lambda: UF.linear_forward(*ops, relu=relu), "linear_forward %d" % k)
    assert np.array_equal(got.cpu().numpy(), oracle.linear_forward(x.numpy(), w.numpy(), b.numpy(), relu))


@pytest.mark.parametrize("knob", [0, 1024])
@pytest.mark.parametrize("n_node,batch", [(ROWS, 1), (2050, 3), (88, 70)])
def test_score_all_entities(n_node, batch, knob):
    """``score_kernel<false>``, ``<true>`` (more than kScoreLdsBatch = 64 queries) and ``score_kernel_lds`` (knob bit 10)."""
    ops = tuple(_t(a) for a in RPL._operands(n_node, batch, "normal"))
    got = _at_both(lambda: RPL._run(knob, ops), "score_all_entities (%d, %d) knob %d" % (n_node, batch, knob))
    assert np.array_equal(got.cpu().numpy(), RPL._oracle(n_node, batch, "normal"))


def _projection_case(n_layers, kind="normal"):
    """``(relation (13, 473, 64), flat weights, table gradients)`` on the host: 6 149 rows."""
    key = ("projection", n_layers, kind)
    if key not in _memo:
        batch, n_rel = 13, 473
        if kind == "grid":
            rng = np.random.default_rng(n_layers)
            g = lambda *shape: torch.from_numpy(XG.grid(rng, shape, q=2, lim=2))
            relation = g(batch, n_rel, 64)
            flat = [g(*shape) for _ in range(n_layers) for shape in ((64, 64), (64,), (64, 64), (64,))]
            grads = [g(n_rel, batch * 64) for _ in range(n_layers)]
        else:
            gen = torch.Generator().manual_seed(100 + n_layers)
            relation = torch.randn(batch, n_rel, 64, generator=gen)
            flat = []
            for _ in range(n_layers):
                flat += [torch.randn(64, 64, generator=gen) * 0.2, torch.randn(64, generator=gen) * 0.1,
                         torch.randn(64, 64, generator=gen) * 0.2, torch.randn(64, generator=gen) * 0.1]
            grads = [torch.randn(n_rel, batch * 64, generator=gen) for _ in range(n_layers)]
        _memo[key] = (relation, flat, grads)
    return _memo[key]


def _group(ts):
    return [tuple(ts[4 * l:4 * l + 4]) for l in range(len(ts) // 4)]


@pytest.mark.parametrize("n_layers", [1, 3])
def test_relation_project(n_layers):
    """``project_kernel``: ceil(2 * n_cu / layers) workgroups per layer, 16 and 6 at 8 compute units."""
    from ultra_torchdrug_amd import functional as UF
    relation, flat, _ = _projection_case(n_layers)
    rel_d, flat_d = relation.to(_dev()), [t.to(_dev()) for t in flat]
    got = _at_both(lambda: [UF.relation_project(rel_d, _group(flat_d)), UF.relation_project(rel_d, _group(flat_d), repeat=2)],
                   "relation_project %d" % n_layers)
    with torch.no_grad():
        want = OracleFunctional(None).relation_project(relation, _group(flat))
    for table, twice, w in zip(got[0], got[1], want):
        assert np.array_equal(table.cpu().numpy(), w.numpy()) and torch.equal(twice, torch.cat([table, table], dim=1))


def test_pna_combine_forward():
    """``pna_combine_kernel``: ``grid = min(n_tiles, n_cu)`` and a double-buffered ``tile += gridDim.x``.  1 541 rows = 32 * 8 * 6
    + 5: six tiles per workgroup and a tail.  The bar of tests/test_pna_gpu.py against the fp64 definition at 8 compute units,
    and the default run's bits."""
    from ultra_torchdrug_amd import functional as UF
    rows, n_query = 32 * 8 * 6 + 5, 3
    with compute_units(SMALL):
        PG.test_epilogue_is_as_close_to_the_fp64_definition_as_aten_in_fp32(rows, n_query)
    x, stats, degree = PG._epilogue_case(rows, n_query, 77)
    gen = torch.Generator().manual_seed(78)
    w = (torch.randn(64, 832, generator=gen) / 832 ** 0.5).to(_dev())
    b, gamma, beta = (torch.randn(64, generator=gen).to(_dev()) * s + o for s, o in ((0.1, 0.0), (0.1, 1.0), (0.1, 0.0)))
    table = UF.pna_node_table(degree)
    for shortcut in (False, True):
        _at_both(lambda: UF.pna_combine_forward(x[:rows], [s[:rows] for s in stats], table, w, b, gamma, beta, 1e-5, relu=True,
                                                shortcut=shortcut, n_query=n_query), "pna_combine_forward")


def _hub_source_graph(n, r, n_query):
    """1 200 nodes; the first ``n_query`` nodes have an edge to every node but the last ten, so a first layer whose boundary nodes
    they are lists almost every (node, query) row: 7 140 rows = 224 tiles for the 2 * n_cu workgroups of the listed epilogue."""
    g = random_graph(seed=5, n_node=n, n_edge=4000, n_rel=r, unique=True)
    hubs = np.repeat(np.arange(n_query), n - 10)
    every = np.tile(np.arange(n - 10), n_query)
    rel = (every + hubs) % r
    dst, src, rels = np.concatenate([g["dst"], every]), np.concatenate([g["src"], hubs]), np.concatenate([g["rel"], rel])
    key = (dst * n + src) * r + rels
    _, first = np.unique(key, return_index=True)
    first.sort()
    return dict(dst=dst[first], src=src[first], rel=rels[first], w=None)


def test_listed_first_layer(oracle, monkeypatch):
    """``first_layer_forward``: the frontier's rows listed, then ``combine_kernel<false, 3>`` on a grid of 2 * n_cu workgroups
    over the list.  The oracle's rspmm over the dense boundary + epilogue (tests/test_memory_bounds_gpu.py), bit for bit."""
    from ultra_torchdrug_amd import RelCSR, functional as UF
    monkeypatch.setattr(UF, "SPARSE_FIRST_LAYER_MIN_ROWS", 0)
    n, r, Q = 1200, 9, 6
    g = _hub_source_graph(n, r, Q)
    _, relation, _, b_value, params, _ = MB._layer_operands(31, n, r, Q)
    b_node = np.arange(Q, dtype=np.int32)[::-1].copy()
    dense = OracleFunctional._dense_boundary((torch.from_numpy(b_node), torch.from_numpy(b_value)), n).numpy().reshape(n, Q, 64)
    _, want = MB._oracle_layer(oracle, g, n, r, 128, relation, dense, (b_node, b_value), params, True, True)
    csr = RelCSR(_t(g["dst"]), _t(g["src"]), _t(g["rel"]), None, n, n, r, piece_len=128)
    ops = [_t(a) for a in (relation, b_node, b_value, *params)]

    def run():
        listed = UF.first_layer_forward(csr, ops[0], (ops[1], ops[2]), *ops[3:], 1e-5, True, True, want_list=True)
        assert listed is not None, "the listed first layer declined"
        out, row_list, count = listed
        assert int(count) > 32 * 2 * SMALL * 4 * 3, "the list must give every wave of the 8-CU grid three tiles"
        return out

    got = _at_both(run, "first_layer_forward")
    assert np.array_equal(got.cpu().numpy(), want)


def test_fused_layer_and_layer_score():
    """``layer_forward`` / ``layer_score_forward`` (csrc/layer_fused.hip: rowgroup_tiling on n_cu) at 8, 24 and 240 compute units:
    the default run's bits, which tests/test_layer_fused_gpu.py holds to rspmm + epilogue (+ score head).  (The entries push no
    launch record: that the geometry ran rests on the setting's status, module docstring.)"""
    from ultra_torchdrug_amd import RelCSR, functional as UF
    for n, e, r, n_query, knob in ((2500, 20000, 30, 3, 0), (1501, 12000, 40, 16, 16)):        # 3 tiles of 64; 4 tiles of 256 columns
        g = random_graph(seed=n, n_node=n, n_edge=e, n_rel=r)
        csr = RelCSR(_t(g["dst"]), _t(g["src"]), _t(g["rel"]), None, n, n, r, wide_ids=True, piece_len=512)
        assert csr.fwd.row_ptr is not None and csr.fwd.n_pieces == 0
        x, relation, b_node, b_value, params, head = MB._layer_operands(n, n, r, n_query)
        ops = [_t(a) for a in (relation, x, b_node, b_value, *params, *head)]

        def run():
            rel_t, x_t, node, value, w, b, gamma, beta, *head_t = ops
            with MB._knob(knob):
                out = UF.layer_forward(csr, rel_t, x_t, (node, value), w, b, gamma, beta, 1e-5, True, True)
                score = UF.layer_score_forward(csr, rel_t, x_t, (node, value), w, b, gamma, beta, 1e-5, True, True, *head_t)
                update = UF.rspmm_forward(csr, rel_t, x_t.flatten(1), "add", "mul", boundary=(node, value)).view(n, n_query, 64)
                two = UF.combine_forward(x_t, update, w, b, gamma, beta, 1e-5, True, True)
            assert out is not None and (score is not None or n_query > 32)
            assert torch.equal(out, two)
            return [out] + ([score] if score is not None else [])

        default = run()
        for n_cu in CU_COUNTS:
            with compute_units(n_cu):
                _same_bits(run(), default, "fused layer at %d compute units" % n_cu)


# ==================================================================================================== block-partial reducers
def _combine_chain(leaves, ln):
    x, u, w, b, gamma, beta = leaves
    pre = torch.nn.functional.linear(torch.cat([x, u], dim=-1), w, b)
    if ln:
        pre = torch.nn.functional.layer_norm(pre, (64,), gamma, beta, 1e-5)
    return pre


def _combine_normal_case():
    """Seeded normals with LayerNorm: ``(gout, fp64 gradients, fp32 ATen gradients)`` of cat -> Linear -> LayerNorm -> relu
    (+ input).  Rows with a pre-activation within 1e-4 of 0 get a zero output gradient (relu is not differentiable there)."""
    key = ("combine", "normal")
    if key not in _memo:
        ops = CP._operands(ROWS, "normal")
        gout = torch.randn(ROWS, 64, generator=torch.Generator().manual_seed(ROWS))
        grads = {}
        for dtype in (torch.float64, torch.float32):
            leaves = [t.detach().clone().to(dtype).requires_grad_() for t in ops]
            pre = _combine_chain(leaves, True)
            if dtype == torch.float64:
                gout[(pre.detach().abs() < 1e-4).any(dim=1)] = 0.0
            (torch.relu(pre) + leaves[0]).backward(gout.to(dtype))
            grads[dtype] = [t.grad.double() for t in leaves]
        _memo[key] = (gout, grads[torch.float64], grads[torch.float32])
    return _memo[key]


def _combine_grid_case():
    """Exact-grid operands without LayerNorm and the fp64 definition of ``relu(Linear(cat[x, u])) + x`` with its gradients.
    Operands are multiples of 1/4 of size at most 2, so z and d_input / d_update are sums of multiples of 1/16, d_weight of
    multiples of 1/16 over 6 149 rows, d_bias of multiples of 1/4: ``assert_exact`` proves each below 2^24 units from the sums
    of the |terms|, and the fp64 results round-trip through float32."""
    key = ("combine", "grid")
    if key not in _memo:
        x, u, w, b = (t.numpy().astype(np.float64) for t in CP._operands(ROWS, "grid")[:4])
        gout = XG.grid(np.random.default_rng(ROWS), (ROWS, 64)).astype(np.float64)
        cat = np.concatenate([x, u], axis=1)
        z = cat @ w.T + b                      # (exact zeros occur: the relu passes gradient where z > 0, as ATen's does)
        d_z = np.where(z > 0, gout, 0.0)
        want = [np.maximum(z, 0.0) + x, d_z @ w[:, :64] + gout, d_z @ w[:, 64:], d_z.T @ cat, d_z.sum(axis=0)]
        a_z = np.abs(gout)
        XG.assert_exact(np.abs(cat) @ np.abs(w).T + np.abs(b), 2.0 ** -4)
        XG.assert_exact(a_z @ np.abs(w[:, :64]) + np.abs(gout), 2.0 ** -4)
        XG.assert_exact(a_z @ np.abs(w[:, 64:]), 2.0 ** -4)
        XG.assert_exact(a_z.T @ np.abs(cat), 2.0 ** -4)
        XG.assert_exact(a_z.sum(axis=0), 2.0 ** -2)
        for t in want:
            assert np.array_equal(t.astype(np.float32).astype(np.float64), t)
        _memo[key] = (gout.astype(np.float32), want)
    return _memo[key]


def _run_combine(ops, gout, ln):
    from ultra_torchdrug_amd import functional as UF
    with torch.enable_grad():
        leaves = [t.detach().requires_grad_() for t in (ops if ln else ops[:4])]
        out = UF.combine(*leaves, *([] if ln else [None, None]), 1e-5, True, True)
        out.backward(gout)
    torch.cuda.synchronize()
    return [out.detach()] + [t.grad for t in leaves]


COMBINE_NAMES = ["out", "d_input", "d_update", "d_weight", "d_bias", "d_ln_weight", "d_ln_bias"]
COMBINE_MODES = [("fused", False), ("split", False), ("fused", True)]
COMBINE_MODE_IDS = ["fused", "split", "fused_keep_pre_norm"]


def _bound(got, truth, aten, floor, what):
    """The project's rule: within ``4 * ref_dev + floor * scale`` of the fp64 chain, ``ref_dev`` the fp32 ATen chain's deviation."""
    scale = float(truth.abs().max())
    err, ref_dev = float((got.double().cpu() - truth).abs().max()), float((aten - truth).abs().max())
    print("%s: HIP %.3g, ATen fp32 %.3g away from fp64; scale %.3g; bound %.3g" % (what, err, ref_dev, scale, 4 * ref_dev + floor * scale))
    assert err <= 4 * ref_dev + floor * scale, (what, err, ref_dev, scale)


@pytest.mark.parametrize("mode,keep", COMBINE_MODES, ids=COMBINE_MODE_IDS)
def test_combine_backward_on_seeded_normals(monkeypatch, mode, keep):
    """``combine_fused_backward_kernel`` (slabs = workgroups <= n_cu, reduced by a second kernel) and the three-kernel form
    (``combine_backward_kernel``, ``linear_wgrad_kernel``, ``dxdu_kernel``; Python sizes their partials from the wave counts the
    library returns).  Floor 2e-5: tests/test_memory_bounds_gpu.py ``_close``.  Measured on an MI355X, worst over the three
    forms and 8 / 256 compute units: d_weight 1.08e-4 away from fp64 (ATen fp32 1.17e-4, scale 350, bound 7.5e-3), d_bias
    1.2e-5 (1.4e-5, 73, 1.5e-3), d_ln_weight 3.5e-5 (3.7e-5, 150, 3.1e-3), d_ln_bias 1.8e-5 (4.1e-5, 132, 2.8e-3): never above
    the fp32 ATen chain's own deviation, 1.4 % of the bound at most."""
    from ultra_torchdrug_amd import functional as UF
    monkeypatch.setenv("ULTRA_COMBINE_BWD", mode)
    monkeypatch.setattr(UF, "KEEP_PRE_NORM", keep)
    gout, truth, aten = _combine_normal_case()
    ops, gout_d = CP._on_device(ROWS, "normal"), gout.to(_dev())
    default = _run_combine(ops, gout_d, True)
    with compute_units(SMALL):
        small = _run_combine(ops, gout_d, True)
    _same_bits(small[:3], default[:3], "combine backward %s: row outputs" % mode)
    for tag, got in (("256", default), ("8", small)):
        for name, g, t, a in zip(COMBINE_NAMES[1:], got[1:], truth, aten):
            _bound(g, t, a, 2e-5, "combine backward %s at %s CUs %s" % (mode, tag, name))


@pytest.mark.parametrize("mode,keep", COMBINE_MODES, ids=COMBINE_MODE_IDS)
def test_combine_backward_on_the_exact_grid(monkeypatch, mode, keep):
    """Every partial sum is exact, so every compute-unit count gives the fp64 definition, whatever the number of partials."""
    from ultra_torchdrug_amd import functional as UF
    monkeypatch.setenv("ULTRA_COMBINE_BWD", mode)
    monkeypatch.setattr(UF, "KEEP_PRE_NORM", keep)
    gout, want = _combine_grid_case()
    ops, gout_d = CP._on_device(ROWS, "grid"), _t(gout)
    runs = {"default": _run_combine(ops, gout_d, False)}
    for n_cu in CU_COUNTS:
        with compute_units(n_cu):
            runs[n_cu] = _run_combine(ops, gout_d, False)
    for tag, got in runs.items():
        for name, g, w in zip(COMBINE_NAMES, got, want):
            assert np.array_equal(g.cpu().numpy().astype(np.float64), w), "combine backward %s at %s compute units: %s" % (mode, tag, name)


def _projection_chain(x, ws):
    lin = torch.nn.functional.linear
    pres = [lin(x, w1, b1) for w1, b1, _, _ in ws]
    tables = [lin(torch.relu(pre), w2, b2).transpose(0, 1).flatten(1) for pre, (_, _, w2, b2) in zip(pres, ws)]
    return pres, tables


def _projection_abs_sums(n_layers):
    """Per output of the projection backward on the grid, the sum of the |terms| of every sum it is made of: the same chain on
    the absolute operands (all non-negative, so the relu passes everything and every product enters with its size).  Any partial
    sum any implementation forms, in any association, is bounded by these."""
    relation, flat, grads = _projection_case(n_layers, "grid")
    x = relation.detach().double().abs().requires_grad_()
    ws = [t.detach().double().abs().requires_grad_() for t in flat]
    pres, tables = _projection_chain(x, _group(ws))
    sum((t * g.double().abs()).sum() for t, g in zip(tables, grads)).backward()
    return [p.detach() for p in pres] + [t.detach() for t in tables], [x.grad] + [t.grad for t in ws]


def _projection_reference(n_layers, kind):
    """fp64 (and fp32) autograd of the reference chain nn.Linear, relu, nn.Linear, transpose.  A table row whose hidden
    pre-activations come within 1e-4 of 0 receives no gradient (relu is not differentiable there); on the grid, where exact zeros
    are frequent and every precision computes the same pre-activation, the relu passes gradient where it is > 0 (ATen's rule)."""
    key = ("projection reference", n_layers, kind)
    if key not in _memo:
        relation, flat, grads = _projection_case(n_layers, kind)
        grads = [g.clone() for g in grads]
        out = {}
        for dtype in (torch.float64, torch.float32):
            x = relation.detach().clone().to(dtype).requires_grad_()
            ws = [t.detach().clone().to(dtype).requires_grad_() for t in flat]
            pres, tables = _projection_chain(x, _group(ws))
            if dtype == torch.float64:
                for pre, g in zip(pres, grads):
                    if kind == "normal":
                        near = (pre.detach().abs() < 1e-4).any(dim=-1)                       # (B, R)
                        g.view(g.shape[0], -1, 64)[near.t()] = 0.0
            sum((t * g.to(dtype)).sum() for t, g in zip(tables, grads)).backward()
            out[dtype] = [x.grad.double()] + [t.grad.double() for t in ws]
        _memo[key] = (grads, out[torch.float64], out[torch.float32])
    return _memo[key]


def _run_projection(relation, flat, grads):
    from ultra_torchdrug_amd import functional as UF
    with torch.enable_grad():
        x = relation.detach().requires_grad_()
        leaves = [t.detach().requires_grad_() for t in flat]
        tables = UF.relation_project_train(x, _group(leaves))
        sum((t * g).sum() for t, g in zip(tables, grads)).backward()
    torch.cuda.synchronize()
    return [x.grad] + [t.grad for t in leaves]


@pytest.mark.parametrize("n_layers", [1, 3])
def test_relation_project_backward(n_layers):
    """``project_bwd_kernel`` + reduce: at most ceil(n_cu / layers) workgroups per layer.  (b) seeded normals, floor 2e-5
    (tests/test_frontier_sampler_gpu.py); measured worst over 8 / 256 compute units: a d_w1 1.65e-4 away from fp64 (ATen fp32
    8.2e-5, scale 372, bound 7.8e-3), d_relation 2.9e-6 (2.8e-6, 12.1, 2.5e-4): 2.1 % of the bound at most.  (a) the exact
    grid: operands multiples of 1/2 of size at most 1, so hidden values are multiples of 1/4 up to 64.5, a d_w2 term a multiple
    of 1/8 up to 64.5 (3.2 M units over 6 149 rows), a d_w1 term likewise: below 2^24 units in the worst case, and asserted from
    the sums of the |terms| of every output (``_projection_abs_sums``)."""
    for kind in ("normal", "grid"):
        relation, flat, _ = _projection_case(n_layers, kind)
        grads, truth, aten = _projection_reference(n_layers, kind)
        ops = (relation.to(_dev()), [t.to(_dev()) for t in flat], [g.to(_dev()) for g in grads])
        if kind == "grid":          # hidden 1/4, tables and every gradient term 1/8: each sum of |terms| below 2^24 units
            forward, backward = _projection_abs_sums(n_layers)
            for t in forward + backward:
                XG.assert_exact(t.numpy(), 2.0 ** -3)
        runs = {"default": _run_projection(*ops)}
        for n_cu in (CU_COUNTS if kind == "grid" else (SMALL,)):
            with compute_units(n_cu):
                runs[n_cu] = _run_projection(*ops)
            _same_bits(runs[n_cu][:1], runs["default"][:1], "relation_project backward: d_relation")
        for tag, got in runs.items():
            for k, (g, t, a) in enumerate(zip(got, truth, aten)):
                what = "relation_project backward %s at %s compute units, output %d" % (kind, tag, k)
                if kind == "grid":
                    assert np.array_equal(t.float().double().numpy(), t.numpy())
                    assert np.array_equal(g.double().cpu().numpy(), t.numpy()), what
                else:
                    _bound(g, t, a, 2e-5, what)


def _head_case(n_node, batch, kind):
    """``(hidden, query, w1, b1, w2, b2, grad)`` on the host and the fp64 definition of the score head's backward.  ``grid``:
    multiples of 1/2 of size at most 1 -- a pre-activation is a multiple of 1/4 up to 129, a d_w2 term a multiple of 1/8 up to
    129 (6.4 M units over 6 150 rows), a d_w1 / d_query term a multiple of 1/8 up to 1: all below 2^24 units in the worst
    case, which the test asserts from the sums of the |terms|; the relu passes gradient where the pre-activation is > 0
    (score_backward_numpy).  ``normal``: entities with a pre-activation within 1e-4 of 0 get
    a zero gradient."""
    key = ("head", n_node, batch, kind)
    if key not in _memo:
        rng = np.random.default_rng(n_node + batch)
        if kind == "grid":
            g = lambda *shape: XG.grid(rng, shape, q=2, lim=2)
            case = [g(n_node, batch, 64), g(batch, 64), g(128, 128), g(128), g(128), g(1), XG.grid(rng, (batch, n_node), q=2, lim=2, zero=0.0)]
        else:
            hidden, query, w1, b1, w2, b2 = RPL._operands(n_node, batch, "normal")
            case = [hidden, query, w1, b1, w2.reshape(128), b2, rng.standard_normal((batch, n_node)).astype(np.float32)]
        hidden, query, w1, b1 = (a.astype(np.float64) for a in case[:4])
        x = np.concatenate([hidden, np.broadcast_to(query[None], (n_node, batch, 64))], axis=2)
        pre = x @ w1.T + b1
        if kind == "normal":
            case[6][:, (np.abs(pre) < 1e-4).any(axis=(1, 2))] = 0.0
        truth = score_backward_numpy(*case[:5], case[6])
        if kind == "grid":
            a_grad, a_w2, a_w1 = np.abs(case[6].astype(np.float64)), np.abs(case[4].astype(np.float64)), np.abs(w1)
            a_pre = a_grad.T[:, :, None] * a_w2[None, None, :]                                   # |d_pre| wherever the relu passes
            XG.assert_exact(np.abs(x) @ a_w1.T + np.abs(b1), 2.0 ** -2)
            XG.assert_exact(a_pre @ a_w1, 2.0 ** -3)                                             # d_hidden, and per entity d_query
            XG.assert_exact((a_pre @ a_w1)[:, :, 64:].sum(axis=0), 2.0 ** -3)                    # d_query
            XG.assert_exact(np.einsum("nbo,nbk->ok", a_pre, np.abs(x)), 2.0 ** -3)               # d_w1
            XG.assert_exact(a_pre.sum(axis=(0, 1)), 2.0 ** -2)                                   # d_b1
            XG.assert_exact(np.einsum("bn,nbo->o", a_grad, np.abs(pre)), 2.0 ** -3)              # d_w2
            XG.assert_exact(a_grad.sum(), 2.0 ** -1)                                             # d_b2
            for t in truth:
                assert np.array_equal(np.asarray(t).astype(np.float32).astype(np.float64), t)
        _memo[key] = (case, truth)
    return _memo[key]


@pytest.mark.parametrize("n_node,batch", [(ROWS, 1), (2050, 3)])
def test_score_all_backward(n_node, batch):
    """``score_backward_kernel``: ceil(n_cu / batch) workgroups per query, the workspace sized from the same rule by
    ``ultra_score_backward_workspace``.  (a) exact grid, every count; (b) seeded normals under the bar of
    tests/test_query_train_gpu.py (``4 * e_aten + 1e-5 * scale``); measured worst at 8 / 256 compute units: d_w2 1.11e-4 away from
    fp64 (ATen fp32 1.17e-4, scale 318), d_b2 1.4e-5 (6.3e-6, 38.8), d_hidden 2.4e-7 (1.8e-7, 0.58): 3.8 % of the bound at most."""
    from ultra_torchdrug_amd import functional as UF
    for kind in ("grid", "normal"):
        case, truth = _head_case(n_node, batch, kind)
        hidden, query, w1, b1, w2, b2, grad = QT._head_tensors(case)

        def run():
            outs = UF.score_all_backward(hidden, query, w1, b1, w2, grad)
            torch.cuda.synchronize()
            return list(outs)

        runs = {"default": run()}
        for n_cu in (CU_COUNTS if kind == "grid" else (SMALL,)):
            with compute_units(n_cu):
                runs[n_cu] = run()
            _same_bits(runs[n_cu][:1], runs["default"][:1], "score_all_backward: d_hidden")
        aten = QT._aten_head(hidden, query, w1, b1, w2, b2, grad) if kind == "normal" else None
        for tag, got in runs.items():
            for k, (name, g, t) in enumerate(zip(QT.HEAD_NAMES, got, truth)):
                what = "score_all_backward %s (%d, %d) at %s compute units: %s" % (kind, n_node, batch, tag, name)
                if kind == "grid":
                    assert np.array_equal(g.cpu().numpy().astype(np.float64).reshape(np.shape(t)), t), what
                else:
                    QT._bars(g.reshape(-1).cpu(), aten[k].reshape(-1).cpu(), torch.from_numpy(np.asarray(t)).reshape(-1), what)


FIRST_LAYER = (1200, 9, 6)          # nodes, relations, queries of the hub-source graph: 7 140 listed rows
FIRST_LAYER_NAMES = ("d_relation", "d_boundary_value", "d_weight", "d_bias", "d_ln_weight", "d_ln_bias")


def _first_layer_chain(leaves, g, ln):
    """The first layer written with index_add: ``(pre-activation, dense boundary)`` for leaves ``relation, b_value, w, b[, gamma,
    beta]`` in the leaves' dtype; the boundary node of query ``q`` is hub ``Q - 1 - q``."""
    n, r, Q = FIRST_LAYER
    rel_l, bv, w, b = leaves[:4]
    dst, src, rel = (torch.from_numpy(g[k]) for k in ("dst", "src", "rel"))
    dense = torch.zeros(n, Q, 64, dtype=bv.dtype).index_put((torch.arange(Q).flip(0), torch.arange(Q)), bv, accumulate=True)
    flat = dense.flatten(1)
    update = torch.zeros(n, Q * 64, dtype=bv.dtype).index_add(0, dst, rel_l[rel] * flat[src]) + flat
    pre = torch.nn.functional.linear(torch.cat([dense, update.view(n, Q, 64)], dim=-1), w, b)
    if ln:
        pre = torch.nn.functional.layer_norm(pre, (64,), leaves[4], leaves[5], 1e-5)
    return pre, dense


def _first_layer_runner(monkeypatch, g, host_leaves, gout):
    """``run()``: ``functional.sum_layer`` with the first-layer promise on the device, forward and backward; asserts that the
    sparse training form was taken.  Returns ``[out] + gradients of the leaves``."""
    from ultra_torchdrug_amd import RelCSR, functional as UF
    monkeypatch.setattr(UF, "SPARSE_FIRST_LAYER_MIN_ROWS", 0)
    monkeypatch.setattr(UF, "SPARSE_FIRST_LAYER_TRAIN_MAX_FRACTION", 1.0)
    taken = []
    real = UF.first_layer_train_forward
    monkeypatch.setattr(UF, "first_layer_train_forward", lambda *a, **k: taken.append(real(*a, **k)) or taken[-1])
    n, r, Q = FIRST_LAYER
    csr = RelCSR(_t(g["dst"]), _t(g["src"]), _t(g["rel"]), None, n, n, r, piece_len=128)
    ops = [t.to(_dev()) for t in host_leaves]
    node_d, gout_d = torch.arange(Q).flip(0).to(_dev()), gout.to(_dev())

    def run():
        with torch.enable_grad():
            leaves = [t.detach().requires_grad_() for t in ops]
            rel_l, bv, w, b = leaves[:4]
            gamma, beta = leaves[4:] if len(leaves) == 6 else (None, None)
            dense = torch.zeros(n, Q, 64, device=_dev()).index_put((node_d, torch.arange(Q, device=_dev())), bv, accumulate=True)
            out = UF.sum_layer(csr, rel_l, dense, dense, (node_d.to(torch.int32), bv), "mul", w, b, gamma, beta, 1e-5, True, True,
                               input_is_boundary=True)
            out.backward(gout_d)
        torch.cuda.synchronize()
        assert taken and taken[-1] is not None, "the layer did not take the sparse training form"
        return [out.detach()] + [t.grad for t in leaves]

    return run


def test_first_layer_training_backward(monkeypatch):
    """``functional.sum_layer`` on the first layer of the hub-source graph of ``test_listed_first_layer``: 7 140 listed rows,
    compacted and run through combine_fused_backward_kernel's slabs by ``ultra_first_layer_epilogue_backward_f32`` -- 224 tiles
    for the 32 waves of an 8-CU grid.  The output, ``d_relation`` and ``d_boundary_value`` (per row and per edge: no slab) carry
    the default run's bits; every gradient is within ``4 * ref_dev + 2e-5 * scale`` of fp64 autograd of the layer written with
    index_add (floor: tests/test_memory_bounds_gpu.py) at both counts.
    Measured: d_weight 7.1e-5 at 256 and 1.21e-4 at 8 compute units away from fp64 (ATen fp32 1.23e-4, scale 384, bound 8.2e-3);
    d_bias 3.9e-4 at both (ATen fp32 5.7e-5, scale 329, bound 6.8e-3: the unlisted rows' share comes from a column sum of its own
    that does not depend on the count) -- 5.7 % of the bound, the most any output uses."""
    n, r, Q = FIRST_LAYER
    g = _hub_source_graph(n, r, Q)
    _, relation, _, b_value, params, _ = MB._layer_operands(41, n, r, Q)
    host = [torch.from_numpy(a) for a in (relation, b_value, *params)]
    gout = torch.randn(n, Q, 64, generator=torch.Generator().manual_seed(42))
    grads = {}
    for dtype in (torch.float64, torch.float32):
        leaves = [t.clone().to(dtype).requires_grad_() for t in host]
        pre, dense = _first_layer_chain(leaves, g, True)
        if dtype == torch.float64:
            gout[(pre.detach().abs() < 1e-4).any(dim=-1)] = 0.0
        (torch.relu(pre) + dense).backward(gout.to(dtype))
        grads[dtype] = [t.grad.double() for t in leaves]
    run = _first_layer_runner(monkeypatch, g, host, gout)
    default = run()
    with compute_units(SMALL):
        small = run()
    _same_bits(small[:3], default[:3], "first layer in training: output, d_relation, d_boundary_value")
    for tag, got in (("256", default), ("8", small)):
        for name, gr, t, a in zip(FIRST_LAYER_NAMES, got[1:], grads[torch.float64], grads[torch.float32]):
            _bound(gr, t, a, 2e-5, "first layer in training at %s CUs %s" % (tag, name))


def test_first_layer_training_backward_on_the_exact_grid(monkeypatch):
    """The same layer without LayerNorm on operands that are multiples of 1/2 of size at most 1: an update entry is a multiple of
    1/4, a pre-activation, a d_weight, d_relation and d_boundary_value term a multiple of 1/8.  The sums of the |terms| of every
    output -- the same chain on the absolute operands, where the relu passes everything -- stay below 2^24 units, so every partial
    sum in any order is exact and 8, 24, 240 and the default count must all give the fp64 definition (the relu passes gradient
    where the pre-activation is > 0, as ATen's)."""
    n, r, Q = FIRST_LAYER
    g = _hub_source_graph(n, r, Q)
    rng = np.random.default_rng(43)
    host = [torch.from_numpy(XG.grid(rng, shape, q=2, lim=2)) for shape in ((r, Q * 64), (Q, 64), (64, 128), (64,))]
    gout = torch.from_numpy(XG.grid(rng, (n, Q, 64), q=2, lim=2))
    want = {}
    for tag, absolute in (("definition", False), ("abs", True)):
        leaves = [(t.double().abs() if absolute else t.double()).requires_grad_() for t in host]
        pre, dense = _first_layer_chain(leaves, g, False)
        out = torch.relu(pre) + dense
        out.backward(gout.double().abs() if absolute else gout.double())
        want[tag] = [out.detach()] + [t.grad for t in leaves]
    for t in want["abs"]:
        XG.assert_exact(t.numpy(), 2.0 ** -3)
    for t in want["definition"]:
        assert np.array_equal(t.float().double().numpy(), t.numpy())
    assert all(bool(t.any()) for t in want["definition"])
    run = _first_layer_runner(monkeypatch, g, host, gout)
    runs = {"default": run()}
    for n_cu in CU_COUNTS:
        with compute_units(n_cu):
            runs[n_cu] = run()
    for tag, got in runs.items():
        for name, gr, t in zip(("out",) + FIRST_LAYER_NAMES, got, want["definition"]):
            assert np.array_equal(gr.double().cpu().numpy(), t.numpy()), "first layer in training on the grid at %s compute units: %s" % (tag, name)


def test_first_layer_training_backward_between_guard_bands(monkeypatch):
    """The case of tests/test_memory_bounds_gpu.py as it stands -- fp64 autograd at 2e-5, guard bands around every allocation,
    the C entry with outputs carved by the test -- under the setting (about a hundred listed rows: no wave loops here; what is
    held is that the entry's workspace and the wave count it is sized from agree at 8 compute units)."""
    with compute_units(SMALL):
        MB.test_sparse_first_layer_in_training_with_its_epilogue_backward(monkeypatch)


# ==================================================================================================== guard bands
def test_reducers_between_guard_bands_at_8_compute_units_and_after(monkeypatch):
    """Every reducer at 8 compute units inside ``guarded_memory`` (ctypes binding: every output, partial buffer and workspace is
    allocated in functional.py, poisoned and banded), then at the default count after the context has exited.  A partial buffer
    sized under one setting and a launch under another would write past it, or leave poison in a slab the reduction adds."""
    from ultra_torchdrug_amd import functional as UF
    monkeypatch.setenv("ULTRA_BINDING", "ctypes")
    dev = _dev()
    gout, truth, aten = _combine_normal_case()
    ops = CP._on_device(ROWS, "normal")
    relation, flat, _ = _projection_case(3)
    p_grads = _projection_reference(3, "normal")[0]
    case, _ = _head_case(2050, 3, "normal")
    head = QT._head_tensors(case)

    def combine(gout, *ops):
        return _run_combine(ops, gout, True)

    def project(relation, *rest):
        return _run_projection(relation, list(rest[3:]), list(rest[:3]))

    def score(*head):
        return list(UF.score_all_backward(*head[:5], head[6]))

    p_truth, p_aten = _projection_reference(3, "normal")[1:]
    h_truth = _head_case(2050, 3, "normal")[1]
    h_aten = QT._aten_head(*head)

    def held(truth, aten, floor):
        def check(result, what):
            for k, (g, t, a) in enumerate(zip(MB._flat(result), truth, aten)):
                _bound(g.reshape(-1), torch.as_tensor(np.asarray(t)).reshape(-1).double(), a.detach().reshape(-1).double().cpu(), floor,
                       "%s, output %d" % (what, k))
        return check

    calls = []
    for mode in ("fused", "split"):
        calls.append(("combine " + mode, combine, [gout.to(dev), *ops], dict(ULTRA_COMBINE_BWD=mode), 3,
                      lambda result, what: held(truth, aten, 2e-5)(result[1:], what)))
    calls.append(("relation_project", project, [relation.to(dev)] + [t.to(dev) for t in p_grads + flat], {}, 1, held(p_truth, p_aten, 2e-5)))
    calls.append(("score_all_backward", score, head, {}, 1, held(h_truth, h_aten, 1e-5)))
    for what, fn, args, env, n_row_outputs, check in calls:
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        with compute_units(SMALL):
            small = MB.run_guarded(fn, *args, widest_row=512, what=what + " at 8 compute units")
        after = MB.run_guarded(fn, *args, widest_row=512, what=what + " after the context")
        _same_bits(small[:n_row_outputs], after[:n_row_outputs], what + ": row outputs")
        check(small, what + " at 8 compute units under the guard")           # (the bars of the tests above)
        check(after, what + " after the context under the guard")


# ==================================================================================================== plan families
# one row of tests/test_launch_paths_gpu.py per family and variant (graphs, calls and expected records are that file's)
PLAN_ROWS = [
    "quad_plain_lp_w", "quad_x_lds_lp_u", "dead_words", "masks_lp_act_u", "masks_first_layer",      # F = 128 / 192: 2 and 3 tiles
    "packed_var0_lp_w", "packed_var1_lp_u", "packed_var2_lp_rel700_w", "packed_var3_lp_u", "packed_F66",
    "general_lp_w", "general_lp_rel700_u",                                                            # relation tile in LDS / not; F = 64: 1 tile
    "rowgroup_g16_lds_r12_F256_w", "rowgroup_g32_lds_r12_F384_u",                                     # 4 tiles of 64, 3 of 128 columns
    "rotate_straddle_hub", "rotate_unit_weights",                                                     # sum, min and max; a split hub row
    "hub", "hub_rel",                                                                                 # fix-up plain and many; F = 64
    "alignment",                                                                                      # add_rows and the sparse boundary
    "concurrent_1024", "concurrent_4096",                                                             # 16 and 64 tiles
]
# The graphs of that file have at most a few hundred 32-edge chunks per plan, which one ticket per wave covers even with one
# workgroup per label.  This one has 12 000 drawn edges over F = 256 (4 tiles x 2 parts): at 8 compute units a workgroup serves a
# part's ~190 chunks alone, four per ticket -- about three tickets for each of its 16 waves; at 256 it draws two or three in all.
EG.GRAPHS["cu_tickets"] = (dict(n_edge=12000, unique=True), 500, 5, 256, False)
_TICKET_GEO = dict(n_tiles=4, split=2, n_slots=8)


def _ticket_rows():
    Q, P, G, FWD, DX, DREL, ADD, MUL, HDR = LP.Q, LP.P, LP.G, LP.FWD, LP.DX, LP.DREL, LP.ADD, LP.MUL, LP.HDR
    tbl = LP._tbl(5)
    quad = [LP.fwd("add", "mul", Q(FWD, ADD, MUL, 1, 0, lds=tbl, **_TICKET_GEO)),
            LP.fwd("max", "add", Q(FWD, "max", "add", 1, 0, lds=tbl, **_TICKET_GEO)),
            LP.bwd("add", "mul", Q(DX, ADD, MUL, 1, 0, lds=tbl, **_TICKET_GEO), Q(DREL, ADD, MUL, 1, 0, lds=HDR, **_TICKET_GEO))]
    packed = [LP.fwd("add", "mul", P(FWD, ADD, MUL, 1, 0, lds=tbl, **_TICKET_GEO)),
              LP.bwd("add", "mul", P(DX, ADD, MUL, 1, 0, lds=tbl, **_TICKET_GEO), P(DREL, ADD, MUL, 1, 0, lds=HDR, **_TICKET_GEO))]
    general = [LP.fwd("add", "mul", G(FWD, ADD, MUL, 1, 1, lds=tbl, **_TICKET_GEO)),
               LP.bwd("add", "mul", G(DX, ADD, MUL, 1, 1, lds=tbl, **_TICKET_GEO), G(DREL, ADD, MUL, 1, 0, lds=HDR, **_TICKET_GEO))]
    return [dict(id="tickets_quad", graph="cu_tickets", knob=2, calls=quad, shape="narrow"),
            dict(id="tickets_packed", graph="cu_tickets", knob=6, calls=packed, shape="narrow"),
            dict(id="tickets_general", graph="cu_tickets", knob=1, calls=general, shape="narrow")]


PLAN_ROWS += ["tickets_quad", "tickets_packed", "tickets_general"]
_LP_ROWS = {row["id"]: row for row in LP.ROWS + _ticket_rows()}
# quad_kernel's concurrent tiles at 240 compute units, by hand (the loop of plan_path.h, as in tests/test_plan_path_cpu.py): 30
# workgroups per label split into 2 teams of 15 wherever a label has at least 2 tile slots, never into 4 (30 % 4 != 0).  Slots per
# label: F = 64 / 128 / 256 -> 8 slots, 1 per label; F = 192 -> 3 tiles x 8 parts, 3 per label; F = 1 024 / 4 096 -> 2 / 8.
QUAD_CONC_240 = {"masks_lp_act_u": 2, "masks_first_layer": 2, "concurrent_1024": 2, "concurrent_4096": 2}


def _default_run(row, k, csr):
    key = ("plan default", row["id"], k)
    if key not in _memo:
        _memo[key] = LP._run_call(row, row["calls"][k], csr, total_compute_units())[0]
    return _memo[key]


@pytest.mark.parametrize("n_cu", CU_COUNTS)
@pytest.mark.parametrize("row_id", PLAN_ROWS)
def test_plan_family(row_id, n_cu):
    """Every call of the row at 8, 24 and 240 compute units: ``LP._run_call`` asserts the launch
    record (family, template arguments, the geometry resolved for ``n_cu``) and the exact-grid definition; here, in addition, the
    default run's bits and the record's geometry against tests/cu_count.py's restatement and the literals of this file."""
    row = _LP_ROWS[row_id]
    csr = LP._csr(row)
    LP._check_shape(row, csr)
    if row_id.startswith("tickets"):
        assert all(int(p.chunks.shape[0]) // _TICKET_GEO["split"] > 2 * 16 * 4 for p in (csr.fwd, csr.by_src)), "two tickets per wave at 8 CUs"
    bpl, grid = {8: (1, 8), 24: (3, 24), 240: (30, 240)}[n_cu]
    with EG._knob(row["knob"]):
        for k in range(len(row["calls"])):
            default = _default_run(row, k, csr)
            with compute_units(n_cu):
                got, records = LP._run_call(row, row["calls"][k], csr, n_cu)
            _same_bits(got, default, "%s call %d at %d compute units" % (row_id, k, n_cu))
            for rec, expected in zip(records, row["calls"][k]["expect"]):
                if rec["family"] == LP.DENSE:
                    continue
                assert (rec["family"], rec["blocks_per_label"], rec["grid"]) == (expected["family"], bpl, grid), rec
                F = EG.GRAPHS[row["graph"]][3] if row["graph"] != "removed" else 128
                columns, width = (F // 2, 64) if rec["family"] == LP.ROTATE else (F, 4 * rec["group"] if rec["family"] == LP.ROWGROUP else 64)
                geo = expected_geometry(n_cu, F, width, rec["family"] == LP.QUAD, row["knob"], columns=columns)
                assert {key: rec[key] for key in geo} == geo, (rec, geo)
                if rec["family"] == LP.QUAD:
                    assert rec["concurrent"] == (QUAD_CONC_240.get(row_id, 1) if n_cu == 240 else 1), rec


@pytest.mark.parametrize("n_cu", CU_COUNTS)
def test_pna_statistics_and_the_raw_csr_entry(n_cu):
    """``pna_statistics`` (csrc/pna.hip: tile_geometry on n_cu) at F = 18, 64, 192 (1, 1 and 3 tiles) and 1 024 (16): the bits of
    the four rspmm calls it replaces and of the default run, and the fp64 definition on the exact grid;
    ``rspmm_forward_csr`` (the raw entry's rowgroup tiling) against the exact-grid definition.  (Neither pushes a launch record:
    module docstring.)"""
    from ultra_torchdrug_amd import functional as UF
    name = "hub_19_pieces"
    csr = PG._csr(name, True)
    relation, x, dense, sparse = PG._operands(name, 1024, 64)
    default = UF.pna_statistics(csr, relation, x, "mul", boundary=sparse)
    with compute_units(n_cu):
        got = UF.pna_statistics(csr, relation, x, "mul", boundary=sparse)
        PG._assert_planes(got, PG._four_calls(csr, relation, x, "mul", boundary=sparse), "F = 1024 at %d compute units" % n_cu)
        _same_bits(got, default, "pna_statistics")
        PG.test_statistics_carry_the_bits_of_the_four_calls(name, True)
        PG.test_statistics_equal_the_fp64_definition_on_the_exact_grid()
        for graph in ("weights_dups", "ragged_isolated"):
            EG.test_raw_csr_entry_equals_the_definition(graph)


# ==================================================================================================== afterwards
def test_a_launch_after_the_last_context_records_the_default_geometry():
    """The setting is one integer of the process: after every context of this file a plan launch must be sized for the whole
    device again, and the wave counts Python sizes its partial buffers from must be the default ones."""
    import ctypes
    from ultra_torchdrug_amd import _lib
    total = total_compute_units()
    row = _LP_ROWS["concurrent_4096"]
    csr = LP._csr(row)
    with compute_units(SMALL):
        _, records = LP._run_call(row, row["calls"][0], csr, SMALL)
        assert (records[0]["blocks_per_label"], records[0]["grid"], records[0]["concurrent"]) == (1, 8, 1)
    _, records = LP._run_call(row, row["calls"][0], csr, total)
    geo = expected_geometry(total, 4096, 64, True)
    assert {key: records[0][key] for key in geo} == geo, records[0]
    if total == 256:
        assert (geo["blocks_per_label"], geo["grid"], geo["concurrent"]) == (32, 256, 8)
    n_waves = ctypes.c_int(0)
    _lib.check(_lib.load().ultra_combine_backward_fused_waves(0, 1 << 20, ctypes.byref(n_waves)))
    assert n_waves.value == 4 * total

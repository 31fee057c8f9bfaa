"""Every kernel that addresses memory through 32-bit byte offsets on the LAST shape its host guard admits, and the 64-bit form
that stands next to it on the FIRST shape the guard refuses and past 2^32 bytes (``tests/address_width.py`` has the cases, the
banded graphs and the reasoning; ``tests/test_address_width_cpu.py`` pins the decisions without a GPU; DESIGN.md "Address width"
has the audit the cases come from).

rspmm plans (F = 1024, a row is 4096 B): one operand has about 2^20 rows, the other side 128.  Edges touch the large side only
next to the byte offsets 2^31, 0xffff0000 and 2^32, at both ends and at the part cuts of rowgroup_kernel; every other row of a
gathered operand is NaN, every other row of a result must hold the empty-row identity.  The reference is the fp64 definition
(``exact_grid.definition``) on the touched rows, re-labelled; operands are exact-grid values, so the WHOLE result is compared
with ``torch.equal`` against an expected tensor built on the device.  Every case asserts, from the library's launch record,
the kernel family that ran, and that it is the one ``plan_path`` gives for the plan as built.

Row epilogues (64 columns, a row is 256 B, 2^24 rows are 4 GiB) at 2^24 - 64, 2^24 - 63, 2^24 - 1 and 2^24 rows: the whole
output equals the same entry on consecutive 2^22-row slices (bit for bit; the ops are row-independent and the small sizes are
held to fp64 elsewhere), the boundary rows equal the fp64 definition of ``tests/test_combine_row_per_lane_gpu.py`` (grid
operands, no LayerNorm: exact), and ``ultra_combine_forward_last_form`` names the kernel.  ``functional.combine``'s backward:
the upstream gradient is zero outside the boundary rows, ``d_input`` / ``d_update`` equal the slice runs bit for bit, the
parameter gradients equal fp64 autograd of the reference chain on the live rows within the bound of
``tests/test_rspmm_gpu.py::test_fused_combine_backward_matches_autograd_of_the_reference_formulation``; the one-pass form runs
up to 2^24 - 64 rows and the three-kernel form above.

The kernels whose address arithmetic is 64-bit throughout have a case past 2^32 bytes each: weight gradients (plain and per
block), the rotate kernels (record family 5), ``pna_statistics`` (planes starting past 2^31, 2^32 and 6 GiB) and the PNA epilogue,
``set_boundary``, the score head over a hidden state past 4 GiB.  d_relation's ``gather2_rows < 2^24`` is held on the device at
F = 4; the listed first-layer epilogue on both sides of its ``2^32 - 65536`` store test; the fused layer, and the same
layer with the score head inside (``layer_score_forward``), on both sides of the first part split; the first layer in training declines above 2^24 - 64 rows and the dense route gives the same numbers.

Each test states its memory need and skips only if the device has less free; each frees its tensors and holds the peak below
48 GiB.
"""
import gc
import zlib

import numpy as np
import pytest
import torch

import address_width as AW
import exact_grid as XG
from test_combine_row_per_lane_gpu import _fp64_definition
from test_rspmm_gpu import epilogue_gradient_bound

pytestmark = pytest.mark.gpu

F = AW.F_RSPMM
NAN = float("nan")


def _dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


def _seed(name):
    return zlib.crc32(name.encode()) % 100000


@pytest.fixture(scope="module")
def decide(tmp_path_factory):
    return AW.build_plan_program(tmp_path_factory.mktemp("address_width"))


@pytest.fixture(autouse=True)
def _memory():
    """Every test starts from an empty cache, frees what it allocated and stays below the cap."""
    _dev()
    gc.collect()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    yield
    gc.collect()
    torch.cuda.empty_cache()
    peak = torch.cuda.max_memory_allocated()
    assert peak < AW.CAP_BYTES, "peak %.1f GiB" % (peak / AW.GIB)


def _need(n_bytes):
    assert n_bytes < AW.CAP_BYTES
    free = torch.cuda.mem_get_info()[0]
    if free < n_bytes:
        pytest.skip("needs %.1f GiB of device memory, %.1f GiB are free" % (n_bytes / AW.GIB, free / AW.GIB))


def _knob(value):
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


def _same(got, want):
    return np.array_equal(got.detach().cpu().numpy().astype(np.float64), want)


def _n_cu():
    from ultra_torchdrug_amd import _lib
    return _lib.device_info(0)["n_cu"]


def _csr(graph, case):
    from ultra_torchdrug_amd import RelCSR
    w = None if graph["w"] is None else _t(graph["w"])
    return RelCSR(_t(graph["dst"]), _t(graph["src"]), _t(graph["rel"]), w, graph["n_dst"], graph["n_src"], graph["n_rel"],
                  chunk_edges=AW.CHUNK_EDGES, piece_len=AW.PIECE_LEN, wide_ids=case.get("wide_ids", False))


def _decision(decide, case, graph, seg, sum="add", mul="mul"):
    """plan_path's answer for the plan AS BUILT: the fields the CPU test presumes must be the plan's own."""
    inp = AW.case_plan_input(case, graph, sum, mul, n_cu=_n_cu())
    assert seg.packed is not None and seg.packed_src_shift == inp["packed_src_shift"], (seg.packed_src_shift, inp)
    assert int(seg.long_rows.shape[0]) == inp["n_long_rows"] and (seg.row_ptr is not None) == bool(inp["has_row_ptr"])
    assert seg.n_rows == inp["n_rows"] and seg.n_edges == inp["n_edges"]
    inp.update(n_pieces=seg.n_pieces, has_workspace=int(seg.workspace_rows > 0), workspace_bytes=seg.workspace_rows * F * 4)
    want = decide([inp])[0]
    assert want["status"] == 0 and want["family"] == case["family"], (want, case)
    return want


def _assert_launched(want, n_records=1, **fields):
    from ultra_torchdrug_amd import _lib
    count, records = _lib.launch_records()
    assert count == n_records, (count, records)
    rec = records[-1]
    assert rec["status"] == 0 and rec["family"] == want["family"], (rec, want)
    if want["family"] == AW.FAM_ROWGROUP:
        assert (rec["split"], rec["n_tiles"], rec["group"]) == (want["split"], want["n_tiles"], want["group"]), (rec, want)
    for key, value in fields.items():
        assert rec[key] == value, (key, rec)


def _operands(case, graph, with_large=True):
    """``(relation, small-side grid operand, large-side operand on the device, its rows as the re-labelled host array)``;
    without the large operand (a call that does not read it) its host rows are zeros."""
    rng = np.random.default_rng(_seed(case["name"]) + 2)
    relation = XG.grid(rng, (graph["n_rel"], F))
    small = XG.grid(rng, (AW.N_SMALL, F), zero=0.0)
    sub = np.zeros((len(graph["rows"]), F), dtype=np.float32)              # rows without an edge are never read
    large = None
    if with_large:
        large, live_values = AW.large_operand(case["n"], F, graph["live"], _seed(case["name"]) + 3)
        sub[np.searchsorted(graph["rows"], graph["live"])] = live_values
    return relation, small, large, sub


# ------------------------------------------------------------------------------------------------ rspmm forward
def _forward(case, graph, decide):
    from ultra_torchdrug_amd import _lib, functional as UF
    n, rows = case["n"], graph["rows"]
    csr = _csr(graph, case)
    dst, src, m_dst, m_src = AW.relabel(graph)
    rng = np.random.default_rng(_seed(case["name"]) + 2)
    relation = XG.grid(rng, (graph["n_rel"], F))
    if case["large"] == "src":
        x_dev, live_values = AW.large_operand(n, F, graph["live"], _seed(case["name"]) + 3)
        x = np.zeros((len(rows), F), dtype=np.float32)                     # rows without an edge are never read
        x[np.searchsorted(rows, graph["live"])] = live_values
    else:
        x = XG.grid(rng, (AW.N_SMALL, F))
        x_dev = _t(x)
    zeros = np.zeros((m_dst, F), dtype=np.float32)
    rel_dev = _t(relation)
    for s, m in case["ops"]:
        XG.assert_all_exact(dst, src, graph["rel"], graph["w"], relation, x, zeros + 2.0, m_dst, m)
        want_rows = XG.definition(dst, src, graph["rel"], graph["w"], relation, x, zeros, m_dst, s, m)[0]
        fill, add_rows, boundary = AW.IDENTITY[s], None, None
        if case["epilogue"] is not None:
            assert s == "add" and case["large"] == "dst"
            terms = XG.abs_sums(dst, src, graph["rel"], graph["w"], relation, x, zeros, m_dst, m)[0]
            if case["epilogue"] == "add_rows":
                add_rows = AW.fill_grid(torch.empty(n, F, dtype=torch.float32, device=_dev()), _seed(case["name"]) + 4)
                extra = add_rows[_t(rows)].cpu().numpy().astype(np.float64)
                fill = add_rows.clone()                                    # an empty row holds 0 + its add_rows row
            else:
                # 16 queries of 64 columns; the nodes are boundary rows: the first, the LAST row of the output, rows without an edge
                picks = np.concatenate([[0, len(rows) - 1], np.searchsorted(rows, graph["empty"][:2]), np.arange(3, 15)]) % len(rows)
                node = rows[picks[:16]]
                value = XG.grid(rng, (16, 64))
                dense = np.zeros((len(rows), 16, 64))
                dense[picks[:16], np.arange(16)] = value
                extra = dense.reshape(len(rows), F)
                boundary = (_t(node.astype(np.int32)), _t(value))
                fill = 0.0
                assert node[1] == n - 1
            XG.assert_exact(terms + np.abs(extra), XG.UNIT)
            want_rows = want_rows + extra
        with _knob(case["knob"]):
            _lib.launch_records_clear()
            out = UF.rspmm_forward(csr, rel_dev, x_dev, s, m, add_rows=add_rows, boundary=boundary)
            torch.cuda.synchronize()
        want = _decision(decide, case, graph, csr.fwd, s, m)
        _assert_launched(want, kind=0, sum=AW.SUM_OPS[s], mul=AW.MUL_OPS[m], unit_w=int(graph["w"] is None))
        if case["large"] == "dst":
            expected = AW.expected_rows(n, F, fill, rows, want_rows)
            assert torch.equal(out, expected), (case["name"], s, m)
            del expected
        else:
            assert _same(out, want_rows), (case["name"], s, m)
        del out, add_rows, fill


@pytest.mark.parametrize("case", AW.FORWARD_CASES, ids=[c["name"] for c in AW.FORWARD_CASES])
def test_forward_at_the_descriptor_limits(case, decide):
    _need(AW.case_bytes(case))
    _forward(case, AW.case_graph(case), decide)


@pytest.mark.parametrize("which", range(4), ids=["before_first_doubling", "after_first_doubling", "before_second_doubling",
                                                   "after_second_doubling"])
def test_rowgroup_parts_around_the_split_doublings(which, decide):
    """Wide ids, no split row: rowgroup_kernel stores each part of the rows through its own descriptor.  The sizes are the last
    before and the first after rowgroup_tiling doubles ``split``, twice, taken from rowgroup_tiling itself; edges sit on both
    sides of every part cut."""
    sizes = AW.rowgroup_split_sizes(decide)
    (n, split) = [(sizes[0][0], sizes[0][1]), (sizes[0][2], sizes[0][3]), (sizes[1][0], sizes[1][1]), (sizes[1][2], sizes[1][3])][which]
    assert sizes[0][3] == 2 * sizes[0][1] and sizes[1][3] == 2 * sizes[1][1]
    for last, before, first, _ in sizes:        # a part is as large as a descriptor of 2^32 - 65536 bytes lets it be, no smaller
        assert -(-last // before) * F * 4 < (1 << 32) - 65536 <= -(-first // before) * F * 4, sizes
    case = dict(name="rowgroup_%d" % which, kind=AW.FWD, large="dst", n=n, family=AW.FAM_ROWGROUP, ops=[("add", "mul"), ("max", "mul")],
                knob=0, weighted=True, epilogue=None, hub=False, wide_ids=True)
    _need(AW.case_bytes(case))
    graph = AW.case_graph(case, cuts=AW.part_cuts(n, split))
    for cut in AW.part_cuts(n, split):
        assert cut - 1 in graph["rows"] and cut in graph["rows"]
    from ultra_torchdrug_amd import _lib
    _forward(case, graph, decide)                               # (asserts the record's split against plan_path's)
    assert _lib.launch_records()[1][-1]["split"] == split


# ------------------------------------------------------------------------------------------------ rspmm sum backward
@pytest.mark.parametrize("case", AW.BACKWARD_CASES, ids=[c["name"] for c in AW.BACKWARD_CASES])
def test_sum_backward_at_the_descriptor_limits(case, decide):
    from ultra_torchdrug_amd import _lib, functional as UF
    _need(AW.case_bytes(case))
    graph = AW.case_graph(case)
    n, rows = case["n"], graph["rows"]
    csr = _csr(graph, case)
    dst, src, m_dst, m_src = AW.relabel(graph)
    d_input_is_large = case["kind"] == AW.DX and case["large"] == "src"
    relation, small, large, sub = _operands(case, graph, with_large=not d_input_is_large)
    x, grad = (small, sub) if case["large"] == "dst" else (sub, small)
    XG.assert_all_exact(dst, src, graph["rel"], graph["w"], relation, x, grad, m_dst, "mul")
    _, d_x, d_r, _, _ = XG.definition(dst, src, graph["rel"], graph["w"], relation, x, grad, m_dst, "add", "mul")
    rel_dev = _t(relation)
    if case["large"] == "dst":
        x_dev, grad_dev = _t(small), large
    elif d_input_is_large:
        # d_input of DistMult does not read `input`: NaN everywhere says so
        x_dev, grad_dev = torch.full((n, F), NAN, dtype=torch.float32, device=_dev()), _t(small)
    else:
        x_dev, grad_dev = large, _t(small)
    _lib.launch_records_clear()
    d_input, d_relation = UF.rspmm_backward(csr, rel_dev, x_dev, None, grad_dev, "add", "mul", need_input=case["kind"] == AW.DX,
                                            need_relation=case["kind"] == AW.DREL)
    torch.cuda.synchronize()
    seg = csr.by_src if case["kind"] == AW.DX else csr.by_rel
    want = _decision(decide, case, graph, seg)
    _assert_launched(want, sum=0, mul=0)
    if case["kind"] == AW.DREL:
        assert _same(d_relation, d_r), case["name"]
    elif case["large"] == "dst":
        assert _same(d_input, d_x), case["name"]
    else:
        assert (d_x[np.searchsorted(rows, graph["empty"])] == 0).all()
        expected = AW.expected_rows(n, F, 0.0, rows, d_x)
        assert torch.equal(d_input, expected), case["name"]


# ------------------------------------------------------------------------------------------------ layer epilogue, forward
def _epilogue_parameters(seed, grid):
    rng = np.random.default_rng(seed)
    if grid:
        w, b = XG.grid(rng, (64, 128)), XG.grid(rng, (64,))
    else:
        w = (rng.standard_normal((64, 128)) / np.sqrt(128)).astype(np.float32)
        b = (0.1 * rng.standard_normal(64)).astype(np.float32)
    gamma = (rng.random(64) + 0.5).astype(np.float32)
    beta = (0.1 * rng.standard_normal(64)).astype(np.float32)
    return w, b, gamma, beta


def _activations(rows, seed):
    dev = _dev()
    x = AW.fill_grid(torch.empty(rows, 64, dtype=torch.float32, device=dev), seed)
    u = AW.fill_grid(torch.empty(rows, 64, dtype=torch.float32, device=dev), seed + 1)
    return x, u


FORWARD_FORMS = {"default": (0, False), "reuse_update": (0, True), "one_wave": (256, False), "lds_rows": (512 | 2048, False)}


# the kernel each (form, rows) must launch, written out: the row-per-lane form up to 2^24 - 1 rows, combine_paired_kernel_lds from
# 2^24 rows and under knob bit 11, combine_kernel under knob bit 8
RPL, LDS, ONE = "combine_paired_kernel", "combine_paired_kernel_lds", "combine_kernel"
EXPECTED_FORM = {
    ("default", 16777152): RPL, ("default", 16777153): RPL, ("default", 16777215): RPL, ("default", 16777216): LDS,
    ("reuse_update", 16777152): RPL, ("reuse_update", 16777153): RPL, ("reuse_update", 16777215): RPL, ("reuse_update", 16777216): LDS,
    ("one_wave", 16777152): ONE, ("one_wave", 16777153): ONE, ("one_wave", 16777215): ONE, ("one_wave", 16777216): ONE,
    ("lds_rows", 16777152): LDS, ("lds_rows", 16777153): LDS, ("lds_rows", 16777215): LDS, ("lds_rows", 16777216): LDS,
}


@pytest.mark.parametrize("form", list(FORWARD_FORMS))
@pytest.mark.parametrize("rows", AW.EPILOGUE_ROWS, ids=["2p24m64", "2p24m63", "2p24m1", "2p24"])
def test_combine_forward_around_4_gib(rows, form):
    """The row-per-lane epilogue on its last row counts (2^24 - 1: a partial last tile whose end is byte 2^32 - 256), the
    column-per-lane form from 2^24 rows, the one-wave kernel and ``reuse_update`` at all four."""
    from ultra_torchdrug_amd import _lib, functional as UF
    _need(AW.epilogue_bytes(rows))
    knob, reuse = FORWARD_FORMS[form]
    x, u = _activations(rows, rows % 1000 + 7)
    w, b, gamma, beta = _epilogue_parameters(11, grid=True)
    w_d, b_d, g_d, be_d = (_t(a) for a in (w, b, gamma, beta))
    brows = AW.boundary_rows(rows, 256)
    assert rows - 1 in brows and ((1 << 31) // 256 in brows)
    index = _t(brows)
    xb, ub = x[index].cpu().numpy(), u[index].cpu().numpy()
    with _knob(knob):
        # (b) the boundary rows against the fp64 definition: no LayerNorm, grid operands -- exact
        out = UF.combine_forward(x, u, w_d, b_d, None, None, 1e-5, True, True, reuse_update=reuse)
        torch.cuda.synchronize()
        assert _lib.combine_forward_last_form() == EXPECTED_FORM[form, rows]
        assert (out.data_ptr() == u.data_ptr()) == reuse
        got = out[index].cpu().numpy().astype(np.float64)
        assert np.array_equal(got, _fp64_definition(xb, ub, w, b, True, True)), "boundary rows differ from the fp64 definition"
        del out
        if reuse:                       # the result went over `update`: draw it again
            AW.fill_grid(u, rows % 1000 + 8)
            assert np.array_equal(u[index].cpu().numpy(), ub)
        # (a) the whole output against the same entry on slices of 2^22 rows
        ref = torch.empty(rows, 64, dtype=torch.float32, device=_dev())
        for r0 in range(0, rows, AW.SLICE_ROWS):
            sl = slice(r0, min(rows, r0 + AW.SLICE_ROWS))
            ref[sl] = UF.combine_forward(x[sl], u[sl].clone() if reuse else u[sl], w_d, b_d, g_d, be_d, 1e-5, True, True,
                                         reuse_update=reuse)
        out = UF.combine_forward(x, u, w_d, b_d, g_d, be_d, 1e-5, True, True, reuse_update=reuse)
        torch.cuda.synchronize()
        assert _lib.combine_forward_last_form() == EXPECTED_FORM[form, rows]
    assert torch.equal(out.view(torch.int32), ref.view(torch.int32)), "the whole output differs from the runs on slices"


# ------------------------------------------------------------------------------------------------ layer epilogue, backward
@pytest.mark.parametrize("rows", AW.EPILOGUE_ROWS, ids=["2p24m64", "2p24m63", "2p24m1", "2p24"])
def test_combine_backward_around_the_one_pass_limit(rows, monkeypatch):
    """``functional.combine`` in training: the one-pass backward up to 2^24 - 64 rows, the three-kernel form above -- where the
    entry of the one-pass form returns ULTRA_ERR_BAD_SHAPE.  Before both autograd functions took the three-kernel form there, this
    call raised at 2^24 - 63 rows (run on an MI355X: ``RuntimeError: libultra_rspmm: bad shape``)."""
    from ultra_torchdrug_amd import functional as UF
    _need(AW.epilogue_bytes(rows, backward=True))
    dev = _dev()
    x, u = _activations(rows, rows % 1000 + 21)
    w, b, gamma, beta = _epilogue_parameters(13, grid=False)
    brows = AW.boundary_rows(rows, 256)
    index = _t(brows)

    # fp64 autograd of the reference chain (cat -> Linear -> LayerNorm -> relu, + input) on the live rows
    x64, u64 = (t[index].cpu().double().requires_grad_() for t in (x, u))
    p64 = [torch.from_numpy(a).double().requires_grad_() for a in (w, b, gamma, beta)]
    ref = torch.nn.functional.layer_norm(torch.nn.functional.linear(torch.cat([x64, u64], dim=-1), p64[0], p64[1]), (64,), p64[2],
                                         p64[3], 1e-5)
    gout_rows = torch.from_numpy(np.random.default_rng(rows % 1000).standard_normal((len(brows), 64)).astype(np.float32))
    gout_rows[(ref.detach().abs() < 1e-4).any(dim=1)] = 0.0          # relu's kink: such a row enters no gradient
    assert int((gout_rows != 0).any(dim=1).sum()) >= len(brows) - 2
    (torch.relu(ref) + x64).backward(gout_rows.double())
    gout = torch.zeros(rows, 64, dtype=torch.float32, device=dev)
    gout[index] = gout_rows.to(dev)

    calls = []
    one_pass = UF._combine_backward_fused
    monkeypatch.setattr(UF, "_combine_backward_fused", lambda *a, **k: (calls.append(1), one_pass(*a, **k))[1])

    def run(xs, us, gs):
        leaves = [xs.detach().requires_grad_(), us.detach().requires_grad_()] + [_t(a).requires_grad_() for a in (w, b, gamma, beta)]
        out = UF.combine(*leaves, 1e-5, True, True)
        out.backward(gs)
        torch.cuda.synchronize()
        return [t.grad for t in leaves]

    grads = run(x, u, gout)
    assert len(calls) == (1 if rows <= (1 << 24) - 64 else 0), "the one-pass form runs up to 2^24 - 64 rows and not above"
    for r0 in range(0, rows, AW.SLICE_ROWS):
        sl = slice(r0, min(rows, r0 + AW.SLICE_ROWS))
        part = run(x[sl], u[sl], gout[sl])
        assert torch.equal(part[0], grads[0][sl]) and torch.equal(part[1], grads[1][sl]), "d_input / d_update, rows from %d" % r0
        del part
    names = ["d_input", "d_update", "d_weight", "d_bias", "d_ln_weight", "d_ln_bias"]
    got = [grads[0][index], grads[1][index]] + grads[2:]
    for name, g, ref_leaf in zip(names, got, [x64, u64] + p64):
        want = ref_leaf.grad
        scale = want.abs().max().item() + 1e-12
        err = (g.cpu().double() - want).abs().max().item()
        print("%s rows %d: err %.3g, scale %.3g" % (name, rows, err, scale))
        assert err <= epilogue_gradient_bound(scale), "%s: err %.3g vs scale %.3g" % (name, err, scale)


# ------------------------------------------------------------------------------------------------ whole layer, backward
SUM_LAYER_NODES = {"2p24m64_rows": 1_048_572, "above": 1_048_573}     # x 16 queries: 2^24 - 64 rows, and 2^24 - 48


@pytest.mark.parametrize("n_node", list(SUM_LAYER_NODES.values()), ids=list(SUM_LAYER_NODES))
def test_sum_layer_backward_around_the_one_pass_limit(n_node, monkeypatch):
    """``functional.sum_layer`` with candidate tiles (16 queries, F = 1024) on a square banded graph: its backward -- the
    epilogue's, then the rspmm backward adding into the same ``d_input`` -- against the same steps called one by one
    (``functional.combine``, held above, and ``rspmm_backward(d_input_add=...)``).  ``d_input`` and ``d_relation`` bit for
    bit; the parameter gradients within the epilogue-backward bound (2^24 - 64 rows: the one-pass form over the listed tiles
    sums in another order).  Above 2^24 - 64 rows the layer must take the three-kernel form instead of raising; there the
    reference's ``functional.combine`` takes the same three-kernel helper, so this comparison holds the layer's wiring around it
    (buffers, flags, the accumulating rspmm backward), and ``test_combine_backward_around_the_one_pass_limit`` holds the helper
    itself against slice runs and fp64."""
    from ultra_torchdrug_amd import RelCSR, functional as UF
    n_query, rows = 16, n_node * 16
    _need(AW.epilogue_bytes(rows, backward=True) + 6 * AW.GIB)
    dev = _dev()
    nodes = AW.boundary_rows(n_node, 4096)
    g = AW.banded_graph(n_node, "dst", nodes, 77 + n_node % 7, hub=False, n_small=len(nodes))
    src = nodes[g["src"]]                                           # both endpoints are boundary nodes
    csr = RelCSR(_t(g["dst"]), _t(src), _t(g["rel"]), None, n_node, n_node, AW.N_REL, chunk_edges=AW.CHUNK_EDGES,
                 piece_len=AW.PIECE_LEN)
    x = AW.fill_grid(torch.empty(rows, 64, dtype=torch.float32, device=dev), 31).view(n_node, n_query, 64)
    relation = _t(XG.grid(np.random.default_rng(5), (AW.N_REL, F)))
    w, b, gamma, beta = _epilogue_parameters(17, grid=False)
    live = (nodes[:, None] * n_query + np.arange(n_query)[None, :]).reshape(-1)        # every query row of a boundary node
    gout = torch.zeros(rows, 64, dtype=torch.float32, device=dev)
    gout[_t(live)] = torch.from_numpy(np.random.default_rng(9).standard_normal((len(live), 64)).astype(np.float32)).to(dev)
    gout = gout.view(n_node, n_query, 64)
    tiles = np.unique(live // 32).astype(np.int32)
    tiles = _t(np.concatenate([tiles, np.full(5, -1, dtype=np.int32)]))

    calls = []
    one_pass = UF._combine_backward_fused
    monkeypatch.setattr(UF, "_combine_backward_fused", lambda *a, **k: (calls.append(1), one_pass(*a, **k))[1])

    def leaves():
        return [x.detach().requires_grad_(), relation.detach().requires_grad_()] + [_t(a).requires_grad_() for a in (w, b, gamma, beta)]

    # the steps one by one
    xs, rel, *params = leaves()
    with torch.no_grad():
        update = UF.rspmm_forward(csr, rel, xs.flatten(1), "add", "mul").view(n_node, n_query, 64)
    update.requires_grad_()
    UF.combine(xs, update, *params, 1e-5, True, True).backward(gout)
    d_x, d_rel = UF.rspmm_backward(csr, rel.detach(), xs.detach().flatten(1), None, update.grad.flatten(1), "add", "mul",
                                   d_input_add=xs.grad.flatten(1))
    want = [d_x.view(n_node, n_query, 64), d_rel] + [p.grad for p in params]
    del update, xs
    calls.clear()

    # the layer
    xs, rel, *params = leaves()
    out = UF.sum_layer(csr, rel, xs, None, None, "mul", *params, 1e-5, True, True, grad_tiles=tiles)
    out.backward(gout)
    torch.cuda.synchronize()
    assert len(calls) == (1 if rows <= (1 << 24) - 64 else 0)
    assert torch.equal(xs.grad, want[0]), "d_input"
    assert torch.equal(rel.grad, want[1]), "d_relation"
    assert bool((rel.grad != 0).any()) and bool((xs.grad[_t(nodes)] != 0).any())
    for name, p, ref in zip(["d_weight", "d_bias", "d_ln_weight", "d_ln_bias"], params, want[2:]):
        scale = ref.abs().max().item() + 1e-12
        err = (p.grad - ref).abs().max().item()
        print("%s nodes %d: err %.3g, scale %.3g" % (name, n_node, err, scale))
        assert err <= epilogue_gradient_bound(scale), "%s: err %.3g vs scale %.3g" % (name, err, scale)


# ------------------------------------------------------------------------------------------------ weight gradients, rotate
def _operator_setup(case, message, block=None):
    """Graph, plan, operands and the fp64 definitions (add and max) of an OPERATOR_CASES case: the large side holds ``input``
    (``large="src"``) or ``output_grad`` (``large="dst"``), the small side the other one."""
    graph = AW.case_graph(case)
    csr = _csr(graph, case)
    dst, src, m_dst, m_src = AW.relabel(graph)
    relation, small, large, sub = _operands(case, graph)
    x, grad = (small, sub) if case["large"] == "dst" else (sub, small)
    XG.assert_all_exact(dst, src, graph["rel"], graph["w"], relation, x, grad, m_dst, message, block)
    want = {s: XG.definition(dst, src, graph["rel"], graph["w"], relation, x, grad, m_dst, s, message, block) for s in ("add", "max")}
    assert want["max"][4].any(), "no tied cell: the min / max convention is not exercised"
    x_dev, grad_dev = (_t(small), large) if case["large"] == "dst" else (large, _t(small))
    return graph, csr, (dst, src, m_dst), (relation, x, grad), want, _t(relation), x_dev, grad_dev


def _output_of(case, graph, rows_value):
    """The forward result as the backward entries read it: the definition's rows, NaN in every row no edge reaches."""
    if case["large"] == "dst":
        return AW.expected_rows(case["n"], F, NAN, graph["rows"], rows_value)
    return _t(rows_value.astype(np.float32))


@pytest.mark.parametrize("case", [c for c in AW.OPERATOR_CASES if c["n"] == AW.PAST_4GIB], ids=lambda c: c["name"])
def test_weight_gradients_past_4_gib(case):
    """``rspmm_backward_weight`` and ``rspmm_backward_weight_blocks`` (block 64): one wave per edge, every index ``long long``.
    ``input`` past 2^32 bytes, and ``output`` / ``output_grad`` past 2^32 bytes; sum and max (every tied edge receives the
    gradient in full), against the definition's weight gradient, per block on that block's columns alone."""
    from ultra_torchdrug_amd import functional as UF
    _need(AW.case_bytes(dict(case, operator=True)))
    graph, csr, (dst, src, m_dst), (relation, x, grad), want, rel_dev, x_dev, grad_dev = _operator_setup(case, "mul")
    for s in ("add", "max"):
        output = _output_of(case, graph, want[s][0])
        d_w = UF.rspmm_backward_weight(csr, rel_dev, x_dev, output, grad_dev, s, "mul")
        assert d_w.shape == (csr.n_edges,) and _same(d_w, want[s][3]), s
        blocks = UF.rspmm_backward_weight_blocks(csr, rel_dev, x_dev, output, grad_dev, s, "mul", block=64)
        per_block = np.stack([XG.definition(dst, src, graph["rel"], graph["w"], relation[:, c:c + 64], x[:, c:c + 64],
                                            grad[:, c:c + 64], m_dst, s, "mul")[3] for c in range(0, F, 64)])
        assert blocks.shape == (F // 64, csr.n_edges) and _same(blocks, per_block), s
        del output


@pytest.mark.parametrize("case", AW.OPERATOR_CASES, ids=lambda c: c["name"])
def test_rotate_kernels_at_the_limits(case):
    """Rotate messages (blocks of 64 columns) over an ``out`` / ``output_grad`` and over an ``input`` of 0xfffef000 bytes and
    past 2^32: forward (sum, max), ``d_input`` / ``d_relation`` (sum) and the weight gradient per block (max) against the
    definition; every plan run writes ``run_rotate_plan``'s record (family 5)."""
    from ultra_torchdrug_amd import _lib, functional as UF
    _need(AW.case_bytes(dict(case, operator=True)))
    n, block = case["n"], 64
    graph, csr, (dst, src, m_dst), (relation, x, grad), want, rel_dev, x_dev, grad_dev = _operator_setup(case, "rotate", block)
    rows = graph["rows"]
    for s in ("add", "max"):
        _lib.launch_records_clear()
        out = UF.rotate_rspmm_forward(csr, rel_dev, x_dev, s, block)
        torch.cuda.synchronize()
        count, records = _lib.launch_records()
        assert count == 1 and records[0]["family"] == 5 and records[0]["status"] == 0 and records[0]["sum"] == AW.SUM_OPS[s], records
        if case["large"] == "dst":
            expected = AW.expected_rows(n, F, AW.IDENTITY[s], rows, want[s][0])
            assert torch.equal(out, expected), s
            del expected
        else:
            assert _same(out, want[s][0]), s
        del out
    _lib.launch_records_clear()
    d_x, d_r = UF.rotate_rspmm_backward(csr, rel_dev, x_dev, None, grad_dev, "add", block)
    torch.cuda.synchronize()
    count, records = _lib.launch_records()
    assert count == 2 and [r["family"] for r in records] == [5, 5] and all(r["status"] == 0 for r in records), records
    assert _same(d_r, want["add"][2]), "d_relation"
    if case["large"] == "dst":
        assert _same(d_x, want["add"][1]), "d_input"
    else:
        assert torch.equal(d_x, AW.expected_rows(n, F, 0.0, rows, want["add"][1])), "d_input"
    del d_x
    output = _output_of(case, graph, want["max"][0])
    d_w = UF.rotate_rspmm_backward_weight_blocks(csr, rel_dev, x_dev, output, grad_dev, "max", block)
    per_block = np.stack([XG.definition(dst, src, graph["rel"], graph["w"], relation[:, c:c + 64], x[:, c:c + 64],
                                        grad[:, c:c + 64], m_dst, "max", "rotate", block)[3] for c in range(0, F, 64)])
    assert _same(d_w, per_block), "d_weight per block"
    assert _same(UF.rotate_rspmm_backward_weight(csr, rel_dev, x_dev, output, grad_dev, "max", block), want["max"][3]), "d_weight"


# ------------------------------------------------------------------------------------------------ d_relation, second gather
@pytest.mark.parametrize("case", AW.GATHER2_CASES, ids=lambda c: c["name"])
def test_d_relation_second_gather_around_2_24_rows(case, decide):
    """F = 4 (16-byte rows): quad_kernel multiplies the destination node of d_relation's second gather with ``__umul24``, so it
    runs up to 2^24 - 1 gathered rows and packed_kernel from 2^24; edges reach the last rows of ``output_grad``."""
    from ultra_torchdrug_amd import _lib, functional as UF
    _need(AW.case_bytes(case))
    Fs = case["F"]
    graph = AW.case_graph(case)
    rows = graph["rows"]
    csr = _csr(graph, case)
    dst, src, m_dst, m_src = AW.relabel(graph)
    rng = np.random.default_rng(_seed(case["name"]))
    relation, x = XG.grid(rng, (graph["n_rel"], Fs)), XG.grid(rng, (AW.N_SMALL, Fs), zero=0.0)
    grad_dev, live_values = AW.large_operand(case["n"], Fs, graph["live"], _seed(case["name"]) + 3)
    grad = np.zeros((len(rows), Fs), dtype=np.float32)
    grad[np.searchsorted(rows, graph["live"])] = live_values
    XG.assert_all_exact(dst, src, graph["rel"], graph["w"], relation, x, grad, m_dst, "mul")
    d_r = XG.definition(dst, src, graph["rel"], graph["w"], relation, x, grad, m_dst, "add", "mul")[2]
    assert np.abs(d_r).sum() > 0
    _lib.launch_records_clear()
    _, got = UF.rspmm_backward(csr, _t(relation), _t(x), None, grad_dev, "add", "mul", need_input=False, need_relation=True)
    torch.cuda.synchronize()
    inp = AW.case_plan_input(case, graph, n_cu=_n_cu())
    seg = csr.by_rel
    assert seg.packed_src_shift == inp["packed_src_shift"] and int(seg.long_rows.shape[0]) == inp["n_long_rows"]
    want = decide([inp])[0]
    assert want["family"] == case["family"]
    _assert_launched(want, kind=2)
    assert _same(got, d_r)


# ------------------------------------------------------------------------------------------------ set_boundary
def test_set_boundary_past_4_gib():
    """``(N, 16, 64)`` fp32 past 2^32 bytes with its count: memberships are non-zero at the boundary nodes only (some below
    the floor, one NaN, one negative); the result equals ``dense_set_boundary`` restated in numpy on those nodes and +0
    everywhere else, bit for bit; query_set.hip does its index arithmetic in ``long long``."""
    from ultra_torchdrug_amd import functional as UF
    n, n_query, dim = AW.SET_BOUNDARY_SHAPE
    _need(2 * n * n_query * dim * 4 + AW.GIB)
    nodes = AW.boundary_rows(n, n_query * dim * 4)
    rng = np.random.default_rng(23)
    m = (rng.integers(1, 9, (n_query, len(nodes))) / 8.0).astype(np.float32)
    m[rng.random(m.shape) < 0.2] = 0.0
    m[0, 0], m[1, 1], m[2, -1] = np.nan, -0.5, 1.0                      # (the last node of the tensor is kept by query 2)
    floor = np.full(n_query, 0.25, dtype=np.float32)
    query = XG.grid(rng, (n_query, dim))
    member = torch.zeros(n_query, n, dtype=torch.float32, device=_dev())
    member[:, _t(nodes)] = _t(m)
    boundary, count = UF.set_boundary(member, _t(query), _t(floor), with_count=True)
    keep = (m > 0) & (m >= floor[:, None])                               # (a NaN compares false)
    want = np.where(keep.T[:, :, None], m.T[:, :, None].astype(np.float64) * query[None].astype(np.float64), 0.0)
    assert keep.any(axis=1).all() and not keep.all() and keep[2, -1]
    assert np.array_equal(count.cpu().numpy(), keep.sum(axis=1))
    expected = AW.expected_rows(n, n_query * dim, 0.0, nodes, want.reshape(len(nodes), -1))
    assert torch.equal(boundary.view(n, -1).view(torch.int32), expected.view(torch.int32))


# ------------------------------------------------------------------------------------------------ PNA
def test_pna_statistics_planes_past_2_31():
    """``(4, 524 289, 1024)``: a plane is 2^31 + 4096 bytes, so planes 1 to 3 start past 2^31, 2^32 and 6 GiB.  Each plane is
    ``torch.equal`` to the ``rspmm_forward`` call it replaces (which runs quad_kernel with store offsets past 2^31) and both to
    the fp64 definition on the touched rows, the identity everywhere else."""
    from ultra_torchdrug_amd import functional as UF
    case = AW.PNA_CASE
    n = case["n"]
    _need(6 * n * F * 4 + AW.GIB)
    graph = AW.case_graph(case)
    rows = graph["rows"]
    csr = _csr(graph, case)
    dst, src, m_dst, m_src = AW.relabel(graph)
    rng = np.random.default_rng(_seed(case["name"]))
    relation, x = XG.grid(rng, (graph["n_rel"], F)), XG.grid(rng, (AW.N_SMALL, F))
    zeros = np.zeros((m_dst, F), dtype=np.float32)
    XG.assert_all_exact(dst, src, graph["rel"], graph["w"], relation, x, zeros, m_dst, "mul")
    # squared operands: terms are multiples of 2^-9 (w / 2, (k / 4)^4)
    XG.assert_exact(XG.abs_sums(dst, src, graph["rel"], graph["w"], relation * relation, x * x, zeros, m_dst, "mul")[0], 2.0 ** -9)
    rel_dev, x_dev = _t(relation), _t(x)
    stats = UF.pna_statistics(csr, rel_dev, x_dev, "mul")
    torch.cuda.synchronize()
    starts = [stats[k].data_ptr() - stats[0].data_ptr() for k in range(4)]
    assert starts[1] > 1 << 31 and starts[2] > 1 << 32 and starts[3] > 6 << 30
    for plane, (s, square) in enumerate((("add", False), ("add", True), ("max", False), ("min", False))):
        r_np, x_np = (relation * relation, x * x) if square else (relation, x)
        replaced = UF.rspmm_forward(csr, _t(r_np), _t(x_np), s, "mul")
        assert torch.equal(stats[plane], replaced), "plane %d differs from the call it replaces" % plane
        want = XG.definition(dst, src, graph["rel"], graph["w"], r_np, x_np, zeros, m_dst, s, "mul")[0]
        expected = AW.expected_rows(n, F, AW.IDENTITY[s], rows, want)
        assert torch.equal(replaced, expected), "plane %d differs from the definition" % plane
        del replaced, expected


def test_pna_combine_forward_past_4_gib():
    """The fused PNA epilogue over 2^24 + 16 rows of 16 queries (input, four statistics and the result past 4 GiB each): the whole
    output equals the same entry on consecutive slices of 2^18 nodes, bit for bit."""
    from ultra_torchdrug_amd import functional as UF
    n_node, n_query = AW.PNA_COMBINE_SHAPE
    rows = n_node * n_query
    _need(8 * rows * 256)
    dev = _dev()
    x = AW.fill_grid(torch.empty(rows, 64, dtype=torch.float32, device=dev), 41)
    planes = [AW.fill_grid(torch.empty(rows, 64, dtype=torch.float32, device=dev), 42 + k) for k in range(4)]
    planes[1].abs_()
    degree = torch.randint(1, 10, (n_node,), generator=torch.Generator(device=dev).manual_seed(5), device=dev).float()
    table = UF.pna_node_table(degree)
    rng = np.random.default_rng(19)
    w = _t((rng.standard_normal((64, 832)) / np.sqrt(832)).astype(np.float32))
    b, gamma, beta = (_t(a) for a in _epilogue_parameters(19, grid=False)[1:])
    out = UF.pna_combine_forward(x, planes, table, w, b, gamma, beta, relu=True, shortcut=True, n_query=n_query)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out[-64:]).all())
    step = 1 << 18
    for v0 in range(0, n_node, step):
        nodes = slice(v0, min(n_node, v0 + step))
        sl = slice(nodes.start * n_query, nodes.stop * n_query)
        part = UF.pna_combine_forward(x[sl], [t[sl] for t in planes], table[nodes], w, b, gamma, beta, relu=True, shortcut=True,
                                      n_query=n_query)
        assert torch.equal(part.view(torch.int32), out[sl].view(torch.int32)), "rows from %d" % sl.start


# ------------------------------------------------------------------------------------------------ score head
@pytest.mark.parametrize("knob", [0, 1024], ids=["row_per_lane", "lds_rows"])
def test_score_all_entities_over_a_hidden_past_4_gib(knob):
    """``hidden`` ``(262 145, 64, 64)`` is 2^32 + 16 384 bytes (the kernels read it with 64-bit addresses; the ``(64, N)`` scores
    go through one descriptor of 67 MB): equal, bit for bit, to the same entry on consecutive slices of 2^14 nodes."""
    from ultra_torchdrug_amd import functional as UF
    n_node, batch = AW.SCORE_SHAPE
    _need(2 * n_node * batch * 256)
    dev = _dev()
    hidden = AW.fill_grid(torch.empty(n_node * batch, 64, dtype=torch.float32, device=dev), 51).view(n_node, batch, 64)
    rng = np.random.default_rng(29)
    query = _t(XG.grid(rng, (batch, 64)))
    w1 = _t((rng.standard_normal((128, 128)) / np.sqrt(128)).astype(np.float32))
    b1, w2, b2 = (_t((0.1 * rng.standard_normal(k)).astype(np.float32)) for k in (128, 128, 1))
    with _knob(knob):
        scores = UF.score_all_entities(hidden, query, w1, b1, w2.view(1, 128), b2)
        torch.cuda.synchronize()
        assert scores.shape == (batch, n_node) and bool(torch.isfinite(scores).all())
        step = 1 << 14
        for v0 in range(0, n_node, step):
            nodes = slice(v0, min(n_node, v0 + step))
            part = UF.score_all_entities(hidden[nodes], query, w1, b1, w2.view(1, 128), b2)
            assert torch.equal(part.view(torch.int32), scores[:, nodes].contiguous().view(torch.int32)), "nodes from %d" % v0


# ------------------------------------------------------------------------------------------------ first layer
def _square_graph(n_node, seed):
    """A square banded graph: both endpoints of every edge are boundary nodes of an ``(n_node, 1024)`` tensor."""
    from ultra_torchdrug_amd import RelCSR
    nodes = AW.boundary_rows(n_node, 4096)
    g = AW.banded_graph(n_node, "dst", nodes, seed, hub=False, n_small=len(nodes))
    src = nodes[g["src"]]
    csr = RelCSR(_t(g["dst"]), _t(src), _t(g["rel"]), None, n_node, n_node, AW.N_REL, chunk_edges=AW.CHUNK_EDGES,
                 piece_len=AW.PIECE_LEN)
    return nodes, g["dst"], src, csr


def _boundary_of(sources, n_query, seed):
    """16 queries whose boundary nodes are sources of the graph (the largest among them), with grid values; also as the dense
    ``(node, query)`` rows it stands for."""
    uniq = np.unique(sources)
    node = uniq[(np.arange(n_query) * 5) % len(uniq)]
    node[0] = uniq[-1]
    value = XG.grid(np.random.default_rng(seed), (n_query, 64), zero=0.0)
    return node, value


@pytest.mark.parametrize("n_node", [1_048_559, 1_048_560], ids=["descriptor_stores", "plain_stores"])
def test_listed_first_layer_on_both_sides_of_its_store_test(n_node):
    """``first_layer_forward`` at 16 queries: 16 776 944 rows (``rows * 256 < 2^32 - 65536``: the listed epilogue stores through
    one descriptor over the whole output, 32-bit offsets) and 16 776 960 rows (plain 64-bit stores).  The whole result equals
    ``rspmm_frontier`` + ``combine_forward(input_boundary=...)`` bit for bit, and the frontier's sums equal the full kernel on
    the dense boundary."""
    from ultra_torchdrug_amd import functional as UF
    n_query = 16
    _need(6 * n_node * 4096)
    nodes, dst, src, csr = _square_graph(n_node, 61)
    node, value = _boundary_of(src, n_query, 62)
    boundary = (_t(node.astype(np.int32)), _t(value))
    relation = _t(XG.grid(np.random.default_rng(63), (AW.N_REL, F), zero=0.0))
    w, b, gamma, beta = (_t(a) for a in _epilogue_parameters(64, grid=False))
    out = UF.first_layer_forward(csr, relation, boundary, w, b, gamma, beta, 1e-5, True, True)
    assert out is not None and out.shape == (n_node, n_query, 64)
    update = UF.rspmm_frontier(csr, relation, boundary)
    dense = torch.zeros(n_node, n_query, 64, dtype=torch.float32, device=_dev())
    dense[boundary[0].long(), torch.arange(n_query, device=_dev())] = boundary[1]
    full = UF.rspmm_forward(csr, relation, dense.view(n_node, F), "add", "mul", boundary=boundary)
    assert torch.equal(update, full), "the frontier's sums differ from the full kernel's"
    reached = (update.view(n_node, n_query, 64) != 0).any(dim=2).sum().item()
    assert reached > n_query and bool((update[n_node - 4:] != 0).any()), "no edge reaches the last rows"
    del dense, full
    want = UF.combine_forward(None, update.view(n_node, n_query, 64), w, b, gamma, beta, 1e-5, True, True, reuse_update=True,
                              input_boundary=boundary)
    assert torch.equal(out.view(torch.int32), want.view(torch.int32)), "the listed first layer differs from the dense form"


def test_first_layer_in_training_takes_the_dense_route_above_the_one_pass_limit(monkeypatch):
    """16 777 168 rows (1 048 573 nodes x 16 queries, above 2^24 - 64): ``first_layer_train_forward`` declines, the layer runs the
    frontier kernel and the dense epilogue, its backward the three-kernel form and the boundary-row kernels; output and
    gradients agree with the same layer run without the first-layer promise (the full kernels)."""
    from ultra_torchdrug_amd import functional as UF
    n_node, n_query = SUM_LAYER_NODES["above"], 16
    rows = n_node * n_query
    _need(AW.epilogue_bytes(rows, backward=True) + 6 * AW.GIB)
    dev = _dev()
    nodes, dst, src, csr = _square_graph(n_node, 71)
    node, value = _boundary_of(src, n_query, 72)
    b_node = _t(node.astype(np.int32))
    relation = _t(XG.grid(np.random.default_rng(73), (AW.N_REL, F), zero=0.0))
    w, b, gamma, beta = _epilogue_parameters(74, grid=False)
    dense = torch.zeros(n_node, n_query, 64, dtype=torch.float32, device=dev)
    dense[b_node.long(), torch.arange(n_query, device=dev)] = _t(value)
    live = (nodes[:, None] * n_query + np.arange(n_query)[None, :]).reshape(-1)
    gout = torch.zeros(rows, 64, dtype=torch.float32, device=dev)
    gout[_t(live)] = torch.from_numpy(np.random.default_rng(75).standard_normal((len(live), 64)).astype(np.float32)).to(dev)
    gout = gout.view(n_node, n_query, 64)
    declined = []
    sparse = UF.first_layer_train_forward
    monkeypatch.setattr(UF, "first_layer_train_forward", lambda *a, **k: (lambda r: (declined.append(r is None), r)[1])(sparse(*a, **k)))

    def run(promise):
        rel, bv = relation.detach().requires_grad_(), _t(value).requires_grad_()
        params = [_t(a).requires_grad_() for a in (w, b, gamma, beta)]
        out = UF.sum_layer(csr, rel, dense, None, (b_node, bv), "mul", *params, 1e-5, True, True, input_is_boundary=promise)
        out.backward(gout)
        torch.cuda.synchronize()
        return out.detach(), [rel.grad, bv.grad] + [p.grad for p in params]

    out_first, grads_first = run(True)
    assert declined == [True], "first_layer_train_forward must decline above 2^24 - 64 rows"
    out_full, grads_full = run(False)
    assert torch.equal(out_first, out_full), "output"
    del out_first, out_full
    for name, got, ref in zip(["d_relation", "d_boundary_value", "d_weight", "d_bias", "d_ln_weight", "d_ln_bias"], grads_first, grads_full):
        scale = ref.abs().max().item() + 1e-12
        err = (got - ref).abs().max().item()
        print("%s: err %.3g, scale %.3g" % (name, err, scale))
        assert scale > 1e-6 and err <= epilogue_gradient_bound(scale), "%s: err %.3g vs scale %.3g" % (name, err, scale)


# ------------------------------------------------------------------------------------------------ fused layer
@pytest.mark.parametrize("n_node", [1_048_559, 1_048_573], ids=["one_part", "two_parts"])
def test_fused_layer_and_score_head_around_the_first_split_doubling(n_node):
    """``layer_forward`` (rspmm + epilogue in one launch, wide ids, no split row) at 16 queries: 1 048 559 nodes are one part of
    0xfffef000 bytes, 1 048 573 nodes two parts (``rowgroup_tiling`` doubles the split from 1 048 560 rows) and an ``input`` of
    2^32 + 53 248 bytes; the whole result equals ``rspmm_forward`` + ``combine_forward`` bit for bit.  ``layer_score_forward``
    (the same kernel with the score head inside: 64-bit reads of ``input``, the ``(16, N)`` scores of 67 MB through one
    descriptor at ``(query * n_rows + row) * 4``) on the same shapes equals ``score_all_entities(layer_forward(...))`` bit for
    bit.  Only the score descriptor's own last admitted shape (``n_query * n_rows * 4 < 2^32 - 65536``: an ``input`` 64 times
    that size) does not fit the memory cap."""
    from ultra_torchdrug_amd import RelCSR, functional as UF
    n_query = 16
    _need(5 * n_node * 4096)
    dev = _dev()
    nodes = AW.boundary_rows(n_node, 4096, cuts=AW.part_cuts(n_node, 2) if n_node >= AW.FIRST_REFUSED else ())
    g = AW.banded_graph(n_node, "dst", nodes, 81, hub=False, n_small=len(nodes))
    src = nodes[g["src"]]
    csr = RelCSR(_t(g["dst"]), _t(src), _t(g["rel"]), None, n_node, n_node, AW.N_REL, chunk_edges=AW.CHUNK_EDGES,
                 piece_len=AW.PIECE_LEN, wide_ids=True)
    assert csr.fwd.row_ptr is not None and csr.fwd.n_pieces == 0
    assert _lib_supported(csr, n_query)
    node, value = _boundary_of(src, n_query, 82)
    boundary = (_t(node.astype(np.int32)), _t(value))
    relation = _t(XG.grid(np.random.default_rng(83), (AW.N_REL, F), zero=0.0))
    w, b, gamma, beta = (_t(a) for a in _epilogue_parameters(84, grid=False))
    x = AW.fill_grid(torch.empty(n_node * n_query, 64, dtype=torch.float32, device=dev), 85).view(n_node, n_query, 64)
    got = UF.layer_forward(csr, relation, x, boundary, w, b, gamma, beta, 1e-5, True, True)
    assert got is not None
    update = UF.rspmm_forward(csr, relation, x.flatten(1), "add", "mul", boundary=boundary).view(n_node, n_query, 64)
    assert bool((update[_t(nodes)] != 0).any())
    want = UF.combine_forward(x, update, w, b, gamma, beta, 1e-5, True, True, reuse_update=True)
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    del want, update
    from ultra_torchdrug_amd import _lib
    assert _lib.load().ultra_layer_score_supported(csr.fwd.pointer, n_query, csr.shape[2])
    rng = np.random.default_rng(86)
    query = _t(XG.grid(rng, (n_query, 64)))
    w1 = _t((rng.standard_normal((128, 128)) / np.sqrt(128)).astype(np.float32))
    b1, w2, b2 = (_t((0.1 * rng.standard_normal(k)).astype(np.float32)) for k in (128, 128, 1))
    scores = UF.layer_score_forward(csr, relation, x, boundary, w, b, gamma, beta, 1e-5, True, True, query, w1, b1, w2.view(1, 128), b2)
    assert scores is not None and scores.shape == (n_query, n_node)
    want_scores = UF.score_all_entities(got, query, w1, b1, w2.view(1, 128), b2)
    assert bool(torch.isfinite(want_scores).all()) and bool((want_scores[:, -4:] != want_scores[:, :4]).any())
    assert torch.equal(scores.view(torch.int32), want_scores.view(torch.int32)), "layer + score head in one launch differs"


def _lib_supported(csr, n_query):
    from ultra_torchdrug_amd import _lib
    return bool(_lib.load().ultra_layer_forward_supported(csr.fwd.pointer, n_query, csr.shape[2]))

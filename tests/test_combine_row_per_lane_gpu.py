"""The row-per-lane form of the paired layer epilogue (combine_paired_kernel: the product issued as mfma(A = weight, B = rows),
LayerNorm / relu / shortcut on the accumulators after 16 half swaps, the prefetch through buffer descriptors over the whole
tensors) against its former column-per-lane form (combine_paired_kernel_lds, knob bit 11),
the one-wave kernel and the oracle: EQUAL int32 bits, no tolerance.

    new       knob 512          combine_paired_kernel
    former    knob 512 | 2048   combine_paired_kernel_lds
    one-wave  knob 256          combine_kernel
    oracle    --                OracleFunctional.combine

Operands are the ones of ``test_combine_paired_gpu.py`` (its memo is shared: every operand set and every oracle result is
computed once per session).  Row counts (a row = 64 floats, a tile = 32 rows, a workgroup = 8 waves): 1 .. 257 for the tail
tile (rows past the end fail the descriptors' range check: they load 0 and are never stored), the store descriptor of a short
tile and fewer tiles than waves; 32 * 24 (+ 5) for several tiles per wave inside one workgroup, the ticket running out and the
prefetch of a tile that is never processed; 32 * 8 * n_cu * 3 + 5 for every workgroup's contiguous range and its boundaries.
On the dyadic grid without LayerNorm the result must also equal the fp64 definition, whatever the order of the additions.
"""
import numpy as np
import pytest
import torch

from oracle_ops import OracleFunctional
from test_combine_paired_gpu import _full_grid_rows, _n_cu, _on_device, _operands, _oracle, _run

pytestmark = pytest.mark.gpu

NEW, FORMER, ONE_WAVE = 512, 512 | 2048, 256
ROWS = [1, 31, 32, 33, 63, 64, 255, 256, 257, 32 * 24, 32 * 24 + 5]


def _bits(t):
    return t.view(torch.int32)


def _fp64_definition(x, u, w, b, relu, shortcut):
    x, u, w, b = (np.asarray(a, dtype=np.float64) for a in (x, u, w, b))
    want = np.concatenate([x, u], axis=1) @ w.T + b
    assert np.abs(want).max() < 2.0 ** 24 / 16            # multiples of 1/16 below 2^20: exact in fp32 in any order
    if relu:
        want = np.where(want <= 0, 0.0, want)
    if shortcut:
        want = want + x
    return want


def _check(rows, kind, ln, relu, shortcut, alias):
    ops = _on_device(rows, kind)
    new = _run(NEW, *ops, ln, relu, shortcut, alias)
    former = _run(FORMER, *ops, ln, relu, shortcut, alias)
    one_wave = _run(ONE_WAVE, *ops, ln, relu, shortcut, alias)
    assert torch.equal(_bits(new), _bits(former)), "the row-per-lane form differs from combine_paired_kernel_lds"
    assert torch.equal(_bits(new), _bits(one_wave)), "the row-per-lane form differs from the one-wave kernel"
    got = new.cpu().numpy()
    want = _oracle(rows, kind, ln, relu, shortcut).numpy()
    assert np.array_equal(got.view(np.int32), want.view(np.int32)), "the row-per-lane form differs from the oracle"
    if kind == "grid" and not ln:
        x, u, w, b = (t.numpy() for t in _operands(rows, kind)[:4])
        assert np.array_equal(got.astype(np.float64), _fp64_definition(x, u, w, b, relu, shortcut)), \
            "the row-per-lane form differs from the fp64 definition"


@pytest.mark.parametrize("alias", [False, True], ids=["separate_out", "out_is_update"])
@pytest.mark.parametrize("kind", ["normal", "grid"])
@pytest.mark.parametrize("rows", ROWS)
def test_row_per_lane_form_equals_the_other_forms_and_the_oracle(rows, kind, alias):
    _check(rows, kind, True, True, True, alias)


@pytest.mark.parametrize("alias", [False, True], ids=["separate_out", "out_is_update"])
@pytest.mark.parametrize("kind", ["normal", "grid"])
def test_row_per_lane_form_on_the_full_grid(kind, alias):
    """Three tiles per wave and a tail: every workgroup's contiguous range, its boundaries, the tail's range check."""
    _check(_full_grid_rows(), kind, True, True, True, alias)


@pytest.mark.parametrize("alias", [False, True], ids=["separate_out", "out_is_update"])
@pytest.mark.parametrize("shortcut", [False, True], ids=["plain", "shortcut"])
@pytest.mark.parametrize("relu", [False, True], ids=["linear", "relu"])
@pytest.mark.parametrize("ln", [False, True], ids=["no_ln", "ln"])
@pytest.mark.parametrize("kind,rows", [("normal", 33), ("grid", 257), ("grid", 32 * 24 + 5)])
def test_row_per_lane_form_epilogue_options(kind, rows, ln, relu, shortcut, alias):
    _check(rows, kind, ln, relu, shortcut, alias)


@pytest.mark.parametrize("alias", [False, True], ids=["separate_out", "out_is_update"])
def test_every_output_column_identifies_itself(alias):
    """No LayerNorm, ``w`` a 0 / 1 matrix with one entry per output (output k copies column (37 k + 11) % 128 of
    cat[input, update]) and bias k / 16: out[row, k] = cat[row, (37 k + 11) % 128] + k / 16, exactly.  A swapped half-swap
    operand order, a wrong column offset of the second register of a pair or a wrong bias register shows as a permutation."""
    rows = 32 * 24 + 5
    x, u = _operands(rows, "grid")[:2]
    source = (37 * np.arange(64) + 11) % 128
    assert len(set(source.tolist())) == 64
    w = np.zeros((64, 128), dtype=np.float32)
    w[np.arange(64), source] = 1.0
    b = (np.arange(64) / 16.0).astype(np.float32)
    want = np.concatenate([x.numpy(), u.numpy()], axis=1).astype(np.float64)[:, source] + b.astype(np.float64)
    assert np.array_equal(want, _fp64_definition(x.numpy(), u.numpy(), w, b, False, False))
    dev = _on_device(rows, "grid")
    ops = (dev[0], dev[1], torch.from_numpy(w).to(dev[0].device), torch.from_numpy(b).to(dev[0].device), dev[4], dev[5])
    new = _run(NEW, *ops, False, False, False, alias)
    for knob in (FORMER, ONE_WAVE):
        assert torch.equal(_bits(new), _bits(_run(knob, *ops, False, False, False, alias)))
    got = new.cpu().numpy().astype(np.float64)
    wrong = np.argwhere(got != want)
    assert wrong.size == 0, "first wrong (row, column): %s" % wrong[:4].tolist()


@pytest.mark.parametrize("alias", [False, True], ids=["separate_out", "out_is_update"])
@pytest.mark.parametrize("ln", [False, True], ids=["no_ln", "ln"])
def test_non_finite_rows_stay_in_their_rows(ln, alias):
    """NaN, +-inf and an inf - inf pair in a few rows of ``update``: those rows are bit-equal across the three kernels, every
    other row is what the oracle gives without them."""
    rows = 32 * 24 + 5
    x, u, w, b, gamma, beta = _on_device(rows, "normal")
    bad = [0, 31, 32, 300, rows - 1]
    poisoned = u.clone()
    for k, r in enumerate(bad):
        poisoned[r, (7 * k) % 64] = (float("nan"), float("inf"), float("-inf"))[k % 3]
    poisoned[300, 5], poisoned[300, 6] = float("inf"), float("-inf")
    new = _run(NEW, x, poisoned, w, b, gamma, beta, ln, True, True, alias)
    former = _run(FORMER, x, poisoned, w, b, gamma, beta, ln, True, True, alias)
    one_wave = _run(ONE_WAVE, x, poisoned, w, b, gamma, beta, ln, True, True, alias)
    assert torch.equal(_bits(new), _bits(former))
    assert torch.equal(_bits(new), _bits(one_wave))
    clean = torch.ones(rows, dtype=torch.bool)
    clean[bad] = False
    assert not torch.isfinite(new[~clean.to(new.device)]).all(dim=1).any(), "a poisoned row came out finite"
    want = _oracle(rows, "normal", ln, True, True)
    assert np.array_equal(new.cpu()[clean].numpy().view(np.int32), want[clean].numpy().view(np.int32)), "a finite row changed"


@pytest.mark.parametrize("alias", [False, True], ids=["separate_out", "out_is_update"])
@pytest.mark.parametrize("side", ["below", "above"])
def test_default_dispatch(side, alias):
    """Either side of the size from which the epilogue prefetches (16 tiles per CU) the default equals knob 256; above it,
    where the default is the row-per-lane form, it also equals knob 2048 (the former paired kernel)."""
    tiles = 16 * _n_cu()
    rows = 32 * (tiles - 1) if side == "below" else 32 * tiles + 1
    ops = _on_device(rows, "normal")
    default = _run(0, *ops, True, True, True, alias)
    assert torch.equal(_bits(default), _bits(_run(ONE_WAVE, *ops, True, True, True, alias)))
    if side == "above":
        assert torch.equal(_bits(default), _bits(_run(2048, *ops, True, True, True, alias)))
    sub = slice(rows - 2000, rows)
    x, u, w, b, gamma, beta = (t if t.dim() == 1 or t.shape[0] == 64 else t[sub] for t in _operands(rows, "normal"))
    with torch.no_grad():
        want = OracleFunctional(None).combine(x, u, w, b, gamma, beta, 1e-5, True, True)
    assert np.array_equal(default[sub].cpu().numpy().view(np.int32), want.numpy().view(np.int32))


def test_captured_graph_replay_equals_the_eager_launch():
    import ultra_torchdrug_amd as U
    from ultra_torchdrug_amd import functional as UF
    rows = 32 * 24 + 5
    x, u, w, b, gamma, beta = _on_device(rows, "normal")
    eager = _run(NEW, x, u, w, b, gamma, beta, True, True, True, False)
    lib = U.require_library()
    lib.ultra_rspmm_force_general_path(NEW)
    try:
        stream = torch.cuda.Stream()
        stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(stream):
            UF.combine_forward(x, u, w, b, gamma, beta, 1e-5, True, True)            # (allocator warm-up on the side stream)
        torch.cuda.current_stream().wait_stream(stream)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = UF.combine_forward(x, u, w, b, gamma, beta, 1e-5, True, True)
    finally:
        lib.ultra_rspmm_force_general_path(0)
    out.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(_bits(out), _bits(eager))


@pytest.mark.parametrize("rows", [1, 33])
def test_rows_past_the_end_are_not_stored(rows):
    """Every store is issued unconditionally over a descriptor of the tile's valid rows: with ``out`` the first ``rows`` rows
    of a buffer 64 rows long, pre-filled with a sentinel, every later row keeps the sentinel."""
    x, u, w, b, gamma, beta = _on_device(rows, "normal")
    sentinel = -123456.75
    buffer = torch.full((64, 64), sentinel, device=x.device)
    buffer[:rows] = u
    update = buffer[:rows]
    import ultra_torchdrug_amd as U
    from ultra_torchdrug_amd import functional as UF
    lib = U.require_library()
    lib.ultra_rspmm_force_general_path(NEW)
    try:
        out = UF.combine_forward(x, update, w, b, gamma, beta, 1e-5, True, True, reuse_update=True)
        torch.cuda.synchronize()
    finally:
        lib.ultra_rspmm_force_general_path(0)
    assert out.data_ptr() == buffer.data_ptr()
    assert bool((buffer[rows:] == sentinel).all()), "a row past the end was written"
    want = _oracle(rows, "normal", True, True, True).numpy()
    assert np.array_equal(buffer[:rows].cpu().numpy().view(np.int32), want.view(np.int32))

"""The paired form of the layer epilogue (combine_paired_kernel: two prefetching waves per SIMD, half the weight in LDS,
tiles drawn from a per-workgroup ticket) against the one-wave kernel it replaces and the oracle: EQUAL bits, no tolerance.

Every case runs three ways: knob 512 (paired form at every size), knob 256 (never the paired form) and
``oracle_combine_forward`` through ``oracle_ops.OracleFunctional.combine``.  Row counts (a row = 64 floats, a tile = 32
rows, a workgroup = 8 waves): 1 .. 257 for the tail tile, the clamp to the last row, a short tile's store descriptor and
fewer tiles than waves; 32 * 24 (+ 5) for several tiles per wave inside ONE workgroup (the ticket running out, the prefetch
of a tile that is never processed); 32 * 8 * n_cu * 3 + 5 for three tiles per wave on the full grid (every workgroup's
contiguous range, the range boundaries).  Operands are seeded normals, and values of the dyadic grid of ``exact_grid.py``:
there every product and partial sum of the Linear is exact in fp32, so without LayerNorm the result must also equal the
fp64 definition, whatever the order of the additions -- a wrong operand pairing cannot hide behind rounding.
"""
import numpy as np
import pytest
import torch

import exact_grid
from oracle_ops import OracleFunctional

pytestmark = pytest.mark.gpu

PAIRED, ONE_WAVE = 512, 256
SMALL_ROWS = [1, 31, 32, 33, 255, 256, 257, 32 * 24, 32 * 24 + 5]
_memo = {}


def _dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def _n_cu():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _full_grid_rows():
    return 32 * 8 * _n_cu() * 3 + 5


def _operands(rows, kind):
    """(x, u, w, b, gamma, beta) on the CPU, computed once per (rows, kind)."""
    key = ("operands", rows, kind)
    if key not in _memo:
        rng = np.random.default_rng(rows * 2 + (kind == "grid"))
        if kind == "grid":
            x, u = exact_grid.grid(rng, (rows, 64)), exact_grid.grid(rng, (rows, 64))
            w, b = exact_grid.grid(rng, (64, 128)), exact_grid.grid(rng, (64,))
        else:
            x = rng.standard_normal((rows, 64)).astype(np.float32)
            u = (3 * rng.standard_normal((rows, 64))).astype(np.float32)
            w = (rng.standard_normal((64, 128)) / np.sqrt(128)).astype(np.float32)
            b = (0.1 * rng.standard_normal(64)).astype(np.float32)
        gamma = (rng.random(64) + 0.5).astype(np.float32)
        beta = (0.1 * rng.standard_normal(64)).astype(np.float32)
        _memo[key] = tuple(torch.from_numpy(a) for a in (x, u, w, b, gamma, beta))
    return _memo[key]


def _on_device(rows, kind):
    key = ("device", rows, kind)
    if key not in _memo:
        _memo[key] = tuple(t.to(_dev()) for t in _operands(rows, kind))
    return _memo[key]


def _oracle(rows, kind, ln, relu, shortcut):
    key = ("oracle", rows, kind, ln, relu, shortcut)
    if key not in _memo:
        x, u, w, b, gamma, beta = _operands(rows, kind)
        with torch.no_grad():
            _memo[key] = OracleFunctional(None).combine(x, u, w, b, gamma if ln else None, beta if ln else None, 1e-5, relu, shortcut)
    return _memo[key]


def _run(knob, x, u, w, b, gamma, beta, ln, relu, shortcut, alias):
    """One launch under a knob value; ``alias``: the result overwrites (a copy of) ``update``."""
    import ultra_torchdrug_amd as U
    from ultra_torchdrug_amd import functional as UF
    lib = U.require_library()
    lib.ultra_rspmm_force_general_path(knob)
    try:
        upd = u.clone() if alias else u
        out = UF.combine_forward(x, upd, w, b, gamma if ln else None, beta if ln else None, 1e-5, relu, shortcut, reuse_update=alias)
        torch.cuda.synchronize()
        assert (out.data_ptr() == upd.data_ptr()) == alias
        return out
    finally:
        lib.ultra_rspmm_force_general_path(0)


def _check(rows, kind, ln, relu, shortcut, alias):
    ops = _on_device(rows, kind)
    paired = _run(PAIRED, *ops, ln, relu, shortcut, alias)
    one_wave = _run(ONE_WAVE, *ops, ln, relu, shortcut, alias)
    assert torch.equal(paired, one_wave), "the paired form differs from the one-wave kernel"
    assert torch.equal(paired.view(torch.int32), one_wave.view(torch.int32))
    got = paired.cpu().numpy()
    assert np.array_equal(got, _oracle(rows, kind, ln, relu, shortcut).numpy()), "the paired form differs from the oracle"
    if kind == "grid" and not ln:
        x, u, w, b = (t.numpy().astype(np.float64) for t in _operands(rows, kind)[:4])
        want = np.concatenate([x, u], axis=1) @ w.T + b
        assert np.abs(want).max() < 2.0 ** 24 / 16            # multiples of 1/16 below 2^20: exact in fp32 in any order
        if relu:
            want = np.where(want <= 0, 0.0, want)
        if shortcut:
            want = want + x
        assert np.array_equal(got.astype(np.float64), want), "the paired form differs from the fp64 definition"


@pytest.mark.parametrize("alias", [False, True], ids=["separate_out", "out_is_update"])
@pytest.mark.parametrize("kind", ["normal", "grid"])
@pytest.mark.parametrize("rows", SMALL_ROWS)
def test_paired_form_equals_one_wave_kernel_and_oracle(rows, kind, alias):
    _check(rows, kind, True, True, True, alias)


@pytest.mark.parametrize("alias", [False, True], ids=["separate_out", "out_is_update"])
@pytest.mark.parametrize("kind", ["normal", "grid"])
def test_paired_form_on_the_full_grid(kind, alias):
    """Three tiles per wave and a tail: every workgroup's contiguous range, its boundaries, the last row's clamp."""
    _check(_full_grid_rows(), kind, True, True, True, alias)


@pytest.mark.parametrize("alias", [False, True], ids=["separate_out", "out_is_update"])
@pytest.mark.parametrize("shortcut", [False, True], ids=["plain", "shortcut"])
@pytest.mark.parametrize("relu", [False, True], ids=["linear", "relu"])
@pytest.mark.parametrize("ln", [False, True], ids=["no_ln", "ln"])
@pytest.mark.parametrize("kind,rows", [("normal", 33), ("grid", 257), ("grid", 32 * 24 + 5)])
def test_paired_form_epilogue_options(kind, rows, ln, relu, shortcut, alias):
    _check(rows, kind, ln, relu, shortcut, alias)


@pytest.mark.parametrize("alias", [False, True], ids=["separate_out", "out_is_update"])
@pytest.mark.parametrize("ln", [False, True], ids=["no_ln", "ln"])
def test_non_finite_rows_stay_in_their_rows(ln, alias):
    """NaN and +-inf in a few rows of ``update``: those rows equal the one-wave kernel's bit for bit (relu keeps NaN:
    ``!(v <= 0) ? v : 0``), every other row is what it is without them."""
    rows = 32 * 24 + 5
    x, u, w, b, gamma, beta = _on_device(rows, "normal")
    bad = [0, 31, 32, 300, rows - 1]
    poisoned = u.clone()
    for k, r in enumerate(bad):
        poisoned[r, (7 * k) % 64] = (float("nan"), float("inf"), float("-inf"))[k % 3]
    poisoned[300, 5], poisoned[300, 6] = float("inf"), float("-inf")
    paired = _run(PAIRED, x, poisoned, w, b, gamma, beta, ln, True, True, alias)
    one_wave = _run(ONE_WAVE, x, poisoned, w, b, gamma, beta, ln, True, True, alias)
    assert torch.equal(paired.view(torch.int32), one_wave.view(torch.int32))
    clean = torch.ones(rows, dtype=torch.bool)
    clean[bad] = False
    assert not torch.isfinite(paired[~clean.to(paired.device)]).all(dim=1).any(), "a poisoned row came out finite"
    want = _oracle(rows, "normal", ln, True, True)
    assert np.array_equal(paired.cpu()[clean].numpy(), want[clean].numpy()), "a finite row changed"


@pytest.mark.parametrize("alias", [False, True], ids=["separate_out", "out_is_update"])
@pytest.mark.parametrize("side", ["below", "above"])
def test_default_dispatch_equals_one_wave_kernel(side, alias):
    """Either side of the size from which the epilogue prefetches (16 tiles per CU): the default equals knob 256."""
    tiles = 16 * _n_cu()
    rows = 32 * (tiles - 1) if side == "below" else 32 * tiles + 1
    ops = _on_device(rows, "normal")
    default = _run(0, *ops, True, True, True, alias)
    one_wave = _run(ONE_WAVE, *ops, True, True, True, alias)
    assert torch.equal(default.view(torch.int32), one_wave.view(torch.int32))
    sub = slice(rows - 2000, rows)
    x, u, w, b, gamma, beta = (t if t.dim() == 1 or t.shape[0] == 64 else t[sub] for t in _operands(rows, "normal"))
    with torch.no_grad():
        want = OracleFunctional(None).combine(x, u, w, b, gamma, beta, 1e-5, True, True)
    assert np.array_equal(default[sub].cpu().numpy(), want.numpy())

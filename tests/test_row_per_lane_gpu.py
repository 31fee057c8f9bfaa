"""The row-per-lane score head (``score_kernel``: the first layer issued as mfma(A = W1, B = rows), relu on the accumulators,
half-wave swaps, the ``w2`` chain from registers) against the form it replaces (``score_kernel_lds``, knob 1024: column per
lane, the row phase through LDS) and ``oracle.score_head_forward``: EQUAL bits, no tolerance.

Every case runs the default form, knob 1024 and the oracle.  Shapes ``(n_node, batch)``, a row = one (node, query) pair of 64
floats, a tile = 32 rows, a workgroup = 4 waves: (1, 1), (37, 3), (33, 31) for tiles that span several nodes and the
``% batch`` path; (200, 32), (150, 64) for the queries' sums ``c`` in LDS up to its limit; (100, 70) for ``c`` from memory;
(1000, 16) for the workload's batch width; and at batch 16 the smallest row count above ``32 * 4 * n_cu * 2 + 5`` (a
multiple of 16) for two tiles per wave on the full grid, the prefetch of a tile that is never processed and the clamp to
the last row.  Operands are seeded normals; once, values of the dyadic grid of ``exact_grid.py`` with limits under which
every partial sum of BOTH layers is exact in fp32 (the test asserts that bound from the operands' absolute values), so the
result must equal the fp64 definition in any order; and once one-hot rows against weights that are distinct in every entry,
so that a permuted output index is a wrong number and not a rounding difference.
"""
import numpy as np
import pytest
import torch

import exact_grid

pytestmark = pytest.mark.gpu

LDS_ROWS = 1024          # knob bit 10: the score head with the column-per-lane product and its LDS row phase
SHAPES = [(1, 1), (37, 3), (33, 31), (200, 32), (150, 64), (100, 70), (1000, 16)]
_memo = {}


def _dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def _full_grid_nodes():
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    return (32 * 4 * n_cu * 2 + 5 + 15) // 16


def _operands(n_node, batch, kind):
    """(hidden, query, w1, b1, w2, b2) as numpy arrays, computed once per case."""
    key = ("operands", n_node, batch, kind)
    if key in _memo:
        return _memo[key]
    rng = np.random.default_rng(1000 * n_node + batch)
    if kind == "grid":
        g = lambda *shape: exact_grid.grid(rng, shape, q=4, lim=2)
        ops = (g(n_node, batch, 64), g(batch, 64), g(128, 128), g(128), g(1, 128), g(1))
    elif kind == "onehot":
        hidden = np.zeros((n_node, batch, 64), dtype=np.float32)
        flat = hidden.reshape(-1, 64)
        flat[np.arange(len(flat)), (7 * np.arange(len(flat))) % 64] = 1.0
        w1 = (1.0 + np.arange(128 * 128).reshape(128, 128) / 2.0 ** 14).astype(np.float32)
        w2 = (1.0 + np.arange(128) / 256.0).astype(np.float32).reshape(1, 128)
        ops = (hidden, np.zeros((batch, 64), dtype=np.float32), w1, np.zeros(128, dtype=np.float32), w2,
               np.full(1, 0.5, dtype=np.float32))
    else:
        f = lambda a: a.astype(np.float32)
        ops = (f(rng.standard_normal((n_node, batch, 64))), f(rng.standard_normal((batch, 64))),
               f(rng.standard_normal((128, 128)) / np.sqrt(128)), f(0.1 * rng.standard_normal(128)),
               f(rng.standard_normal((1, 128)) / np.sqrt(128)), f(0.1 * rng.standard_normal(1)))
    _memo[key] = ops
    return ops


def _oracle(n_node, batch, kind):
    key = ("oracle", n_node, batch, kind)
    if key not in _memo:
        from oracle import oracle as O
        _memo[key] = O.score_head_forward(*_operands(n_node, batch, kind))
    return _memo[key]


def _run(knob, ops):
    """One launch of the score head under a knob value; ``ops`` on the device."""
    import ultra_torchdrug_amd as U
    from ultra_torchdrug_amd import functional as UF
    lib = U.require_library()
    lib.ultra_rspmm_force_general_path(knob)
    try:
        out = UF.score_all_entities(*ops)
        torch.cuda.synchronize()
        return out
    finally:
        lib.ultra_rspmm_force_general_path(0)


def _check(n_node, batch, kind):
    ops = tuple(torch.from_numpy(a).to(_dev()) for a in _operands(n_node, batch, kind))
    new, old = _run(0, ops), _run(LDS_ROWS, ops)
    assert new.shape == (batch, n_node)
    assert torch.equal(new, old), "the row-per-lane form differs from the LDS form"
    assert torch.equal(new.view(torch.int32), old.view(torch.int32))
    got = new.cpu().numpy()
    assert np.array_equal(got, _oracle(n_node, batch, kind)), "the row-per-lane form differs from the oracle"
    return got


@pytest.mark.parametrize("n_node,batch", SHAPES)
def test_row_per_lane_score_head_equals_lds_form_and_oracle(n_node, batch):
    _check(n_node, batch, "normal")


def test_row_per_lane_score_head_on_the_full_grid():
    """Two tiles per wave and a tail on every SIMD of the device: the carried (node, query) of a tile's first row, the
    prefetch past the end, the last row's clamp."""
    _check(_full_grid_nodes(), 16, "normal")


@pytest.mark.parametrize("n_node,batch", [(37, 3), (1000, 16), (100, 70)])
def test_row_per_lane_score_head_equals_the_fp64_definition_on_the_exact_grid(n_node, batch):
    hidden, query, w1, b1, w2, b2 = (a.astype(np.float64) for a in _operands(n_node, batch, "grid"))
    cat = np.concatenate([hidden, np.broadcast_to(query, (n_node, batch, 64))], axis=-1)
    # operands are multiples of 1/4: first-layer terms are multiples of 1/16, second-layer terms of 1/64; the sums of the
    # |terms| bound every partial sum in any order
    abs1 = np.abs(cat) @ np.abs(w1).T + np.abs(b1)
    abs2 = abs1 @ np.abs(w2[0]) + np.abs(b2)
    assert abs1.max() < 2.0 ** 24 / 16 and abs2.max() < 2.0 ** 24 / 64
    first = cat @ w1.T + b1
    want = (np.where(first <= 0, 0.0, first) @ w2[0] + b2[0]).T
    got = _check(n_node, batch, "grid")
    assert np.array_equal(got.astype(np.float64), want), "the row-per-lane form differs from the fp64 definition"


@pytest.mark.parametrize("n_node,batch", [(33, 31), (200, 32)])
def test_a_permuted_output_index_is_a_wrong_number(n_node, batch):
    """One-hot rows pick single columns of a first layer whose entries are all distinct (and positive: relu keeps them); the
    second layer's weights are distinct too.  Every product pairing is then visible in the score."""
    hidden, _, w1, _, w2, b2 = (a.astype(np.float64) for a in _operands(n_node, batch, "onehot"))
    got = _check(n_node, batch, "onehot")
    want = ((hidden @ w1[:, :64].T) @ w2[0] + b2[0]).T
    # the first layer is exact here (one non-zero product per chain); the second rounds 128 times, each by at most 2^-24 of a
    # partial sum that same-sign terms keep below the total
    np.testing.assert_allclose(got, want, rtol=2.0 ** -17, atol=0)
    assert len(np.unique(want.T.reshape(-1)[:64])) == 64       # rows 0..63 pick the 64 columns once each: 64 different scores


def test_non_finite_rows_stay_in_their_rows():
    """NaN, +inf, -inf and an inf / -inf pair in a few rows of ``hidden``: both forms agree on those rows in their int32
    bits, every other row is what it is without them."""
    n_node, batch = 200, 32
    ops = [torch.from_numpy(a).to(_dev()) for a in _operands(n_node, batch, "normal")]
    rows = n_node * batch
    bad = [0, 31, 32, 300, rows - 1]
    poisoned = ops[0].clone()
    flat = poisoned.view(rows, 64)
    for k, r in enumerate(bad):
        flat[r, (7 * k) % 64] = (float("nan"), float("inf"), float("-inf"))[k % 3]
    flat[300, 5], flat[300, 6] = float("inf"), float("-inf")
    ops[0] = poisoned
    new, old = _run(0, tuple(ops)), _run(LDS_ROWS, tuple(ops))
    assert torch.equal(new.view(torch.int32), old.view(torch.int32))
    got = new.cpu().t().reshape(rows)                                       # (B, N) -> row = node * batch + query
    clean = torch.ones(rows, dtype=torch.bool)
    clean[bad] = False
    assert not torch.isfinite(got[~clean]).any(), "a poisoned row came out finite"
    want = torch.from_numpy(_oracle(n_node, batch, "normal")).t().reshape(rows)
    assert torch.equal(got[clean], want[clean]), "a finite row changed"


def test_captured_score_head_replays_with_new_rows():
    """One ``torch.cuda.graph`` of the score head at the workload's batch width, replayed twice over changed ``hidden``."""
    from ultra_torchdrug_amd import functional as UF
    n_node, batch = 1000, 16
    ops = [torch.from_numpy(a).to(_dev()) for a in _operands(n_node, batch, "normal")]
    static = ops[0].clone()
    ops[0] = static
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        UF.score_all_entities(*ops)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = UF.score_all_entities(*ops)
    gen = torch.Generator(device="cpu").manual_seed(3)
    for _ in range(2):
        fresh = torch.randn(n_node, batch, 64, generator=gen).to(_dev())
        static.copy_(fresh)
        graph.replay()
        torch.cuda.synchronize()
        eager = UF.score_all_entities(fresh, *ops[1:])
        assert torch.equal(captured.view(torch.int32), eager.view(torch.int32))

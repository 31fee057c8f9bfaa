"""Exact-grid parity without a GPU (``tests/exact_grid.py``): the CPU operators of the product (``generalized_rspmm`` and
``rotate_rspmm`` on CPU tensors: ``csrc/torch_ext.cpp``) and the C oracle against the plain fp64 definition, on inputs where
fp32 arithmetic is exact -- ``np.array_equal`` on every entry, ties of min / max included (8 - 30 % of the cells): every tied
edge receives the gradient in full.

The product has no CPU kernel for ``d_weight`` (``generalized_rspmm`` refuses a sparse tensor that requires grad on CPU
tensors); on the host that gradient is the oracle's, which is compared here, and the HIP kernel's is compared in
``tests/test_exact_grid_gpu.py``."""
import numpy as np
import pytest
import torch

import exact_grid as XG
from graphs import random_graph

SUMS = ["add", "min", "max"]
# name: (graph kwargs, nodes, relations, F, rotate block)
CASES = {
    # zipf draws repeat triples: merged weights, zeros among them
    "duplicates_grid_weights": (dict(n_edge=3000, skew=True), 200, 7, 128, 64),
    # a hub row of 1 451 distinct triples out of 2 600 drawn (split by the oracle's pieces), rows without edges, F no multiple of anything
    "hub_isolated_ragged_F": (dict(n_edge=6000, hub_row=5, hub_edges=2600, isolated=150), 400, 5, 100, 20),
}
_cache = {}


def _case(case, message="mul"):
    """Graph and operands of a case, built once.  Rotate operands come from the grid ``|k| <= 4``: a rotate message is a
    difference of two products and ties less often than one product (4 - 10 % of the cells with ``|k| <= 8``, 11 - 17 % here)."""
    lim = 4 if message == "rotate" else 8
    if (case, lim) not in _cache:
        kw, n, r, F, block = CASES[case]
        g = random_graph(seed=len(case), n_node=n, n_rel=r, **kw)
        rng = np.random.default_rng(len(case) + 1)
        g["w"] = XG.grid_weights(rng, len(g["dst"]))
        relation, x = XG.grid(rng, (r, F), lim=lim), XG.grid(rng, (n, F), lim=lim)
        grad = XG.grid(rng, (n, F), zero=0.0)
        _cache[(case, lim)] = (g, n, r, F, block, relation, x, grad)
    return _cache[(case, lim)]


def _definition(case, sum, message):
    key = (case, sum, message)
    if key not in _cache:
        g, n, r, F, block, relation, x, grad = _case(case, message)
        if (case, message) not in _cache:
            XG.assert_all_exact(g["dst"], g["src"], g["rel"], g["w"], relation, x, grad, n, message, block)
            _cache[(case, message)] = True
        want = XG.definition(g["dst"], g["src"], g["rel"], g["w"], relation, x, grad, n, sum, message, block)
        if sum != "add":
            XG.assert_ties_matter(want[4], g["dst"], n, grad)
        _cache[key] = want
    return _cache[key]


def _same(got, want):
    return np.array_equal(np.asarray(got, dtype=np.float64), want)


def _csr(g, n, r):
    from ultra_torchdrug_amd import RelCSR
    t = torch.from_numpy
    return RelCSR(t(g["dst"]), t(g["src"]), t(g["rel"]), t(g["w"]), n, n, r)


def test_the_cases_hold_what_their_names_say():
    for case in CASES:
        g, n, r = _case(case)[:3]
        dst, _, _, w = XG.coalesce(g["dst"], g["src"], g["rel"], g["w"], n, r)
        assert (w == 0).any()
        if case == "duplicates_grid_weights":
            assert len(dst) < 0.9 * len(g["dst"]) and w.max() > 2.0
        else:
            deg = np.bincount(dst, minlength=n)
            assert deg.max() >= 1000 and (deg == 0).sum() >= 150


def test_grid_generators():
    rng = np.random.default_rng(0)
    v = XG.grid(rng, (200, 50))
    assert v.dtype == np.float32 and np.array_equal(v * 4, np.rint(v * 4)) and np.abs(v).max() == 2.0
    zeros = v == 0
    assert 0.25 < zeros.mean() < 0.4 and 0.3 < np.signbit(v[zeros]).mean() < 0.7
    w = XG.grid_weights(rng, 1000)
    assert w.dtype == np.float32 and set(np.unique(w)) == {0.0, 0.5, 1.0, 1.5, 2.0}
    with pytest.raises(AssertionError):
        XG.assert_exact(np.array([2.0 ** 19]), XG.UNIT)              # 2^24 * 2^-5
    with pytest.raises(AssertionError):
        XG.assert_exact(np.array([0.3]), XG.UNIT)
    XG.assert_exact(np.array([2.0 ** 19 - XG.UNIT, 0.0]), XG.UNIT)


def test_definition_on_a_hand_worked_tie():
    """Two edges into node 0 with the same message, a third below it: max feeds both tied edges in full."""
    dst, src, rel = [0, 0, 0], [0, 1, 2], [0, 0, 0]
    relation, x = np.array([[2.0]]), np.array([[1.0], [1.0], [0.5]])
    grad = np.array([[3.0], [0.0], [0.0]])
    out, d_x, d_r, d_w, tied = XG.definition(dst, src, rel, [1.0, 1.0, 1.0], relation, x, grad, 3, "max", "mul")
    assert out[0, 0] == 2.0 and out[1, 0] == -XG.FLT_MAX and tied[0, 0] and not tied[1, 0]
    assert d_x[:, 0].tolist() == [6.0, 6.0, 0.0] and d_r[0, 0] == 6.0 and d_w.tolist() == [6.0, 6.0, 0.0]
    out, d_x, d_r, d_w, tied = XG.definition(dst, src, rel, None, relation, x, grad, 3, "add", "mul")
    assert out[0, 0] == 5.0 and d_x[:, 0].tolist() == [6.0, 6.0, 6.0] and d_r[0, 0] == 7.5 and not tied.any()
    # rotate, one pair: (1 + 2i) * (3 + 4i) = -5 + 10i, weight 0.5
    out, d_x, d_r, d_w, _ = XG.definition([0], [0], [0], [0.5], np.array([[3.0, 4.0]]), np.array([[1.0, 2.0]]),
                                          np.array([[1.0, 1.0]]), 1, "min", "rotate", block=2)
    assert out.tolist() == [[-2.5, 5.0]] and d_w.tolist() == [5.0]
    assert d_x.tolist() == [[3.5, -0.5]] and d_r.tolist() == [[1.5, -0.5]]


@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("sum", SUMS)
@pytest.mark.parametrize("mul", ["mul", "add"])
def test_cpu_operator_equals_the_definition(case, sum, mul):
    from ultra_torchdrug_amd import functional as UF
    g, n, r, F, block, relation, x, grad = _case(case)
    out_w, d_x_w, d_r_w, _, _ = _definition(case, sum, mul)
    rel_t, x_t = torch.from_numpy(relation).requires_grad_(), torch.from_numpy(x).requires_grad_()
    out = UF.generalized_rspmm(_csr(g, n, r), rel_t, x_t, sum=sum, mul=mul)
    out.backward(torch.from_numpy(grad))
    assert _same(out.detach().numpy(), out_w), "forward"
    assert _same(x_t.grad.numpy(), d_x_w), "d_input"
    assert _same(rel_t.grad.numpy(), d_r_w), "d_relation"


@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("sum", SUMS)
def test_cpu_rotate_operator_equals_the_definition(case, sum):
    from ultra_torchdrug_amd import rotate_rspmm
    g, n, r, F, block, relation, x, grad = _case(case, "rotate")
    out_w, d_x_w, d_r_w, _, _ = _definition(case, sum, "rotate")
    rel_t, x_t = torch.from_numpy(relation).requires_grad_(), torch.from_numpy(x).requires_grad_()
    out = rotate_rspmm(_csr(g, n, r), rel_t, x_t, sum=sum, block=block)
    out.backward(torch.from_numpy(grad))
    assert _same(out.detach().numpy(), out_w), "forward"
    assert _same(x_t.grad.numpy(), d_x_w), "d_input"
    assert _same(rel_t.grad.numpy(), d_r_w), "d_relation"


@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("sum", SUMS)
@pytest.mark.parametrize("mul", ["mul", "add"])
@pytest.mark.parametrize("piece", [0, 48])
def test_oracle_equals_the_definition(oracle, case, sum, mul, piece):
    """The C oracle, sequential and in pieces: forward, d_input, d_relation and d_weight."""
    g, n, r, F, block, relation, x, grad = _case(case)
    out_w, d_x_w, d_r_w, d_w_w, _ = _definition(case, sum, mul)
    csr_o = oracle.coalesce_csr(g["dst"], g["src"], g["rel"], g["w"], n, n, r)
    assert csr_o.n_edges == len(d_w_w) and (piece == 0 or np.diff(csr_o.row_ptr).max() > piece)
    out = oracle.rspmm_forward(csr_o, relation, x, sum, mul, piece=piece)
    assert _same(out, out_w), "forward"
    d_r, d_x, d_w = oracle.rspmm_backward(csr_o, relation, x, out, grad, sum, mul, piece=piece, need_weight_grad=True)
    assert _same(d_x, d_x_w), "d_input"
    assert _same(d_r, d_r_w), "d_relation"
    assert _same(d_w, d_w_w), "d_weight"

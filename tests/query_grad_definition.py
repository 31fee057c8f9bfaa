"""Shared by tests/test_query_train_{cpu,gpu}.py: the two backwards of ``include/ultra_rspmm.h`` that training through logical
queries adds -- ``ultra_set_boundary_backward_f32`` and ``ultra_score_backward_f32`` -- restated in numpy fp64 from the header
alone, and the dyadic-grid inputs on which the first of them is exact in fp32.  This module imports neither the oracle nor the
package."""
import numpy as np

from exact_grid import grid


def keep_mask(member, floor=None):
    """bool ``(Q, N)``: the forward's rule, in fp32 -- ``m > 0`` and ``m >= floor[q]``; comparisons with a NaN are false."""
    member = np.asarray(member, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        keep = member > 0
        if floor is not None:
            keep &= member >= np.asarray(floor, dtype=np.float32)[:, None]
    return keep


def set_boundary_backward_numpy(d_boundary, member, floor, query):
    """``(d_member (Q, N), d_query (Q, D))`` in fp64.  A row that is not kept is SELECTED away: its ``d_boundary`` and ``query``
    values are never touched, it gives ``+0.0`` and adds nothing to ``d_query``."""
    keep = keep_mask(member, floor)
    n_query, n_node = keep.shape
    dim = np.shape(query)[1]
    d_member = np.zeros((n_query, n_node))
    d_query = np.zeros((n_query, dim))
    for q in range(n_query):
        rows = np.nonzero(keep[q])[0]
        if len(rows) == 0:
            continue
        g = np.asarray(d_boundary[rows, q, :], dtype=np.float64)
        d_member[q, rows] = (g * np.asarray(query[q], dtype=np.float64)[None, :]).sum(axis=1)
        d_query[q] = (np.asarray(member[q, rows], dtype=np.float64)[:, None] * g).sum(axis=0)
    return d_member, d_query


def score_backward_numpy(hidden, query, w1, b1, w2, grad):
    """``(d_hidden (N, B, 64), d_query (B, 64), d_w1 (128, 128), d_b1 (128,), d_w2 (128,), d_b2 (1,))`` in fp64 of
    ``score[b, n] = w2 . relu(W1 . cat[hidden[n, b], query[b]] + b1) + b2`` for ``grad`` ``(B, N)``; the ReLU passes gradient
    where the pre-activation is ``> 0``."""
    hidden, query, w1, b1, w2, grad = (np.asarray(a, dtype=np.float64) for a in (hidden, query, w1, b1, w2, grad))
    n_node, batch, _ = hidden.shape
    w2 = w2.reshape(128)
    x = np.concatenate([hidden, np.broadcast_to(query[None], (n_node, batch, 64))], axis=2)          # (N, B, 128)
    pre = x @ w1.T + b1
    d_pre = np.where(pre > 0, grad.T[:, :, None] * w2[None, None, :], 0.0)
    d_x = d_pre @ w1
    d_w1 = np.einsum("nbo,nbk->ok", d_pre, x)
    d_w2 = np.einsum("bn,nbo->o", grad, np.maximum(pre, 0.0))
    return d_x[:, :, :64], d_x[:, :, 64:].sum(axis=0), d_w1, d_pre.sum(axis=(0, 1)), d_w2, np.array([grad.sum()])


def grid_set_case(n_query, n_node, dim, seed):
    """``(member (Q, N), query (Q, D), floor (Q,), d_boundary (N, Q, D))`` fp32 numpy arrays for the set boundary's backward:
    memberships ``k / 4`` in ``(0, 2]`` with a share of zeros of both signs, negatives and NaN; ``d_boundary`` and ``query`` on
    the grid of tests/exact_grid.py.  Every term of ``d_member`` and ``d_query`` is a multiple of 1/16 of size at most 4, so up
    to 2^24 / 64 = 262 144 nodes every partial sum is exact in fp32 in any order.  The floors: 1.0 (on the grid: ties stay),
    0.875 (off it) -- both cut -- and, with three or more queries, row 2 keeps NOTHING (all its members are zero, negative or
    NaN), and there ``query`` holds ``inf`` and NaN; ``d_boundary`` holds ``inf`` / NaN at entries that are not kept."""
    rng = np.random.default_rng(seed)
    member = (rng.integers(1, 9, size=(n_query, n_node)) / 4.0).astype(np.float32)
    kind = rng.random((n_query, n_node))
    member[kind < 0.10] = 0.0
    member[(kind >= 0.10) & (kind < 0.15)] = -0.0
    negative = (kind >= 0.15) & (kind < 0.25)
    member[negative] = -member[negative]
    member[(kind >= 0.25) & (kind < 0.30)] = np.nan
    query = grid(rng, (n_query, dim))
    d_boundary = grid(rng, (n_node, n_query, dim))
    floor = np.full(n_query, 1.0, dtype=np.float32)
    floor[1::3] = 0.875
    if n_query > 2:
        row = member[2]
        row[row > 0] = -row[row > 0]
        query[2, 0] = np.inf
        query[2, dim - 1] = np.nan
    never = ~keep_mask(member, None)                              # not kept with or without the floor
    at = np.nonzero(never.T)                                      # (v, q) pairs
    pick = rng.random(len(at[0])) < 0.5
    d_boundary[at[0][pick], at[1][pick], 0] = np.inf
    d_boundary[at[0][pick], at[1][pick], dim - 1] = np.nan
    return member, query, floor, d_boundary


def grid_head_case(n_node, batch, seed, zero_rows=True):
    """``(hidden (N, B, 64), query (B, 64), w1 (128, 128), b1 (128,), w2 (128,), b2 (1,), grad (B, N))`` fp32 numpy arrays on
    the grid: every pre-activation is a sum of at most 129 multiples of 1/16 of size at most 4, exact in fp32 and fp64 alike,
    so no ReLU side can differ between the precisions.  ``zero_rows``: a fifth of the rows of ``grad`` (entities) are all
    zero."""
    rng = np.random.default_rng(seed)
    hidden = grid(rng, (n_node, batch, 64))
    query = grid(rng, (batch, 64))
    w1 = grid(rng, (128, 128))
    b1 = grid(rng, (128,))
    w2 = grid(rng, (128,))
    b2 = grid(rng, (1,))
    grad = grid(rng, (batch, n_node), zero=0.0)
    if zero_rows:
        grad[:, rng.random(n_node) < 0.2] = 0.0
    return hidden, query, w1, b1, w2, b2, grad

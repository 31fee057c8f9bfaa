"""Test infrastructure (numpy only): the per-query relation tables of ``NeuralBellmanFordNetwork`` and their three gradients as a
plain fp64 definition, written from ``include/ultra_rspmm.h`` alone:

    out[l][r, b, d]   = bias[l][r*D + d] + sum_k w[l][r*D + d, k] * query[b, k]
    d_w[l][(r,d), k]  = sum_b grad[l][r, b, d] * query[b, k]
    d_bias[l][(r,d)]  = sum_b grad[l][r, b, d]
    d_query[b, k]     = sum_l sum_(r,d) grad[l][r, b, d] * w[l][(r,d), k]

``grad[l] = None`` stands for zeros.  Beside each value the sum of the ABSOLUTE terms of every entry, which the exact-grid tests
(``exact_grid.assert_exact``) and the fp32 forward-error bounds need.  This module imports neither the oracle nor the package."""
import numpy as np


def _f64(a):
    return np.asarray(a, dtype=np.float64)


def tables(query, weights, biases, n_rel, absolute=False):
    """``[out_l (n_rel, batch * D_l)]``; ``absolute``: the sums of |terms| (``|bias| + sum_k |w| |query|``) instead."""
    q = _f64(query)
    q = np.abs(q) if absolute else q
    out = []
    for w, b in zip(weights, biases):
        w, b = _f64(w), _f64(b)
        if absolute:
            w, b = np.abs(w), np.abs(b)
        D = w.shape[0] // n_rel if n_rel else 0
        full = q @ w.T + b                                   # (batch, n_rel * D)
        out.append(full.reshape(len(q), n_rel, D).transpose(1, 0, 2).reshape(n_rel, len(q) * D))
    return out


def gradients(query, weights, grads, n_rel, absolute=False):
    """``(d_w list, d_bias list, d_query)``; ``absolute``: the sums of |terms| instead."""
    q = _f64(query)
    q = np.abs(q) if absolute else q
    batch, K = q.shape
    d_w, d_b = [], []
    d_q = np.zeros((batch, K))
    for w, g in zip(weights, grads):
        w = _f64(w)
        w = np.abs(w) if absolute else w
        D = w.shape[0] // n_rel if n_rel else 0
        if g is None:
            d_w.append(np.zeros_like(w))
            d_b.append(np.zeros(w.shape[0]))
            continue
        g = _f64(g).reshape(n_rel, batch, D)
        g = np.abs(g) if absolute else g
        rows = g.transpose(0, 2, 1).reshape(n_rel * D, batch)           # [(r, d), b]
        d_w.append(rows @ q)
        d_b.append(rows.sum(1))
        d_q += rows.T @ w
    return d_w, d_b, d_q

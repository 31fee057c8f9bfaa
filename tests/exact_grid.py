"""Test infrastructure (numpy only): rspmm on inputs where fp32 arithmetic is EXACT, and its plain fp64 definition.

Operands drawn from a small dyadic grid (``k / 4`` with ``|k| <= 8``, weights multiples of 0.5) make every product and every
partial sum of every kernel exactly representable in fp32, whatever the order of the additions, the piece length, the
kernel variant, wave shuffles or fp-contraction.  Every implementation of the operator must then EQUAL the fp64 definition
below -- ``np.array_equal``, no tolerance, nothing masked -- and min / max reductions tie in a large share of the cells
(zeros of either sign, zero weights, equal products), so the backward's equality mask ``output == w * message`` is exercised
where it matters: the convention (torchdrug's) is that EVERY tied edge receives the gradient in full.

The definition is written from ``include/ultra_rspmm.h`` alone:

    out[v]        = SUM over the coalesced edges (v, u, r, w) of  w * message(relation[r], input[u])
    d_input[u]   += (g * mask) * w * d message / d input          g = output_grad[v]
    d_relation[r]+= (g * mask) * w * d message / d relation       mask = (w * message == out[v]) under min / max, else 1
    d_weight[e]   = sum over the columns of (g * mask) * message  (the UNWEIGHTED message)

with ``message`` = ``rel * x`` (DistMult), ``rel + x`` (TransE) or the complex product of the rotate layout (per query block
of ``block`` columns: real parts in the first half, imaginary parts in the second).  An empty row holds 0 / +FLT_MAX /
-FLT_MAX.  This module imports neither the oracle nor the package.
"""
import numpy as np

FLT_MAX = float(np.finfo(np.float32).max)
# With the default grid: a forward / d_input / d_relation term is w (1/2) x two grid values (1/4 each), a d_weight term is
# three grid values.
UNIT = 2.0 ** -5
UNIT_WEIGHT = 2.0 ** -6


def grid(rng, shape, q=4, lim=8, zero=0.3):
    """float32 values ``k / q`` with integer ``1 <= |k| <= lim``, except for a share ``zero`` of the entries, which are exact
    zeros, half of those ``-0.0`` (``zero=0``: no entry is zero)."""
    k = rng.integers(1, lim + 1, size=shape) * rng.choice([-1, 1], size=shape)
    values = (k / float(q)).astype(np.float32)
    is_zero = rng.random(shape) < zero
    negative = rng.random(shape) < 0.5
    values[is_zero] = 0.0
    values[is_zero & negative] = -0.0
    return values


def grid_weights(rng, n, zero=0.1):
    """float32 multiples of 0.5 in [0, 2]; a share ``zero`` of them exactly 0."""
    w = (rng.integers(1, 5, size=n) / 2.0).astype(np.float32)
    w[rng.random(n) < zero] = 0.0
    return w


def coalesce(dst, src, rel, w, n_src, n_rel):
    """Distinct (dst, src, rel) triples sorted by that key, weights of duplicates summed (``w=None``: ones): the forward-plan
    order of the coalesced edges."""
    dst, src, rel = (np.asarray(a, dtype=np.int64) for a in (dst, src, rel))
    w = np.ones(len(dst)) if w is None else np.asarray(w, dtype=np.float64)
    key = (dst * n_src + src) * n_rel + rel
    uniq, inverse = np.unique(key, return_inverse=True)
    wsum = np.zeros(len(uniq))
    np.add.at(wsum, inverse.reshape(-1), w)
    return uniq // (n_src * n_rel), (uniq // n_rel) % n_src, uniq % n_rel, wsum


def _pairs(a, half):
    """(E, C) -> real and imaginary halves (E, C / (2 half), half) of every query block."""
    a = a.reshape(a.shape[0], -1, 2, half)
    return a[:, :, 0], a[:, :, 1]


def _columns(re, im):
    return np.stack([re, im], axis=2).reshape(re.shape[0], -1)


def _message(message, rl, xs, half, s):
    """Unweighted messages (E, C).  ``s`` = -1: the definition; +1 on absolute operands: the sum of the |terms|."""
    if message == "mul":
        return rl * xs
    if message == "add":
        return rl + xs
    (xr, xi), (rr, ri) = _pairs(xs, half), _pairs(rl, half)
    return _columns(xr * rr + s * (xi * ri), xr * ri + xi * rr)


def _gradient_terms(message, gm, y, rl, xs, half, s):
    """Per edge and column, before the weight: the terms of d_input, d_relation and d_weight for the masked gradient ``gm``."""
    if message == "mul":
        return gm * rl, gm * xs, gm * y
    if message == "add":
        return gm, gm, gm * y
    (xr, xi), (rr, ri), (gr, gi) = _pairs(xs, half), _pairs(rl, half), _pairs(gm, half)
    t_x = _columns(gr * rr + gi * ri, gi * rr + s * (gr * ri))
    t_r = _columns(gr * xr + gi * xi, gi * xr + s * (gr * xi))
    return t_x, t_r, gm * y


def _evaluate(dst, src, rel, w, relation, x, grad, n_rows, sum, message, block, absolute):
    if message not in ("mul", "add", "rotate") or sum not in ("add", "min", "max"):
        raise ValueError((sum, message))
    relation, x, grad = (np.asarray(a, dtype=np.float64) for a in (relation, x, grad))
    n_src, n_rel, F = x.shape[0], relation.shape[0], x.shape[1]
    dst, src, rel, w = coalesce(dst, src, rel, w, n_src, n_rel)
    s = -1.0
    if absolute:
        relation, x, grad, w, s = np.abs(relation), np.abs(x), np.abs(grad), np.abs(w), 1.0
    E = len(dst)
    half = 0
    if message == "rotate":
        if block is None or block <= 0 or block % 2 or F % block:
            raise ValueError("rotate messages need an even block that divides F")
        half = block // 2
    fill = {"add": 0.0, "min": FLT_MAX, "max": -FLT_MAX}[sum]
    reduce_at = {"add": np.add.at, "min": np.minimum.at, "max": np.maximum.at}[sum]
    out = np.full((n_rows, F), fill)
    d_x, d_r, d_w = np.zeros_like(x), np.zeros_like(relation), np.zeros(E)
    holders = np.zeros((n_rows, F), dtype=np.int64)
    # column slabs (whole query blocks for rotate) keep the (E, columns) temporaries small
    step = max(1, 1_000_000 // max(E, 1))
    if half:
        step = max(block, step // block * block)
    wc = w[:, None]
    for c0 in range(0, F, step):
        sl = slice(c0, min(F, c0 + step))
        rl, xs, g = relation[rel, sl], x[src, sl], grad[dst, sl]
        y = _message(message, rl, xs, half, s)
        wy = wc * y
        reduce_at(out[:, sl], dst, wy)
        gm = g
        if sum != "add":
            mask = wy == out[dst, sl]                      # EVERY tied edge (per component for rotate)
            np.add.at(holders[:, sl], dst, mask)
            gm = g * mask
        t_x, t_r, t_w = _gradient_terms(message, gm, y, rl, xs, half, s)
        np.add.at(d_x[:, sl], src, wc * t_x)
        np.add.at(d_r[:, sl], rel, wc * t_r)
        d_w += t_w.sum(axis=1)
    return out, d_x, d_r, d_w, holders > 1


def definition(dst, src, rel, w, relation, x, grad, n_rows, sum, message, block=None):
    """``(out, d_input, d_relation, d_weight, tied)`` in fp64 -- see the module docstring.  ``dst / src / rel / w``: the edges as
    given (duplicates allowed, ``w=None``: ones); ``d_weight``: one entry per COALESCED edge in (dst, src, rel) order;
    ``tied`` (n_rows, F) bool: the cells whose extreme is held by more than one edge (all False for ``sum="add"``)."""
    return _evaluate(dst, src, rel, w, relation, x, grad, n_rows, sum, message, block, False)


def abs_sums(dst, src, rel, w, relation, x, grad, n_rows, message, block=None):
    """``(out, d_input, d_relation, d_weight)``: per entry the fp64 sum of the |terms| of the unmasked sums (an upper bound of
    what any min / max mask lets through; for TransE ``|w| (|rel| + |x|)`` bounds ``|w (rel + x)|``)."""
    return _evaluate(dst, src, rel, w, relation, x, grad, n_rows, "add", message, block, True)[:4]


def assert_exact(terms_abs_sum, unit):
    """The precondition that makes a zero-tolerance comparison legitimate: every term of every sum is an integer multiple of
    ``unit`` and the sum of |terms| of every entry stays below ``2^24 * unit`` -- then every partial sum, in any order, is an
    integer multiple of ``unit`` below ``2^24 * unit`` and therefore exactly representable in fp32.  Computed from the
    definition's side only; a shape that violates it needs a smaller grid or hub, never a relaxed assertion."""
    t = np.asarray(terms_abs_sum, dtype=np.float64)
    if t.size == 0:
        return
    assert np.isfinite(t).all()
    scaled = t / unit
    assert np.array_equal(scaled, np.rint(scaled)), "a term is not a multiple of 2^%d" % int(np.log2(unit))
    assert t.max() < 2.0 ** 24 * unit, "sum of |terms| %.6g reaches 2^24 * unit = %.6g" % (t.max(), 2.0 ** 24 * unit)


def assert_all_exact(dst, src, rel, w, relation, x, grad, n_rows, message, block=None):
    """:func:`assert_exact` for all four quantities of a case."""
    out, d_x, d_r, d_w = abs_sums(dst, src, rel, w, relation, x, grad, n_rows, message, block)
    for t in (out, d_x, d_r):
        assert_exact(t, UNIT)
    assert_exact(d_w, UNIT_WEIGHT)


def tie_share(tied, dst, n_rows):
    """Share of the cells of non-empty rows that are tied."""
    live = np.bincount(np.asarray(dst, dtype=np.int64), minlength=n_rows) > 0
    cells = int(live.sum()) * tied.shape[1]
    return float(tied[live].sum()) / max(cells, 1)


def assert_ties_matter(tied, dst, n_rows, grad):
    """What keeps a min / max case from silently going tie-free: at least 5 % of the non-empty cells are tied (the sparsest
    case measured 8 %) and the output gradient is non-zero on every tied cell, so a wrong mask changes the result."""
    share = tie_share(tied, dst, n_rows)
    assert share >= 0.05, "only %.1f %% of the cells are tied" % (100 * share)
    assert (np.asarray(grad)[tied] != 0).all()

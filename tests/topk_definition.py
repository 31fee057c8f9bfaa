"""Shared by tests/test_answers_{cpu,gpu}.py: the top-K answers of a score row restated in numpy from the definition in
include/ultra_rspmm.h -- a ``lexsort`` on (entity index, NaN-last descending score) over the row with the known completions
removed.  Nothing is imported from the package; the completions come from a plain ``(E, 3)`` array of ``(h, t, r)`` triples."""
import numpy as np


def completions(triples, side, anchor, rel):
    """The DISTINCT entities that complete ``(anchor, rel, ?)`` (``side`` 0: tails of head ``anchor``) or ``(?, rel, anchor)``
    (``side`` 1: heads of tail ``anchor``) among ``triples``, an ``(E, 3)`` integer array of ``(h, t, r)`` rows."""
    triples = np.asarray(triples)
    hit = (triples[:, side] == anchor) & (triples[:, 2] == rel)
    return np.unique(triples[hit, 1 - side])


def topk_row(row, k, known=()):
    """``(index int64 (k,), value fp32 (k,))`` of one fp32 row: candidates = every position outside ``known``, ordered by score
    descending as floats (``-0.0 == +0.0``), equal scores by ascending position, NaN scores after every number (``-inf``
    included) and by ascending position among themselves; slots past the last candidate hold ``-1`` / ``-inf``."""
    row = np.asarray(row, dtype=np.float32)
    free = np.setdiff1d(np.arange(len(row)), np.asarray(known, dtype=np.int64))
    score = row[free]
    nan = np.isnan(score)
    falling = -np.where(nan, np.float32(0), score)            # ascending in it = descending in the score; +-0.0 compare equal
    order = np.lexsort((free, falling, nan))                  # last key first: numbers before NaN, then the score, then the index
    best = free[order][:k]
    index = np.full(k, -1, dtype=np.int64)
    value = np.full(k, -np.inf, dtype=np.float32)
    index[:len(best)] = best
    value[:len(best)] = row[best]
    return index, value


def topk_rows(pred, k, known_rows):
    """:func:`topk_row` over the rows of ``pred`` ``(Q, N)``; ``known_rows``: per row its known completions (``None``: no filter).
    Returns ``(index (Q, k), value (Q, k))``."""
    pred = np.asarray(pred, dtype=np.float32)
    pairs = [topk_row(pred[q], k, () if known_rows is None else known_rows[q]) for q in range(len(pred))]
    return np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])


def same_bits(a, b):
    """fp32 arrays equal bit for bit (NaN payloads and the sign of zero included)."""
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    return a.shape == b.shape and bool(np.array_equal(a.view(np.uint32), b.view(np.uint32)))


def special_scores(rows, n, seed):
    """fp32 ``(rows, 2, n)`` normal draws with NaN, both infinities and ``-0.0`` next to ``+0.0`` planted in every row, and one
    row of nothing but NaN."""
    import torch
    g = torch.Generator().manual_seed(seed)
    pred = torch.randn(rows, 2, n, generator=g)
    pred[:, :, 5::41] = float("nan")
    pred[:, :, 7::53] = float("inf")
    pred[:, :, 2::47] = -float("inf")
    pred[:, :, 100:104] = torch.tensor([0.0, -0.0, -0.0, 0.0])
    pred[:, :, 200:203] = torch.tensor([-0.0, 0.0, -0.0])
    pred[:, :, 30::17] = pred[:, :, 30::17].clamp(max=0.0) * 0.0          # zeros of both signs, spread out (-0.0 where negative)
    pred[2] = float("nan")
    return pred

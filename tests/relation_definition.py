"""Shared by tests/test_relation_{cpu,gpu}.py: relation prediction -- which candidate relations are known for a pair (h, t), the
filtered rank of a target relation and the K best relations -- restated in numpy from the definition in include/ultra_rspmm.h
(DESIGN.md section 20), over a plain ``(E, 3)`` array of ``(h, t, r)`` triples.  Nothing is imported from the package."""
from fractions import Fraction

import numpy as np

from topk_definition import same_bits, topk_row  # noqa: F401  (same_bits is re-exported to the tests)


def triple_set(triples):
    return {(int(h), int(t), int(r)) for h, t, r in np.asarray(triples)}


def known_row(facts, h, t, cand, n_rel, n_node=None):
    """bool ``(C,)``: candidate id ``c`` in ``[0, n_rel)`` is known iff ``(h, t, c)`` is a triple, ``c`` in ``[n_rel, 2 n_rel)`` iff
    ``(t, h, c - n_rel)`` is one (the triple ``t --(c - n_rel)--> h``); any other id never is.  ``facts``: :func:`triple_set`."""
    out = np.zeros(len(cand), dtype=bool)
    if n_node is not None and not (0 <= h < n_node and 0 <= t < n_node):
        return out
    for j, c in enumerate(np.asarray(cand).tolist()):
        if 0 <= c < n_rel:
            out[j] = (int(h), int(t), c) in facts
        elif n_rel <= c < 2 * n_rel:
            out[j] = (int(t), int(h), c - n_rel) in facts
    return out


def rank_row(row, cand, known, target):
    """``1 + #{j : not known[j] and row[j] >= row[j*]}`` with ``j*`` the first position that lists ``target`` (fp32 comparison:
    false for a NaN on either side; a target that is not known counts itself); 0 when ``target`` is -1 / ``None`` / not listed."""
    if target is None or target < 0:
        return 0
    at = np.flatnonzero(np.asarray(cand) == target)
    if len(at) == 0:
        return 0
    row = np.asarray(row, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        return 1 + int(np.count_nonzero(~known & (row >= row[at[0]])))


def select(score, cand, triples, h, t, target, n_rel, k, filtered=True, n_node=None):
    """The five results for a block ``score`` ``(P, C)``: dict of ``top_index (P, k)``, ``top_value (P, k)``, ``rank (P,)``,
    ``n_free (P,)``, ``known (P, C)``; ``cand=None`` is the identity list, ``target=None`` gives rank 0."""
    score = np.asarray(score, dtype=np.float32)
    n_pair, n_cand = score.shape
    cand = np.arange(n_cand, dtype=np.int64) if cand is None else np.asarray(cand, dtype=np.int64)
    facts = triple_set(triples) if filtered else set()
    out = {"top_index": np.full((n_pair, k), -1, dtype=np.int64), "top_value": np.full((n_pair, k), -np.inf, dtype=np.float32),
           "rank": np.zeros(n_pair, dtype=np.int64), "n_free": np.zeros(n_pair, dtype=np.int64),
           "known": np.zeros((n_pair, n_cand), dtype=np.uint8)}
    for p in range(n_pair):
        known = known_row(facts, int(h[p]), int(t[p]), cand, n_rel, n_node) if filtered else np.zeros(n_cand, dtype=bool)
        index, value = topk_row(score[p], k, np.flatnonzero(known))
        out["top_index"][p] = np.where(index < 0, -1, cand[np.maximum(index, 0)]) if n_cand else index
        out["top_value"][p] = value
        out["rank"][p] = rank_row(score[p], cand, known, None if target is None else int(target[p]))
        out["n_free"][p] = n_cand - int(known.sum())
        out["known"][p] = known
    return out


def metrics(ranks):
    """The ranking metrics of the ranks > 0 as exact fractions, and how many ranks are 0 (skipped)."""
    ranked = [int(r) for r in ranks if r > 0]
    n = len(ranked)
    out = {"skipped": len(ranks) - n}
    if n:
        out["mrr"] = sum(Fraction(1, r) for r in ranked) / n
        out["mr"] = Fraction(sum(ranked), n)
        for top in (1, 3, 10):
            out["hits@%d" % top] = Fraction(sum(r <= top for r in ranked), n)
    return out

"""Shared by tests/test_candidates_{cpu,gpu}.py: the definition of ``ultra_candidate_select_f32`` (include/ultra_rspmm.h) restated
in plain Python and numpy, and the seeded cases both files score.  Per query the list is filtered with a Python ``set`` of the
known completions and the candidates are sorted as tuples ``(class, -score, entity)``; nothing is imported from the package, and
nothing is compared with a tolerance: ids, counts and ranks are integers, values are bit patterns."""
import itertools

import numpy as np

OUTPUTS = ("top_index", "top_value", "rank", "n_free", "member")
SLICE = 32768                                   # list positions per workgroup; a longer max_len takes the two-launch form
GRID = np.array([-1.5, -1.0, -0.5, 0.0, 0.5, 1.0, 1.5, 2.0], dtype=np.float32)
GRID_WEIGHTS = np.array([0.5, 0.2, 0.1, 0.05, 0.05, 0.04, 0.03, 0.03])     # sum of squares 0.31: ties are common


def completion_sets(triples, side):
    """``{(anchor, rel): set of the other entity}`` of ``(E, 3)`` rows of (h, t, r): ``side`` 0 the tails of (h, r, ?), ``side``
    1 the heads of (?, r, t)."""
    found = {}
    for row in np.asarray(triples).tolist():
        found.setdefault((row[side], row[2]), set()).add(row[1 - side])
    return found


def completion_keys(triples, side, n_rel, n_node):
    """The sorted distinct keys ``(anchor * n_rel + rel) * n_node + other`` of ``triples``, int64."""
    t = np.asarray(triples, dtype=np.int64).reshape(-1, 3)
    return np.unique((t[:, side] * n_rel + t[:, 2]) * n_node + t[:, 1 - side])


def select_row(row, listed, known, target, k):
    """One query: ``listed`` its list of entities (``None``: every entity), ``known`` a set, ``target`` an entity, -1 or None."""
    row = np.asarray(row, dtype=np.float32)
    score = row.tolist()                                        # Python floats hold every fp32 exactly
    listed = range(len(score)) if listed is None else [int(e) for e in listed]
    cand = [e for e in listed if e not in known]
    # (class, -score, entity): numbers before NaN; -(-0.0) == -(+0.0) in Python, so zeros of both signs tie
    best = sorted(cand, key=lambda e: (1, 0.0, e) if score[e] != score[e] else (0, -score[e], e))[:k]
    index = np.full(k, -1, dtype=np.int64)
    value = np.full(k, -np.inf, dtype=np.float32)
    index[:len(best)] = best
    value[:len(best)] = row[best] if best else []
    rank, member = 0, 0
    if target is not None and target >= 0:
        pos = score[target]
        rank = 1 + sum(1 for e in cand if pos <= score[e])      # false for a NaN on either side
        member = int(target in (listed if isinstance(listed, range) else set(listed)))
    return index, value, rank, len(cand), member


def select(pred, sets, set_of, known_rows, target, k, max_len=None):
    """The five outputs of the operator as a dict of arrays.  ``sets``: a list of ascending entity arrays; ``set_of``: per query a
    set id or -1 (``None``: -1 for all); ``known_rows``: per query a set of completions (``None``: nothing is filtered);
    ``target``: per query an entity or -1 (``None``: no target); ``max_len``: only the first ``max_len`` positions of a list."""
    pred = np.asarray(pred, dtype=np.float32)
    rows = []
    for q in range(len(pred)):
        s = -1 if set_of is None else int(set_of[q])
        listed = None if s == -1 else sets[s]
        if max_len is not None:
            listed = (range(len(pred[q])) if listed is None else listed)[:max_len]
        rows.append(select_row(pred[q], listed, set() if known_rows is None else known_rows[q],
                               None if target is None else int(target[q]), k))
    out = {"top_index": np.stack([r[0] for r in rows]), "top_value": np.stack([r[1] for r in rows])}
    for i, name in ((2, "rank"), (3, "n_free")):
        out[name] = np.array([r[i] for r in rows], dtype=np.int64)
    out["member"] = np.array([r[4] for r in rows], dtype=np.uint8)
    return out


def subsets():
    """Every non-empty subset of the outputs, 31 of them."""
    return [c for n in range(1, 6) for c in itertools.combinations(OUTPUTS, n)]


# -------------------------------------------------------------------------------------------------------------- the cases
def grid_scores(rng, rows, n):
    """fp32 ``(rows, n)`` on the 8-value grid, the low values drawn more often, with zeros of both signs, both infinities and
    NaN planted in every row."""
    pred = rng.choice(GRID, size=(rows, n), p=GRID_WEIGHTS).astype(np.float32)
    where = rng.permutation(n)
    share = max(n // 40, 1)
    for i, v in enumerate((np.float32(-0.0), np.float32("inf"), np.float32("-inf"), np.float32("nan"))):
        pred[:, where[i * share:(i + 1) * share]] = v
    return pred


def make_case(n_node, lengths, seed, n_rel=3, n_all=1, all_known=(), known_share=0.15, nan_target=None):
    """One call's inputs: a set of every length in ``lengths`` (query ``i`` takes set ``i``) and ``n_all`` queries that take every
    entity; every query has its own ``(anchor, rel)`` with ``known_share`` of its list among its completions -- the queries in
    ``all_known`` have their whole list there -- plus 20 completions anywhere; the targets cycle through an entity inside the
    list, one outside it and -1; ``nan_target``: a query whose target scores NaN."""
    rng = np.random.default_rng(seed)
    sets = [np.sort(rng.choice(n_node, size=n, replace=False)).astype(np.int64) for n in lengths]
    n_query = len(lengths) + n_all
    set_of = np.array(list(range(len(lengths))) + [-1] * n_all, dtype=np.int64)
    anchor = rng.choice(n_node, size=n_query, replace=False).astype(np.int64)
    rel = rng.integers(0, n_rel, n_query).astype(np.int64)
    pred = grid_scores(rng, n_query, n_node)
    triples, target = [], []
    for q in range(n_query):
        listed = np.arange(n_node) if set_of[q] == -1 else sets[set_of[q]]
        known = listed if q in all_known else listed[rng.random(len(listed)) < known_share]
        known = np.union1d(known, rng.integers(0, n_node, 20))
        triples.append(np.stack([np.full(len(known), anchor[q]), known, np.full(len(known), rel[q])], axis=1))
        outside = np.setdiff1d(np.arange(min(n_node, 4 * len(listed) + 8)), listed)
        kind = q % 3 if len(listed) else 1
        if kind == 1 and len(outside) == 0:
            kind = 0
        target.append(int(listed[len(listed) // 2]) if kind == 0 else int(outside[len(outside) // 3]) if kind == 1 else -1)
    target = np.array(target, dtype=np.int64)
    if nan_target is not None:
        assert target[nan_target] >= 0
        pred[nan_target, target[nan_target]] = np.float32("nan")
    triples = np.concatenate(triples).astype(np.int64)
    known_rows = completion_sets(triples, 0)
    return {"n_node": n_node, "n_rel": n_rel, "sets": sets, "set_of": set_of, "anchor": anchor, "rel": rel, "pred": pred,
            "target": target, "triples": triples, "keys": completion_keys(triples, 0, n_rel, n_node),
            "known_rows": [known_rows.get((int(a), int(r)), set()) for a, r in zip(anchor, rel)],
            "max_len": max([len(s) for s in sets] + [n_node if n_all else 0])}


def tie_fraction(case):
    """The share of compared pairs -- two candidates of one query, as the ordering compares them, and a query's target against
    each of its candidates, as the rank does -- whose scores are equal as floats (a NaN equals nothing)."""
    ties = pairs = 0
    for q in range(len(case["pred"])):
        s = case["set_of"][q]
        listed = np.arange(case["n_node"]) if s == -1 else case["sets"][s]
        cand = np.array([e for e in listed.tolist() if e not in case["known_rows"][q]], dtype=np.int64)
        score = case["pred"][q, cand]
        count = np.unique(score[~np.isnan(score)], return_counts=True)[1].astype(np.int64)
        ties += int((count * (count - 1) // 2).sum())
        pairs += len(cand) * (len(cand) - 1) // 2
        if case["target"][q] >= 0:
            ties += int((score == case["pred"][q, case["target"][q]]).sum())
            pairs += len(cand)
    return ties / max(pairs, 1)


# the sizes where the walk changes shape: wave and workgroup edges, the tile of 1024, a list whose first tile alone overflows the
# 896 free LDS slots (a flush inside the walk), then the slice edge and three slices
EDGE_LENGTHS = [0, 1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2000]
CASES = {
    # query 3 (64 items) has every candidate among its completions; query 1 has one candidate at most: fewer than any k
    "edges": dict(n_node=3000, lengths=EDGE_LENGTHS, seed=11, n_all=2, all_known=(3,), nan_target=6),
    "slice": dict(n_node=80000, lengths=[SLICE, 5], seed=12, n_all=0, nan_target=0),               # one launch at its longest
    "slices": dict(n_node=80000, lengths=[SLICE, SLICE + 1, 70001], seed=13, n_all=1, all_known=(1,), nan_target=0),
}
_made = {}


def case(name):
    """The case ``name`` of :data:`CASES`, built once per process and never changed."""
    if name not in _made:
        _made[name] = make_case(**CASES[name])
    return _made[name]


_wanted = {}


def expected(name, k, filtered=True, with_sets=True, with_target=True):
    """:func:`select` of a case, computed once per process."""
    key = (name, k, filtered, with_sets, with_target)
    if key not in _wanted:
        c = case(name)
        _wanted[key] = select(c["pred"], c["sets"], c["set_of"] if with_sets else None, c["known_rows"] if filtered else None,
                              c["target"] if with_target else None, k)
    return _wanted[key]

"""Shared by tests/test_constrained_negatives_{cpu,gpu}.py: the definition of ``ultra_constrained_negative`` (include/ultra_rspmm.h)
restated in plain Python and numpy, and the seeded cases both files draw from.  Per row the list is filtered with a Python ``set``
of the known completions and indexed with the fp32 product ``rand * n_free``, truncated and clamped; nothing is imported from the
package and nothing is compared with a tolerance: entities and counts are integers."""
import numpy as np

from candidate_definition import completion_keys, completion_sets

CHUNK = 32768                                   # list positions per bitmap of the kernel; a longer list is walked twice
BELOW_ONE = np.nextafter(np.float32(1), np.float32(0))


def index_of(r, n_free):
    """``min((long long)(r * (float)n_free), n_free - 1)`` with the product in fp32; a negative product or a NaN gives 0."""
    x = np.float32(r) * np.float32(n_free)
    if not x >= 0:
        return 0
    return min(int(x), n_free - 1)


def draw_row(n_node, listed, known, rand_row, min_free=1):
    """One row: ``listed`` its list of entities (``None``: every entity), ``known`` a set.  Returns ``(entities, set-side count)``."""
    every = [e for e in range(n_node) if e not in known]
    free = every if listed is None else [int(e) for e in listed if 0 <= int(e) < n_node and int(e) not in known]
    source = free if len(free) >= min_free else every          # the fallback: the unconstrained strict draw
    if not source:
        return [0] * len(rand_row), len(free)
    return [source[index_of(r, len(source))] for r in rand_row], len(free)


def draw(n_node, sets, set_of, known_rows, rand, min_free=1):
    """``(out int64 (B, S), n_free int64 (B,))``.  ``sets``: a list of ascending entity arrays; ``set_of``: per row a set id, -1 for
    every entity, anything outside ``[-1, len(sets))`` for the empty list (``None``: -1 for all)."""
    out, count = [], []
    for q in range(len(rand)):
        s = -1 if set_of is None else int(set_of[q])
        listed = None if s == -1 else (sets[s] if 0 <= s < len(sets) else [])
        row, n_free = draw_row(n_node, listed, known_rows[q], rand[q], min_free)
        out.append(row)
        count.append(n_free)
    return np.array(out, dtype=np.int64).reshape(len(rand), -1), np.array(count, dtype=np.int64)


def edge_rand(rng, rows, n_sample):
    """fp32 ``(rows, n_sample)`` uniform numbers in ``[0, 1)`` with ``0.0``, the largest float below 1, ``0.5`` and exactly ``1.0``
    (clamped to the last free entity) planted in every row."""
    rand = rng.random((rows, n_sample), dtype=np.float32)
    for i, v in enumerate((np.float32(0), BELOW_ONE, np.float32(0.5), np.float32(1))):
        rand[:, i::11] = v
    return rand


def make_case(n_node, lengths, seed, n_rel=3, n_all=1, known_share=0.15, n_sample=128, known_of=None):
    """One call's inputs, built like ``candidate_definition.make_case``: a set of every length in ``lengths`` (row ``i`` takes set
    ``i``) and ``n_all`` rows that take every entity; every row has its own ``(anchor, rel)`` with ``known_share`` of its list among
    its completions plus 20 completions anywhere.  ``known_of``: ``{row: function(list) -> known entities}`` replaces a row's."""
    rng = np.random.default_rng(seed)
    sets = [np.sort(rng.choice(n_node, size=n, replace=False)).astype(np.int64) for n in lengths]
    rows = len(lengths) + n_all
    set_of = np.array(list(range(len(lengths))) + [-1] * n_all, dtype=np.int64)
    anchor = rng.choice(n_node, size=rows, replace=False).astype(np.int64)
    rel = rng.integers(0, n_rel, rows).astype(np.int64)
    triples = []
    for q in range(rows):
        listed = np.arange(n_node) if set_of[q] == -1 else sets[set_of[q]]
        if known_of is not None and q in known_of:
            known = np.asarray(known_of[q](listed), dtype=np.int64)
        else:
            known = np.union1d(listed[rng.random(len(listed)) < known_share], rng.integers(0, n_node, 20))
        triples.append(np.stack([np.full(len(known), anchor[q]), known, np.full(len(known), rel[q])], axis=1))
    triples = np.concatenate(triples).astype(np.int64).reshape(-1, 3)
    found = completion_sets(triples, 0)
    return {"n_node": n_node, "n_rel": n_rel, "sets": sets, "set_of": set_of, "anchor": anchor, "rel": rel,
            "rand": edge_rand(rng, rows, n_sample), "keys": completion_keys(triples, 0, n_rel, n_node),
            "known_rows": [found.get((int(a), int(r)), set()) for a, r in zip(anchor, rel)]}


# the sizes where the walk changes shape: wave and workgroup edges, the tile of 256 positions, the words of the bitmap, then the
# chunk edge and three chunks
EDGE_LENGTHS = [0, 1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2000]
CASES = {
    "edges": dict(n_node=3000, lengths=EDGE_LENGTHS, seed=21, n_all=2),
    "chunk": dict(n_node=80000, lengths=[CHUNK], seed=22, n_all=0),                  # one walk at its longest
    # two and three chunks, a -1 row; the second chunk of the first list is its last item alone, kept free (every 7th before it
    # is known), so that a rand just below 1 lands there
    "chunks": dict(n_node=80000, lengths=[CHUNK + 1, 70001], seed=23, n_all=1, known_of={0: lambda l: l[:-1:7]}),
    # only the list's first and only its last item are free; everything free but the list's middle chunk (no free entity
    # between two chunks that have some); the same with the first chunk empty
    "ends": dict(n_node=100000, lengths=[2000, 70001, 3 * CHUNK, 3 * CHUNK], seed=24, n_all=0,
                 known_of={0: lambda l: l[1:-1], 1: lambda l: l[1:-1], 2: lambda l: l[CHUNK:2 * CHUNK], 3: lambda l: l[:CHUNK]}),
}
_made, _wanted = {}, {}


def case(name):
    """The case ``name`` of :data:`CASES`, built once per process and never changed."""
    if name not in _made:
        _made[name] = make_case(**CASES[name])
    return _made[name]


def expected(name, n_sample=128, min_free=1, with_sets=True):
    """:func:`draw` of a case on the first ``n_sample`` columns of its ``rand``, computed once per process."""
    key = (name, n_sample, min_free, with_sets)
    if key not in _wanted:
        c = case(name)
        _wanted[key] = draw(c["n_node"], c["sets"], c["set_of"] if with_sets else None, c["known_rows"], c["rand"][:, :n_sample],
                            min_free)
    return _wanted[key]


def wide_rand(name, n_sample, seed=3):
    """fp32 ``(rows, n_sample)`` for a case whose own ``rand`` is narrower (``n_sample`` past one workgroup's width)."""
    return edge_rand(np.random.default_rng(seed), len(case(name)["set_of"]), n_sample)

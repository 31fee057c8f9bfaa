"""Knowledge-graph inputs for the hot path: seeded synthetic graphs of the benchmark shapes and a triple reader.

The reference downloads its datasets at run time (``/root/reference/ultra/dataset.py:165,179,450-460``) and
takes FB15k237 / WN18RR from torchdrug; there is no network here, so benchmarks and tests use synthetic graphs of
the same sizes.  A ``(h, r, t)``-per-line reader of the same shape as ``dataset.py:69-96`` lets a
real split be used when one is present on disk.
"""
import os

import numpy as np
import torch

from .graph import Graph

# name: (num_node, train triples, base relations)   -- sizes from SURVEY.md 8a / 8d
SHAPES = {
    "S-codexs": (2034, 32888, 42),
    "S-wn18rr": (40943, 86835, 11),
    "S-fb15k237": (14541, 272115, 237),
    "S-codexm": (17050, 185584, 51),
    "S-stress": (10_000_000, 50_000_000, 500),
    "S-tiny": (300, 2000, 6),
}
DEFAULT_SEED = 1024     # the reference's default seed (ultra/util.py:77)


def _zipf_ranks(rng, n, size, alpha):
    """Ranks 0..n-1 with P(k) ~ 1/(k+1)^alpha (alpha <= 0: uniform)."""
    if alpha <= 0:
        return rng.integers(0, n, size)
    p = 1.0 / np.arange(1, n + 1, dtype=np.float64) ** alpha
    cdf = np.cumsum(p)
    cdf /= cdf[-1]
    return np.minimum(np.searchsorted(cdf, rng.random(size), side="right"), n - 1)


def synthetic_triples(name_or_shape, seed=DEFAULT_SEED, alpha=None):
    """``(h, t, r)`` int64 triples ``(T, 3)`` in the reference's column order (``ultra/task.py:123``).
    Heads, tails and relations ~ Zipf(alpha) (alpha=1 for the KG shapes, uniform for S-stress); duplicates and
    drawn until exactly the requested number of DISTINCT triples exists, so E = 2 * triples after inverses."""
    n_node, n_triple, n_rel = SHAPES[name_or_shape] if isinstance(name_or_shape, str) else name_or_shape
    if alpha is None:
        alpha = 0.0 if name_or_shape == "S-stress" else 1.0
    rng = np.random.default_rng(seed)
    dedup = n_node * n_node * n_rel < 2 ** 62
    triples = np.zeros((0, 3), dtype=np.int64)
    want = n_triple
    for _ in range(64):                    # oversample until n_triple DISTINCT triples exist (hubs collide often)
        m = int((want - len(triples)) * 1.3) + 16
        new = np.stack([_zipf_ranks(rng, n_node, m, alpha), _zipf_ranks(rng, n_node, m, alpha),
                        _zipf_ranks(rng, n_rel, m, alpha)], axis=1).astype(np.int64)
        triples = np.concatenate([triples, new])
        if dedup:
            key = (triples[:, 0] * n_node + triples[:, 1]) * n_rel + triples[:, 2]
            _, first = np.unique(key, return_index=True)
            triples = triples[np.sort(first)]
        if len(triples) >= want:
            break
    triples = triples[:want]
    # hubs get arbitrary ids
    node_perm, rel_perm = rng.permutation(n_node), rng.permutation(n_rel)
    triples = np.stack([node_perm[triples[:, 0]], node_perm[triples[:, 1]], rel_perm[triples[:, 2]]], axis=1)
    return triples, n_node, n_rel


def synthetic_kg(name_or_shape="S-fb15k237", seed=DEFAULT_SEED, device="cpu", alpha=None):
    """Fact graph (edge_list rows = (h, t, r), as torchdrug KG datasets store them) of a benchmark shape."""
    triples, n_node, n_rel = synthetic_triples(name_or_shape, seed, alpha)
    return Graph(torch.from_numpy(triples).to(device), num_node=n_node, num_relation=n_rel)


def stress_task(device, n_node=None, n_triple=None, n_rel=None, seed=DEFAULT_SEED):
    """BASELINE config 5 as a TASK: the shipped 6 x 64d architecture (seeded random init) over S-stress built ON THE DEVICE --
    uniform heads / tails / relations (duplicates, about 1 in 10^4, are merged by the plans) -- with every triple
    a fact.  10 M nodes / 50 M triples / 500 relations by default: 100 M edges and 1 000 relations as rspmm sees them.
    Returns ``(task in eval mode, generator)``; the generator continues the seeded stream (test batches)."""
    from .task import build_ultra
    d_node, d_triple, d_rel = SHAPES["S-stress"]
    n_node, n_triple, n_rel = int(n_node or d_node), int(n_triple or d_triple), int(n_rel or d_rel)
    gen = torch.Generator(device=device).manual_seed(seed)
    cols = [torch.randint(0, n, (n_triple,), device=device, generator=gen) for n in (n_node, n_node, n_rel)]
    triples = torch.stack(cols, dim=1)
    del cols
    torch.manual_seed(seed)
    task = build_ultra(n_rel).to(device).eval()
    task.preprocess(Graph(triples, None, n_node, n_rel))
    return task, gen


class CandidateSets:
    """``S`` sets of entities in CSR form, the admissible answers of ``task.answer(candidates=...)``, ``task.rank_among`` and
    ``functional.candidate_select``: ``ptr`` int64 ``(S + 1,)``, ``items`` int32 ``(ptr[S],)`` with the
    items of every set ASCENDING and DISTINCT, each in ``[0, num_node)``; ``max_len`` the longest set's length (a host int).
    The constructor checks all of that with ONE host read (``validate=False``: the caller vouches for it and passes
    ``max_len``).  :meth:`to` moves it."""

    def __init__(self, ptr, items, num_node, max_len=None, validate=True):
        ptr, items = torch.as_tensor(ptr), torch.as_tensor(items)
        num_node = int(num_node)
        if ptr.dtype != torch.int64 or ptr.dim() != 1 or ptr.numel() < 1:
            raise ValueError("CandidateSets: ptr must be int64 (S + 1,), got %s %s" % (ptr.dtype, tuple(ptr.shape)))
        if items.dtype != torch.int32 or items.dim() != 1 or items.device != ptr.device:
            raise ValueError("CandidateSets: items must be int32 (ptr[S],) on %s, got %s %s on %s"
                             % (ptr.device, items.dtype, tuple(items.shape), items.device))
        if not 1 <= num_node < 2 ** 31:
            raise ValueError("CandidateSets: num_node must be in [1, 2^31), got %d" % num_node)
        self.ptr, self.items, self.num_node = ptr.contiguous(), items.contiguous(), num_node
        if validate:
            n = items.numel()
            length = ptr[1:] - ptr[:-1]
            bad_ptr = (ptr[0] != 0) | (ptr[-1] != n) | (length < 0).any()
            bad_item = ((items < 0) | (items >= num_node)).any()
            starts = torch.zeros(n + 1, dtype=torch.bool, device=ptr.device)
            starts[ptr.clamp(0, n)] = True                                       # position i begins a set
            bad_order = (~((items[1:] > items[:-1]) | starts[1:n])).any() if n > 1 else torch.zeros((), dtype=torch.bool, device=ptr.device)
            longest = length.max() if length.numel() else torch.zeros((), dtype=torch.int64, device=ptr.device)
            bad_ptr, bad_item, bad_order, longest = torch.stack([bad_ptr.long(), bad_item.long(), bad_order.long(), longest]).tolist()
            if bad_ptr:
                raise ValueError("CandidateSets: ptr must start at 0, never decrease and end at len(items) = %d" % n)
            if bad_item:
                raise ValueError("CandidateSets: items outside [0, %d)" % num_node)
            if bad_order:
                raise ValueError("CandidateSets: the items of a set must be ascending and distinct")
            max_len = longest
        elif max_len is None:
            raise ValueError("CandidateSets: validate=False needs max_len")
        self.max_len = int(max_len)

    @property
    def num_sets(self):
        return self.ptr.numel() - 1

    def __len__(self):
        return self.num_sets

    @property
    def device(self):
        return self.ptr.device

    def to(self, device):
        """The same sets on ``device`` (not validated again)."""
        return CandidateSets(self.ptr.to(device), self.items.to(device), self.num_node, self.max_len, validate=False)

    def set(self, s):
        """The items of set ``s``, int32 (a view)."""
        first, last = self.ptr[s:s + 2].tolist()
        return self.items[first:last]


def _sets_from_keys(keys, n_sets, num_node):
    """:class:`CandidateSets` from int64 keys ``set * num_node + entity`` (any order, duplicates merged)."""
    keys = torch.unique(keys)                                                    # sorted and distinct
    ptr = torch.searchsorted(keys, torch.arange(n_sets + 1, dtype=torch.int64, device=keys.device) * num_node)
    return CandidateSets(ptr, (keys % num_node).to(torch.int32), num_node)


def relation_candidates(triples, num_node, num_relation):
    """The type constraints a graph implies, ``2R`` :class:`CandidateSets` from ``(n, 3)`` rows of ``(h, t, r)``: set ``r`` is
    ``{t : (h, r, t)}``, the RANGE of ``r`` -- the admissible tails of ``(h, r, ?)`` -- and set ``r + R`` is ``{h : (h, r, t)}``,
    the range of the inverse relation, i.e. the DOMAIN of ``r`` -- the admissible heads of ``(?, r, t)``, which the package asks
    as ``(t, r + R, ?)``.  A relation without a triple gets the empty set.  Ids out of range raise ``ValueError``."""
    triples = torch.as_tensor(triples)
    num_node, num_relation = int(num_node), int(num_relation)
    if triples.dim() != 2 or triples.shape[1] != 3 or triples.dtype != torch.int64:
        raise ValueError("relation_candidates takes int64 (n, 3) rows of (h, t, r), got %s %s" % (triples.dtype, tuple(triples.shape)))
    if num_relation < 0 or not 1 <= num_node < 2 ** 31:
        raise ValueError("relation_candidates: %d entities and %d relations" % (num_node, num_relation))
    h, t, r = triples.t()
    if len(triples):
        lo, hi_node, hi_rel = torch.stack([triples.min(), torch.max(h.max(), t.max()), r.max()]).tolist()
        if lo < 0 or hi_node >= num_node or hi_rel >= num_relation:
            raise ValueError("relation_candidates: triples out of range for %d entities and %d relations: min id %d, max entity "
                             "%d, max relation %d" % (num_node, num_relation, lo, hi_node, hi_rel))
    return _sets_from_keys(torch.cat([r * num_node + t, (r + num_relation) * num_node + h]), 2 * num_relation, num_node)


def candidate_sets(lists, num_node, device=None):
    """:class:`CandidateSets` from user-supplied types: ``lists`` is a sequence of Python lists or integer tensors of entity ids,
    one per set, in any order and with repeats -- they are sorted and deduplicated.  An id outside ``[0, num_node)`` raises
    ``ValueError``."""
    num_node = int(num_node)
    if not 1 <= num_node < 2 ** 31:
        raise ValueError("candidate_sets: num_node must be in [1, 2^31), got %d" % num_node)
    keys = []
    for i, ids in enumerate(lists):
        ids = torch.as_tensor(ids, device=device).reshape(-1) if not (isinstance(ids, (list, tuple)) and len(ids) == 0) \
            else torch.zeros(0, dtype=torch.int64, device=device)
        if ids.dtype.is_floating_point or ids.dtype == torch.bool:
            raise ValueError("candidate_sets: set %d holds %s, expected entity ids" % (i, ids.dtype))
        ids = ids.long()
        if len(ids) and (int(ids.min()) < 0 or int(ids.max()) >= num_node):
            raise ValueError("candidate_sets: set %d has ids outside [0, %d)" % (i, num_node))
        keys.append(i * num_node + ids)
    keys = torch.cat(keys) if keys else torch.zeros(0, dtype=torch.int64, device=device)
    return _sets_from_keys(keys, len(lists), num_node)


def load_triples(path, entity_vocab=None, relation_vocab=None):
    """Read ``h<TAB>r<TAB>t`` lines (the layout of ``ultra/dataset.py:69-96``) into ``(h, t, r)`` ids."""
    entity_vocab = {} if entity_vocab is None else entity_vocab
    relation_vocab = {} if relation_vocab is None else relation_vocab
    rows = []
    with open(os.path.expanduser(path)) as fin:
        for line in fin:
            parts = line.split()
            if len(parts) != 3:
                continue
            h, r, t = parts
            rows.append((entity_vocab.setdefault(h, len(entity_vocab)), entity_vocab.setdefault(t, len(entity_vocab)),
                         relation_vocab.setdefault(r, len(relation_vocab))))
    return np.asarray(rows, dtype=np.int64).reshape(-1, 3), entity_vocab, relation_vocab


SPLIT_FILES = ("train.txt", "valid.txt", "test.txt")


def load_split_dir(path):
    """A transductive dataset directory in the reference's layout (``ultra/dataset.py:33-66``): ``train.txt``, ``valid.txt``
    and ``test.txt`` of ``h<TAB>r<TAB>t`` lines, ONE entity / relation vocabulary built in that order (``build_vocab`` reads
    the three files one after the other with shared dictionaries).  Returns ``(triples (T, 3) int64 rows of (h, t, r) = train +
    valid + test concatenated, counts [n_train, n_valid, n_test], num_node, num_relation)`` -- what ``self.triplets`` /
    ``self.num_samples`` hold there."""
    path = os.path.expanduser(path)
    entity_vocab, relation_vocab = {}, {}
    parts = []
    for name in SPLIT_FILES:
        file = os.path.join(path, name)
        if not os.path.isfile(file):
            raise FileNotFoundError("%s: a transductive split directory holds %s" % (file, ", ".join(SPLIT_FILES)))
        rows, entity_vocab, relation_vocab = load_triples(file, entity_vocab, relation_vocab)
        parts.append(rows)
    return np.concatenate(parts), [len(p) for p in parts], len(entity_vocab), len(relation_vocab)


def task_from_split_dir(path, checkpoint=None, device="cpu", **task_kwargs):
    """The shipped 6 x 64d Ultra over a real split directory: the train triples carry messages, valid + test belong to the
    filter graph (``ultra/task.py:31-63``), weights from ``checkpoint`` (``td_ultra_3g.pth`` / ``td_ultra_4g.pth`` layout,
    ``ultra/util.py:233-276``) or seeded random init.  Returns ``(task in eval mode on device, splits)`` with
    ``splits = {"train" | "valid" | "test": (n, 3) tensors}``."""
    from .checkpoint import load_checkpoint
    from .task import build_ultra
    triples, counts, n_node, n_rel = load_split_dir(path)
    triples = torch.from_numpy(triples)
    fact_mask = torch.zeros(len(triples), dtype=torch.bool)
    fact_mask[:counts[0]] = True
    torch.manual_seed(DEFAULT_SEED)
    task = build_ultra(n_rel, **task_kwargs)
    missing = unexpected = None
    if checkpoint is not None:
        missing, unexpected = load_checkpoint(task, checkpoint, map_location="cpu")
    task.preprocess(Graph(triples, num_node=n_node, num_relation=n_rel), fact_mask)
    task.to(device).eval()
    bounds = np.cumsum([0] + counts)
    splits = {name.split(".")[0]: triples[bounds[i]:bounds[i + 1]] for i, name in enumerate(SPLIT_FILES)}
    task.checkpoint_keys = (missing, unexpected)
    return task, splits


def sample_queries(graph, structure, n_query, generator=None):
    """``n_query`` logical queries of one structure grounded on ``graph`` -- a graph WITH inverse edges, such as
    ``task.message_graph()`` or ``graph.undirected(add_inverse=True)`` -- so that each has an answer by construction (DESIGN.md
    section 18; host-side and small: a Python loop per query).  Returns ``(anchors int64 (Q, A), relations int64 (Q, P), targets
    int64 (Q,))`` on the CPU, columns in the order ``task.answer_query`` consumes them.

    A query is grounded backwards from a target entity drawn uniformly.  ``('e', ops)``: ``ops`` are walked in reverse and every
    ``'r'`` picks, uniformly, one edge of non-zero weight that ENDS in the current node, records its relation and moves to its
    start; the node reached is the anchor.  ``((node, ...), ops)``: ``ops`` are walked back the same way, then the inner node is
    grounded at the node reached.  Every branch of an intersection or union is grounded at the same node, except a branch whose
    ops hold an ``'n'``: that one is grounded at a node drawn independently.  A node without an in-edge is a dead end: the target
    is drawn again, at most 100 times, then ``RuntimeError``.  The draw is a function of the generator's state alone.  A query
    without ``'n'`` contains its target in its exact answers on ``graph``."""
    from .task import parse_query_structure
    tree, n_anchor, n_relation = parse_query_structure(structure)
    n_node, n_query = graph.num_node, int(n_query)
    edges = graph.edge_list[graph.edge_weight != 0].cpu()
    order = torch.argsort(edges[:, 1], stable=True)
    tail_of, rel_of = edges[order, 0].tolist(), edges[order, 2].tolist()
    start = torch.searchsorted(edges[order, 1].contiguous(), torch.arange(n_node + 1)).tolist()

    def draw(n):
        return int(torch.randint(0, n, (1,), generator=generator))

    class DeadEnd(Exception):
        pass

    def walk_back(at, ops, relations):
        """``relations`` of the ``'r'`` in ``ops`` (forward order) are appended; returns the node in front of ``ops``."""
        found = []
        for op in reversed(ops):
            if op != "r":
                continue
            lo, hi = start[at], start[at + 1]
            if hi == lo:
                raise DeadEnd()
            e = lo + draw(hi - lo)
            found.append(rel_of[e])
            at = tail_of[e]
        relations.extend(reversed(found))
        return at

    def ground(node, at, anchors, relations):
        """Appends the anchors and relations of ``node`` (depth-first, left to right) grounded at entity ``at``."""
        kind = node[0]
        if kind == "e":
            anchors.append(walk_back(at, node[1], relations))
        elif kind == "ops":
            mine = []                                     # the inner node's relations come first
            at = walk_back(at, node[2], mine)
            ground(node[1], at, anchors, relations)
            relations.extend(mine)
        else:
            for child in node[1]:
                negated = "n" in (child[1] if child[0] == "e" else child[2] if child[0] == "ops" else ())
                ground(child, draw(n_node) if negated else at, anchors, relations)

    anchors = torch.zeros(n_query, n_anchor, dtype=torch.int64)
    relations = torch.zeros(n_query, n_relation, dtype=torch.int64)
    targets = torch.zeros(n_query, dtype=torch.int64)
    if n_query and n_node < 1:
        raise RuntimeError("sample_queries: the graph has no nodes")
    for q in range(n_query):
        for _ in range(100):
            target, a, r = draw(n_node), [], []
            try:
                ground(tree, target, a, r)
            except DeadEnd:
                continue
            break
        else:
            raise RuntimeError("sample_queries: 100 targets in a row led to a node without an in-edge (%d nodes, %d edges)"
                               % (n_node, len(edges)))
        anchors[q] = torch.tensor(a, dtype=torch.int64)
        relations[q] = torch.tensor(r, dtype=torch.int64)
        targets[q] = target
    return anchors, relations, targets


def sample_query_negatives(answers, num_negative, generator=None):
    """``num_negative`` negatives per query for ``task.query_loss``: int64 ``(Q, K)`` uniform draws WITH replacement among the
    entities that are ``False`` in the bool ``(Q, N)`` answer matrix ``answers`` -- such as ``task.query_answers(...,
    graph="filter")``, so that no known answer is ever a negative -- on the device of ``answers``.  Draw
    ``k`` of row ``q`` is the ``floor(u * n_q)``-th non-answer in ascending entity order, ``u`` uniform in ``[0, 1)`` from
    ``generator`` (a CPU generator, or ``None`` for the global one): a function of the generator's state alone.  A row in which
    every entity answers raises ``ValueError``."""
    if answers.dim() != 2 or answers.dtype != torch.bool:
        raise ValueError("sample_query_negatives: answers must be bool (Q, N), got %s %s" % (answers.dtype, tuple(answers.shape)))
    num_negative = int(num_negative)
    if num_negative < 1:
        raise ValueError("sample_query_negatives: num_negative must be positive, got %d" % num_negative)
    free = ~answers
    n_free = free.sum(dim=1)
    if answers.shape[0] and int(n_free.min()) == 0:
        raise ValueError("sample_query_negatives: a query whose answers are all %d entities has no negative" % answers.shape[1])
    u = torch.rand(answers.shape[0], num_negative, dtype=torch.float64, generator=generator).to(answers.device)
    rank = (u * n_free.unsqueeze(-1)).floor().long().clamp(max=(n_free - 1).unsqueeze(-1))        # 0-based among the non-answers
    # the entity at which the running count of non-answers first exceeds the rank
    return torch.searchsorted(free.long().cumsum(dim=1), rank + 1)

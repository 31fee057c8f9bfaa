"""Relation prediction without a GPU: ``functional.relation_select`` on CPU tensors (its dense twin) and ``task.relation_scores`` /
``task.answer_relation`` / ``engine.answer_relation`` / ``engine.evaluate_relations`` on CPU tensors, against a case computed by
hand and against the numpy restatement of the definition (tests/relation_definition.py)."""
from fractions import Fraction

import numpy as np
import pytest
import torch

import relation_definition as RD
from sampled_graphs import small_task, tied_scores, wide_graph
from topk_definition import same_bits, special_scores

NAN, INF = float("nan"), float("inf")

# 6 nodes, 3 relations; rows of (h, t, r)
TRIPLES = [(0, 1, 0), (0, 1, 2), (1, 0, 1), (2, 3, 0), (2, 3, 1), (2, 3, 2), (4, 5, 1), (5, 5, 0), (0, 1, 0)]
PAIRS = [(0, 1), (2, 3), (3, 2), (1, 2), (5, 5)]
# candidate ids 0 .. 5 (3 .. 5: the inverses of 0 .. 2)
SCORES = [[0.5, 2.0, 9.0, 2.0, 7.0, -1.0],        # (0, 1): 0 and 2 hold; 1 --1--> 0 holds, so the inverse id 4 is known
          [1.0, 2.0, 3.0, 4.0, 5.0, 6.0],         # (2, 3): every forward id is known
          [3.0, 3.0, 1.0, 8.0, 8.0, 8.0],         # (3, 2): known only under the inverse ids
          [NAN, 0.0, -0.0, -INF, 1.0, NAN],       # (1, 2): nothing is known
          [4.0, 1.0, 2.0, 3.0, 0.0, 5.0]]         # (5, 5): the loop 5 --0--> 5 is known as 0 and as its inverse 3
KNOWN = [[1, 0, 1, 0, 1, 0], [1, 1, 1, 0, 0, 0], [0, 0, 0, 1, 1, 1], [0, 0, 0, 0, 0, 0], [1, 0, 0, 1, 0, 0]]
TARGET = [0, 2, 1, 0, -1]
RANK = [3, 4, 3, 1, 0]              # known target: others at least as high, + 1; unknown target (3, 2): itself too; NaN: nothing; -1
TOP4 = [[1, 3, 5, -1], [5, 4, 3, -1], [0, 1, 2, -1], [4, 1, 2, 3], [5, 2, 1, 4]]
TOP4_VALUE = [[2.0, 2.0, -1.0, -INF], [6.0, 5.0, 4.0, -INF], [3.0, 3.0, 1.0, -INF], [1.0, 0.0, -0.0, -INF], [5.0, 2.0, 1.0, 0.0]]
N_FREE = [3, 3, 3, 6, 4]


def _graph():
    from ultra_torchdrug_amd.graph import Graph
    return Graph(torch.tensor(TRIPLES, dtype=torch.long), num_node=6, num_relation=3)


def _select(score, cand, graph, h, t, target, k, **kw):
    from ultra_torchdrug_amd import functional as UF
    return UF.relation_select(score, cand, graph.completion_keys(0), graph.completion_keys(1), h, t, target, graph.num_relation,
                              graph.num_node, k, **kw)


def _same(got, want, what=None):
    """A ``RelationSelection`` against the definition's dict: integers equal, floats bit for bit."""
    for name in ("top_index", "rank", "n_free", "known"):
        if getattr(got, name) is not None:
            assert np.array_equal(getattr(got, name).cpu().numpy(), want[name]), (name, what)
    if got.top_value is not None:
        assert same_bits(got.top_value.cpu().numpy(), want["top_value"]), what


def test_the_hand_computed_case():
    graph = _graph()
    score = torch.tensor(SCORES)
    h, t = torch.tensor(PAIRS).t()
    got = _select(score, None, graph, h, t, torch.tensor(TARGET), 4)
    assert got.known.dtype == torch.uint8 and got.known.tolist() == KNOWN
    assert got.n_free.tolist() == N_FREE and got.rank.tolist() == RANK
    assert got.top_index.tolist() == TOP4 and same_bits(got.top_value.numpy(), np.array(TOP4_VALUE, dtype=np.float32))
    # the restatement agrees with the literals, so the larger cases below can rest on it
    _same(got, RD.select(SCORES, None, TRIPLES, h.tolist(), t.tolist(), TARGET, 3, 4, n_node=6))
    # the forward ids alone: the inverse ids are no candidates, the key array of side 1 is never consulted
    fwd = _select(score[:, :3], None, graph, h, t, torch.tensor(TARGET), 2)
    assert fwd.known.tolist() == [row[:3] for row in KNOWN] and fwd.n_free.tolist() == [1, 0, 3, 3, 2]
    assert fwd.top_index.tolist() == [[1, -1], [-1, -1], [0, 1], [1, 2], [2, 1]]
    assert fwd.rank.tolist() == [2, 1, 3, 1, 0]
    # unfiltered: nothing is known, every target counts itself
    from ultra_torchdrug_amd import functional as UF
    raw = UF.relation_select(score, None, None, None, None, None, torch.tensor(TARGET), 3, 6, 4)
    assert raw.known.sum() == 0 and raw.n_free.tolist() == [6] * 5 and raw.rank.tolist() == [6, 5, 6, 1, 0]
    assert raw.top_index.tolist() == [[2, 4, 1, 3], [5, 4, 3, 2], [3, 4, 5, 0], [4, 1, 2, 3], [5, 0, 3, 2]]
    # a list: unsorted, id 1 twice, id 7 out of range (never known); ties go by POSITION, the ids returned are cand[j]
    cand = torch.tensor([4, 1, 1, 7, 0])
    listed = _select(torch.tensor([[1.0, 5.0, 5.0, 5.0, 9.0]] * 2), cand, graph, torch.tensor([0, 2]), torch.tensor([1, 3]),
                     torch.tensor([1, 3]), 5)
    assert listed.known.tolist() == [[1, 0, 0, 0, 1], [0, 1, 1, 0, 1]] and listed.n_free.tolist() == [3, 2]
    assert listed.top_index.tolist() == [[1, 1, 7, -1, -1], [7, 4, -1, -1, -1]]
    assert listed.rank.tolist() == [4, 0]               # target 1: its first position, itself and two ties; target 3: not listed
    assert listed.top_value[1].tolist() == [5.0, 1.0, -INF, -INF, -INF]


@pytest.mark.parametrize("scores", ["tied", "special"])
def test_the_dense_twin_equals_the_definition(scores):
    from ultra_torchdrug_amd import functional as UF
    graph = wide_graph(full_row=True)
    triples = graph.edge_list.numpy()
    g = torch.Generator().manual_seed(3)
    e = graph.edge_list[torch.randint(0, len(triples), (12,), generator=g)]
    h = torch.cat([e[:, 0], torch.tensor([299, 7, 1])])
    t = torch.cat([e[:, 1], torch.tensor([0, 299, 1])])
    target = torch.cat([e[:, 2], torch.tensor([-1, 9, 4])])
    pred = (tied_scores if scores == "tied" else special_scores)(len(h), 300, seed=7)[:, 0]
    for cand in (None, torch.tensor([9, 3, 3, 12, 0, 6, -2, 5])):
        n_cand = 10 if cand is None else len(cand)
        block = pred[:, 95:95 + n_cand]                                 # a strided view with NaN, zeros of both signs and ties
        for k in (1, 10, 128):
            got = UF.relation_select(block, cand, graph.completion_keys(0), graph.completion_keys(1), h, t, target, 5, 300, k)
            _same(got, RD.select(block.numpy(), cand, triples, h.tolist(), t.tolist(), target.tolist(), 5, k, n_node=300), (k, cand))
    some = UF.relation_select(pred[:, :10], None, None, None, None, None, None, 5, 300, 3, outputs=("top_index", "n_free"))
    assert some.top_value is None and some.rank is None and some.known is None and some.n_free.tolist() == [10] * len(h)
    empty = UF.relation_select(pred[:0, :10], None, graph.completion_keys(0), graph.completion_keys(1), h[:0], t[:0], None, 5, 300, 3)
    assert empty.top_index.shape == (0, 3) and empty.known.shape == (0, 10) and empty.rank.shape == (0,)
    none = UF.relation_select(pred[:, :0], None, graph.completion_keys(0), graph.completion_keys(1), h, t, target, 5, 300, 3)
    assert (none.top_index == -1).all() and (none.top_value == -INF).all() and not none.rank.any() and not none.n_free.any()
    for bad in (dict(k=0), dict(k=129), dict(n_rel=0), dict(score=pred[:, :10].double()), dict(h=h.int()), dict(h=h[:3]),
                dict(cand=torch.arange(9)), dict(target=target[:2]), dict(outputs=("best",)), dict(outputs=())):
        args = dict(dict(score=pred[:, :10], cand=None, keys_head=graph.completion_keys(0), keys_tail=graph.completion_keys(1), h=h,
                         t=t, target=target, n_rel=5, n_node=300, k=3), **bad)
        with pytest.raises(RuntimeError):
            UF.relation_select(**args)


@pytest.fixture(scope="module")
def small():
    graph = wide_graph()
    task = small_task(graph)
    e = graph.edge_list
    # six pairs over three heads: edges of the graph (their relation is known), constructed pairs, h == t, the last node
    first = e[(e[:, 0] == 11) & (e[:, 2] == 1)][0]
    pairs = [[11, int(first[1])], [int(e[0, 0]), int(e[0, 1])], [11, 299], [int(e[0, 0]), int(e[0, 0])], [299, 5], [11, 11]]
    assert len({p[0] for p in pairs}) == 3
    return {"graph": graph, "task": task, "pairs": torch.tensor(pairs)}


def test_relation_scores_are_the_logits_of_predict(small):
    task, pairs = small["task"], small["pairs"]
    h, t = pairs.t()
    score, cand = task.relation_scores(h, t, inverse=True, batch_size=5)
    assert score.shape == (6, 10) and score.dtype == torch.float32 and cand.tolist() == list(range(10))
    with torch.no_grad():
        for p, (a, b) in enumerate(pairs.tolist()):
            for c in range(10):
                want = task.predict(torch.tensor([[a, b, c]]))[0, 0, b] if c < 5 else task.predict(torch.tensor([[b, a, c - 5]]))[0, 1, b]
                # the same arithmetic in batches of another size: the host BLAS may order a sum differently (a few ulp of fp32)
                assert torch.allclose(score[p, c], want, rtol=1e-4, atol=1e-5), (p, c)
    fwd, ids = task.relation_scores(h, t)
    assert ids.tolist() == [0, 1, 2, 3, 4] and torch.allclose(fwd, score[:, :5], rtol=1e-4, atol=1e-5)
    some, ids = task.relation_scores(h, t, candidates=[7, 2, 2])
    assert ids.tolist() == [7, 2, 2] and torch.allclose(some, score[:, [7, 2, 2]], rtol=1e-4, atol=1e-5)
    assert torch.equal(some[:, 1], some[:, 2])
    # one query column per distinct (head, candidate): 3 heads x 10 candidates, in batches of 5
    seen = []
    inner = task._first_hop
    task._first_hop = lambda anchor, relation: (seen.append(len(anchor)), inner(anchor, relation))[1]
    try:
        task.relation_scores(h, t, inverse=True, batch_size=7)
    finally:
        del task._first_hop
    assert sum(seen) == 3 * 10 and max(seen) == 7 and len(seen) == 5


def test_task_and_engine_calls_equal_the_definition_on_their_scores(small):
    from ultra_torchdrug_amd import engine
    task, graph, pairs = small["task"], small["graph"], small["pairs"]
    triples = graph.edge_list.numpy()
    h, t = pairs.t()
    for kw in (dict(), dict(inverse=True), dict(candidates=torch.tensor([8, 1, 1, 0, 6]))):
        score, cand = task.relation_scores(h, t, **kw)
        for filtered in (True, False):
            want = RD.select(score.numpy(), cand.numpy(), triples, h.tolist(), t.tolist(), None, 5, 4, filtered=filtered)
            runs = {"task": task.answer_relation(h, t, k=4, filtered=filtered, **kw),
                    "engine": engine.answer_relation(task, h, t, k=4, pair_batch=4, filtered=filtered, **kw)}
            for name, (relations, values) in runs.items():
                assert relations.dtype == torch.int64 and values.dtype == torch.float32, name
                assert np.array_equal(relations.numpy(), want["top_index"]), (name, kw, filtered)
                # (the engine scores the pairs in other batches: on the host a BLAS sum may differ by a few ulp between batch
                # shapes -- tests/test_relation_gpu.py holds the device to equal bits)
                if name == "task":
                    assert same_bits(values.numpy(), want["top_value"]), (name, kw, filtered)
                else:
                    assert np.allclose(values.numpy(), want["top_value"], rtol=1e-4, atol=1e-5), (name, kw, filtered)
    known = RD.select(np.zeros((6, 10), np.float32), None, triples, h.tolist(), t.tolist(), None, 5, 1)["known"]
    assert known[0, 1] == 1 and known.sum() >= 2                                  # the hub edge (11, ?, 1) is known
    # evaluation: edges of the graph (their relation is known) and constructed triples, against the definition's ranks
    rows = torch.cat([graph.edge_list[::1700], torch.tensor([[11, 299, 3], [299, 5, 0], [11, 11, 4]])])
    for kw in (dict(), dict(inverse=True), dict(candidates=[4, 0, 2, 7])):
        score, cand = task.relation_scores(rows[:, 0], rows[:, 1], **kw)
        want = RD.select(score.numpy(), cand.numpy(), triples, rows[:, 0].tolist(), rows[:, 1].tolist(), rows[:, 2].tolist(), 5, 1)
        got = engine.evaluate_relations(task, rows, pair_batch=3, **kw)
        assert np.array_equal(got["ranks"].numpy(), want["rank"]), kw
        exact = RD.metrics(want["rank"])
        assert got["skipped"] == exact["skipped"] == int((want["rank"] == 0).sum())
        assert ("candidates" in kw) == (got["skipped"] > 0)
        for name in ("mrr", "mr", "hits@1", "hits@3", "hits@10"):
            assert got[name] == pytest.approx(float(exact[name]), rel=1e-12), (name, kw)


def test_evaluate_relations_metrics_as_fractions():
    """The hand-computed case through ``engine.evaluate_relations``: the scores of a pair are the rows written above."""
    from ultra_torchdrug_amd import engine
    task = small_task(_graph())
    table = {pair: row for pair, row in zip(PAIRS, SCORES)}
    task._relation_scores = lambda h, t, cand, batch_size: torch.tensor([table[pair] for pair in zip(h.tolist(), t.tolist())])[:, cand]
    rows = torch.tensor([[0, 1, 0], [2, 3, 2], [3, 2, 1], [1, 2, 0]])
    got = engine.evaluate_relations(task, rows, inverse=True)
    assert got["ranks"].tolist() == [3, 4, 3, 1] and got["skipped"] == 0
    assert got["mrr"] == pytest.approx(float(Fraction(23, 48)), rel=1e-12) and got["mr"] == pytest.approx(11 / 4, rel=1e-12)
    assert (got["hits@1"], got["hits@3"], got["hits@10"]) == (0.25, 0.75, 1.0)
    # candidates 0 and 1: relation 2 of the second triple is no candidate -- skipped, not ranked
    got = engine.evaluate_relations(task, rows, candidates=[0, 1], pair_batch=2)
    assert got["ranks"].tolist() == [2, 0, 3, 1] and got["skipped"] == 1
    assert got["mrr"] == pytest.approx(float(Fraction(11, 18)), rel=1e-12) and got["mr"] == pytest.approx(2.0, rel=1e-12)
    assert got["hits@1"] == pytest.approx(1 / 3, rel=1e-12) and got["hits@3"] == 1.0 and got["hits@10"] == 1.0
    unfiltered = engine.evaluate_relations(task, rows, inverse=True, filtered=False)
    assert unfiltered["ranks"].tolist() == [6, 5, 6, 1]
    relations, values = engine.answer_relation(task, [0, 2, 3, 1, 5], [1, 3, 2, 2, 5], k=4, inverse=True, pair_batch=2)
    assert relations.tolist() == TOP4 and same_bits(values.numpy(), np.array(TOP4_VALUE, dtype=np.float32))


def test_range_errors_and_no_pairs(small):
    from ultra_torchdrug_amd import engine
    task = small["task"]
    ok = (torch.tensor([1, 2]), torch.tensor([3, 4]))
    for bad in (dict(h=torch.tensor([1, 300])), dict(t=torch.tensor([-1, 0])), dict(candidates=[0, 10]), dict(candidates=[-1]),
                dict(h=torch.tensor([1])), dict(h=torch.tensor([1.0, 2.0])), dict(candidates=torch.tensor([0.5]))):
        args = dict(dict(h=ok[0], t=ok[1]), **bad)
        with pytest.raises(ValueError):
            task.relation_scores(**args)
        with pytest.raises(ValueError):
            task.answer_relation(**args)
        with pytest.raises(ValueError):
            engine.answer_relation(task, **args)
    for k in (0, 129):
        with pytest.raises(ValueError):
            task.answer_relation(*ok, k=k)
        with pytest.raises(ValueError):
            engine.answer_relation(task, *ok, k=k)
    with pytest.raises(ValueError):
        task.relation_scores(*ok, batch_size=0)
    with pytest.raises(ValueError):
        engine.evaluate_relations(task, torch.tensor([[1, 2, 5]]))            # relation 5 of 5
    with pytest.raises(ValueError):
        engine.evaluate_relations(task, torch.tensor([[1, 2]]))
    none = torch.zeros(0, dtype=torch.long)
    score, cand = task.relation_scores(none, none, inverse=True)
    assert score.shape == (0, 10) and len(cand) == 10
    for relations, values in (task.answer_relation(none, none, k=3), engine.answer_relation(task, none, none, k=3)):
        assert relations.shape == (0, 3) and relations.dtype == torch.int64 and values.shape == (0, 3)
    got = engine.evaluate_relations(task, torch.zeros(0, 3, dtype=torch.long))
    assert got["skipped"] == 0 and got["ranks"].shape == (0,) and got["mrr"] != got["mrr"]
    score, cand = task.relation_scores(*ok, candidates=[])
    assert score.shape == (2, 0) and (task.answer_relation(*ok, k=2, candidates=[])[0] == -1).all()


def test_binding_lists_the_entry():
    from ultra_torchdrug_amd import _lib, _torch_ext, backend, functional as UF
    assert {"ultra_relation_select_f32", "ultra_relation_select_limit"} <= set(_lib.EXPORTS) and _lib.ABI_VERSION == 8
    assert len(_lib.SIGNATURES["ultra_relation_select_f32"][1]) == 23 and "relation_select" in _torch_ext.OPS
    assert backend.get().relation_select is UF.relation_select and UF.relation_select_limit() == 4096
    lib = _lib.load()
    BAD_SHAPE, NULL_POINTER = 2, 3
    call = lambda **kw: lib.ultra_relation_select_f32(*[dict(dict(
        score=8, n_pair=2, n_cand=4, row_stride=4, cand=None, keys_head=None, n_keys_head=0, keys_tail=None, n_keys_tail=0, h=None,
        t=None, index_stride=1, target=None, target_stride=1, n_rel=2, n_node=9, k=3, top_index=8, top_value=8, rank=None, n_free=None,
        known=None, stream=None), **kw)[name] for name in (
        "score n_pair n_cand row_stride cand keys_head n_keys_head keys_tail n_keys_tail h t index_stride target target_stride n_rel "
        "n_node k top_index top_value rank n_free known stream").split()])
    # refused before any device work (the pointers are never followed)
    for bad in (dict(n_pair=-1), dict(n_cand=-1), dict(n_cand=2 ** 31), dict(row_stride=3), dict(k=0), dict(k=129), dict(n_rel=0),
                dict(n_node=0), dict(n_node=2 ** 31, n_rel=4), dict(n_keys_head=-1), dict(index_stride=-1)):
        assert call(**bad) == BAD_SHAPE, bad
    for bad in (dict(top_index=None, top_value=None), dict(score=None), dict(n_keys_head=5), dict(keys_head=8, n_keys_head=5),
                dict(keys_tail=8, h=8)):
        assert call(**bad) == NULL_POINTER, bad
    assert call(n_pair=0) == 0

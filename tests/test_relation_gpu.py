"""MI355X: relation prediction on the device -- ``ultra_relation_select_f32`` on its one-pass and multi-pass forms against the numpy
restatement of the definition (tests/relation_definition.py: integers equal, floats bit for bit), with 64-bit keys, captured into a
hipGraph and between guard bands; ``task.relation_scores`` against the logits of ``predict``; ``task.answer_relation`` /
``engine.answer_relation`` / ``engine.evaluate_relations`` against the CPU task and the definition."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import relation_definition as RD
from sampled_graphs import small_task, tied_scores, wide_graph
from topk_definition import same_bits, special_scores

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L = 4096                                        # ultra_relation_select_limit(): the longest one-pass candidate list
LIST = [9, 3, 3, 12, 0, 6, -2, 5]               # unsorted, 3 twice, 12 and -2 out of range for 5 relations


def _dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _same(got, want, what=None):
    """A ``RelationSelection`` of the device against the definition's dict: integers equal, floats bit for bit."""
    for name in ("top_index", "rank", "n_free", "known"):
        if getattr(got, name) is not None:
            assert getattr(got, name).dtype == (torch.uint8 if name == "known" else torch.int64), name
            assert np.array_equal(getattr(got, name).cpu().numpy(), want[name]), (name, what)
    if got.top_value is not None:
        assert got.top_value.dtype == torch.float32 and same_bits(got.top_value.cpu().numpy(), want["top_value"]), what


def _equal(a, b):
    for x, y in zip(a, b):
        assert (x is None) == (y is None)
        if x is not None:
            assert x.dtype == y.dtype and (same_bits(x.cpu().numpy(), y.cpu().numpy()) if x.is_floating_point() else torch.equal(x, y))


# ------------------------------------------------------------------------------------------------ 300 nodes, 5 relations
@pytest.fixture(scope="module")
def wide():
    from ultra_torchdrug_amd.graph import Graph
    e = wide_graph(full_row=True).edge_list.numpy()

    def between(a, b):
        return ((e[:, 0] == a) & (e[:, 1] == b)) | ((e[:, 0] == b) & (e[:, 1] == a))

    e = e[~(between(250, 251) | between(30, 31) | between(20, 21))]
    full = [(20, 21, r) for r in range(5)] + [(21, 20, r) for r in range(5)]
    e = np.concatenate([e, np.array(full + [(31, 30, 2), (299, 0, 1), (5, 299, 4), (299, 299, 3)], dtype=np.int64)])
    # rows of (h, t, target): every candidate known | none known, target not known | known only under the inverse id 7 |
    # a target no list holds | the last node as h, as t and as both | edges of the graph
    rows = [(20, 21, 3), (250, 251, 3), (30, 31, 2), (250, 251, 11), (299, 0, 1), (5, 299, 4), (299, 299, 8), (7, 100, 2),
            (13, 5, 0), (11, int(e[(e[:, 0] == 11) & (e[:, 2] == 1)][0, 1]), 1), (0, 0, -1)] + e[::1500].tolist()
    rows = np.array(rows, dtype=np.int64)
    facts = RD.triple_set(e)
    ids = np.arange(10)
    assert RD.known_row(facts, 20, 21, ids, 5).all() and not RD.known_row(facts, 250, 251, ids, 5).any()
    assert RD.known_row(facts, 30, 31, ids, 5).tolist() == [c == 7 for c in ids]
    assert RD.known_row(facts, 299, 0, ids, 5)[1] and RD.known_row(facts, 5, 299, ids, 5)[4] and RD.known_row(facts, 0, 299, ids, 5)[6]
    assert RD.known_row(facts, 299, 299, ids, 5)[[3, 8]].all()
    graph = Graph(torch.from_numpy(e), num_node=300, num_relation=5).to(_dev())
    return {"graph": graph, "triples": e, "rows": torch.from_numpy(rows)}


def _wide_call(wide, score, cand, k, rows=None, **kw):
    from ultra_torchdrug_amd import functional as UF
    graph = wide["graph"]
    rows = wide["rows"].to(score.device) if rows is None else rows
    return UF.relation_select(score, cand, graph.completion_keys(0), graph.completion_keys(1), rows[:, 0], rows[:, 1], rows[:, 2],
                              5, 300, k, **kw)


@pytest.mark.parametrize("scores", ["tied", "special"])
@pytest.mark.parametrize("k", [1, 10, 128])
def test_the_kernel_equals_the_definition(wide, k, scores):
    from ultra_torchdrug_amd import functional as UF
    dev, rows = _dev(), wide["rows"]
    h, t, target = (rows[:, i].tolist() for i in range(3))
    pred = (tied_scores if scores == "tied" else special_scores)(len(rows), 300, seed=60 + k)
    pred_d, rows_d = pred.to(dev), rows.to(dev)
    for cand in (None, "2R", LIST):
        n_cand = 5 if cand is None else 10 if cand == "2R" else len(LIST)
        ids = None if n_cand != len(LIST) else torch.tensor(LIST)
        for start in (95, 125):                                          # zeros of both signs and -inf | a NaN among numbers
            view = pred_d[:, 0, start:start + n_cand]
            assert view.stride(0) == 600 and rows_d[:, 0].stride(0) == 3
            got = _wide_call(wide, view, None if ids is None else ids.to(dev), k)
            want = RD.select(pred[:, 0, start:start + n_cand].numpy(), ids, wide["triples"], h, t, target, 5, k, n_node=300)
            _same(got, want, (cand, start, k))
            again = _wide_call(wide, view.contiguous(), None if ids is None else ids.to(dev), k, rows=rows_d.t().contiguous().t())
            _equal(got, again)
            raw = UF.relation_select(view, None if ids is None else ids.to(dev), None, None, None, None, rows_d[:, 2], 5, 300, k)
            _same(raw, RD.select(pred[:, 0, start:start + n_cand].numpy(), ids, wide["triples"], h, t, target, 5, k, filtered=False),
                  (cand, start, k, "unfiltered"))
    assert got.n_free[1] == len(LIST)
    full = _wide_call(wide, pred_d[:, 0, :10], None, k)
    assert full.n_free[0] == 0 and (full.top_index[0] == -1).all() and full.rank[0] == 1 and full.n_free[1] == 10
    one =_wide_call(wide, pred_d[2:3, 0, :10], None, k, rows=rows_d[2:3])
    assert one.known.tolist() == [[0] * 7 + [1, 0, 0]] and one.rank.tolist() == [1 + int((pred[2, 0, :10] >= pred[2, 0, 2]).sum()) - int(pred[2, 0, 7] >= pred[2, 0, 2])]
    empty = _wide_call(wide, pred_d[:0, 0, :10], None, k, rows=rows_d[:0])
    assert empty.top_index.shape == (0, k) and empty.known.shape == (0, 10)
    none = _wide_call(wide, pred_d[:, 0, :0], None, k)
    assert (none.top_index == -1).all() and (none.top_value == -float("inf")).all() and not none.rank.any() and not none.n_free.any()


def test_each_output_alone_and_each_left_out(wide):
    from ultra_torchdrug_amd import functional as UF
    dev = _dev()
    pred = tied_scores(len(wide["rows"]), 300, seed=3).to(dev)[:, 1, 40:50]
    full = _wide_call(wide, pred, None, 10)
    for name in UF.RELATION_OUTPUTS:
        rest = tuple(n for n in UF.RELATION_OUTPUTS if n != name)
        for outputs in ((name,), rest):
            got = _wide_call(wide, pred, None, 10, outputs=outputs)
            _equal(got, [value if n in outputs else None for n, value in zip(UF.RELATION_OUTPUTS, full)])


@pytest.fixture(scope="module")
def many():
    """20 nodes and as many relations as the longest list: three pairs, about half of the relations known for two of them."""
    n_rel = L + 1
    rng = np.random.default_rng(11)
    parts = [np.stack([np.full(n_rel, a), np.full(n_rel, b), np.arange(n_rel)], axis=1)[rng.random(n_rel) < 0.5]
             for a, b in ((3, 4), (19, 19))]
    parts.append(np.stack([rng.integers(0, 20, 3000), rng.integers(0, 20, 3000), rng.integers(0, n_rel, 3000)], axis=1))
    e = np.concatenate(parts).astype(np.int64)
    e = e[~((e[:, 0] == 0) & (e[:, 1] == 19))]
    rows = torch.tensor([[3, 4, 0], [19, 19, 64], [0, 19, 1]])
    return {"triples": e, "rows": rows, "graphs": {}}


def _many_graph(many, n_rel):
    from ultra_torchdrug_amd.graph import Graph
    if n_rel not in many["graphs"]:
        e = many["triples"][many["triples"][:, 2] < n_rel]
        many["graphs"][n_rel] = (e, Graph(torch.from_numpy(e), num_node=20, num_relation=n_rel).to(_dev()))
    return many["graphs"][n_rel]


@pytest.mark.parametrize("n_cand", [1, 63, 64, 65, 257, L, L + 1])
def test_list_lengths_around_the_wave_and_the_lds_limit(many, n_cand):
    from ultra_torchdrug_amd import functional as UF
    assert UF.relation_select_limit() == L
    dev = _dev()
    triples, graph = _many_graph(many, n_cand)
    rows = many["rows"].clone()
    rows[:, 2] = rows[:, 2].clamp(max=n_cand - 1)
    pred = tied_scores(3, n_cand, seed=n_cand)[:, 0]
    if n_cand >= 257:
        pred = torch.cat([pred, special_scores(3, n_cand, seed=n_cand)[:, 0]])
        rows = torch.cat([rows, rows])
    h, t, target = (rows[:, i].tolist() for i in range(3))
    pred_d, rows_d = pred.to(dev), rows.to(dev)
    for k in (1, 128):
        got = UF.relation_select(pred_d, None, graph.completion_keys(0), graph.completion_keys(1), rows_d[:, 0], rows_d[:, 1],
                                 rows_d[:, 2], n_cand, 20, k)
        want = RD.select(pred.numpy(), None, triples, h, t, target, n_cand, k)
        _same(got, want, (n_cand, k))
    assert n_cand < 64 or 0 < want["n_free"][0] < n_cand
    if n_cand > 1:                                                       # a list in another order: ties go by position, not by id
        cand = torch.arange(n_cand - 1, -1, -1)
        got = UF.relation_select(pred_d, cand.to(dev), graph.completion_keys(0), graph.completion_keys(1), rows_d[:, 0],
                                 rows_d[:, 1], rows_d[:, 2], n_cand, 20, 128)
        _same(got, RD.select(pred.numpy(), cand, triples, h, t, target, n_cand, 128), (n_cand, "reversed"))


# ------------------------------------------------------------------------------------------------ 70 000 nodes, 3 relations
@pytest.fixture(scope="module")
def big():
    from ultra_torchdrug_amd.graph import Graph
    n, r = 70_000, 3
    rng = np.random.default_rng(5)
    e = np.stack([rng.integers(0, n, 20000), rng.integers(0, n, 20000), rng.integers(0, r, 20000)], axis=1)
    # the key of (69999, 1, 69998) cut to 32 bits is the key of another triple: that one is in the graph, the first is not
    key = (69999 * r + 1) * n + 69998
    assert key > 3 * 2 ** 32
    low = key % 2 ** 32
    alias = (low // (r * n), low % n, (low // n) % r)
    extra = [(69999, 69998, 0), (69999, 69998, 2), (69998, 69999, 1), (40000, 3, 1), (69999, 69999, 2), alias]
    e = np.concatenate([e, np.array(extra, dtype=np.int64)])
    e = e[~((e[:, 0] == 69999) & (e[:, 1] == 69998) & (e[:, 2] == 1))]
    rows = torch.tensor([[69999, 69998, 1], [69998, 69999, 1], [40000, 3, 1], [3, 40000, 4], [1, 2, 0], [69999, 69999, 5],
                         list(alias[:2]) + [alias[2]]])
    facts = RD.triple_set(e)
    assert RD.known_row(facts, 69999, 69998, np.arange(6), r).tolist() == [True, False, True, False, True, False]
    assert RD.known_row(facts, 3, 40000, np.arange(6), r)[4]
    graph = Graph(torch.from_numpy(e), num_node=n, num_relation=r).to(_dev())
    assert int(graph.completion_keys(0)[-1]) > 2 ** 32
    return {"graph": graph, "triples": e, "rows": rows}


def test_keys_beyond_32_bits(big):
    from ultra_torchdrug_amd import functional as UF
    dev, graph, rows = _dev(), big["graph"], big["rows"]
    pred = tied_scores(len(rows), 6, seed=9)[:, 0]
    rows_d = rows.to(dev)
    got = UF.relation_select(pred.to(dev), None, graph.completion_keys(0), graph.completion_keys(1), rows_d[:, 0], rows_d[:, 1],
                             rows_d[:, 2], 3, 70_000, 6)
    _same(got, RD.select(pred.numpy(), None, big["triples"], rows[:, 0].tolist(), rows[:, 1].tolist(), rows[:, 2].tolist(), 3, 6))
    assert got.known[0].tolist() == [1, 0, 1, 0, 1, 0] and got.known[-1][int(rows[-1, 2])] == 1


# ------------------------------------------------------------------------------------------------ capture
def test_relation_select_captured_into_a_hipgraph(big):
    from ultra_torchdrug_amd import functional as UF
    dev, graph, rows = _dev(), big["graph"], big["rows"]
    rows_d = rows.to(dev)
    h, t, target = (rows[:, i].tolist() for i in range(3))
    scores = [tied_scores(len(rows), 6, seed=s)[:, 0].contiguous() for s in (21, 22, 23)]
    static = scores[0].to(dev)
    call = lambda s: UF.relation_select(s, None, graph.completion_keys(0), graph.completion_keys(1), rows_d[:, 0], rows_d[:, 1],
                                        rows_d[:, 2], 3, 70_000, 4)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call(static)                                                     # warm-up: the outputs enter the allocator's cache
    torch.cuda.current_stream().wait_stream(side)
    captured = torch.cuda.CUDAGraph()
    with torch.cuda.graph(captured, stream=side):
        got = call(static)
    for score in scores[1:]:                                             # two replays, new scores in the same buffer
        static.copy_(score.to(dev))
        captured.replay()
        torch.cuda.synchronize()
        _same(got, RD.select(score.numpy(), None, big["triples"], h, t, target, 3, 4), "replay")
        _equal(got, call(score.to(dev)))


# ------------------------------------------------------------------------------------------------ memory bounds
@pytest.mark.parametrize("n_cand", [65, L + 1])
def test_the_launch_stays_inside_its_operands(many, n_cand, monkeypatch):
    """Inputs between NaN / zero bands, outputs poisoned between pattern bands (the ctypes binding allocates them in
    ``functional.py``, where the guard sees them): no guard word changes and the results equal the definition, so every output
    word was written."""
    from guarded_memory import guarded, has_poison
    from ultra_torchdrug_amd import functional as UF
    monkeypatch.setenv("ULTRA_BINDING", "ctypes")
    dev = _dev()
    triples, graph = _many_graph(many, n_cand)
    rows = many["rows"].clone()
    rows[:, 2] = rows[:, 2].clamp(max=n_cand - 1)
    pred = tied_scores(3, n_cand, seed=77)[:, 0].contiguous()
    cand = torch.arange(n_cand - 1, -1, -1)
    with guarded("functional") as guard:
        args = [guard.banded(x.to(dev)) for x in (pred, cand, graph.completion_keys(0), graph.completion_keys(1),
                                                  rows[:, 0].contiguous(), rows[:, 1].contiguous(), rows[:, 2].contiguous())]
        got = UF.relation_select(args[0], args[1], args[2], args[3], args[4], args[5], args[6], n_cand, 20, 128)
        guard.check()
        assert not has_poison(got.top_value)
        _same(got, RD.select(pred.numpy(), cand, triples, rows[:, 0].tolist(), rows[:, 1].tolist(), rows[:, 2].tolist(), n_cand, 128))


# ------------------------------------------------------------------------------------------------ model level
def _pairs(graph):
    e = graph.edge_list
    first = e[(e[:, 0] == 11) & (e[:, 2] == 1)][0]
    a, b = int(e[0, 0]), int(e[0, 1])
    pairs = torch.tensor([[11, int(first[1])], [a, b], [11, 299], [a, a], [299, 5], [11, 11]])
    assert len(set(pairs[:, 0].tolist())) == 3
    return pairs


@pytest.fixture(scope="module")
def small():
    graph = wide_graph()
    task = small_task(graph)
    pairs = _pairs(graph)
    rows = torch.cat([graph.edge_list[::1700], torch.tensor([[11, 299, 3], [299, 5, 0], [11, 11, 4]])])
    cpu = {}
    for name, kw in (("R", dict()), ("2R", dict(inverse=True)), ("list", dict(candidates=[8, 1, 1, 0, 6]))):
        cpu[name] = task.answer_relation(pairs[:, 0], pairs[:, 1], k=4, **kw)
    return {"task": task.to(_dev()), "graph": graph, "pairs": pairs, "rows": rows, "cpu": cpu}


def _scores_child(path):
    """In a fresh process (either binding): the (6, 10) scores of the fixture's pairs."""
    graph = wide_graph()
    task = small_task(graph).to(_dev())
    pairs = _pairs(graph).to(_dev())
    torch.save(task.relation_scores(pairs[:, 0], pairs[:, 1], inverse=True)[0].cpu(), path)


def test_relation_scores_are_the_bits_of_predict(small, tmp_path):
    dev, task, pairs = _dev(), small["task"], small["pairs"].to(_dev())
    h, t = pairs[:, 0], pairs[:, 1]
    score, cand = task.relation_scores(h, t, inverse=True)
    assert score.shape == (6, 10) and score.dtype == torch.float32 and cand.tolist() == list(range(10))
    want = torch.empty_like(score)
    with torch.no_grad():
        for p, (a, b) in enumerate(pairs.tolist()):
            for c in range(10):
                triple = torch.tensor([[a, b, c]] if c < 5 else [[b, a, c - 5]], device=dev)
                want[p, c] = task.predict(triple)[0, 0 if c < 5 else 1, b]
    assert torch.equal(score, want)
    assert torch.equal(task.relation_scores(h, t, inverse=True, batch_size=5)[0], score)
    assert torch.equal(task.relation_scores(h, t)[0], score[:, :5])
    assert torch.equal(task.relation_scores(h, t, candidates=[7, 2, 2])[0], score[:, [7, 2, 2]])
    # with the relation cache.  The relation stack of this 16-wide model runs through the BLAS library, which gives a relation
    # computed next to batch mates other last bits than the same relation alone (measured on an MI355X: 41 of these 60 scores
    # move by one ulp, 2.4e-7, with tables built 5 relations at a time; `predict` moves with them) -- so the cache that keeps
    # the bits of the uncached call is the one built one relation at a time; tables built side by side give the bits of
    # `predict` WITH that cache.  (The shipped 64-wide stack has its own kernels and one set of bits: the next test.)
    task.cache_relation_representations(batch_size=1)
    try:
        assert torch.equal(task.relation_scores(h, t, inverse=True)[0], score)
    finally:
        task.clear_relation_cache()
    task.cache_relation_representations()
    try:
        cached = task.relation_scores(h, t, inverse=True)[0]
        with torch.no_grad():
            for p, c in ((0, 1), (1, 7), (3, 0), (4, 9), (5, 4)):
                a, b = pairs[p].tolist()
                triple = torch.tensor([[a, b, c]] if c < 5 else [[b, a, c - 5]], device=dev)
                assert torch.equal(cached[p, c], task.predict(triple)[0, 0 if c < 5 else 1, b]), (p, c)
    finally:
        task.clear_relation_cache()
    # the other binding, in a fresh process
    path = str(tmp_path / "ctypes.pt")
    code = "import sys; sys.path[:0] = [sys.argv[1], sys.argv[1] + '/tests']; import test_relation_gpu as T; T._scores_child(sys.argv[2])"
    proc = subprocess.run([sys.executable, "-c", code, ROOT, path], env=dict(os.environ, ULTRA_BINDING="ctypes"), timeout=300,
                          capture_output=True, text=True)
    assert proc.returncode == 0, proc.stderr[-3000:]
    assert torch.equal(torch.load(path), score.cpu())


def test_one_query_column_per_head_and_candidate(small):
    """3 heads x 10 candidates = 30 columns for 6 pairs, not 60: counted at ``_first_hop`` on the small model and at the model's
    own fused all-entity scoring on a 64-wide one."""
    from ultra_torchdrug_amd.task import build_ultra
    dev, pairs = _dev(), small["pairs"].to(_dev())

    def counted(owner, name, count):
        seen, inner = [], getattr(owner, name)
        setattr(owner, name, lambda *args, **kw: (seen.append(count(*args)), inner(*args, **kw))[1])
        return seen

    task = small["task"]
    seen = counted(task, "_first_hop", lambda anchor, relation: len(anchor))
    try:
        task.relation_scores(pairs[:, 0], pairs[:, 1], inverse=True, batch_size=7)
    finally:
        del task._first_hop
    assert sum(seen) == 30 and max(seen) == 7 and len(seen) == 5
    torch.manual_seed(5)
    wide_task = build_ultra(5, hidden_dims=(64,) * 2, rel_layers=2, num_negative=8, full_batch_eval=True)
    wide_task.preprocess(small["graph"])
    wide_task = wide_task.eval().to(dev)
    seen = counted(wide_task.model, "score_all_entities", lambda graph, rel, h_index, r_index: len(h_index))
    try:
        score, _ = wide_task.relation_scores(pairs[:, 0], pairs[:, 1], inverse=True)
    finally:
        del wide_task.model.score_all_entities
    assert sum(seen) == 30 and len(seen) == 2
    with torch.no_grad():
        a, b = pairs[4].tolist()
        assert torch.equal(score[4, 2], wide_task.predict(torch.tensor([[a, b, 2]], device=dev))[0, 0, b])
        assert torch.equal(score[4, 8], wide_task.predict(torch.tensor([[b, a, 3]], device=dev))[0, 1, b])
    wide_task.cache_relation_representations()                               # the default cache: the same bits on this stack
    assert torch.equal(wide_task.relation_scores(pairs[:, 0], pairs[:, 1], inverse=True)[0], score)


def test_answers_and_evaluation_on_the_device(small):
    from ultra_torchdrug_amd import engine
    dev, task, graph = _dev(), small["task"], small["graph"]
    triples = graph.edge_list.numpy()
    pairs, rows = small["pairs"].to(dev), small["rows"].to(dev)
    h, t = pairs[:, 0], pairs[:, 1]
    for name, kw in (("R", dict()), ("2R", dict(inverse=True)), ("list", dict(candidates=[8, 1, 1, 0, 6]))):
        score, cand = task.relation_scores(h, t, **kw)
        # the definition on the device's OWN scores (fp32 differences between host and device must not flip a tie) ...
        want = RD.select(score.cpu().numpy(), cand.cpu().numpy(), triples, h.tolist(), t.tolist(), None, 5, 4)
        runs = {"task": task.answer_relation(h, t, k=4, **kw), "engine": engine.answer_relation(task, h, t, k=4, pair_batch=4, **kw)}
        for run, (relations, values) in runs.items():
            assert relations.dtype == torch.int64 and values.dtype == torch.float32 and relations.shape == (6, 4), run
            assert np.array_equal(relations.cpu().numpy(), want["top_index"]), (run, name)
            at = (relations.clamp(min=0)[:, :, None] == cand[None, None, :]).long().argmax(dim=2)      # first position of the id
            gathered = torch.where(relations < 0, torch.full_like(values, -float("inf")), score.gather(1, at))
            assert torch.equal(values, gathered), (run, name)                    # relation_scores, gathered
            assert torch.equal(relations.cpu(), small["cpu"][name][0]), (run, name)   # ... and the CPU task's relations
    cpu_task = small_task(graph)
    for kw in (dict(), dict(inverse=True), dict(candidates=[4, 0, 2, 7])):
        score, cand = task.relation_scores(rows[:, 0], rows[:, 1], **kw)
        want = RD.select(score.cpu().numpy(), cand.cpu().numpy(), triples, rows[:, 0].tolist(), rows[:, 1].tolist(),
                         rows[:, 2].tolist(), 5, 1)
        got = engine.evaluate_relations(task, rows, pair_batch=3, **kw)
        assert got["ranks"].dtype == torch.int64 and np.array_equal(got["ranks"].cpu().numpy(), want["rank"]), kw
        assert torch.equal(got["ranks"].cpu(), engine.evaluate_relations(cpu_task, rows.cpu(), **kw)["ranks"]), kw
        exact = RD.metrics(want["rank"])
        assert got["skipped"] == exact["skipped"] and ("candidates" in kw) == (got["skipped"] > 0)
        for name in ("mrr", "mr", "hits@1", "hits@3", "hits@10"):
            assert got[name] == pytest.approx(float(exact[name]), rel=1e-12), (name, kw)


def test_relation_select_refuses_bad_arguments(wide):
    dev = _dev()
    rows = wide["rows"].to(dev)
    pred = tied_scores(len(rows), 300, seed=1).to(dev)[:, 0, :10]
    _wide_call(wide, pred, None, 3)
    keys = wide["graph"].completion_keys(0)
    from ultra_torchdrug_amd import functional as UF
    base = dict(score=pred, cand=None, keys_head=keys, keys_tail=wide["graph"].completion_keys(1), h=rows[:, 0], t=rows[:, 1],
                target=rows[:, 2], n_rel=5, n_node=300, k=3)
    for bad in (dict(k=0), dict(k=129), dict(h=rows[:, 0].int()), dict(h=rows[:, 0].cpu()), dict(keys_head=keys.cpu()),
                dict(keys_tail=keys.int()), dict(score=pred.double()), dict(score=pred[:, ::2]), dict(cand=torch.arange(10)),
                dict(target=rows[:, 2].cpu()), dict(h=None), dict(n_rel=0), dict(score=pred.cpu())):
        with pytest.raises(RuntimeError):
            UF.relation_select(**dict(base, **bad))
    torch.cuda.synchronize()

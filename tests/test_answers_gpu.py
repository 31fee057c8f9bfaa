"""MI355X: top-K answers on the device -- ``ultra_topk_keys`` on its one-launch path (rows of at most 32768 candidates), through
its LDS buffer flushes and on the two-launch path, ``task.answer`` / ``engine.answer`` eager and replayed, and the call captured
into a hipGraph.  Indices and values are held to the numpy restatement of the definition (tests/topk_definition.py) exactly:
integers equal, floats bit for bit."""
import numpy as np
import pytest
import torch

from sampled_graphs import small_task, tied_scores, wide_batch, wide_graph
from topk_definition import completions, same_bits, special_scores, topk_rows

pytestmark = pytest.mark.gpu


def _dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _check(got, pred, k, known, what=None):
    """``got`` = (value, index) of the device against the definition on the host scores ``pred`` (Q, N)."""
    value, index = got
    want_index, want_value = topk_rows(pred.numpy(), k, known)
    assert index.dtype == torch.int64 and value.dtype == torch.float32 and tuple(index.shape) == tuple(value.shape) == want_index.shape
    assert np.array_equal(index.cpu().numpy(), want_index), what
    assert same_bits(value.cpu().numpy(), want_value), what


# ------------------------------------------------------------------------------------------------ one launch, N = 300
@pytest.fixture(scope="module")
def wide():
    graph = wide_graph(full_row=True)
    batch = wide_batch(graph)
    triples = graph.edge_list.numpy()
    known = [[completions(triples, side, int(b[side]), int(b[2])) for b in batch] for side in (0, 1)]
    free = [300 - len(c) for c in known[0]]
    assert 0 in free and any(0 < f <= 30 for f in free) and 300 in free
    return {"graph": graph.to(_dev()), "batch": batch, "known": known}


@pytest.mark.parametrize("scores", ["tied", "special"])
@pytest.mark.parametrize("k", [1, 10, 128])
def test_one_launch_path_equals_the_definition(wide, k, scores):
    from ultra_torchdrug_amd import functional as UF
    dev, graph, batch = _dev(), wide["graph"], wide["batch"]
    pred = tied_scores(len(batch), 300, seed=40 + k) if scores == "tied" else special_scores(len(batch), 300, seed=50 + k)
    pred_d, batch_d = pred.to(dev), batch.to(dev)
    for side in (0, 1):
        view, anchor, rel = pred_d[:, side], batch_d[:, side], batch_d[:, 2]
        assert view.stride(0) == 600 and anchor.stride(0) == 3 and not anchor.is_contiguous()
        got = UF.topk_keys(view, k, graph.completion_keys(side), anchor, rel, 5, n_node=300)
        _check(got, pred[:, side], k, wide["known"][side], (side, k))
        again = UF.topk_keys(view.contiguous(), k, graph.completion_keys(side), anchor.contiguous(), rel.contiguous(), 5)
        assert torch.equal(again[1], got[1]) and same_bits(again[0].cpu().numpy(), got[0].cpu().numpy())
        _check(UF.topk_keys(view, k, None, anchor, rel, 5), pred[:, side], k, None, (side, k, "unfiltered"))
        one = UF.topk_keys(view[4:5], k, graph.completion_keys(side), anchor[4:5], rel[4:5], 5, n_node=300)
        assert torch.equal(one[1], got[1][4:5])
    empty = UF.topk_keys(pred_d[:0, 0], k, graph.completion_keys(0), batch_d[:0, 0], batch_d[:0, 2], 5)
    assert empty[0].shape == (0, k) and empty[1].shape == (0, k)


# ------------------------------------------------------------------------------------------------ buffer flushes, N = 20 000
def _hub_graph(n, seed, hub_tails):
    """``n`` nodes, 3 relations, 20 000 random triples and the hub query (3, 0, ?) with the tails ``hub_tails``."""
    from ultra_torchdrug_amd.graph import Graph
    rng = np.random.default_rng(seed)
    e = np.stack([rng.integers(0, n, 20000), rng.integers(0, n, 20000), rng.integers(0, 3, 20000)], axis=1)
    hub = np.stack([np.full(len(hub_tails), 3), np.asarray(hub_tails), np.zeros(len(hub_tails), dtype=np.int64)], axis=1)
    triples = np.concatenate([e, hub]).astype(np.int64)
    return Graph(torch.from_numpy(triples), num_node=n, num_relation=3), triples, hub


@pytest.mark.parametrize("k", [10, 128])
def test_buffer_flushes_on_the_one_launch_path(k):
    """An ascending row (every candidate beats the threshold: a flush per tile), a descending and a constant one, whose winners
    -- the low indices -- are the hub's 500 known tails."""
    from ultra_torchdrug_amd import functional as UF
    dev, n = _dev(), 20_000
    graph, triples, _ = _hub_graph(n, 5, np.arange(500))
    pred = torch.stack([torch.arange(n).float(), torch.arange(n, 0, -1).float(), torch.full((n,), 0.25)])
    anchor, rel = torch.tensor([3, 3, 3]), torch.tensor([0, 0, 0])
    known = [completions(triples, 0, 3, 0)] * 3
    assert len(known[0]) >= 500
    got = UF.topk_keys(pred.to(dev), k, graph.to(dev).completion_keys(0), anchor.to(dev), rel.to(dev), 3, n_node=n)
    _check(got, pred, k, known)
    free = np.setdiff1d(np.arange(n), known[0])
    assert got[1][0].tolist() == free[::-1][:k].tolist() and got[1][1].tolist() == free[:k].tolist() == got[1][2].tolist()


# ------------------------------------------------------------------------------------------------ two launches, N = 70 000
@pytest.fixture(scope="module")
def long_rows():
    """The graph of test_rank_statistics_past_the_sliced_rank_threshold (70 000 nodes: two full slices and one of 4 464; a hub
    query with 500 known tails) and five score rows."""
    n = 70_000
    rng = np.random.default_rng(3)
    from ultra_torchdrug_amd.graph import Graph
    e = np.stack([rng.integers(0, n, 20000), rng.integers(0, n, 20000), rng.integers(0, 3, 20000)], axis=1)
    hub = np.stack([np.full(500, 3), rng.permutation(n)[:500], np.zeros(500, dtype=np.int64)], axis=1)
    triples = np.concatenate([e, hub]).astype(np.int64)
    graph = Graph(torch.from_numpy(triples), num_node=n, num_relation=3)
    g = torch.Generator().manual_seed(12)
    tied = tied_scores(2, n, seed=9)[:, 0]                                   # rows 0, 1
    shared = torch.randn(n, generator=g)                                     # row 2: one shared maximum across the slices
    planted = [0, 32767, 32768, 65535, 65536, 69999]
    hub_tails = hub[:10, 1].tolist()
    shared[planted + hub_tails] = 9.0
    last = torch.randn(n, generator=g)                                       # row 3: the best 128 all in the last slice
    last[65536 + 2 * torch.arange(200)] += 20.0
    rising = torch.arange(n).float()                                         # row 4
    pred = torch.stack([tied[0], tied[1], shared, last, rising])
    anchor = torch.tensor([3, int(e[0, 0]), 3, 3, 3])                        # the hub query and an ordinary one
    rel = torch.tensor([0, int(e[0, 2]), 0, 0, 0])
    known = [completions(triples, 0, int(a), int(r)) for a, r in zip(anchor, rel)]
    assert len(known[0]) >= 500 and not set(planted) & set(known[2].tolist())
    return {"n": n, "graph": graph, "pred": pred, "anchor": anchor, "rel": rel, "known": known, "planted": planted,
            "hub_tails": hub_tails}


@pytest.mark.parametrize("k", [10, 128])
def test_two_launch_path_equals_the_definition(long_rows, k):
    from ultra_torchdrug_amd import functional as UF
    dev, n, pred = _dev(), long_rows["n"], long_rows["pred"]
    keys = long_rows["graph"].to(dev).completion_keys(0)
    got = UF.topk_keys(pred.to(dev), k, keys, long_rows["anchor"].to(dev), long_rows["rel"].to(dev), 3, n_node=n)
    _check(got, pred, k, long_rows["known"])
    index = got[1].cpu()
    # the shared maximum: the planted entities in index order across the slices, none of the hub's known tails
    assert index[2, :6].tolist() == long_rows["planted"] and not set(index[2].tolist()) & set(long_rows["hub_tails"])
    assert int(index[3].min()) >= 65536                                      # every answer from the last slice
    assert index[4].tolist() == np.setdiff1d(np.arange(n), long_rows["known"][4])[::-1][:k].tolist()
    _check(UF.topk_keys(pred.to(dev), k, None, long_rows["anchor"].to(dev), long_rows["rel"].to(dev), 3), pred, k, None)


# ------------------------------------------------------------------------------------------------ the rank kernel agrees
def test_listed_answers_rank_where_they_are_listed(long_rows):
    """On a tie-free row ``filtered_rank_keys`` ranks the j-th answer j + 2: the j better answers, itself (an unfiltered
    candidate is no known truth, so it counts itself) and the leading 1."""
    from ultra_torchdrug_amd import functional as UF
    dev, n, k = _dev(), long_rows["n"], 128
    g = torch.Generator().manual_seed(21)
    row = torch.randperm(n, generator=g).float()                             # distinct scores
    short_graph, _, _ = _hub_graph(20_000, 5, np.arange(0, 20_000, 40))
    for rows, keys, note in ((row[None, :], long_rows["graph"].to(dev).completion_keys(0), "two launches"),
                             (row[None, :20_000].contiguous(), short_graph.to(dev).completion_keys(0), "one launch")):
        rows_d = rows.to(dev)
        anchor, rel = torch.tensor([3], device=dev), torch.tensor([0], device=dev)
        _, index = UF.topk_keys(rows_d, k, keys, anchor, rel, 3, n_node=rows.shape[1])
        ranks = UF.filtered_rank_keys(rows_d.repeat(k, 1), index[0], keys, anchor.repeat(k), rel.repeat(k), 3, rows.shape[1])
        assert ranks.tolist() == [j + 2 for j in range(k)], note


# ------------------------------------------------------------------------------------------------ model level
@pytest.fixture(scope="module")
def small():
    graph = wide_graph()
    task = small_task(graph)
    with torch.no_grad():                                                    # (as in tests/test_answers_cpu.py: the known
        task.model.mlp.layers[-1].weight.neg_()                              # completions lead every unfiltered list)
    batch = wide_batch(graph)
    queries = {}
    for head in (False, True):
        side = 1 if head else 0
        queries[head] = (batch[:, side].clone(), batch[:, 2].clone(), task.answer(batch[:, side], batch[:, 2], k=10, head=head))
    triples = graph.edge_list.numpy()
    known = {head: [completions(triples, 1 if head else 0, int(b[1 if head else 0]), int(b[2])) for b in batch]
             for head in (False, True)}
    return {"task": task.to(_dev()), "batch": batch, "queries": queries, "known": known}


@pytest.mark.parametrize("head", [False, True])
def test_task_and_engine_answers_on_the_device(small, head):
    from ultra_torchdrug_amd import engine
    dev, task, batch = _dev(), small["task"], small["batch"]
    side = 1 if head else 0
    anchor, relation, (cpu_entities, _) = small["queries"][head]
    with torch.no_grad():
        pred = task.predict(batch.to(dev))[:, side]
    # the definition on the device's OWN scores (fp32 differences between host and device must not flip a tie) ...
    want_index, _ = topk_rows(pred.cpu().numpy(), 10, small["known"][head])
    runs = {"task": task.answer(anchor.to(dev), relation.to(dev), k=10, head=head),
            "engine eager": engine.answer(task, anchor.to(dev), relation.to(dev), k=10, head=head, batch_size=2, graphed=False),
            "engine graphed": engine.answer(task, anchor.to(dev), relation.to(dev), k=10, head=head, batch_size=2, graphed=True)}
    for name, (entities, scores) in runs.items():
        assert entities.dtype == torch.int64 and scores.dtype == torch.float32 and entities.shape == (len(batch), 10), name
        assert np.array_equal(entities.cpu().numpy(), want_index), name
        assert torch.equal(scores, pred.gather(1, entities)), name           # the device's own predict scores
        assert torch.equal(entities.cpu(), cpu_entities), name               # ... and the CPU task's entities


def test_engine_answer_replays_the_fused_score_head():
    """A 64-wide model has the fused all-entity score head: ``engine.answer`` scores its chunks through one captured
    ``GraphedScores`` and equals ``task.answer`` chunk for chunk, eager and replayed."""
    from ultra_torchdrug_amd import engine
    from ultra_torchdrug_amd.task import build_ultra
    dev = _dev()
    graph = wide_graph()
    torch.manual_seed(5)
    task = build_ultra(graph.num_relation, hidden_dims=(64,) * 2, rel_layers=2, num_negative=8, full_batch_eval=True)
    task.preprocess(graph)
    task = task.eval().to(dev)
    g = torch.Generator().manual_seed(4)
    anchor, relation = torch.randint(0, 300, (21,), generator=g).to(dev), torch.randint(0, 5, (21,), generator=g).to(dev)
    anchor[0], relation[0] = 11, 1
    probe = engine.GraphedScores(task, anchor[:4], relation[:4], relation[:4], graphed=False)
    assert probe(anchor[:4], relation[:4], relation[:4]) is not None
    for head in (False, True):
        want = []
        for i in range(0, 21, 4):                                            # chunks of 4, the last one repeating its end
            ids = torch.arange(i, i + 4, device=dev).clamp(max=20)
            want.append(task.answer(anchor[ids], relation[ids], k=10, head=head))
        want = torch.cat([w[0] for w in want])[:21], torch.cat([w[1] for w in want])[:21]
        keys = task.graph.completion_keys(1 if head else 0)
        hub = keys[(keys >= (11 * 5 + 1) * 300) & (keys < (11 * 5 + 2) * 300)] - (11 * 5 + 1) * 300
        assert head or (len(hub) == 40 and not set(want[0][0].tolist()) & set(hub.tolist()))
        for graphed in (False, True):
            got = engine.answer(task, anchor, relation, k=10, head=head, batch_size=2, graphed=graphed)
            assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), (head, graphed)


# ------------------------------------------------------------------------------------------------ capture
@pytest.mark.parametrize("n", [300, 70_000])
def test_topk_keys_captured_into_a_hipgraph(n):
    from ultra_torchdrug_amd import functional as UF
    dev, k = _dev(), 10
    graph, triples, _ = _hub_graph(n, 8, np.arange(0, n, max(n // 100, 1))[:100])
    keys = graph.to(dev).completion_keys(0)
    anchor, rel = torch.tensor([3, 5], device=dev), torch.tensor([0, 1], device=dev)
    known = [completions(triples, 0, 3, 0), completions(triples, 0, 5, 1)]
    first, second = tied_scores(2, n, seed=31)[:, 0].contiguous(), tied_scores(2, n, seed=32)[:, 0].contiguous()
    static = first.to(dev)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        UF.topk_keys(static, k, keys, anchor, rel, 3, n_node=n)              # warm-up (the workspace enters the allocator's cache)
    torch.cuda.current_stream().wait_stream(side)
    captured = torch.cuda.CUDAGraph()
    with torch.cuda.graph(captured, stream=side):
        value, index = UF.topk_keys(static, k, keys, anchor, rel, 3, n_node=n)
    captured.replay()
    _check((value, index), first, k, known, "replay on the captured scores")
    static.copy_(second.to(dev))
    captured.replay()
    torch.cuda.synchronize()
    _check((value, index), second, k, known, "replay on new scores")
    eager = UF.topk_keys(second.to(dev), k, keys, anchor, rel, 3, n_node=n)
    assert torch.equal(eager[1], index) and torch.equal(eager[0], value)


# ------------------------------------------------------------------------------------------------ refusals
def test_topk_keys_refuses_bad_arguments(wide):
    from ultra_torchdrug_amd import functional as UF
    dev, graph = _dev(), wide["graph"]
    batch = wide["batch"].to(dev)
    pred = tied_scores(len(batch), 300, seed=1).to(dev)
    keys = graph.completion_keys(0)
    args = lambda **kw: dict(dict(pred=pred[:, 0], k=10, keys=keys, anchor=batch[:, 0], rel=batch[:, 2], n_rel=5, n_node=300), **kw)
    UF.topk_keys(**args())
    flat = pred.reshape(-1)
    for bad in (dict(k=0), dict(k=129), dict(anchor=batch[:, 0].int()), dict(n_node=301),
                dict(pred=flat.as_strided((len(batch), 300), (150, 1))), dict(pred=pred[:, 0].double()),
                dict(pred=pred[:, 0, ::2], n_node=150), dict(keys=keys.int()), dict(keys=keys.cpu()), dict(anchor=batch[:, 0].cpu()),
                dict(rel=batch[:, 2].cpu()), dict(pred=pred[:, 0].cpu())):
        with pytest.raises(RuntimeError):
            UF.topk_keys(**args(**bad))
    torch.cuda.synchronize()

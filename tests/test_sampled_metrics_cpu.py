"""CPU: the sampled ranking metrics of the reference's inductive task (ultra/task.py:463-523) -- ``hits@K_N``, the chance
that fewer than K of N uniformly drawn unfiltered negatives outrank the positive, and ``toy_eval``, the rank among 50
negatives drawn without replacement -- on the dense-mask path of ``task.rank_statistics`` and in ``task.evaluate``."""
import numpy as np
import pytest
import torch

from sampled_graphs import S, binomial_fp64, dense_samples, draw_numpy, edge_rand, ring_graph, small_task, tied_scores, wide_batch, wide_graph

SAMPLED = ("hits@10_50", "hits@1_50", "hits@3_20")


def _bare_task(**kwargs):
    from ultra_torchdrug_amd.task import build_ultra
    return build_ultra(4, hidden_dims=(16,) * 2, input_dim=16, rel_hidden=16, rel_layers=2, **kwargs)


# ------------------------------------------------------------------------------------------------ the formula
def test_sampled_hits_equal_the_fp64_binomial_sum():
    """evaluate's fp32 evaluation of the reference expression against exact binomials in fp64: 1e-5 absolute (each of the
    at most K positive terms carries ~2N ulps of relative error, 6e-6 at N = 50, and the terms sum to at most 1; measured
    on the CPU the fp32 expression stays within 3.1e-6 over these counts).  Before the sampled names were parsed,
    ``hits@10_50`` was read as ``hits@1050``: ranking [[30, 2000]] gave exactly 1.0 and 0.0."""
    pairs = [(1, 51), (52, 51), (7, 51), (1, 260), (30, 260), (261, 260), (100, 260), (30, 14541), (2000, 14541),
             (14542, 14541), (1, 14541), (700, 14541), (3, 10_000_000), (1_000_000, 10_000_000), (10_000_001, 10_000_000),
             (5_000_000, 10_000_000)]
    names = SAMPLED + tuple(n + "-tail" for n in SAMPLED) + tuple(n + "-head" for n in SAMPLED)
    task = _bare_task(metric=names)
    assert task.needs_statistics and not _bare_task().needs_statistics
    for a, b in zip(pairs[0::2], pairs[1::2]):
        ranking = torch.tensor([[a[0], b[0]]], dtype=torch.long)
        count = torch.tensor([[a[1], b[1]]], dtype=torch.long)
        metric = task.evaluate(ranking, num_candidates=count)
        for name in SAMPLED:
            k, n = (int(v) for v in name[5:].split("_"))
            tail, head = binomial_fp64(a[0], a[1], k, n), binomial_fp64(b[0], b[1], k, n)
            assert abs(float(metric[name + "-tail"]) - tail) <= 1e-5, (name, a)
            assert abs(float(metric[name + "-head"]) - head) <= 1e-5, (name, b)
            assert abs(float(metric[name]) - 0.5 * (tail + head)) <= 1e-5, (name, a, b)
    metric = task.evaluate(torch.tensor([[30, 2000]]), num_candidates=torch.tensor([[14541, 14541]]))
    assert 0.99 < float(metric["hits@10_50-tail"]) < 1.0 and 0.0 < float(metric["hits@10_50-head"]) < 0.9
    assert float(metric["hits@10_50-tail"]) == pytest.approx(binomial_fp64(30, 14541, 10, 50), abs=1e-5)
    assert float(metric["hits@10_50-head"]) == pytest.approx(binomial_fp64(2000, 14541, 10, 50), abs=1e-5)


def test_sampled_metric_without_candidate_counts_raises():
    task = _bare_task(metric=("mrr", "hits@10_50"))
    with pytest.raises(ValueError, match="hits@10_50"):
        task.evaluate(torch.tensor([[30, 2000]]))
    with pytest.raises(ValueError):
        _bare_task(metric=("hits@10_50_2",)).evaluate(torch.tensor([[1, 1]]), num_candidates=torch.tensor([[60, 60]]))
    # threshold metrics and the default tuple are what they were
    plain = _bare_task()
    assert plain.metric == ("mr", "mrr", "hits@1", "hits@3", "hits@10", "mrr-tail", "hits@1-tail", "hits@10-tail")
    got = plain.evaluate(torch.tensor([[1, 4], [11, 2]]))
    assert float(got["hits@3"]) == 0.5 and float(got["hits@10-tail"]) == 0.5 and float(got["mr"]) == 4.5


# ------------------------------------------------------------------------------------------------ rank_statistics
def test_rank_statistics_columns_on_cpu_tensors():
    graph = wide_graph(full_row=True)
    task = small_task(graph, metric=("mrr", "hits@10_50"))
    batch = wide_batch(graph)
    pred = tied_scores(len(batch), 300, seed=1)
    stats = task.rank_statistics(batch, pred=pred)
    mask, target = task.target(batch)
    assert stats.shape == (len(batch), 2, 4) and stats.dtype == torch.int64
    assert torch.equal(stats[..., 0], task.get_ranking(pred, (mask, target)))
    assert torch.equal(stats[..., 0], task.rank_batch(batch, pred=pred))
    assert torch.equal(stats[..., 1], mask.sum(-1))
    assert not stats[..., 2:].any()                                   # no toy_eval: nothing is drawn
    assert int(stats[-4, 0, 1]) == 300 and int(stats[-3, 0, 1]) == 0  # (9, 3, ?): no completion; (7, 2, ?): every node


def test_toy_eval_with_exactly_fifty_candidates_ranks_among_all_of_them():
    """Every query of the ring graph has exactly 50 unfiltered candidates, so whatever the uniform numbers are the draw
    is all of them: the two counts are sums over the mask -- a check that restates nothing of the draw."""
    graph = ring_graph()
    task = small_task(graph, toy_eval=True, metric=("mr", "mrr", "hits@10", "hits@10_50"))
    batch = graph.edge_list[torch.arange(0, 2688, 97)]
    pred = tied_scores(len(batch), 64, seed=2)
    mask, target = task.target(batch)
    assert torch.equal(mask.sum(-1), torch.full((len(batch), 2), 50))
    pos = pred.gather(-1, target.unsqueeze(-1))
    for rand in (edge_rand(len(batch), seed=3), torch.rand(len(batch), 2, S), None):
        stats = task.rank_statistics(batch, pred=pred, rand=rand)
        assert torch.equal(stats[..., 1], mask.sum(-1))
        assert torch.equal(stats[..., 3], ((pos <= pred) & mask).sum(-1))
        assert torch.equal(stats[..., 2], ((pos < pred) & mask).sum(-1))
        assert (stats[..., 2] != stats[..., 3]).any()                 # the ties count
        if rand is not None:
            drawn = dense_samples(pred, target, mask, rand).sort(dim=-1).values
            assert torch.equal(drawn, mask.nonzero()[:, 2].view(len(batch), 2, S))
    ranking = task.toy_ranking(stats)
    assert ranking.dtype == torch.float32 and torch.equal(ranking, 0.5 * (stats[..., 2] + stats[..., 3]).float() + 1)
    metric = task.evaluate(ranking, num_candidates=stats[..., 1])
    assert float(metric["mr"]) == pytest.approx(float(ranking.mean()))
    assert float(metric["hits@10"]) == pytest.approx(float((ranking <= 10).float().mean()))
    want = np.mean([binomial_fp64(float(r), 51, 10, 50) for r in ranking.reshape(-1)])      # fp_rate = (ranking - 1) / 51
    assert float(metric["hits@10_50"]) == pytest.approx(want, abs=1e-5)
    with pytest.raises(ValueError):                                   # the reference asserts num_sample == 50
        small_task(graph, toy_eval=True, metric=("hits@3_20",)).evaluate(ranking, num_candidates=stats[..., 1])


def test_toy_eval_draw_is_the_definition_restated_in_numpy():
    graph = wide_graph()
    task = small_task(graph, toy_eval=True, metric=("mrr", "hits@10_50"))
    batch = wide_batch(graph)
    pred = tied_scores(len(batch), 300, seed=4)
    rand = edge_rand(len(batch), seed=5)
    mask, target = task.target(batch)
    count = mask.sum(-1)
    assert int(count.min()) >= 260 and int(count.min()) == 260        # at most 40 completions per query (the hub: exactly 40)
    stats = task.rank_statistics(batch, pred=pred, rand=rand)
    samples = dense_samples(pred, target, mask, rand)
    assert samples.shape == (len(batch), 2, S) and samples.dtype == torch.int64
    pos = pred.gather(-1, target.unsqueeze(-1))
    for b in range(len(batch)):
        for side in (0, 1):
            free = mask[b, side].nonzero().flatten().numpy()
            want = draw_numpy(free, rand[b, side].numpy())
            got = samples[b, side].tolist()
            assert got == want, (b, side)
            assert len(set(got)) == S and all(mask[b, side, e] for e in got)            # distinct and unfiltered
            neg = pred[b, side, got]
            assert int(stats[b, side, 2]) == int((pos[b, side] < neg).sum())
            assert int(stats[b, side, 3]) == int((pos[b, side] <= neg).sum())
    assert torch.equal(stats[..., 1], count)
    assert torch.equal(stats[..., 0], task.get_ranking(pred, (mask, target)))


def test_toy_eval_with_fewer_than_fifty_candidates_raises_at_evaluate():
    graph = ring_graph(extra=[(0, 40, 0)])                            # a 15th tail for (0, 0, ?): 49 candidates
    task = small_task(graph, toy_eval=True, metric=("mrr", "hits@10_50"))
    batch = torch.tensor([[0, 3, 0], [5, 9, 1]])
    pred = tied_scores(2, 64, seed=6)
    rand = edge_rand(2, seed=7)
    stats = task.rank_statistics(batch, pred=pred, rand=rand)
    samples = dense_samples(pred, *reversed(task.target(batch)), rand)
    assert stats[:, :, 1].tolist() == [[49, 50], [50, 50]]            # (the extra triple is no head of (?, 0, 3))
    assert (samples[0, 0] >= 0).sum() == 49 and int(samples[0, 0, -1]) == -1
    with pytest.raises(ValueError, match="49"):
        task.evaluate(task.toy_ranking(stats), num_candidates=stats[..., 1])
    with pytest.raises(ValueError):
        task.evaluate(task.toy_ranking(stats))
    task.evaluate(task.toy_ranking(stats[1:]), num_candidates=stats[1:, :, 1])


# ------------------------------------------------------------------------------------------------ per relation, the driver
def test_metric_per_rel_groups_the_per_query_sampled_scores():
    graph = wide_graph()
    task = small_task(graph, metric=("mrr", "hits@10_50", "hits@10_50-head"), metric_per_rel=True)
    g = torch.Generator().manual_seed(8)
    n = 40
    ranking = torch.randint(1, 250, (n, 2), generator=g)
    count = torch.randint(260, 300, (n, 2), generator=g)
    rel = torch.randint(0, 5, (n,), generator=g)
    metric = task.evaluate(ranking, rel=rel, num_candidates=count)
    value = np.array([[binomial_fp64(int(ranking[i, s]), int(count[i, s]), 10, 50) for s in (0, 1)] for i in range(n)])
    assert float(metric["hits@10_50"]) == pytest.approx(value.mean(), abs=1e-5)
    assert float(metric["hits@10_50-head"]) == pytest.approx(value[:, 1].mean(), abs=1e-5)
    for ridx in range(10):
        side, r = divmod(ridx, 5)                                     # tails under r, heads under r + num_relation
        rows = (rel == r).numpy()
        want = value[rows, side].mean() if rows.any() else 0.0
        assert float(metric["hits@10_50_rel_%d" % ridx]) == pytest.approx(want, abs=1e-5), ridx
        want = (1 / ranking[torch.from_numpy(rows), side].double()).mean() if rows.any() else 0.0
        assert float(metric["mrr_rel_%d" % ridx]) == pytest.approx(float(want), abs=1e-6), ridx
    assert "hits@10_50-head_rel_0" not in metric


def test_engine_evaluate_on_cpu_does_not_depend_on_the_batch_size():
    """The driver on CPU tensors: the (n, 2, 4) statistics go through the triple loop, the sampled metric is the formula on
    the dense-mask ranks and counts, and under toy_eval the uniform numbers are drawn once for the whole set."""
    from ultra_torchdrug_amd import engine
    graph = wide_graph()
    test = wide_batch(graph)
    task = small_task(graph, metric=("mrr", "hits@10", "hits@10_50"))
    metric, ranking = engine.evaluate(task, test, batch_size=4)
    with torch.no_grad():
        pred = torch.cat([task.predict(test[i:i + 4]) for i in range(0, len(test), 4)])
        mask, target = task.target(test)
    rank = task.get_ranking(pred, (mask, target))
    assert ranking.dtype == torch.int64 and torch.equal(ranking, rank)
    want = np.mean([binomial_fp64(int(r), int(c), 10, 50) for r, c in zip(rank.reshape(-1), mask.sum(-1).reshape(-1))])
    assert float(metric["hits@10_50"]) == pytest.approx(want, abs=1e-5)
    assert float(metric["mrr"]) == pytest.approx(float((1 / rank.float()).mean()))
    toy = small_task(graph, toy_eval=True, metric=("mrr", "hits@10", "hits@10_50"))
    runs = [engine.evaluate(toy, test, batch_size=b, generator=torch.Generator().manual_seed(11)) for b in (4, 16, 3)]
    assert runs[0][1].dtype == torch.float32 and runs[0][1].shape == (len(test), 2)
    for other in runs[1:]:
        assert torch.equal(other[1], runs[0][1])
        assert {k: float(v) for k, v in other[0].items()} == {k: float(v) for k, v in runs[0][0].items()}
    rand = torch.rand(len(test), 2, S, generator=torch.Generator().manual_seed(11))
    stats = toy.rank_statistics(test, pred=pred, rand=rand)
    assert torch.equal(runs[0][1], toy.toy_ranking(stats))


# ------------------------------------------------------------------------------------------------ the C entries (no GPU touched)
def test_entries_are_bound_and_check_their_arguments_before_any_launch():
    from ultra_torchdrug_amd import _lib
    lib = _lib.load()
    assert {"ultra_filter_counts", "ultra_sampled_rank_keys"} <= set(_lib.EXPORTS) and _lib.ABI_VERSION == 8
    BAD_SHAPE, NULL_POINTER = 2, 3

    def sampled(n_query, n_sample):
        return lib.ultra_sampled_rank_keys(None, n_query, 4, 4, None, 1, None, 0, None, None, 1, 1, None, n_sample, None, None,
                                           None, None)
    assert sampled(1, 65) == BAD_SHAPE and sampled(1, 0) == BAD_SHAPE and sampled(0, 65) == BAD_SHAPE
    assert sampled(1, 64) == NULL_POINTER and sampled(1, 1) == NULL_POINTER and sampled(0, 50) == 0
    assert lib.ultra_filter_counts(None, 0, None, None, 1, 3, 1, 0, None, None) == BAD_SHAPE          # n_node = 0
    assert lib.ultra_filter_counts(None, 0, None, None, 1, 3, 1, 9, None, None) == NULL_POINTER
    assert lib.ultra_filter_counts(None, 0, None, None, 1, 0, 1, 9, None, None) == 0


# ------------------------------------------------------------------------------------------------ two ranks (gloo)
def _toy_rank_worker(rank, world, port, out_dir):
    import os
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    for p in (os.path.dirname(here), here):
        if p not in sys.path:
            sys.path.insert(0, p)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank), OMP_NUM_THREADS="2")
    torch.set_num_threads(2)
    from ultra_torchdrug_amd import engine
    engine.init_distributed("gloo")
    graph = wide_graph()
    task = small_task(graph, toy_eval=True, metric=("mrr", "hits@10_50"))
    torch.manual_seed(100 + rank)                                     # ranks seeded apart, no generator given
    metric, ranking = engine.evaluate(task, wide_batch(graph), batch_size=4)
    torch.save(dict(ranking=ranking, metric={k: float(v) for k, v in metric.items()}), os.path.join(out_dir, "rank%d.pt" % rank))
    torch.distributed.destroy_process_group()


def test_two_ranks_seeded_apart_draw_the_same_uniform_numbers(tmp_path):
    """In a process group rank 0's uniform numbers are broadcast: both ranks return the rankings of ONE process that draws
    from rank 0's seed, whatever the other rank's generator holds and wherever the shard boundaries fall."""
    import os
    import socket
    import torch.multiprocessing as mp
    from ultra_torchdrug_amd import engine
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    mp.spawn(_toy_rank_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    r0, r1 = (torch.load(os.path.join(tmp_path, "rank%d.pt" % r)) for r in range(2))
    assert torch.equal(r0["ranking"], r1["ranking"]) and r0["metric"] == r1["metric"]
    graph = wide_graph()
    task = small_task(graph, toy_eval=True, metric=("mrr", "hits@10_50"))
    torch.manual_seed(100)
    metric, ranking = engine.evaluate(task, wide_batch(graph), batch_size=4)
    assert torch.equal(ranking, r0["ranking"]) and {k: float(v) for k, v in metric.items()} == r0["metric"]

"""MI355X: the sampled ranking metrics on the device -- ``ultra_filter_counts`` and ``ultra_sampled_rank_keys`` against the
dense-mask CPU path for the same uniform numbers (integers: ``torch.equal``, no tolerance), ``task.rank_statistics`` past the
sliced rank kernel's threshold, and ``engine.evaluate`` eager / replayed as a hipGraph / over unique queries."""
import numpy as np
import pytest
import torch

from sampled_graphs import S, binomial_fp64, dense_samples, edge_rand, small_task, tied_scores, wide_batch, wide_graph

pytestmark = pytest.mark.gpu


def _dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def wide():
    """The 300-node graph with a full and a nearly full completion row: CPU masks and targets (the reference side, computed
    once) and the graph on the device."""
    graph = wide_graph(full_row=True)
    task = small_task(graph, toy_eval=True, metric=("mrr", "hits@10_50"))
    batch = wide_batch(graph)
    mask, target = task.target(batch)
    assert int(mask[8, 0].sum()) == 0 and 0 < int(mask[9, 0].sum()) <= 30      # (7, 2, ?): no candidate; (13, 0, ?): fewer than 50
    return {"graph": graph.to(_dev()), "batch": batch, "mask": mask, "target": target}


# ------------------------------------------------------------------------------------------------ filter_counts
def test_filter_counts_equal_the_dense_mask_sums(wide):
    from ultra_torchdrug_amd import functional as UF
    dev, graph = _dev(), wide["graph"]
    batch = wide["batch"].to(dev)
    want = wide["mask"].sum(-1)
    assert int(want[7, 0]) == 300 and int(want[8, 0]) == 0                    # no completion at all; every node completes
    for side in (0, 1):
        keys = graph.completion_keys(side)
        anchor, rel = batch[:, side], batch[:, 2]                            # strided views of the (B, 3) batch
        assert anchor.stride(0) == 3 and not anchor.is_contiguous()
        got = UF.filter_counts(keys, anchor, rel, 5, 300)
        assert got.dtype == torch.int64 and torch.equal(got.cpu(), want[:, side])
        assert torch.equal(UF.filter_counts(keys, anchor.contiguous(), rel.contiguous(), 5, 300), got)
        assert torch.equal(UF.filter_counts(keys, anchor.contiguous(), rel, 5, 300), got)      # strides differ: copies
        assert torch.equal(UF.filter_counts(keys, anchor[:1], rel[:1], 5, 300), got[:1])
        assert UF.filter_counts(None, anchor, rel, 5, 300).tolist() == [300] * len(batch)      # unfiltered ranking
        assert UF.filter_counts(keys, anchor[:0], rel[:0], 5, 300).shape == (0,)
    with pytest.raises(RuntimeError):
        UF.filter_counts(graph.completion_keys(0), batch[:, 0].int(), batch[:, 2], 5, 300)
    with pytest.raises(RuntimeError):
        UF.filter_counts(graph.completion_keys(0), batch[:, 0].cpu(), batch[:, 2].cpu(), 5, 300)


# ------------------------------------------------------------------------------------------------ sampled_rank_keys
@pytest.mark.parametrize("n_sample", [1, 50, 64])
def test_sampled_rank_keys_equal_the_dense_path_for_the_same_uniform_numbers(wide, n_sample):
    from ultra_torchdrug_amd import functional as UF
    from ultra_torchdrug_amd.task import dense_sampled_ranks
    dev, graph = _dev(), wide["graph"]
    batch, mask, target = wide["batch"], wide["mask"], wide["target"]
    pred = tied_scores(len(batch), 300, seed=20 + n_sample)
    rand = edge_rand(len(batch), seed=30 + n_sample, n_sample=n_sample)
    pred_d, rand_d, batch_d, target_d = pred.to(dev), rand.to(dev), batch.to(dev), target.to(dev)
    differ = 0
    for side in (0, 1):
        want = dense_sampled_ranks(pred[:, side], target[:, side], mask[:, side], rand[:, side].contiguous())
        view = pred_d[:, side]                                               # a strided side view of the (B, 2, N) scores
        assert view.stride(0) == 600
        got = UF.sampled_rank_keys(view, target_d[:, side], graph.completion_keys(side), batch_d[:, side], batch_d[:, 2], 5,
                                   rand_d[:, side], n_node=300, return_samples=True)
        torch.cuda.synchronize()
        for g, w, what in zip(got, want, ("optimistic", "pessimistic", "samples")):
            assert g.dtype == torch.int64 and torch.equal(g.cpu(), w), (what, side)
        samples = got[2].cpu()
        assert torch.equal((samples >= 0).sum(-1), mask[:, side].sum(-1).clamp(max=n_sample))      # S_eff = min(S, n_free)
        for b in range(len(batch)):
            drawn = samples[b][samples[b] >= 0]
            assert len(set(drawn.tolist())) == len(drawn) and bool(mask[b, side][drawn].all())     # distinct, unfiltered
        pair = UF.sampled_rank_keys(view, target_d[:, side], graph.completion_keys(side), batch_d[:, side], batch_d[:, 2], 5,
                                    rand_d[:, side], n_node=300)
        assert len(pair) == 2 and torch.equal(pair[0], got[0]) and torch.equal(pair[1], got[1])
        differ += int((got[0] != got[1]).sum())
        # keys = None: every entity is a candidate (the unfiltered ranking)
        free = UF.sampled_rank_keys(view, target_d[:, side], None, batch_d[:, side], batch_d[:, 2], 5, rand_d[:, side],
                                    return_samples=True)
        want = dense_sampled_ranks(pred[:, side], target[:, side], torch.ones_like(mask[:, side]), rand[:, side].contiguous())
        assert all(torch.equal(g.cpu(), w) for g, w in zip(free, want))
    assert differ > 0 or n_sample == 1                                      # exact ties with the positive were drawn


def test_sampled_rank_keys_refuses_what_its_neighbours_refuse(wide):
    from ultra_torchdrug_amd import functional as UF
    dev, graph = _dev(), wide["graph"]
    batch, target = wide["batch"].to(dev), wide["target"].to(dev)
    pred = tied_scores(len(batch), 300, seed=1).to(dev)
    keys = graph.completion_keys(0)
    args = lambda **kw: dict(dict(pred=pred[:, 0], target=target[:, 0], keys=keys, anchor=batch[:, 0], rel=batch[:, 2], n_rel=5,
                                  rand=torch.rand(len(batch), S, device=dev), n_node=300), **kw)
    UF.sampled_rank_keys(**args())
    for bad in (dict(rand=torch.rand(len(batch), 65, device=dev)), dict(rand=torch.rand(len(batch), 0, device=dev)),
                dict(n_node=301), dict(pred=pred[:, 0].double()), dict(rand=torch.rand(len(batch), S)),
                dict(target=target[:, 0].int()), dict(keys=keys.int()), dict(pred=pred[:, 0, ::2])):
        with pytest.raises(RuntimeError):
            UF.sampled_rank_keys(**args(**bad))
    torch.cuda.synchronize()


def test_rank_statistics_past_the_sliced_rank_threshold():
    """70 000 candidates (> 2 * 32768: the rank comes from the sliced kernels): all four columns and the drawn entities
    equal the dense-mask CPU path."""
    from ultra_torchdrug_amd import functional as UF
    from ultra_torchdrug_amd.graph import Graph
    n = 70_000
    rng = np.random.default_rng(3)
    e = np.stack([rng.integers(0, n, 20000), rng.integers(0, n, 20000), rng.integers(0, 3, 20000)], axis=1)
    hub = np.stack([np.full(500, 3), rng.permutation(n)[:500], np.zeros(500, dtype=np.int64)], axis=1)
    graph = Graph(torch.from_numpy(np.concatenate([e, hub]).astype(np.int64)), num_node=n, num_relation=3)
    task = small_task(graph, toy_eval=True, metric=("mrr", "hits@10_50"))
    batch = torch.tensor([hub[7].tolist(), e[0].tolist(), [n - 1, n - 2, 2]])
    pred, rand = tied_scores(3, n, seed=9), edge_rand(3, seed=10)
    want = task.rank_statistics(batch, pred=pred, rand=rand)
    want_samples = dense_samples(pred, *reversed(task.target(batch)), rand)
    assert n - 510 <= int(want[0, 0, 1]) <= n - 500 and int(want[..., 0].max()) > 1000
    dev = _dev()
    task.to(dev)
    got = task.rank_statistics(batch.to(dev), pred=pred.to(dev), rand=rand.to(dev))
    assert got.dtype == torch.int64 and torch.equal(got.cpu(), want)
    fact = task.graph
    samples = UF.sampled_rank_keys(pred.to(dev)[:, 0], batch.to(dev)[:, 1], fact.completion_keys(0), batch.to(dev)[:, 0],
                                   batch.to(dev)[:, 2], 3, rand.to(dev)[:, 0], n_node=n, return_samples=True)[2]
    assert torch.equal(samples.cpu(), want_samples[:, 0])


# ------------------------------------------------------------------------------------------------ engine.evaluate
METRIC = ("mrr", "hits@10", "hits@10_50")


def _inductive(toy_eval, metric_per_rel=False):
    """500 nodes, 8 relations: messages on the inference fact graph, rankings filtered by the whole inference graph; the test
    triples share heads and tails, one query has 120 known tails."""
    from ultra_torchdrug_amd.data import synthetic_triples
    from ultra_torchdrug_amd.graph import Graph
    from ultra_torchdrug_amd.task import build_ultra
    train, _, _ = synthetic_triples((500, 3000, 8), 41, alpha=0.0)
    inf, _, _ = synthetic_triples((500, 3300, 8), 42, alpha=0.0)
    rng = np.random.default_rng(43)
    hub = np.stack([np.full(120, 5), rng.permutation(500)[:120], np.ones(120, dtype=np.int64)], axis=1)
    fact, held = np.concatenate([inf[:3000], hub[:100]]), np.concatenate([inf[3000:], hub[100:]])
    torch.manual_seed(44)
    task = build_ultra(8, metric=METRIC, toy_eval=toy_eval, metric_per_rel=metric_per_rel)
    g_train = Graph(torch.from_numpy(train), num_node=500, num_relation=8)
    g_fact = Graph(torch.from_numpy(fact), num_node=500, num_relation=8)
    g_all = Graph(torch.from_numpy(np.concatenate([fact, held])), num_node=500, num_relation=8)
    task.preprocess_inductive(g_train, g_train, g_fact, graph=g_train, inductive_graph=g_all)
    base = torch.from_numpy(held[:40])
    shared_head = base[:12].clone(); shared_head[:, 1] = base[12:24, 1]         # same (h, r), other tails
    shared_tail = base[:12].clone(); shared_tail[:, 0] = base[24:36, 0]         # same (t, r), other heads
    test = torch.cat([base, shared_head, shared_tail, torch.from_numpy(hub[100:106]), base[:3]])      # 73: 9 batches of 8 + 1
    return task.to(_dev()).eval().use("test"), test


def _formula(rank, count, k=10, n=50):
    """The reference expression (ultra/task.py:497-506) with torch ops, fp32, per query."""
    import math
    fp_rate = (rank - 1).float() / count
    score = 0
    for i in range(k):
        num_comb = math.factorial(n) / math.factorial(i) / math.factorial(n - i)
        score += num_comb * (fp_rate ** i) * ((1 - fp_rate) ** (n - i))
    return score


def test_evaluate_sampled_hits_is_the_formula_on_dense_ranks_and_mask_sums():
    from ultra_torchdrug_amd import engine
    task, test = _inductive(toy_eval=False, metric_per_rel=True)
    dev = _dev()
    metric, ranking = engine.evaluate(task, test, batch_size=8)
    with torch.no_grad():
        pred = torch.cat([task.predict(test[i:i + 8].to(dev)) for i in range(0, len(test), 8)])
        mask, target = task.target(test.to(dev))
        rank = task.get_ranking(pred, (mask, target))
    count = mask.sum(-1)
    assert ranking.dtype == torch.int64 and torch.equal(ranking, rank)
    assert int(count.min()) <= 500 - 120 and int(count.max()) >= 495
    value = _formula(rank, count)
    # the same fp32 expression on the same integers: what may differ is the order of the mean's additions (146 values in [0, 1])
    assert abs(float(metric["hits@10_50"]) - float(value.mean())) <= 1e-6
    want64 = np.mean([binomial_fp64(int(r), int(c), 10, 50) for r, c in zip(rank.reshape(-1).cpu(), count.reshape(-1).cpu())])
    assert abs(float(metric["hits@10_50"]) - want64) <= 1e-5
    assert float(metric["mrr"]) == pytest.approx(float((1 / rank.float()).mean()), abs=1e-6)
    assert float(metric["hits@10"]) == pytest.approx(float((rank <= 10).float().mean()), abs=1e-6)
    rel = test[:, 2]
    for ridx in range(16):
        side, r = divmod(ridx, 8)
        rows = (rel == r).to(dev)
        want = float(value[rows, side].mean()) if bool(rows.any()) else 0.0
        assert abs(float(metric["hits@10_50_rel_%d" % ridx]) - want) <= 1e-6, ridx
    other, other_ranking = engine.evaluate(task, test, batch_size=8, graphed=False, unique_queries=False)
    assert torch.equal(other_ranking, ranking) and all(torch.equal(other[k], metric[k]) for k in metric)


def test_toy_eval_is_the_same_eager_graphed_and_over_unique_queries():
    from ultra_torchdrug_amd import engine
    from ultra_torchdrug_amd.engine import GraphedPredict
    from ultra_torchdrug_amd.task import dense_sampled_ranks
    task, test = _inductive(toy_eval=True)
    dev = _dev()

    def run(**kwargs):
        generator = torch.Generator(device=dev).manual_seed(77)
        return engine.evaluate(task, test, batch_size=8, generator=generator, **kwargs)

    metric, ranking = run(graphed=False, unique_queries=False)
    assert ranking.dtype == torch.float32 and ranking.shape == (len(test), 2)
    for kwargs in (dict(graphed=True, unique_queries=False), dict(graphed=False, unique_queries=True)):
        other, other_ranking = run(**kwargs)
        assert torch.equal(other_ranking, ranking), kwargs
        assert all(torch.equal(other[k], metric[k]) for k in metric), kwargs
    other, other_ranking = engine.evaluate(task, test, batch_size=5, graphed=False, unique_queries=False,
                                           generator=torch.Generator(device=dev).manual_seed(77))
    assert torch.equal(other_ranking, ranking)                               # every triple has its own row of uniform numbers
    # ... and it is the definition: the dense-mask path on the same scores and the same uniform numbers
    rand = torch.rand(len(test), 2, S, generator=torch.Generator(device=dev).manual_seed(77), device=dev)
    with torch.no_grad():
        pred = torch.cat([task.predict(test[i:i + 8].to(dev)) for i in range(0, len(test), 8)])
        mask, target = task.target(test.to(dev))
    rows = 2 * len(test)
    opt, pess, _ = dense_sampled_ranks(pred.cpu().reshape(rows, 500), target.cpu().reshape(rows), mask.cpu().reshape(rows, 500),
                                       rand.cpu().reshape(rows, S))
    assert torch.equal(ranking.cpu(), (0.5 * (opt + pess) + 1).view(-1, 2))
    assert float(metric["hits@10_50"]) == pytest.approx(
        np.mean([binomial_fp64(float(r), 51, 10, 50) for r in ranking.reshape(-1).cpu()]), abs=1e-5)
    assert float(metric["mrr"]) == pytest.approx(float((1 / ranking).mean()), abs=1e-6)
    assert 1 <= float(ranking.min()) and float(ranking.max()) <= S + 1
    # GraphedPredict.statistics: a replayed batch, then the count and sampling kernels eagerly on the static scores
    batches = [test[i:i + 8].to(dev) for i in (0, 8, 16)]
    replay = GraphedPredict(task, batches[0], with_ranks=True)
    for i, batch in enumerate(batches[1:] + [batches[0][:5]], start=1):
        batch_rand = rand[8 * i: 8 * i + len(batch)] if len(batch) == 8 else rand[:5]
        got = replay.statistics(batch, batch_rand)
        want = task.rank_statistics(batch, rand=batch_rand)
        assert got.shape == (len(batch), 2, 4) and torch.equal(got, want), i
        assert got[..., 2:].any()

"""Hop distances without a GPU: the CPU key of ``torch.ops.ultra_mi.hop_distance`` (through ``functional.hop_distance`` and
``Graph.hop_distance``) against the two definitions of tests/hop_definition.py, and the layers above it -- ``task.hop_distance``,
``engine.evaluate_by_distance``, ``answer(with_hops=True)`` -- on the small task of the CPU answer tests.  Integers: every
comparison is exact."""
import numpy as np
import pytest
import torch

from hop_definition import (graph_of, iteration_form, path_graph, queue_form, random_edges, small_graphs, star_with_rows)
from sampled_graphs import small_task, wide_batch, wide_graph


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def _operator(graph, sources, num_iters=100, targets=None):
    """The operator through both of its Python entries (they must agree): Graph.hop_distance and functional on the raw triple."""
    from ultra_torchdrug_amd import functional as UF
    sources = torch.as_tensor(np.asarray(sources), dtype=torch.long)
    got = graph.hop_distance(sources, num_iters, targets)
    row_ptr, src, _, w = graph.relcsr.csr_arrays
    again = UF.hop_distance((row_ptr, src, w), sources, num_iters, targets)
    assert got.dtype == torch.int32 and torch.equal(got, again)
    return got


@pytest.mark.parametrize("name", sorted(small_graphs()))
def test_operator_equals_both_definitions_on_the_constructed_graphs(name):
    n, node_in, node_out, sources = small_graphs()[name]
    for num_iters in (100, 2, 0):
        want = iteration_form(n, node_in, node_out, sources, num_iters)
        assert np.array_equal(want.numpy(), queue_form(n, node_in, node_out, sources, num_iters)), (name, num_iters)
        got = _operator(graph_of(n, node_in, node_out), sources, num_iters)
        assert got.shape == (n, len(sources)) and torch.equal(got, want), (name, num_iters)
    if name == "directed_5_cycle":                       # direction matters: d(0, 4) = 4, d(4, 0) = 1
        full = _operator(graph_of(n, node_in, node_out), sources)
        assert int(full[4, 0]) == 4 and int(full[0, 1]) == 1
    if name == "isolated_source":                        # column 0: node 5 reaches only itself
        full = _operator(graph_of(n, node_in, node_out), sources)
        assert full[:, 0].tolist() == [n] * 5 + [0]


def test_path_graph_holds_the_cap_and_the_sentinel():
    n, node_in, node_out = path_graph(130)
    graph = graph_of(n, node_in, node_out)
    got = _operator(graph, [0])
    assert got[:, 0].tolist() == list(range(101)) + [130] * 29          # the node 101 hops out holds N
    assert torch.equal(got, iteration_form(n, node_in, node_out, [0]))
    assert _operator(graph, [0], 0)[:, 0].tolist() == [0] + [130] * 129
    assert _operator(graph, [0], 1)[:, 0].tolist() == [0, 1] + [130] * 128
    assert _operator(graph, [3, 129], 1).t().tolist() == [[130] * 3 + [0, 1] + [130] * 125, [130] * 129 + [0]]


@pytest.mark.parametrize("group", [16, 32, 64])
def test_hub_row_and_rows_around_the_group_size(group):
    n, node_in, node_out = star_with_rows(group)
    graph = graph_of(n, node_in, node_out)
    deg = np.bincount(node_out, minlength=n)
    assert deg[0] == 5000 and deg[1:6].tolist() == [0, 1, group - 1, group, group + 1]
    sources = [0, 6, 7, int(node_in[5000]), n - 1, 6]                 # the centre, leaves, the feeder of row 2, a filler row
    got = _operator(graph, sources)
    assert np.array_equal(got.numpy(), queue_form(n, node_in, node_out, sources))
    assert torch.equal(_operator(graph, sources, 3), iteration_form(n, node_in, node_out, sources, 3))


@pytest.fixture(scope="module")
def word_cases():
    """N = 1000 and N = 1031 (no multiple of 64), 129 sources with a repeated one: the queue BFS once per graph."""
    cases = {}
    for n in (1000, 1031):
        node_in, node_out = random_edges(n, 3 * n, seed=n)
        rng = np.random.default_rng(n + 1)
        sources = rng.integers(0, n, 129)
        sources[1] = sources[0]
        sources[128] = sources[64]
        cases[n] = (node_in, node_out, sources, queue_form(n, node_in, node_out, sources), graph_of(n, node_in, node_out))
    return cases


@pytest.mark.parametrize("n", [1000, 1031])
@pytest.mark.parametrize("n_source", [1, 63, 64, 65, 129])
def test_source_counts_around_the_word_size(word_cases, n, n_source):
    node_in, node_out, sources, want, graph = word_cases[n]
    got = _operator(graph, sources[:n_source])
    assert got.shape == (n, n_source) and np.array_equal(got.numpy(), want[:, :n_source])
    if n_source > 1:
        assert torch.equal(got[:, 0], got[:, 1])                     # a repeated source: equal columns
    assert int(want.max()) == n and 2 < int(want[want < n].max()) < 100      # the graph has unreachable pairs and real depth


def test_zero_weight_edges_do_not_exist(word_cases):
    from ultra_torchdrug_amd import functional as UF
    n = 1031
    node_in, node_out, sources, want_all, graph = word_cases[n]
    sources = sources[:70]
    rng = np.random.default_rng(5)
    weight = rng.choice(np.array([0.0, 0.5, 1.0], dtype=np.float32), size=len(node_in), p=[0.4, 0.3, 0.3])
    keep = weight != 0
    want = queue_form(n, node_in[keep], node_out[keep], sources)
    assert not np.array_equal(want, want_all[:, :70])                 # the removal changes distances
    weighted = graph_of(n, node_in, node_out, weight)
    assert weighted.relcsr.csr_arrays[3] is not None
    assert np.array_equal(_operator(weighted, sources).numpy(), want)
    # Graph.reweighted: the plans of the unit-weight graph, other weights
    assert np.array_equal(_operator(graph.reweighted(_t(weight)), sources).numpy(), want)
    # w = None against an all-ones w, and a weight that is merely not 1 changes nothing
    row_ptr, src, _, _ = graph.relcsr.csr_arrays
    unit = UF.hop_distance((row_ptr, src, None), _t(sources))
    assert np.array_equal(unit.numpy(), want_all[:, :70])
    assert torch.equal(UF.hop_distance((row_ptr, src, torch.ones(src.numel())), _t(sources)), unit)
    assert torch.equal(UF.hop_distance((row_ptr, src, torch.full((src.numel(),), -2.5)), _t(sources)), unit)


@pytest.mark.parametrize("per_source", [1, 7])
def test_targets_form_equals_a_gather_from_the_matrix(word_cases, per_source):
    n = 1000
    node_in, node_out, sources, want, graph = word_cases[n]
    rng = np.random.default_rng(per_source)
    targets = rng.integers(0, n, (129, per_source))
    targets[:, 0] = sources                                           # target == source
    unreachable = np.argwhere(want == n)
    assert len(unreachable)
    v, b = unreachable[0]
    targets[b, per_source - 1] = v                                    # an unreachable target
    for num_iters in (100, 3):
        matrix = _operator(graph, sources, num_iters)
        got = _operator(graph, sources, num_iters, _t(targets))
        assert got.shape == (129, per_source) and got.dtype == torch.int32
        assert torch.equal(got, matrix.t().gather(1, _t(targets)))
    full = _operator(graph, sources, 100, _t(targets))
    assert int(full[b, per_source - 1]) == n
    others = np.arange(129) != b
    assert (full[_t(others), 0] == 0).all()                           # target == source


def test_bad_arguments_raise():
    from ultra_torchdrug_amd import functional as UF
    n, node_in, node_out, _ = small_graphs()["two_components"]
    row_ptr, src, _, w = graph_of(n, node_in, node_out).relcsr.csr_arrays
    sources = torch.tensor([0, 5])
    UF.hop_distance((row_ptr, src, w), sources)
    with pytest.raises(ValueError):
        UF.hop_distance((row_ptr, src, w), sources, num_iters=-1)
    for bad in (torch.tensor([0, n]), torch.tensor([-1, 0])):
        with pytest.raises(RuntimeError):
            UF.hop_distance((row_ptr, src, w), bad)
        with pytest.raises(RuntimeError):
            UF.hop_distance((row_ptr, src, w), sources, targets=bad[:, None])
    with pytest.raises(RuntimeError):
        UF.hop_distance((row_ptr.long(), src.long(), w), sources)                    # an int64 CSR
    with pytest.raises(RuntimeError):
        UF.hop_distance((row_ptr, src, w), sources.int())
    with pytest.raises(RuntimeError):
        UF.hop_distance((row_ptr, src, w), sources, targets=torch.zeros(3, 2, dtype=torch.long))
    with pytest.raises(RuntimeError):
        UF.hop_distance((row_ptr, src, w), sources.to("meta"))                       # mixed devices
    with pytest.raises(RuntimeError):
        UF.hop_distance((row_ptr.flip(0), src, w), sources)                          # a malformed CSR
    with pytest.raises(TypeError):
        UF.hop_distance(row_ptr, sources)


def test_binding_lists_the_entries_and_keeps_the_abi():
    from ultra_torchdrug_amd import _lib, _torch_ext
    assert {"ultra_hop_distance", "ultra_hop_distance_workspace"} <= set(_lib.EXPORTS) and _lib.ABI_VERSION == 8
    assert "hop_distance" in _torch_ext.OPS
    lib = _lib.load()
    assert lib.ultra_hop_distance_workspace(1000) == 3 * 8 * 1000 + 16 and lib.ultra_hop_distance_workspace(0) == 0


def test_models_return_the_reference_layout():
    from ultra_torchdrug_amd.model import TransferNBFNet
    from ultra_torchdrug_amd.rel_model import RelNBFNet
    n, node_in, node_out, sources = small_graphs()["two_components"]
    graph = graph_of(n, node_in, node_out)
    got = TransferNBFNet._get_shortest_distance(None, graph, torch.tensor(sources))
    assert got.dtype == torch.int32 and torch.equal(got, iteration_form(n, node_in, node_out, sources))
    every = RelNBFNet._get_shortest_distance(None, graph, num_iters=2)
    assert every.shape == (n, n) and torch.equal(every, iteration_form(n, node_in, node_out, list(range(n)), 2))


# ------------------------------------------------------------------------------------------------ task and engine
@pytest.fixture(scope="module")
def small():
    graph = wide_graph()
    task = small_task(graph)
    g = torch.Generator().manual_seed(11)
    triples = torch.cat([wide_batch(graph), graph.edge_list[torch.randint(0, 9000, (20,), generator=g)],
                         torch.stack([torch.randint(0, 300, (40,), generator=g), torch.randint(0, 300, (40,), generator=g),
                                      torch.randint(0, 5, (40,), generator=g)], dim=1),
                         torch.tensor([[17, 17, 2], [11, 11, 1]])])
    e = graph.edge_list.numpy()
    und = (np.concatenate([e[:, 0], e[:, 1]]), np.concatenate([e[:, 1], e[:, 0]]))       # the graph with inverse edges
    return {"graph": graph, "task": task, "triples": triples, "und": und}


def _pair_distances(und, heads, tails, num_iters):
    heads = np.asarray(heads)
    distinct, inverse = np.unique(heads, return_inverse=True)
    table = queue_form(300, und[0], und[1], distinct, num_iters)
    return table[np.asarray(tails), inverse]


def test_task_hop_distance_equals_the_definition(small):
    task, triples = small["task"], small["triples"]
    for num_iters in (100, 2, 1):
        got = task.hop_distance(triples, num_iters=num_iters)
        assert got.dtype == torch.int32 and got.shape == (len(triples),)
        assert np.array_equal(got.numpy(), _pair_distances(small["und"], triples[:, 0], triples[:, 1], num_iters))
    # head to tail == tail to head in the graph with inverse edges
    assert torch.equal(task.hop_distance(triples), task.hop_distance(triples[:, [1, 0, 2]]))
    assert task.hop_distance(triples[:0]).shape == (0,)
    assert task.message_graph() is task.model._undirected(task.fact_graph)


@pytest.mark.parametrize("max_hops", [None, 1])
def test_evaluate_by_distance_partitions_the_triples(small, max_hops):
    from ultra_torchdrug_amd import engine
    task, triples = small["task"], small["triples"]
    metrics, ranking = engine.evaluate(task, triples, batch_size=8)
    by_distance, distance, again = engine.evaluate_by_distance(task, triples, max_hops=max_hops, batch_size=8)
    hops = 2 if max_hops is None else max_hops                        # the small task has two layers
    assert torch.equal(again, ranking)
    assert torch.equal(distance, task.hop_distance(triples, num_iters=hops))
    assert set(by_distance) <= set(range(hops + 1)) | {"beyond"} and 0 in by_distance and 1 in by_distance
    assert ("beyond" in by_distance) == (max_hops == 1)               # 300 nodes, 9000 triples: everything within two hops
    assert sum(bucket["count"] for bucket in by_distance.values()) == len(triples)
    for name, bucket in by_distance.items():
        mask = (distance > hops) if name == "beyond" else (distance == name)
        assert bucket["count"] == int(mask.sum()) > 0
        want = task.evaluate(ranking[mask])
        assert set(bucket) == set(want) | {"count"}
        for key, value in want.items():
            assert torch.equal(bucket[key], value), (name, key)
    whole = task.evaluate(ranking)
    assert all(torch.equal(whole[k], metrics[k]) for k in metrics)


@pytest.mark.parametrize("head", [False, True])
def test_answers_with_hops(small, head):
    from ultra_torchdrug_amd import engine
    task = small["task"]
    g = torch.Generator().manual_seed(3)
    anchor, relation = torch.randint(0, 300, (21,), generator=g), torch.randint(0, 5, (21,), generator=g)
    plain = task.answer(anchor, relation, k=128, head=head)
    entities, scores, hops = task.answer(anchor, relation, k=128, head=head, with_hops=True)
    assert len(plain) == 2 and torch.equal(plain[0], entities) and torch.equal(plain[1], scores)       # unchanged without
    assert hops.dtype == torch.int32 and hops.shape == (21, 128)
    table = queue_form(300, small["und"][0], small["und"][1], anchor.numpy(), 2)       # two layers
    want = np.where(entities.numpy() < 0, -1, table[entities.clamp(min=0).numpy(), np.arange(21)[:, None]])
    assert np.array_equal(hops.numpy(), want)
    e_plain = engine.answer(task, anchor, relation, k=10, head=head, batch_size=8)
    e_ent, e_score, e_hops = engine.answer(task, anchor, relation, k=10, head=head, batch_size=8, with_hops=True)
    assert len(e_plain) == 2 and torch.equal(e_plain[0], e_ent) and torch.equal(e_plain[1], e_score)
    assert np.array_equal(e_hops.numpy(), table[e_ent.numpy(), np.arange(21)[:, None]])
    # a query whose every entity is a known completion lists nothing: -1 slots
    full = small_task(wide_graph(full_row=True))
    ent, _, hop = full.answer(torch.tensor([7]), torch.tensor([2]), k=5, with_hops=True)
    assert (ent == -1).all() and (hop == -1).all()


def test_evaluate_by_distance_passes_relations_and_candidate_counts():
    """A task with a sampled metric and per-relation metrics: every bucket gets the ``rel=`` / ``num_candidates=`` rows that
    ``engine.evaluate`` itself would pass."""
    from sampled_graphs import ring_graph
    from ultra_torchdrug_amd import engine
    graph = ring_graph()
    task = small_task(graph, metric=("mrr", "hits@10_50"), metric_per_rel=True)
    triples = graph.edge_list[::97][:30]
    _, ranking = engine.evaluate(task, triples, batch_size=8)
    statistics = torch.cat([task.rank_statistics(triples[i:i + 8]) for i in range(0, len(triples), 8)])
    for max_hops in (None, 0):
        by_distance, distance, again = engine.evaluate_by_distance(task, triples, max_hops=max_hops, batch_size=8)
        hops = 2 if max_hops is None else 0
        assert torch.equal(again, ranking) and sum(b["count"] for b in by_distance.values()) == len(triples)
        assert ("beyond" in by_distance) == (max_hops == 0)
        for name, bucket in by_distance.items():
            mask = (distance > hops) if name == "beyond" else (distance == name)
            want = task.evaluate(ranking[mask], rel=triples[mask][:, 2], num_candidates=statistics[mask][..., 1])
            assert set(want) | {"count"} == set(bucket) and all(torch.equal(bucket[k], want[k]) for k in want), name

"""Host side of the exact answer sets: the dense torch twins of ``ultra_sets_project`` /
``ultra_sets_rank`` against the numpy definitions of tests/query_exact_definition.py, the packed-set plumbing, ``task.query_answers``
and ``engine.evaluate_queries`` on CPU tensors, ``data.sample_queries``, and the binding table."""
import numpy as np
import pytest
import torch

from query_definition import SHAPES
from query_exact_definition import (NEGATION_FREE, adjacency, as_bits, hand_exact, hard_targets, held_out_task, metrics_numpy,
                                    pack_numpy, project_numpy, projection_graph, ranks_double_loop, ranks_numpy, sampled_ids,
                                    with_inverses)


def _graph(n_node, n_rel, node_in, node_out, rel, weight):
    from ultra_torchdrug_amd.graph import Graph
    edges = torch.from_numpy(np.stack([node_in, node_out, rel], axis=1).astype(np.int64).reshape(-1, 3))
    return Graph(edges, None if weight is None else torch.from_numpy(np.asarray(weight, dtype=np.float32)), n_node, n_rel)


@pytest.fixture(scope="module")
def task():
    return held_out_task()


@pytest.mark.parametrize("n_query", [1, 63, 64, 65, 130])
def test_packing_round_trips(n_query):
    from ultra_torchdrug_amd import functional as UF
    g = torch.Generator().manual_seed(n_query)
    for n_node in (1, 63, 65):
        member = torch.rand(n_query, n_node, generator=g) < 0.3
        bits = UF.pack_sets(member)
        assert bits.dtype == torch.int64 and bits.shape == (n_node, (n_query + 63) // 64)
        assert np.array_equal(bits.numpy().view(np.uint64), pack_numpy(member.numpy()))
        assert torch.equal(UF.unpack_sets(bits, n_query), member)
        assert not (bits & ~UF.column_mask(n_query)).any()
        nodes = torch.randint(0, n_node, (n_query,), generator=g)
        nodes[n_query // 2:] = nodes[0]                                          # repeated anchors, also inside one word
        seeded = UF.seed_sets(nodes, n_node)
        want = torch.zeros(n_query, n_node, dtype=torch.bool)
        want[torch.arange(n_query), nodes] = True
        assert torch.equal(seeded, UF.pack_sets(want)) and torch.equal(UF.unpack_sets(seeded, n_query), want)
    with pytest.raises(RuntimeError):
        UF.seed_sets(torch.tensor([3]), 3)


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("group", [16, 32, 64])
def test_dense_projection_equals_the_numpy_definition(group, weighted):
    from ultra_torchdrug_amd import functional as UF
    n_node, n_rel, node_in, node_out, rel, weight = projection_graph(group, weighted)
    graph = _graph(n_node, n_rel, node_in, node_out, rel, weight)
    assert (graph.relcsr.csr_arrays[3] is not None) == weighted
    adj = adjacency(n_node, n_rel, node_in, node_out, rel, weight)
    rng = np.random.default_rng(group)
    for n_query in (1, 65, 130):
        member = rng.random((n_query, n_node)) < 0.05
        relation = rng.integers(0, n_rel, n_query)
        relation[:3] = (0, n_rel - 1, 3)[:n_query]                              # the ends, and the relation no edge carries
        want = project_numpy(adj, member, relation)
        got = UF.project_sets_exact(graph.relcsr, as_bits(member, "cpu"), torch.from_numpy(relation))
        assert np.array_equal(got.numpy().view(np.uint64), pack_numpy(want)), (group, weighted, n_query)
        assert want.any() and (n_query < 3 or not want[2].any())
    with pytest.raises(RuntimeError):
        UF.project_sets_exact(graph.relcsr, as_bits(member, "cpu"), torch.from_numpy(relation) + n_rel)
    with pytest.raises(TypeError):
        UF.project_sets_exact(graph.relcsr.csr_arrays, as_bits(member, "cpu"), torch.from_numpy(relation))


def test_dense_ranks_equal_the_double_loop():
    from ultra_torchdrug_amd import functional as UF
    g = torch.Generator().manual_seed(4)
    n_query, n_node = 5, 70
    pred = torch.randint(0, 6, (n_query, n_node), generator=g).float() * 0.5
    pred[0, 3], pred[1, 5], pred[2, 7], pred[3, 9] = float("nan"), float("inf"), float("-inf"), -0.0
    excluded = torch.rand(n_query, n_node, generator=g) < 0.3
    counts = [0, 1, 7, 70, 3]
    entity = torch.cat([torch.randperm(n_node, generator=g)[:c] for c in counts])
    pred[3, 11] = float("nan")                                                  # query 3 ranks every entity: a NaN target too
    ptr = torch.tensor(np.concatenate([[0], np.cumsum(counts)]))
    want = ranks_double_loop(pred.numpy(), excluded.numpy(), ptr.numpy(), entity.numpy())
    assert np.array_equal(want, ranks_numpy(pred.numpy(), excluded.numpy(), ptr.numpy(), entity.numpy()))
    got = UF.set_ranks(pred, UF.pack_sets(excluded), ptr, entity)
    assert got.dtype == torch.int64 and np.array_equal(got.numpy(), want)
    free = UF.set_ranks(pred, None, ptr, entity)
    assert np.array_equal(free.numpy(), ranks_double_loop(pred.numpy(), np.zeros_like(excluded.numpy()), ptr.numpy(), entity.numpy()))
    for bad in (dict(ptr=ptr[:-1]), dict(ptr=ptr.flip(0)), dict(entity=entity + n_node), dict(pred=pred.double())):
        with pytest.raises(RuntimeError):
            UF.set_ranks(bad.get("pred", pred), UF.pack_sets(excluded), bad.get("ptr", ptr), bad.get("entity", entity))


@pytest.mark.parametrize("name", list(SHAPES))
def test_query_answers_equal_the_hand_executor(task, name):
    anchors, relations, _ = sampled_ids(task, name, 70)
    for which, graph in (("fact", task.fact_graph), ("filter", task.graph)):
        want = hand_exact(with_inverses(graph), name, anchors.numpy(), relations.numpy())
        got = task.query_answers(name, anchors, relations, graph=which)
        assert got.dtype == torch.bool and got.shape == (70, 60)
        assert np.array_equal(got.numpy(), want), (name, which)
        assert want.any()
    with pytest.raises(ValueError):
        task.query_answers(name, anchors, relations, graph="test")
    with pytest.raises(ValueError):
        task.query_answers(name, anchors, relations + 8)
    assert task.query_answers(name, anchors[:0], relations[:0]).shape == (0, 60)


@pytest.mark.parametrize("name", list(SHAPES))
def test_sample_queries(task, name):
    from ultra_torchdrug_amd import data
    anchors, relations, targets = sampled_ids(task, name)
    assert anchors.shape == (64, SHAPES[name][0]) and relations.shape == (64, SHAPES[name][1]) and targets.shape == (64,)
    assert anchors.dtype == relations.dtype == targets.dtype == torch.int64
    assert 0 <= int(anchors.min()) and int(anchors.max()) < 60 and 0 <= int(relations.min()) and int(relations.max()) < 8
    again = sampled_ids(task, name)
    assert all(torch.equal(a, b) for a, b in zip((anchors, relations, targets), again))
    other = sampled_ids(task, name, seed=4)
    assert not all(torch.equal(a, b) for a, b in zip((anchors, relations, targets), other))
    if name in NEGATION_FREE:
        answers = hand_exact(with_inverses(task.graph), name, anchors.numpy(), relations.numpy())
        assert answers[np.arange(64), targets.numpy()].all(), name
    from ultra_torchdrug_amd.graph import Graph
    with pytest.raises(RuntimeError):
        data.sample_queries(Graph(num_node=5, num_relation=2), name, 1, torch.Generator().manual_seed(0))
    empty = data.sample_queries(task.message_graph(), name, 0, torch.Generator().manual_seed(0))
    assert empty[0].shape == (0, SHAPES[name][0]) and empty[1].shape == (0, SHAPES[name][1])


@pytest.mark.parametrize("name", list(SHAPES))
def test_evaluate_queries_on_the_host(task, name):
    from ultra_torchdrug_amd import engine
    from ultra_torchdrug_amd.task import parse_query_structure
    anchors, relations, _ = sampled_ids(task, name)
    easy = hand_exact(with_inverses(task.fact_graph), name, anchors.numpy(), relations.numpy())
    full = hand_exact(with_inverses(task.graph), name, anchors.numpy(), relations.numpy())
    hard, excluded, ptr, query, entity = hard_targets(easy, full)
    assert (hard.any(axis=1)).sum() >= 8, name
    tree = parse_query_structure(name)[0]
    with torch.no_grad():
        scores = torch.cat([task.query_memberships(tree, anchors[i:i + 16], relations[i:i + 16]).float() for i in range(0, 64, 16)])
    want_rank = ranks_numpy(scores.numpy(), excluded, ptr, entity)
    want = metrics_numpy(query, want_rank, 64)
    got, (got_query, got_entity, got_rank) = engine.evaluate_queries(task, name, anchors, relations, return_ranks=True)
    assert np.array_equal(got_query.numpy(), query) and np.array_equal(got_entity.numpy(), entity)
    assert got_rank.dtype == torch.int64 and np.array_equal(got_rank.numpy(), want_rank)
    assert set(got) == set(want)
    for key, value in want.items():
        assert abs(got[key] - value) <= 1e-12, (name, key, got[key], value)
    assert engine.evaluate_queries(task, name, anchors, relations) == got


def test_evaluate_queries_without_hard_answers(task):
    from ultra_torchdrug_amd import engine
    got = engine.evaluate_queries(task, "2p", torch.zeros(0, 1, dtype=torch.int64), torch.zeros(0, 2, dtype=torch.int64))
    assert got["num_queries"] == got["num_evaluated"] == got["num_hard_answers"] == 0 and np.isnan(got["mrr"])


def test_filtered_answers_on_the_host(task):
    from topk_definition import topk_rows
    from ultra_torchdrug_amd import engine
    from ultra_torchdrug_amd.task import parse_query_structure
    anchors, relations, _ = sampled_ids(task, "2p", 10)
    known = task.query_answers("2p", anchors, relations, graph="filter")
    plain = task.answer_query("2p", anchors, relations, k=10)
    assert all(torch.equal(a, b) for a, b in zip(plain, task.answer_query("2p", anchors, relations, k=10, filtered=False)))
    entities, membership = task.answer_query("2p", anchors, relations, k=10, filtered=True)
    listed = entities >= 0
    assert listed.any() and not known[torch.arange(10)[:, None].expand_as(entities)[listed], entities[listed]].any()
    with torch.no_grad():
        p = task.query_memberships(parse_query_structure("2p")[0], anchors, relations).float()
    index, value = topk_rows(torch.where(known, torch.zeros_like(p), p).numpy(), 10, None)
    assert np.array_equal(entities.numpy(), np.where(value > 0, index, -1))
    assert np.array_equal(membership.numpy(), np.where(value > 0, value, np.float32(0)))
    batched = engine.answer_query(task, "2p", anchors, relations, k=10, batch_size=4, filtered=True)
    assert torch.equal(batched[0], entities) and torch.equal(batched[1], membership)


def test_the_binding_lists_the_new_entries():
    from ultra_torchdrug_amd import _lib
    for name in ("ultra_sets_project_workspace", "ultra_sets_project", "ultra_sets_rank"):
        assert name in _lib.SIGNATURES and name in _lib.EXPORTS
    assert len(_lib.SIGNATURES["ultra_sets_project"][1]) == 14 and len(_lib.SIGNATURES["ultra_sets_rank"][1]) == 10

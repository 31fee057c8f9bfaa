"""MI355X: exact answer sets of logical queries -- ``ultra_sets_project`` and ``ultra_sets_rank`` against
the numpy definitions of tests/query_exact_definition.py, exactly, at the word, tile and block edges of the kernels; between
poisoned, guard-banded allocations; their status codes; the projection replayed from a hipGraph; ``task.query_answers`` for the 14
structures against the hand-written executor and the CPU twin; ``engine.evaluate_queries`` and the filtered ``answer_query``."""
import numpy as np
import pytest
import torch

from guarded_memory import guarded
from query_definition import SHAPES
from query_exact_definition import (RANK_TARGETS, RANK_TILE, SEGMENT, adjacency, as_bits, hand_exact, hard_targets, held_out_task, long_row_graph,
                                    metrics_numpy, pack_numpy, project_edges_numpy, project_numpy, projection_graph, ranks_double_loop, ranks_numpy,
                                    sampled_ids, with_inverses)
from topk_definition import topk_rows

pytestmark = pytest.mark.gpu


def _dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _graph(n_node, n_rel, node_in, node_out, rel, weight):
    from ultra_torchdrug_amd.graph import Graph
    edges = torch.from_numpy(np.stack([node_in, node_out, rel], axis=1).astype(np.int64).reshape(-1, 3))
    return Graph(edges, None if weight is None else torch.from_numpy(np.asarray(weight, dtype=np.float32)), n_node, n_rel)


def _words(bits):
    return bits.cpu().numpy().view(np.uint64)


def _dirty(bits, n_query):
    """``bits`` with every bit of the columns ``>= n_query`` set: they must not reach an output."""
    from ultra_torchdrug_amd import functional as UF
    out = bits.clone()
    out[:, -1] |= ~UF.column_mask(n_query, bits.device)[-1]
    return out


# ------------------------------------------------------------------------------------------------ plumbing
@pytest.mark.parametrize("n_query", [1, 63, 64, 65, 130])
def test_packing_round_trips_on_the_device(n_query):
    from ultra_torchdrug_amd import functional as UF
    dev = _dev()
    g = torch.Generator().manual_seed(n_query)
    for n_node in (1, 63, 65, 1000):
        member = torch.rand(n_query, n_node, generator=g) < 0.3
        bits = UF.pack_sets(member.to(dev))
        assert bits.dtype == torch.int64 and bits.is_cuda and np.array_equal(_words(bits), pack_numpy(member.numpy()))
        assert torch.equal(UF.unpack_sets(bits, n_query).cpu(), member)
        nodes = torch.randint(0, n_node, (n_query,), generator=g)
        nodes[n_query // 2:] = nodes[0]                                          # repeated anchors, also inside one word
        want = np.zeros((n_query, n_node), dtype=bool)
        want[np.arange(n_query), nodes.numpy()] = True
        assert np.array_equal(_words(UF.seed_sets(nodes.to(dev), n_node)), pack_numpy(want))


# ------------------------------------------------------------------------------------------------ ultra_sets_project
@pytest.mark.parametrize("n_node", [1, 63, 65, 1000])
def test_projection_at_the_word_edges(n_node):
    """Q = 1, 63, 64, 65, 130 -- one word short, full, and one more; three words -- and 300 (five words: a second word tile)
    on random graphs of 6 relations; relations repeat across the queries; the unused bits of the input's last word are all set."""
    from ultra_torchdrug_amd import functional as UF
    dev = _dev()
    rng = np.random.default_rng(n_node)
    n_rel, n_edge = 6, 5 * n_node
    node_in, node_out, rel = rng.integers(0, n_node, n_edge), rng.integers(0, n_node, n_edge), rng.integers(0, n_rel, n_edge)
    graph = _graph(n_node, n_rel, node_in, node_out, rel, None).to(dev)
    adj = adjacency(n_node, n_rel, node_in, node_out, rel)
    for n_query in (1, 63, 64, 65, 130, 300):
        member = rng.random((n_query, n_node)) < max(0.05, 1.0 / n_node)
        relation = rng.integers(0, n_rel, n_query)
        want = project_numpy(adj, member, relation)
        bits = as_bits(member, dev)
        got = UF.project_sets_exact(graph.relcsr, _dirty(bits, n_query), torch.from_numpy(relation).to(dev))
        assert got.dtype == torch.int64 and got.shape == bits.shape
        assert np.array_equal(_words(got), pack_numpy(want)), (n_node, n_query)
        twin = UF.project_sets_exact(graph.cpu().relcsr, bits.cpu(), torch.from_numpy(relation))
        assert torch.equal(got.cpu(), twin)
    assert n_node == 1 or want.any()


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("group", [16, 32, 64])
def test_projection_on_every_lane_group_width(group, weighted):
    """Graphs whose mean in-degree selects 16, 32 and 64 lanes a row: a row longer than four rounds of the group, empty rows, a
    self-loop, zero-weight edges (weighted plan), a relation no edge carries, relation ids 0 and 2R - 1."""
    from ultra_torchdrug_amd import functional as UF
    dev = _dev()
    n_node, n_rel, node_in, node_out, rel, weight = projection_graph(group, weighted)
    graph = _graph(n_node, n_rel, node_in, node_out, rel, weight).to(dev)
    row_ptr, _, _, w = graph.relcsr.csr_arrays
    assert (w is not None) == weighted and int(row_ptr[1]) > 4 * group and int(row_ptr[4]) == int(row_ptr[1])
    mean = int(row_ptr[-1]) // n_node
    assert {16: mean < 24, 32: 24 <= mean < 48, 64: mean >= 48}[group]
    adj = adjacency(n_node, n_rel, node_in, node_out, rel, weight)
    rng = np.random.default_rng(group)
    for n_query in (3, 64, 130):
        member = rng.random((n_query, n_node)) < 0.02
        member[0, 4] = True                                                      # the self-loop's source
        relation = rng.integers(0, n_rel, n_query)
        relation[:3] = (n_rel - 1, 0, 3)                                         # the ends, and the relation no edge carries
        want = project_numpy(adj, member, relation)
        got = UF.project_sets_exact(graph.relcsr, _dirty(as_bits(member, dev), n_query), torch.from_numpy(relation).to(dev))
        assert np.array_equal(_words(got), pack_numpy(want)), (group, weighted, n_query)
        assert want[0, 4] and want[1].any() and not want[2].any() and not want[:, 1:4].any()
    if weighted:                                                                 # the dropped edges matter
        assert not np.array_equal(want, project_numpy(adjacency(n_node, n_rel, node_in, node_out, rel), member, relation))


def test_projection_strides_over_the_rows():
    """40 000 rows at 16 lanes a row are 2 500 blocks' worth: more than the grid's 2 048, so blocks take a second round, and the
    last round is ragged.  Held to the edge-list form of the definition, which the small graph below holds to the adjacency."""
    from ultra_torchdrug_amd import functional as UF
    dev = _dev()
    rng = np.random.default_rng(40)
    small = (50, rng.integers(0, 50, 200), rng.integers(0, 50, 200), rng.integers(0, 6, 200))
    member, relation = rng.random((9, 50)) < 0.2, rng.integers(0, 6, 9)
    assert np.array_equal(project_edges_numpy(*small, member, relation), project_numpy(adjacency(50, 6, *small[1:]), member, relation))
    n_node, n_rel, n_query = 40_000, 6, 65
    node_in, node_out, rel = rng.integers(0, n_node, 3 * n_node), rng.integers(0, n_node, 3 * n_node), rng.integers(0, n_rel, 3 * n_node)
    graph = _graph(n_node, n_rel, node_in, node_out, rel, None).to(dev)
    member, relation = rng.random((n_query, n_node)) < 0.01, rng.integers(0, n_rel, n_query)
    want = project_edges_numpy(n_node, node_in, node_out, rel, member, relation)
    got = UF.project_sets_exact(graph.relcsr, _dirty(as_bits(member, dev), n_query), torch.from_numpy(relation).to(dev))
    assert np.array_equal(_words(got), pack_numpy(want)) and want[:, -100:].any() and want[:, 2048 * 16:].any()


@pytest.mark.parametrize("weighted", [False, True])
def test_projection_of_rows_longer_than_a_group_walks(weighted):
    """Rows of 2 600, ``SEGMENT``, ``SEGMENT + 1`` and ``SEGMENT - 1`` edges: what lies beyond a row's first ``SEGMENT`` edges
    comes from the tail launch.  Queries 0 and 1 are one-hot at the LAST edge of rows 2 and 0 (rows are in source order) under
    that edge's relation, so their bit at that row exists through a tail edge alone; one and five words."""
    from ultra_torchdrug_amd import functional as UF
    dev = _dev()
    n_node, n_rel, node_in, node_out, rel, weight = long_row_graph(weighted)
    graph = _graph(n_node, n_rel, node_in, node_out, rel, weight).to(dev)
    row_ptr, src, rel_d, w = graph.relcsr.csr_arrays
    assert (w is not None) == weighted
    assert row_ptr[:5].tolist() == [0, 2 * n_node, 2 * n_node + SEGMENT, 2 * n_node + 2 * SEGMENT + 1, 2 * n_node + 3 * SEGMENT]
    adj = adjacency(n_node, n_rel, node_in, node_out, rel, weight)
    rng = np.random.default_rng(3)
    for n_query in (5, 300):
        member = rng.random((n_query, n_node)) < 0.002
        relation = rng.integers(0, n_rel, n_query)
        for q, row in ((0, 2), (1, 0)):
            last = int(row_ptr[row + 1]) - 1
            member[q] = False
            member[q, int(src[last])] = True
            relation[q] = int(rel_d[last])
            if weighted and row == 0:
                assert float(w[last]) != 0
        want = project_numpy(adj, member, relation)
        assert want[0, 2] and want[1, 0]
        got = UF.project_sets_exact(graph.relcsr, _dirty(as_bits(member, dev), n_query), torch.from_numpy(relation).to(dev))
        assert np.array_equal(_words(got), pack_numpy(want)), (weighted, n_query)
    with guarded("functional") as guard:
        csr = tuple(None if a is None else guard.banded(a) for a in graph.relcsr.csr_arrays)
        got = UF.project_sets_exact(csr, guard.banded(as_bits(member, dev)), guard.banded(torch.from_numpy(relation).to(dev)),
                                    n_relation=n_rel)
    assert np.array_equal(_words(got), pack_numpy(want))


def test_projection_between_guard_bands():
    """Both tail shapes of the walk (a last word tile of one word, a last block of rows) with every operand between bands and
    the output and the workspace poisoned: the definition exactly, so every output word was written."""
    from ultra_torchdrug_amd import functional as UF
    dev = _dev()
    n_node, n_rel, node_in, node_out, rel, weight = projection_graph(16, True)
    graph = _graph(n_node, n_rel, node_in, node_out, rel, weight).to(dev)
    adj = adjacency(n_node, n_rel, node_in, node_out, rel, weight)
    rng = np.random.default_rng(9)
    for n_query in (65, 300):
        member = rng.random((n_query, n_node)) < 0.02
        relation = rng.integers(0, n_rel, n_query)
        with guarded("functional") as guard:
            csr = tuple(None if a is None else guard.banded(a) for a in graph.relcsr.csr_arrays)
            got = UF.project_sets_exact(csr, guard.banded(_dirty(as_bits(member, dev), n_query)),
                                        guard.banded(torch.from_numpy(relation).to(dev)), n_relation=n_rel)
            guard.check()
            assert len(guard.records) >= 7                                       # six operands, the output, the workspace
        assert np.array_equal(_words(got), pack_numpy(project_numpy(adj, member, relation))), n_query


def test_projection_replays_from_a_hipgraph():
    from ultra_torchdrug_amd import functional as UF
    dev = _dev()
    n_node, n_rel, node_in, node_out, rel, weight = projection_graph(32, True)
    graph = _graph(n_node, n_rel, node_in, node_out, rel, weight).to(dev)
    adj = adjacency(n_node, n_rel, node_in, node_out, rel, weight)
    rng = np.random.default_rng(2)
    n_query = 70
    cases = [(rng.random((n_query, n_node)) < 0.03, rng.integers(0, n_rel, n_query)) for _ in range(3)]
    static_bits, static_rel = as_bits(cases[0][0], dev), torch.from_numpy(cases[0][1]).to(dev)
    graph.relcsr.csr_arrays                                                      # built outside the capture
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        UF.project_sets_exact(graph.relcsr, static_bits, static_rel)             # warm-up: the outputs enter the allocator's cache
    torch.cuda.current_stream().wait_stream(side)
    captured = torch.cuda.CUDAGraph()
    with torch.cuda.graph(captured, stream=side):
        out = UF.project_sets_exact(graph.relcsr, static_bits, static_rel)
    for member, relation in cases:
        static_bits.copy_(as_bits(member, dev))
        static_rel.copy_(torch.from_numpy(relation).to(dev))
        captured.replay()
        torch.cuda.synchronize()
        assert np.array_equal(_words(out), pack_numpy(project_numpy(adj, member, relation)))
        assert torch.equal(UF.project_sets_exact(graph.relcsr, static_bits, static_rel), out)


# ------------------------------------------------------------------------------------------------ ultra_sets_rank
def _rank_case(n_node, counts, seed):
    """Scores on a grid of six values (exact ties) with NaN, both infinities and both zeros planted, a third of the entities
    excluded per query, and ``counts[q]`` targets for query ``q`` (entities may repeat), among them excluded ones and others."""
    g = torch.Generator().manual_seed(seed)
    n_query = len(counts)
    pred = torch.randint(0, 6, (n_query, n_node), generator=g).float() * 0.5 - 1.0
    pred[:, 3::17] = float("nan")
    pred[:, 5::19] = float("inf")
    pred[:, 7::23] = float("-inf")
    pred[:, 2::29] = -0.0
    excluded = torch.rand(n_query, n_node, generator=g) < 0.33
    entity = torch.cat([torch.randint(0, n_node, (c,), generator=g) for c in counts] + [torch.zeros(0, dtype=torch.int64)])
    ptr = torch.from_numpy(np.concatenate([[0], np.cumsum(counts)]).astype(np.int64))
    return pred, excluded, ptr, entity


def _check_ranks(pred, excluded, ptr, entity, definition, stride_pad=0, guard=None):
    from ultra_torchdrug_amd import functional as UF
    dev = _dev()
    n_query, n_node = pred.shape
    wide = torch.full((n_query, n_node + stride_pad), 9.0)
    wide[:, :n_node] = pred
    keep = guard.banded if guard is not None else (lambda t: t)
    pred_d = keep(wide.to(dev))[:, :n_node]
    got = UF.set_ranks(pred_d, keep(UF.pack_sets(excluded.to(dev))), keep(ptr.to(dev)), keep(entity.to(dev)))
    want = definition(pred.numpy(), excluded.numpy(), ptr.numpy(), entity.numpy())
    assert got.dtype == torch.int64 and got.shape == entity.shape
    assert np.array_equal(got.cpu().numpy(), want), (n_node, stride_pad)
    return want


@pytest.mark.parametrize("n_node", [RANK_TILE - 1, RANK_TILE, RANK_TILE + 1])
def test_ranks_equal_the_double_loop(n_node):
    """N one below, at and one above the entity tile; 0, 1 and one below / at / one above a target block of targets per query;
    exact ties, NaN and both infinities among the scores and the thresholds; excluded and free targets; a strided ``pred``."""
    counts = [0, 1, RANK_TARGETS - 1, RANK_TARGETS, RANK_TARGETS + 1, 0, 3]
    pred, excluded, ptr, entity = _rank_case(n_node, counts, seed=n_node)
    at = excluded[4, entity[ptr[4]:ptr[5]]]
    assert at.any() and not at.all()
    assert torch.isnan(pred[4, entity[ptr[4]:ptr[5]]]).any() and torch.isinf(pred[4, entity[ptr[4]:ptr[5]]]).any()
    want = _check_ranks(pred, excluded, ptr, entity, ranks_double_loop)
    assert want.min() == 1 and want.max() > 100
    _check_ranks(pred, excluded, ptr, entity, ranks_numpy, stride_pad=5)


def test_ranks_of_a_query_with_more_target_blocks_than_the_grid_strides():
    """One query with 16 blocks of targets and one more target: the blocks stride over the grid's 16; 65 queries: two words."""
    counts = [2] * 64 + [16 * RANK_TARGETS + 1]
    pred, excluded, ptr, entity = _rank_case(70, counts, seed=1)
    _check_ranks(pred, excluded, ptr, entity, ranks_numpy)
    from ultra_torchdrug_amd import functional as UF
    free = UF.set_ranks(pred.to(_dev()), None, ptr.to(_dev()), entity.to(_dev()))
    assert np.array_equal(free.cpu().numpy(), ranks_numpy(pred.numpy(), np.zeros_like(excluded.numpy()), ptr.numpy(), entity.numpy()))


@pytest.mark.parametrize("n_node", [RANK_TILE - 1, RANK_TILE + 1])
def test_ranks_between_guard_bands(n_node):
    counts = [RANK_TARGETS + 1, 0, 1]
    pred, excluded, ptr, entity = _rank_case(n_node, counts, seed=n_node + 7)
    with guarded("functional") as guard:
        _check_ranks(pred, excluded, ptr, entity, ranks_numpy, stride_pad=3, guard=guard)
        guard.check()
        assert len(guard.records) >= 5


# ------------------------------------------------------------------------------------------------ status codes
def test_status_codes_come_back_before_device_work():
    from ultra_torchdrug_amd import _lib
    dev = _dev()
    n_node, n_rel, node_in, node_out, rel, weight = projection_graph(16, True)
    row_ptr, src, rel_d, w = _graph(n_node, n_rel, node_in, node_out, rel, weight).to(dev).relcsr.csr_arrays
    n_edges, n_query = src.numel(), 65
    bits = torch.zeros(n_node, 2, dtype=torch.int64, device=dev)
    relation = torch.zeros(n_query, dtype=torch.int64, device=dev)
    out = torch.empty_like(bits)
    ws_bytes = int(_lib.load().ultra_sets_project_workspace(n_rel, n_query))
    assert ws_bytes == 8 * n_rel * 2 and _lib.load().ultra_sets_project_workspace(0, 5) == 0
    ws = torch.empty(ws_bytes // 8, dtype=torch.int64, device=dev)
    good = [row_ptr, src, rel_d, w, n_node, n_edges, n_rel, bits, relation, n_query, out, ws, ws_bytes]
    _lib.launch(dev, "ultra_sets_project", *good)
    for at, value, message in ((4, -1, "shape"), (5, -1, "shape"), (6, -1, "shape"), (9, -1, "shape"), (5, 2 ** 31, "shape"),
                               (4, 2 ** 31 - 1, "shape"), (9, 64 * 4 * 65536, "shape"), (10, bits, "shape"), (0, None, "NULL"),
                               (1, None, "NULL"), (2, None, "NULL"), (7, None, "NULL"), (8, None, "NULL"), (10, None, "NULL"),
                               (11, None, "NULL"), (12, ws_bytes - 8, "workspace")):
        args = list(good)
        args[at] = value
        with pytest.raises(RuntimeError, match=message):
            _lib.launch(dev, "ultra_sets_project", *args)
    pred = torch.zeros(3, n_node, device=dev)
    ptr = torch.tensor([0, 1, 1, 2], device=dev)
    entity = torch.tensor([0, 5], device=dev)
    rank = torch.empty(2, dtype=torch.int64, device=dev)
    good = [pred, 3, n_node, n_node, None, ptr, entity, 2, rank]
    _lib.launch(dev, "ultra_sets_rank", *good)
    for at, value, message in ((1, -1, "shape"), (2, -1, "shape"), (7, -1, "shape"), (3, n_node - 1, "shape"), (1, 2 ** 31, "shape"),
                               (0, None, "NULL"), (5, None, "NULL"), (6, None, "NULL"), (8, None, "NULL")):
        args = list(good)
        args[at] = value
        with pytest.raises(RuntimeError, match=message):
            _lib.launch(dev, "ultra_sets_rank", *args)
    torch.cuda.synchronize()
    assert rank.tolist() == [n_node + 1, n_node + 1]                             # all scores tie: pessimistic


# ------------------------------------------------------------------------------------------------ the Python surface
@pytest.fixture(scope="module")
def tasks():
    host = held_out_task()
    return host, held_out_task().to(_dev())


@pytest.fixture(scope="module")
def evaluated(tasks):
    """Per structure, once: the sampled queries and the definition's exact sets on both graphs."""
    host = tasks[0]
    out = {}
    for name in SHAPES:
        anchors, relations, _ = sampled_ids(host, name)
        easy = hand_exact(with_inverses(host.fact_graph), name, anchors.numpy(), relations.numpy())
        full = hand_exact(with_inverses(host.graph), name, anchors.numpy(), relations.numpy())
        out[name] = (anchors, relations, easy, full)
    return out


@pytest.mark.parametrize("name", list(SHAPES))
def test_query_answers_equal_the_hand_executor(tasks, evaluated, name):
    host, task = tasks
    anchors, relations, easy, full = evaluated[name]
    for which, want in (("fact", easy), ("filter", full)):
        got = task.query_answers(name, anchors.to(_dev()), relations.to(_dev()), graph=which)
        assert got.dtype == torch.bool and got.is_cuda and got.shape == (64, 60)
        assert torch.equal(got.cpu(), torch.from_numpy(want)), (name, which)
        assert torch.equal(got.cpu(), host.query_answers(name, anchors, relations, graph=which)), (name, which)
    assert full.any() and (full & ~easy).any()


@pytest.mark.parametrize("name", list(SHAPES))
def test_evaluate_queries_equals_the_definition(tasks, evaluated, name):
    from ultra_torchdrug_amd import engine
    from ultra_torchdrug_amd.task import parse_query_structure
    task, dev = tasks[1], _dev()
    anchors, relations, easy, full = evaluated[name]
    hard, excluded, ptr, query, entity = hard_targets(easy, full)
    assert hard.any(axis=1).sum() >= 8, name                                     # the test does not pass on nothing
    anchors, relations = anchors.to(dev), relations.to(dev)
    tree = parse_query_structure(name)[0]
    with torch.no_grad():
        scores = torch.cat([task.query_memberships(tree, anchors[i:i + 16], relations[i:i + 16]).float() for i in range(0, 64, 16)])
    want_rank = ranks_double_loop(scores.cpu().numpy(), excluded, ptr, entity)
    want = metrics_numpy(query, want_rank, 64)
    got, (got_query, got_entity, got_rank) = engine.evaluate_queries(task, name, anchors, relations, return_ranks=True)
    assert got_rank.dtype == torch.int64 and got_rank.is_cuda
    assert np.array_equal(got_query.cpu().numpy(), query) and np.array_equal(got_entity.cpu().numpy(), entity)
    assert np.array_equal(got_rank.cpu().numpy(), want_rank), name
    assert set(got) == set(want) and got["num_evaluated"] >= 8 and got["num_hard_answers"] == len(entity)
    for key, value in want.items():
        assert abs(got[key] - value) <= 1e-12, (name, key, got[key], value)


@pytest.mark.parametrize("name", ["2p", "3i", "pin"])
def test_filtered_answers(tasks, evaluated, name):
    from ultra_torchdrug_amd import engine
    from ultra_torchdrug_amd.task import parse_query_structure
    task, dev = tasks[1], _dev()
    anchors, relations, _, full = evaluated[name]
    anchors, relations = anchors[:12].to(dev), relations[:12].to(dev)
    known = torch.from_numpy(full[:12])
    with torch.no_grad():
        p = task.query_memberships(parse_query_structure(name)[0], anchors, relations).float().cpu()
    for filtered, scores in ((False, p), (True, torch.where(known, torch.zeros_like(p), p))):
        index, value = topk_rows(scores.numpy(), 60, None)
        entities, membership = task.answer_query(name, anchors, relations, k=60, filtered=filtered)
        assert np.array_equal(entities.cpu().numpy(), np.where(value > 0, index, -1)), (name, filtered)
        assert np.array_equal(membership.cpu().numpy(), np.where(value > 0, value, np.float32(0))), (name, filtered)
        batched = engine.answer_query(task, name, anchors, relations, k=60, batch_size=5, filtered=filtered)
        assert torch.equal(batched[0], entities) and torch.equal(batched[1], membership)
        if not filtered:
            default = task.answer_query(name, anchors, relations, k=60)
            assert torch.equal(default[0], entities) and torch.equal(default[1].view(torch.int32), membership.view(torch.int32))
            assert known[torch.arange(12)[:, None].expand(12, 60), entities.cpu().clamp(min=0)].any()     # something to filter
    listed = (entities >= 0).cpu()
    assert listed.any() and not known[torch.arange(12)[:, None].expand(12, 60)[listed], entities.cpu()[listed]].any()

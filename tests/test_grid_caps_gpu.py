"""MI355X: every launcher whose grid is clamped by a constant, held to its results PAST the clamp (DESIGN.md section 2,
"Constant grid caps"; the table there names the case of each launcher).

The kernels behind these launchers cover what the grid does not with a loop, and state carries from one pass of that loop to the
next: a wave-private LDS row, a count reported once, whole-wave shuffles that need every lane in every pass, the ragged last
pass.  The per-kernel files sit below the clamps, where only the first pass runs.  Every case here has two whole passes and a
ragged third (``trips(...) >= 3`` from the constants of tests/grid_caps.py), puts the decisive data into the later passes, runs
between poisoned guard-banded allocations (tests/guarded_memory.py: a dropped pass is the NaN or -1 poison, not whatever the
allocator held) and is held to the independent definition and the bar of the kernel's own test file: integers and bitmaps
exactly, floats at the bar quoted beside each assertion.  Each floating-point case prints its distance from fp64 beside the fp32
ATen chain's."""
import numpy as np
import pytest
import torch

import guarded_memory as GM
import test_cu_count_gpu as CU
import test_memory_bounds_gpu as MB
import test_row_per_lane_gpu as RPL
from grid_caps import (CAPS, alternating_path, degree_graph, planted_triples, relation_planes_numpy, set_boundary_backward_tiles,
                       set_boundary_items, trips)
from oracle_ops import OracleFunctional

pytestmark = pytest.mark.gpu

HEAD_NAMES = ("score", "d_hidden", "d_query", "d_w1", "d_b1", "d_w2", "d_b2")


def _dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


def _held(got, truth, aten, what, rel=2e-5, floor=1e-7):
    """The bar of the kernel's own file (``MB._close``: ``rel`` of the result's largest entry, plus ``floor``), after printing
    the distance from fp64 beside the fp32 ATen chain's."""
    truth = truth.detach().double().cpu()
    err = float((got.detach().double().cpu() - truth).abs().max())
    ref = float((aten.detach().double().cpu() - truth).abs().max())
    print("%s: HIP %.3g, ATen fp32 %.3g away from fp64; scale %.3g" % (what, err, ref, float(truth.abs().max())))
    MB._close(got, truth, what, rel=rel, floor=floor)


# ==================================================================================================== score_candidates
def _head_chain(ops, t_index, gout, dtype):
    """``[score] + gradients`` of the reference chain (``OracleFunctional.score_candidates``: index, cat, two Linear) in ``dtype``."""
    leaves = [t.to(dtype).requires_grad_() for t in ops]
    score = OracleFunctional.score_candidates(leaves[0], leaves[1], t_index, *leaves[2:])
    score.backward(gout.to(dtype))
    return [score.detach()] + [t.grad for t in leaves]


def _head_call(gout, t_index, *ops):
    from ultra_torchdrug_amd import functional as UF
    with torch.enable_grad():
        leaves = [t.detach().requires_grad_() for t in ops]
        score = UF.score_candidates(leaves[0], leaves[1], t_index, *leaves[2:])
        score.backward(gout)
    return [score.detach()] + [t.grad for t in leaves]


def _plant_repeats(t_index, per_trip):
    """Three identical candidates inside each query whose rows straddle a pass of the forward grid, on both sides of the cut."""
    batch, per_row = t_index.shape
    planted = 0
    for cut in range(per_trip, batch * per_row, per_trip):
        b, j = divmod(cut, per_row)
        if 2 <= j <= per_row - 3:                                  # rows b * per_row + j - 2 (before the cut), + j, + j + 2 (after it)
            t_index[b, j - 2] = t_index[b, j] = t_index[b, j + 2] = (7 * b + 3) % 300
            planted += 1
    return planted


@pytest.mark.parametrize("batch,per_row", [(55, 160), (26, 160)])
def test_score_candidates_takes_the_row_loop_past_256_workgroups(batch, per_row):
    """``score_rows_forward_kernel``: 8 800 rows are two passes of the 256 x 16 waves and 608 rows (38 workgroups) of a third;
    4 160 rows give only FOUR workgroups a second pass.  A wave rewrites its LDS row behind an ``lgkmcnt`` wait in every pass.
    The backward's weight-gradient slices have 550 = 34 * 16 + 6 rows (260 = 16 * 16 + 4): the 16-row unroll's tail.  Scores and
    all six gradients against fp64 autograd of the reference chain at 2e-5 of each result's scale + 1e-7."""
    n_node, rows = 300, batch * per_row
    assert trips(rows, CAPS["score_rows_forward"]) >= (3 if batch == 55 else 2)
    assert rows % CAPS["score_rows_forward"] != 0                   # the last pass leaves most of the grid without a row
    ops = [torch.from_numpy(a) for a in RPL._operands(n_node, batch, "normal")]
    gen = torch.Generator().manual_seed(rows)
    t_index = torch.randint(0, n_node, (batch, per_row), generator=gen)
    assert _plant_repeats(t_index, CAPS["score_rows_forward"]) == trips(rows, CAPS["score_rows_forward"]) - 1
    gout = torch.randn(batch, per_row, generator=gen)
    truth, aten = _head_chain(ops, t_index, gout, torch.float64), _head_chain(ops, t_index, gout, torch.float32)
    dev = _dev()
    got = MB.run_guarded(_head_call, gout.to(dev), t_index.to(dev), *(t.to(dev) for t in ops), what="score_candidates")
    last = slice(2 * CAPS["score_rows_forward"] if batch == 55 else CAPS["score_rows_forward"], None)
    assert float(truth[0].reshape(-1)[last].abs().min()) > 0, "the later passes' scores must be there to lose"
    for name, g, t, a in zip(HEAD_NAMES, got, truth, aten):
        _held(g, t, a, "%s at %d x %d rows" % (name, batch, per_row))
    _held(got[0].reshape(-1)[last], truth[0].reshape(-1)[last], aten[0].reshape(-1)[last], "scores of the last pass")


def test_score_candidates_backward_fills_a_hidden_gradient_past_the_fill_grid():
    """``zero_fill_kernel`` behind ``ultra_score_rows_backward_f32``: ``d_hidden`` of 20 200 nodes x 26 queries is 8 403 200
    float4, past the 8 388 608 from which the fill's grid stays at 4 096 workgroups (8.01 passes of the grid).  Everything
    outside the candidates' rows must carry the bits of +0 and nothing the poison; the candidates' rows and the other gradients
    against the fp64 chain on the GATHERED rows (the distinct candidate nodes compacted: the same function of them)."""
    n_node, batch, per_row = 20_200, 26, 160
    n4 = n_node * batch * 16
    assert n4 > CAPS["zero_fill_clamp_binds"] and trips(n4, CAPS["zero_fill"]) >= 3
    rng = np.random.default_rng(n4)
    hidden = torch.from_numpy(rng.standard_normal((n_node, batch, 64), dtype=np.float32))
    ops = [hidden] + [torch.from_numpy(a) for a in RPL._operands(300, batch, "normal")[1:]]
    gen = torch.Generator().manual_seed(n4)
    t_index = torch.randint(0, n_node, (batch, per_row), generator=gen)
    t_index[:, -1] = n_node - 1                                    # the last row of the tensor is a candidate of every query
    t_index[3, 7] = t_index[3, 99]                                 # ... and one node twice in a query
    gout = torch.randn(batch, per_row, generator=gen)
    nodes, compact = torch.unique(t_index, return_inverse=True)
    small = [hidden[nodes]] + ops[1:]
    truth, aten = _head_chain(small, compact, gout, torch.float64), _head_chain(small, compact, gout, torch.float32)
    dev = _dev()
    got = MB.run_guarded(_head_call, gout.to(dev), t_index.to(dev), *(t.to(dev) for t in ops), what="score_candidates, large N")
    d_hidden = got[1]
    assert tuple(d_hidden.shape) == (n_node, batch, 64) and not GM.has_poison(d_hidden)
    written = torch.zeros(n_node, batch, dtype=torch.bool, device=dev)
    written[t_index.to(dev), torch.arange(batch, device=dev)[:, None]] = True
    nonzero_bits = (d_hidden.view(torch.int32) != 0).any(dim=-1)
    assert not bool((nonzero_bits & ~written).any()), "d_hidden outside the candidates' rows is not +0"
    assert bool(nonzero_bits[-1].all()), "the tensor's last rows are candidates: they carry a gradient"
    for name, g, t, a in zip(HEAD_NAMES, [got[0], d_hidden[nodes.to(dev)]] + got[2:], truth, aten):
        _held(g, t, a, "%s at %d nodes" % (name, n_node))


def test_score_candidates_without_rows():
    """The empty end of the same loops.  ``score_candidates_supported`` refuses ``K = 0`` (so ``_ScoreRows`` never allocates a
    ``d_query`` that nothing fills), the operator raises, and the C entry's no-rows branch -- reachable through the C ABI alone
    -- zeroes ``d_query`` with the parameter gradients.  ``B = 0`` is admitted: empty scores, zero parameter gradients."""
    from ultra_torchdrug_amd import _lib, functional as UF
    dev = _dev()
    ops = [torch.from_numpy(a).to(dev) for a in RPL._operands(11, 3, "normal")]
    none = torch.zeros(3, 0, dtype=torch.int64, device=dev)
    assert not UF.score_candidates_supported(ops[0], ops[1], none, ops[2], ops[4])
    with pytest.raises(RuntimeError, match="score_candidates"):
        UF.score_candidates(ops[0], ops[1], none, *ops[2:])
    with GM.guarded("functional") as guard:
        outs = [guard.carve(shape, torch.float32, dev) for shape in ((11, 3, 64), (3, 64), (128, 128), (128,), (128,), (1,))]
        scratch = guard.carve((16 * 129 * 129,), torch.float32, dev)
        _lib.launch(dev, "ultra_score_rows_backward_f32", None, ops[1], None, ops[2], ops[4], None, None, None, None, scratch, *outs,
                    11, 3, 0)
        guard.check()
    for name, t in zip(HEAD_NAMES[1:], outs):
        assert not bool(t.view(torch.int32).any()), "%s of a call without rows is not +0" % name

    def call(hidden, query, t_index, *head):
        with torch.enable_grad():
            leaves = [t.detach().requires_grad_() for t in (hidden, query, *head)]
            score = UF.score_candidates(leaves[0], leaves[1], t_index, *leaves[2:])
            score.sum().backward()
        return [score.detach()] + [t.grad for t in leaves]

    empty = MB.run_guarded(call, torch.zeros(11, 0, 64, device=dev), torch.zeros(0, 64, device=dev),
                           torch.zeros(0, 5, dtype=torch.int64, device=dev), *ops[2:], what="score_candidates, B = 0")
    assert tuple(empty[0].shape) == (0, 5) and tuple(empty[1].shape) == (11, 0, 64) and tuple(empty[2].shape) == (0, 64)
    for name, t in zip(HEAD_NAMES[3:], empty[3:]):
        assert not bool(t.view(torch.int32).any()), "%s of a call without queries is not +0" % name


# ==================================================================================================== hop distances
def _hop_runs(monkeypatch, n_node, node_in, node_out, sources, targets, weight=None, num_iters=100):
    """Matrix and targets form, polled and with a fixed level count, through the C ABI between guard bands (the graph and its
    CSR built inside the guard): ``(mean in-degree of the coalesced CSR, [matrix, pairs, matrix, pairs])``."""
    from hop_definition import graph_of
    from ultra_torchdrug_amd import functional as UF
    monkeypatch.setenv("ULTRA_BINDING", "ctypes")
    seen = {}

    def call(sources, targets):
        graph = graph_of(n_node, node_in, node_out, weight).to(_dev())
        seen["mean"] = graph.relcsr.csr_arrays[1].numel() // n_node
        return [UF.hop_distance(graph.relcsr, sources, num_iters), UF.hop_distance(graph.relcsr, sources, num_iters, targets=targets),
                UF.hop_distance(graph.relcsr, sources, num_iters, poll=False),
                UF.hop_distance(graph.relcsr, sources, num_iters, targets=targets, poll=False)]

    got = MB.run_guarded(call, _t(sources), _t(targets), modules=("functional", "relcsr", "graph"), what="hop_distance")
    return seen["mean"], got


def _hop_check(got, want, sources, targets):
    want_pairs = want[targets, np.arange(len(sources))[:, None]]
    for matrix, pairs in (got[:2], got[2:]):
        assert matrix.dtype == torch.int32 and np.array_equal(matrix.cpu().numpy(), want)
        assert pairs.dtype == torch.int32 and np.array_equal(pairs.cpu().numpy(), want_pairs)


def _hop_ids(n_node, per_trip, n_source, seed):
    """Sources and targets: random ones, and a node of each pass of the level kernel among both."""
    rng = np.random.default_rng(seed)
    sources = rng.integers(0, n_node, n_source)
    sources[:3] = (n_node - 2, per_trip + 1, 1)
    targets = rng.integers(0, n_node, (n_source, 7))
    targets[:, 0], targets[:, 1] = n_node - 1, 2 * per_trip + 3
    return sources, targets


HOP_GRAPHS = {16: (65_573, 3), 32: (32_805, 30), 64: (16_421, 50)}          # lanes a row: (nodes, mean in-degree)


@pytest.mark.parametrize("group", [16, 32, 64])
def test_hop_levels_take_a_third_round(monkeypatch, group):
    """``hop_level_kernel<G>`` hands its rows out over at most 2 048 workgroups of 256 / G rows: 65 573, 32 805 and 16 421
    nodes are two rounds and 37 rows for G = 16, 32 and 64 (G from the mean in-degree of the coalesced CSR, asserted).  The fresh
    bits of all rounds go into ONE count per wave.  Three sources (a node of each round among them); the queue BFS of
    tests/hop_definition.py, exactly."""
    from hop_definition import queue_form
    n_node, degree = HOP_GRAPHS[group]
    per_trip = CAPS["hop_level_%d" % group]
    assert trips(n_node, per_trip) >= 3 and n_node % per_trip % (256 // group) != 0
    node_in, node_out = degree_graph(n_node, degree, seed=n_node)
    sources, targets = _hop_ids(n_node, per_trip, 3, seed=group)
    want = queue_form(n_node, node_in, node_out, sources)
    assert (want[2 * per_trip:] < n_node).any() and (want[per_trip:2 * per_trip] < n_node).any()
    mean, got = _hop_runs(monkeypatch, n_node, node_in, node_out, sources, targets)
    assert {16: mean < 24, 32: 24 <= mean < 48, 64: mean >= 48}[group], (group, mean)
    _hop_check(got, want, sources, targets)


def test_hop_levels_with_zero_weights_take_a_third_round(monkeypatch):
    """The weighted form (``HAS_W``) on the G = 16 graph: every third edge has weight 0 and does not exist."""
    from hop_definition import queue_form
    n_node, degree = HOP_GRAPHS[16]
    per_trip = CAPS["hop_level_16"]
    assert trips(n_node, per_trip) >= 3
    node_in, node_out = degree_graph(n_node, degree, seed=n_node + 1)
    key = node_in * n_node + node_out
    _, first = np.unique(key, return_index=True)                    # distinct edges: no weight is summed with another
    node_in, node_out = node_in[np.sort(first)], node_out[np.sort(first)]
    weight = np.full(len(node_in), 1.5, dtype=np.float32)
    weight[::3] = 0.0
    sources, targets = _hop_ids(n_node, per_trip, 3, seed=7)
    live = weight != 0
    want = queue_form(n_node, node_in[live], node_out[live], sources)
    assert not np.array_equal(want, queue_form(n_node, node_in, node_out, sources)), "the dropped edges must matter"
    assert (want[2 * per_trip:] < n_node).any()
    mean, got = _hop_runs(monkeypatch, n_node, node_in, node_out, sources, targets, weight=weight)
    assert mean < 24
    _hop_check(got, want, sources, targets)


def test_hop_levels_from_a_word_of_sources_and_one(monkeypatch):
    """65 sources on the G = 64 graph: two blocks of sources, so ``hop_clear_kernel`` and the counter words run twice, and the
    distance matrix of 16 421 x 65 entries takes ``hop_fill_kernel`` past its 524 288 entries a pass.  The level cap of 6 is
    above the graph's eccentricities (asserted); the ATen iteration of tests/hop_definition.py, exactly."""
    from hop_definition import iteration_form
    n_node, degree = HOP_GRAPHS[64]
    per_trip = CAPS["hop_level_64"]
    assert trips(n_node, per_trip) >= 3 and trips(n_node * 65, CAPS["hop_fill"]) >= 3
    node_in, node_out = degree_graph(n_node, degree, seed=n_node)
    sources, targets = _hop_ids(n_node, per_trip, 65, seed=65)
    want = iteration_form(n_node, node_in, node_out, sources, num_iters=6).numpy()
    assert want.max() < 6 and (want[2 * per_trip:, 64] > 0).any()
    mean, got = _hop_runs(monkeypatch, n_node, node_in, node_out, sources, targets, num_iters=6)
    assert mean >= 48
    _hop_check(got, want, sources, targets)


def test_hop_levels_along_a_path_that_alternates_between_the_rounds(monkeypatch):
    """A path of 148 nodes among 65 573 whose consecutive nodes alternate between ids below 1 000 and rows of the third (then
    the second) round: every level has ONE fresh node, at odd levels found after the first round, at even levels in it and not
    in the last.  A count lost or overwritten across rounds ends ``poll`` early; a shuffle that misses lanes loses the node."""
    from hop_definition import queue_form
    n_node, per_trip = HOP_GRAPHS[16][0], CAPS["hop_level_16"]
    path, node_in, node_out = alternating_path(n_node, per_trip)
    assert trips(n_node, per_trip) >= 3 and len(path) == 148 and path[1] >= 2 * per_trip and per_trip <= path[-1] < 2 * per_trip
    sources = np.array([path[0], path[1], path[75]])
    targets = np.stack([path[[-1, -2, 74, 75, 1, 2, 0]]] * 3)
    want = queue_form(n_node, node_in, node_out, sources, num_iters=200)
    assert want[path[-1], 0] == 147 and want[path[-1], 1] == 146 and want[path[0], 1] == n_node
    mean, got = _hop_runs(monkeypatch, n_node, node_in, node_out, sources, targets, num_iters=200)
    _hop_check(got, want, sources, targets)                         # polled (ends when a level adds nothing), and 200 levels enqueued


def test_hop_clear_takes_a_third_pass(monkeypatch):
    """``hop_clear_kernel`` over 1 048 613 nodes (two passes of 524 288 and 37): the targets form from one source over a
    handful of edges that end in the last pass's nodes.  A bitmap word the clear leaves out holds the guard's all-ones poison:
    every source would have reached that node already."""
    from hop_definition import queue_form
    n_node = 2 * CAPS["hop_clear"] + 37
    assert trips(n_node, CAPS["hop_clear"]) >= 3
    chain = np.array([5, n_node - 1, CAPS["hop_clear"] + 9, n_node - 30, 77, 2 * CAPS["hop_clear"] + 1])
    node_in, node_out = np.concatenate([chain[:-1], [n_node - 9]]), np.concatenate([chain[1:], [n_node - 8]])
    sources = np.array([5])
    targets = np.array([[n_node - 1, CAPS["hop_clear"] + 9, n_node - 30, 77, 2 * CAPS["hop_clear"] + 1, n_node - 8, n_node - 2, 5]])
    want = queue_form(n_node, node_in, node_out, sources)[targets[0], 0]
    assert want.tolist() == [1, 2, 3, 4, 5, n_node, n_node, 0]
    from hop_definition import graph_of
    from ultra_torchdrug_amd import functional as UF
    monkeypatch.setenv("ULTRA_BINDING", "ctypes")

    def call(sources, targets):
        graph = graph_of(n_node, node_in, node_out).to(_dev())
        return [UF.hop_distance(graph.relcsr, sources, targets=targets), UF.hop_distance(graph.relcsr, sources, 8, targets=targets, poll=False)]

    for pairs in MB.run_guarded(call, _t(sources), _t(targets), modules=("functional", "relcsr", "graph"), what="hop_distance, 2^20 nodes"):
        assert pairs.dtype == torch.int32 and pairs.cpu().numpy()[0].tolist() == want.tolist()


def test_hop_distance_without_sources(monkeypatch):
    """The empty end: no source, or no target per source -- empty results of the documented shapes, no launch."""
    from hop_definition import graph_of
    from ultra_torchdrug_amd import functional as UF
    monkeypatch.setenv("ULTRA_BINDING", "ctypes")
    dev = _dev()
    graph = graph_of(9, [0, 1], [1, 2]).to(dev)
    none = torch.zeros(0, dtype=torch.int64, device=dev)
    for poll in (None, False):
        assert tuple(UF.hop_distance(graph.relcsr, none, poll=poll).shape) == (9, 0)
        assert tuple(UF.hop_distance(graph.relcsr, none, targets=none.view(0, 4), poll=poll).shape) == (0, 4)
        assert tuple(UF.hop_distance(graph.relcsr, torch.tensor([1], device=dev), targets=none.view(1, 0), poll=poll).shape) == (1, 0)


# ==================================================================================================== relation graph
def test_relation_marks_take_a_third_pass():
    """``relation_marks_kernel``: a wave per entity over at most 8 192 workgroups of 4 -- 65 573 entities are two passes and 37
    (not a multiple of a workgroup's four).  The head-head pairs (3, 4) and (2, 4) exist at one entity of the second pass each,
    (0, 5) at one of the third.  The four planes against the reference's incidence products in numpy, and the relation graph's
    edge list against the torch builder of ``test_native_relation_graph_equals_the_reference_products`` (the sparse products on
    a CPU copy), exactly."""
    from ultra_torchdrug_amd import functional as UF
    from ultra_torchdrug_amd.graph import Graph
    from ultra_torchdrug_amd.rel_model import construct_relation_graph
    n_node, per_trip = 65_573, CAPS["relation_marks"]
    assert trips(n_node, per_trip) >= 3 and n_node % per_trip % 4 != 0
    triples, n_rel, planted = planted_triples(n_node, per_trip)
    both = np.concatenate([triples, np.stack([triples[:, 1], triples[:, 0], triples[:, 2] + n_rel], axis=1)])
    want = relation_planes_numpy(both, n_node, 2 * n_rel)
    first_pass = both[(both[:, 0] < per_trip) & (both[:, 1] < per_trip)]
    without = relation_planes_numpy(first_pass, n_node, 2 * n_rel)
    for node, r1, r2 in planted:
        assert node >= per_trip and want[0, r1, r2] and want[0, r2, r1] and not without[0, r1, r2]
    assert planted[-1][0] >= 2 * per_trip
    got = MB.run_guarded(lambda e: UF.relation_graph_blocks(e, n_node, 2 * n_rel), _t(both), what="relation_graph_blocks")
    assert got.dtype == torch.bool and np.array_equal(got.cpu().numpy(), want)
    cpu = Graph(torch.from_numpy(triples), num_node=n_node, num_relation=n_rel)
    built = MB.run_guarded(lambda e: construct_relation_graph(Graph(e, num_node=n_node, num_relation=n_rel)).edge_list, _t(triples),
                           modules=("functional", "relcsr", "graph", "rel_model"), what="construct_relation_graph")
    assert torch.equal(built.cpu(), construct_relation_graph(cpu).edge_list)


def test_relation_marks_without_entities():
    """The empty end: no entity and no edge -- four all-False planes, no poison read as a mark."""
    from ultra_torchdrug_amd import functional as UF
    none = torch.zeros(0, 3, dtype=torch.int64, device=_dev())
    for n_node in (0, 5):
        got = MB.run_guarded(lambda e: UF.relation_graph_blocks(e, n_node, 3), none, what="relation_graph_blocks, empty")
        assert tuple(got.shape) == (4, 3, 3) and not bool(got.any())


# ==================================================================================================== set boundary
SET_SHAPE = (40, 89_605)            # queries (3 chunks of 16), nodes (1 401 tiles of 64): 4 203 items


@pytest.mark.parametrize("dim", [8, 3], ids=["16_byte_pieces", "scalar_pieces"])
def test_set_boundary_takes_a_third_pass(dim):
    """``set_boundary_kernel<4 / 1>``: 4 203 items for 2 048 workgroups -- two passes and 107 items, the LDS tile restaged behind
    a barrier in each, counts added per item.  tests/query_definition.py's numpy definition, bit for bit, with and without the
    floor, memberships a strided view with NaN padding."""
    from query_definition import set_boundary_numpy, special_members
    from topk_definition import same_bits
    from ultra_torchdrug_amd import functional as UF
    n_query, n_node = SET_SHAPE
    assert trips(set_boundary_items(n_query, n_node), CAPS["set_boundary"]) >= 3
    member, query, floor = special_members(n_query, n_node, seed=n_node + dim, dim=dim)
    wide = torch.full((n_query, n_node + 3), float("nan"))
    wide[:, :n_node] = member
    want_b, want_c = set_boundary_numpy(member.numpy(), query.numpy(), floor.numpy())
    want_b0, want_c0 = set_boundary_numpy(member.numpy(), query.numpy(), None)
    later = 2 * CAPS["set_boundary"] // 3 * 64                     # the first node of the third pass
    assert want_b[later:].any() and want_c.max() > 0

    def call(wide, query, floor):
        return [UF.set_boundary(wide[:, :n_node], query, floor, with_count=True), UF.set_boundary(wide[:, :n_node], query, None, with_count=True)]

    (b, c), (b0, c0) = MB.run_guarded(call, wide.to(_dev()), query.to(_dev()), floor.to(_dev()), widest_row=n_query * dim * 4,
                                      what="set_boundary")
    assert same_bits(b.cpu().numpy(), want_b) and np.array_equal(c.cpu().numpy(), want_c) and c.dtype == torch.int32
    assert same_bits(b0.cpu().numpy(), want_b0) and np.array_equal(c0.cpu().numpy(), want_c0)


@pytest.mark.parametrize("dim", [8, 3], ids=["16_byte_pieces", "scalar_pieces"])
def test_set_boundary_backward_takes_a_third_pass(dim):
    """``set_boundary_backward_kernel<4 / 1>``: ``backward_shape`` gives each of the three chunks 2 048 / 3 = 682 workgroups for
    its 1 401 tiles -- two passes and 37 tiles, ``d_query`` kept in registers over all of them.  Inputs on the dyadic grid
    (exact in fp32 up to 262 144 nodes): tests/query_grad_definition.py's numpy definition, entry for entry."""
    from query_grad_definition import grid_set_case, keep_mask, set_boundary_backward_numpy
    from ultra_torchdrug_amd import functional as UF
    n_query, n_node = SET_SHAPE
    tiles, blocks = set_boundary_backward_tiles(n_query, n_node)
    assert trips(tiles, blocks) >= 3 and n_node < 262_144
    member, query, floor, d_boundary = grid_set_case(n_query, n_node, dim, seed=dim)
    want_member, want_query = set_boundary_backward_numpy(d_boundary, member, floor, query)
    assert np.abs(want_member[:, 2 * blocks * 64:]).max() > 0
    dev = _dev()

    def call(d_boundary, member, query, floor):
        return list(UF.set_boundary_backward(d_boundary, member, query, floor))

    d_member, d_query = MB.run_guarded(call, *(torch.from_numpy(a).to(dev) for a in (d_boundary, member, query, floor)),
                                       widest_row=n_query * dim * 4, what="set_boundary_backward")
    assert np.array_equal(d_member.cpu().numpy().astype(np.float64), want_member)
    assert not d_member.view(torch.int32).cpu().numpy()[~keep_mask(member, floor)].any()         # +0.0 BITS where nothing is kept
    assert np.array_equal(d_query.cpu().numpy().astype(np.float64), want_query)


def test_set_boundary_refuses_an_empty_shape():
    """The empty end: no query, no node or no column is refused before any launch, forward and backward."""
    from ultra_torchdrug_amd import functional as UF
    dev = _dev()
    for n_query, n_node, dim in ((0, 5, 4), (2, 0, 4), (2, 5, 0)):
        member, query = torch.zeros(n_query, n_node, device=dev), torch.zeros(n_query, dim, device=dev)
        with pytest.raises(RuntimeError, match="set_boundary"):
            UF.set_boundary(member, query, None, with_count=True)
        with pytest.raises(RuntimeError, match="set_boundary_backward"):
            UF.set_boundary_backward(torch.zeros(n_node, n_query, dim, device=dev), member, query)


# ==================================================================================================== copies and statistics
def test_relation_stack_inputs_take_a_third_pass():
    """``relation_stack_inputs_kernel``: three loops share one stride of 1 024 x 256 float4.  6 layers x 90 relations x 67
    queries are 578 880 items: two passes and 54 592 (213 workgroups and a quarter).  Every table row equals its weight row bit
    for bit, ``ones`` is all 1, ``node32`` is ``h_index`` read through a stride of 3."""
    from ultra_torchdrug_amd import functional as UF
    n_layers, n_rel, n_query = 6, 90, 67
    items = n_layers * n_rel * n_query * 16
    assert trips(items, CAPS["relation_stack_inputs"]) >= 3 and items % CAPS["relation_stack_inputs"] % 256 != 0
    gen = torch.Generator().manual_seed(items)
    weights = [torch.randn(n_rel, 64, generator=gen) for _ in range(n_layers)]
    spread = torch.randint(0, n_rel, (n_query, 3), generator=gen)
    want_tables = torch.stack(weights).unsqueeze(2).expand(-1, -1, n_query, -1).reshape(n_layers, n_rel, n_query * 64)

    def call(spread, *weights):
        h_index = spread[:, 1]
        assert h_index.stride(0) == 3
        return list(UF.relation_stack_inputs(list(weights), h_index))

    dev = _dev()
    tables, ones, node32 = MB.run_guarded(call, spread.to(dev), *(w.to(dev) for w in weights), widest_row=n_query * 256,
                                          what="relation_stack_inputs")
    assert torch.equal(tables.cpu().view(torch.int32), want_tables.contiguous().view(torch.int32))
    assert torch.equal(ones.cpu(), torch.ones(n_query, 64))
    assert node32.dtype == torch.int32 and torch.equal(node32.cpu().long(), spread[:, 1])


def test_relation_stack_inputs_without_relations_or_queries():
    """The empty end: no query -- three empty tensors, no launch; no relation -- empty tables, ``ones`` and ``node32`` written."""
    from ultra_torchdrug_amd import functional as UF
    dev = _dev()

    def call(h_index, *weights):
        return list(UF.relation_stack_inputs(list(weights), h_index))

    none = torch.zeros(0, dtype=torch.int64, device=dev)
    with GM.guarded("functional") as guard:
        tables, ones, node32 = call(none, torch.zeros(5, 64, device=dev))
        assert tuple(tables.shape) == (1, 5, 0) and tuple(ones.shape) == (0, 64) and tuple(node32.shape) == (0,) and guard.records
    h_index = torch.tensor([4, 0, 2], device=dev)
    tables, ones, node32 = MB.run_guarded(call, h_index, torch.zeros(0, 64, device=dev), torch.zeros(0, 64, device=dev),
                                          what="relation_stack_inputs, no relation")
    assert tuple(tables.shape) == (2, 0, 3 * 64) and torch.equal(ones.cpu(), torch.ones(3, 64)) and node32.cpu().tolist() == [4, 0, 2]


@pytest.mark.parametrize("repeat", [0, 5])
def test_statistics_over_all_1024_blocks_and_a_tail(repeat):
    """``statistics_partial_kernel``: 9 000 003 floats are 2 250 000 float4 -- all 1 024 workgroups run, each over a range of
    2 198 float4 (8.6 rounds of its 256 threads, the last workgroup's range ragged), and the last one takes the 3-element tail.
    ``Tensor.norm / mean / std`` in fp64 at the 1e-5 relative bar of tests/test_memory_bounds_gpu.py, with and without the
    repeated part.  The tail holds the largest values: without it the norm is off by a third."""
    from ultra_torchdrug_amd import functional as UF
    numel = 9_000_003
    assert trips(numel, CAPS["statistics"]) >= 3 and numel % 4 == 3
    gen = torch.Generator().manual_seed(numel)
    values = torch.randn(numel, generator=gen) * 2 + 0.5
    values[-3:] = torch.tensor([3000.0, -2500.0, 2000.0])
    values[CAPS["statistics"] * 2 + 5] = -4000.0                   # ... and one in the ninth round of a middle workgroup
    extra = torch.randn(7, 64, generator=gen) if repeat else None
    dev = _dev()
    got = MB.run_guarded(lambda v, e: UF.statistics(v, e, repeat), values.to(dev), None if extra is None else extra.to(dev), what="statistics")
    flat = values.double() if extra is None else torch.cat([values.double(), extra.double().reshape(1, -1).expand(repeat, -1).reshape(-1)])
    want = torch.stack([flat.norm(), flat.mean(), flat.std()])
    f32 = flat.float()
    aten = torch.stack([f32.norm(), f32.mean(), f32.std()]).double()
    for k, name in enumerate(("norm", "mean", "std")):
        print("statistics %s (repeat %d): HIP %.3g, ATen fp32 %.3g away from fp64; value %.6g"
              % (name, repeat, abs(float(got[k]) - float(want[k])), abs(float(aten[k]) - float(want[k])), float(want[k])))
    torch.testing.assert_close(got.cpu(), want.float(), rtol=1e-5, atol=1e-6)


def test_statistics_of_nothing():
    """The empty end: no element -- norm 0, mean 0 (the kernel's choice where ``Tensor.mean`` gives NaN), std NaN; the one
    partial the single workgroup writes is read, nothing unwritten."""
    from ultra_torchdrug_amd import functional as UF
    got = MB.run_guarded(lambda v: UF.statistics(v), torch.zeros(0, device=_dev()), what="statistics, empty")
    assert got.cpu().tolist()[:2] == [0.0, 0.0] and bool(torch.isnan(got[2])) and not GM.has_poison(got)


# ==================================================================================================== first layer in training
def _epilogue_chain(d, u, params, gout, dtype):
    """fp64 / fp32 autograd of the layer epilogue alone on the given rows: ``[out, d_input, d_update, d_weight, d_bias,
    d_ln_weight, d_ln_bias]`` of ``relu(LayerNorm(Linear(cat[d, u]))) + d``."""
    with torch.enable_grad():
        d, u = d.to(dtype).requires_grad_(), u.to(dtype).requires_grad_()
        w, b, gamma, beta = (torch.as_tensor(p).to(dtype).requires_grad_() for p in params)
        pre = torch.nn.functional.layer_norm(torch.nn.functional.linear(torch.cat([d, u], dim=-1), w, b), (64,), gamma, beta, 1e-5)
        out = torch.relu(pre) + d
        return [out.detach(), pre.detach()] + list(torch.autograd.grad(out, [d, u, w, b, gamma, beta], gout.to(dtype)))


def test_first_layer_in_training_gathers_and_scatters_a_third_pass(monkeypatch):
    """``gather_rows_kernel`` / ``scatter_rows_kernel`` (a fixed grid of 1 024 workgroups, 16 listed rows each a pass):
    ``sum_layer`` in training on the hub-source graph of tests/test_cu_count_gpu.py at 3 000 nodes and 12 queries, whose
    boundary nodes reach all nodes but ten -- more than 32 768 listed rows (asserted from the device's count).  Output,
    ``d_relation``, ``d_boundary_value``, ``d_weight``, ``d_bias`` and the LayerNorm pair against fp64 autograd of the layer
    written with index_add, at that file's bar (``4 * ref_dev + 2e-5 * scale``)."""
    from ultra_torchdrug_amd import functional as UF
    n, r, Q = 3000, 9, 12
    monkeypatch.setenv("ULTRA_BINDING", "ctypes")
    monkeypatch.setattr(CU, "FIRST_LAYER", (n, r, Q))
    counts = []
    real = UF.first_layer_train_forward

    def recording(*args, **kwargs):
        taken = real(*args, **kwargs)
        if taken is not None:
            counts.append(int(taken[3]))
        return taken

    monkeypatch.setattr(UF, "first_layer_train_forward", recording)
    g = CU._hub_source_graph(n, r, Q)
    _, relation, _, b_value, params, _ = MB._layer_operands(41, n, r, Q)
    host = [torch.from_numpy(a) for a in (relation, b_value, *params)]
    gout = torch.randn(n, Q, 64, generator=torch.Generator().manual_seed(42))
    grads, outs = {}, {}
    for dtype in (torch.float64, torch.float32):
        leaves = [t.clone().to(dtype).requires_grad_() for t in host]
        pre, dense = CU._first_layer_chain(leaves, g, True)
        if dtype == torch.float64:
            gout[(pre.detach().abs() < 1e-4).any(dim=-1)] = 0.0       # relu is not differentiable at 0 (tests/test_rspmm_gpu.py)
        out = torch.relu(pre) + dense
        out.backward(gout.to(dtype))
        grads[dtype], outs[dtype] = [t.grad.double() for t in leaves], out.detach().double()
    run = CU._first_layer_runner(monkeypatch, g, host, gout)
    got = MB.run_guarded(run, modules=("functional", "relcsr"), widest_row=256 * Q, what="first layer in training, 12 hubs")
    assert len(counts) == 2 and counts[0] == counts[1] and counts[0] <= n * Q
    assert trips(counts[0], CAPS["gather_rows"]) >= 3 and counts[0] % CAPS["gather_rows"] % 16 != 0, counts
    CU._bound(got[0], outs[torch.float64], outs[torch.float32], 2e-5, "first layer in training, %d listed rows: output" % counts[0])
    for name, gr, t, a in zip(CU.FIRST_LAYER_NAMES, got[1:], grads[torch.float64], grads[torch.float32]):
        CU._bound(gr, t, a, 2e-5, "first layer in training, %d listed rows: %s" % (counts[0], name))


FILL_SHAPE = (44_003, 9, 12)        # nodes, relations, queries: 528 036 rows of 64 floats = 8 448 576 float4


def _fill_case(seed):
    """A sparse graph over ``FILL_SHAPE`` whose first layer touches a few hundred of the 528 036 rows, the LAST row among them."""
    from graphs import random_graph
    n, r, Q = FILL_SHAPE
    assert n * Q * 16 > CAPS["zero_fill_clamp_binds"] and trips(n * Q * 16, CAPS["zero_fill"]) >= 3
    g = random_graph(seed=seed, n_node=n, n_edge=60_000, n_rel=r, unique=True)
    _, relation, _, b_value, params, _ = MB._layer_operands(seed, 8, r, Q)
    deg_out = np.bincount(g["src"], minlength=n)
    b_node = np.flatnonzero(deg_out >= 3)[:Q].astype(np.int32)
    b_node[-1], b_node[-2] = n - 1, int(deg_out.argmax())           # query Q - 1 starts at the last node: row n * Q - 1 is listed
    return g, relation, b_node, b_value, params


def test_first_layer_fills_run_past_4096_workgroups(oracle, monkeypatch):
    """``zero_fill_kernel`` behind ``ultra_rspmm_frontier_f32`` and ``const_fill_kernel`` behind both sparse first-layer entries:
    528 036 rows are 8 448 576 float4, past the 8 388 608 from which the fill grids stay at 4 096 workgroups (8.06 passes).  The
    oracle's rspmm over the dense boundary, bit for bit and with the bits of +0 in every row no edge reaches; the layer's output
    against the oracle's epilogue on the rows that differ from the constant row and on ONE untouched row, bit for bit."""
    from ultra_torchdrug_amd import RelCSR, functional as UF
    monkeypatch.setattr(UF, "SPARSE_FIRST_LAYER_MIN_ROWS", 0)
    monkeypatch.setattr(UF, "SPARSE_FIRST_LAYER_TRAIN_MAX_FRACTION", 1.0)
    n, r, Q = FILL_SHAPE
    g, relation, b_node, b_value, params = _fill_case(5)
    from_boundary = np.isin(g["src"], b_node)
    reached = np.unique(np.concatenate([g["dst"][from_boundary], b_node]))
    local = np.searchsorted(reached, np.arange(n).clip(max=reached[-1]))                  # node -> its place among the reached nodes
    sub = {k: g[k][from_boundary] for k in ("dst", "src", "rel")}
    sub = dict(dst=local[sub["dst"]], src=local[sub["src"]], rel=sub["rel"], w=None)     # the same edges over the reached nodes alone
    m = len(reached)
    node_sub = local[b_node].astype(np.int32)
    dense_sub = OracleFunctional._dense_boundary((torch.from_numpy(node_sub), torch.from_numpy(b_value)), m + 1).numpy().reshape(m + 1, Q, 64)
    want_update, want_out = MB._oracle_layer(oracle, sub, m + 1, r, 128, relation, dense_sub, (node_sub, b_value), params, True, True)
    assert not want_update[m].any() and not dense_sub[m].any()                           # row m: a node nothing reaches
    constant = want_out[m, 0]
    assert all(np.array_equal(want_out[m, q], constant) for q in range(Q))

    def call(dst, src, rel, relation, b_node, b_value, w, b, gamma, beta):
        csr = RelCSR(dst, src, rel, None, n, n, r, piece_len=128)
        update = UF.rspmm_frontier(csr, relation, (b_node, b_value))
        out = UF.first_layer_forward(csr, relation, (b_node, b_value), w, b, gamma, beta, 1e-5, True, True)
        trained = UF.first_layer_train_forward(csr, relation, (b_node, b_value), w, b, gamma, beta, 1e-5, True, True)
        assert out is not None and trained is not None, "a sparse first-layer entry declined"
        return [update, out, trained[1]]

    args = [_t(g[k]) for k in ("dst", "src", "rel")] + [_t(a) for a in (relation, b_node, b_value, *params)]
    update, out, out_t = MB.run_guarded(call, *args, modules=("functional", "relcsr"), widest_row=256 * Q, what="first-layer fills")
    rows = _t(reached)
    update = update.view(n, Q, 64)
    assert np.array_equal(update[rows].cpu().numpy(), want_update[:m]) and bool(update[-1, -1].any())
    untouched = torch.ones(n, dtype=torch.bool, device=_dev())
    untouched[rows] = False
    assert not bool(update[untouched].view(torch.int32).any()), "a row of the frontier's output that no edge reaches is not +0"
    for name, t in (("first_layer_forward", out), ("first_layer_train_forward", out_t)):
        assert np.array_equal(t[rows].cpu().numpy(), want_out[:m]), name
        assert bool((t[untouched].view(torch.int32) == _t(constant).view(torch.int32)).all()), name + ": a row outside the list is not the constant row"


def test_first_layer_backward_fills_an_input_gradient_past_the_fill_grid(monkeypatch):
    """``zero_fill_kernel`` behind ``ultra_first_layer_epilogue_backward_f32`` (``d_input`` of 528 036 rows), the C entry on
    outputs the test carves.  ``d_input`` and ``d_update`` at the listed rows and the parameter gradients against fp64 autograd
    of the epilogue on the listed rows plus, by linearity, ONE zero row whose upstream gradient is the column sum over all
    unlisted rows (they share that row's operands); ``d_input`` outside the list carries the bits of +0, ``d_update`` there is
    unwritten.  Bar: 2e-5 of each gradient's scale (tests/test_memory_bounds_gpu.py's case of this entry)."""
    from ultra_torchdrug_amd import RelCSR, _lib, functional as UF
    monkeypatch.setattr(UF, "SPARSE_FIRST_LAYER_MIN_ROWS", 0)
    monkeypatch.setattr(UF, "SPARSE_FIRST_LAYER_TRAIN_MAX_FRACTION", 1.0)
    n, r, Q = FILL_SHAPE
    rows = n * Q
    g, relation, b_node, b_value, params = _fill_case(6)
    dev = _dev()
    gout = torch.randn(rows, 64, generator=torch.Generator().manual_seed(rows))
    dst_t, src_t, rel_t, relation_t, node_t, value_t, *params_t = [_t(g[k]) for k in ("dst", "src", "rel")] + [_t(a) for a in (relation, b_node, b_value, *params)]
    with torch.no_grad(), GM.guarded("functional", "relcsr", widest_row=256) as guard:
        csr = RelCSR(dst_t, src_t, rel_t, None, n, n, r, piece_len=128)
        update, _, row_list, list_count = UF.first_layer_train_forward(csr, relation_t, (node_t, value_t), *params_t, 1e-5, True, True)
        listed = row_list[:int(list_count)]
        listed = listed[listed >= 0].long()
        dense = torch.zeros(n, Q, 64, device=dev).index_put((node_t.long(), torch.arange(Q, device=dev)), value_t, accumulate=True).view(rows, 64)
        # the definition, on the host: the listed rows, and one zero row for all the others
        at = listed.cpu()
        d_l, u_l = dense[listed].cpu(), update.view(rows, 64)[listed].cpu()
        pre = _epilogue_chain(torch.cat([d_l, torch.zeros(1, 64)]), torch.cat([u_l, torch.zeros(1, 64)]), params, torch.zeros(len(at) + 1, 64),
                              torch.float64)[1]
        assert float(pre[-1].abs().min()) > 1e-4, "the constant row sits on the relu's kink"
        gout[at[(pre[:-1].abs() < 1e-4).any(dim=-1)]] = 0.0                      # relu is not differentiable at 0
        unlisted = torch.ones(rows, dtype=torch.bool)
        unlisted[at] = False
        rest = gout.double()[unlisted].sum(dim=0, keepdim=True)
        want, aten = (_epilogue_chain(torch.cat([d_l, torch.zeros(1, 64)]), torch.cat([u_l, torch.zeros(1, 64)]), params,
                                      torch.cat([gout[at].double(), rest]), dtype) for dtype in (torch.float64, torch.float32))
        gout_t = gout.to(dev)
        grads = [guard.carve((rows, 64), torch.float32, dev), guard.carve((rows, 64), torch.float32, dev),
                 guard.carve((64, 128), torch.float32, dev)] + [guard.carve((64,), torch.float32, dev) for _ in range(3)]
        ws = UF.torch.empty(int(_lib.load().ultra_first_layer_epilogue_backward_workspace(0, row_list.numel())) // 4, dtype=torch.float32,
                            device=dev)
        _lib.launch(dev, "ultra_first_layer_epilogue_backward_f32", dense, update, gout_t, row_list, list_count, row_list.numel(),
                    *UF._epilogue(*params_t, 1e-5, True, True), *grads, ws, ws.numel() * 4, rows)
        guard.check()
    assert 0 < listed.numel() < rows and int(listed.max()) == rows - 1
    d_input, d_update = grads[0], grads[1]
    _held(d_input[listed], want[2][:-1], aten[2][:-1], "d_input at the listed rows", floor=1e-6)
    _held(d_update[listed], want[3][:-1], aten[3][:-1], "d_update at the listed rows", floor=1e-6)
    off = unlisted.to(dev)
    assert not bool(d_input[off].view(torch.int32).any()), "d_input outside the list is not +0"
    assert bool((d_update[off].view(torch.int32) == GM._signed(GM.POISON_F32, 32)).all()), "d_update was written outside the list"
    MB.assert_no_poison([d_input] + grads[2:], "ultra_first_layer_epilogue_backward_f32")
    for name, grad, w, a in zip(("d_weight", "d_bias", "d_ln_weight", "d_ln_bias"), grads[2:], want[4:], aten[4:]):
        _held(grad.view(w.shape), w, a, name + " over 528 036 rows", floor=1e-6)


def test_combine_backward_on_listed_tiles_fills_past_the_fill_grid():
    """``zero_fill_kernel`` behind ``ultra_combine_backward_fused_f32`` with a tile list (the last layer's backward: the upstream
    gradient is zero outside the candidates' tiles): ``d_input`` and ``d_update`` of 528 036 rows are zero-filled, then the
    listed tiles written -- the first, the last (4 rows) and 37 between.  fp64 autograd of the epilogue on the listed tiles' rows
    at 2e-5 of each gradient's scale; every other row carries the bits of +0."""
    from ultra_torchdrug_amd import functional as UF
    n, _, Q = FILL_SHAPE
    rows = n * Q
    n_tiles = trips(rows, 32)
    assert rows * 16 > CAPS["zero_fill_clamp_binds"] and rows % 32 == 4
    rng = np.random.default_rng(rows)
    tiles = np.unique(np.concatenate([[0, n_tiles - 1, CAPS["zero_fill"] * 8 // 16 // 32], rng.integers(0, n_tiles, 37)])).astype(np.int32)
    tile_list = np.full(len(tiles) + 5, -1, dtype=np.int32)
    tile_list[:len(tiles)] = tiles
    at = (tiles[:, None].astype(np.int64) * 32 + np.arange(32)).reshape(-1)
    at = torch.from_numpy(at[at < rows])
    _, _, _, _, params, _ = MB._layer_operands(9, 8, 3, 2)
    gen = torch.Generator().manual_seed(rows)
    x = torch.randn(rows, 64, generator=gen)                       # input and update: the same rows (they are only read)
    gout = torch.zeros(rows, 64)
    gout[at] = torch.randn(len(at), 64, generator=gen)
    pre = _epilogue_chain(x[at], x[at], params, gout[at], torch.float64)[1]
    gout[at[(pre.abs() < 1e-4).any(dim=-1)]] = 0.0                 # relu is not differentiable at 0
    want, aten = (_epilogue_chain(x[at], x[at], params, gout[at], dtype) for dtype in (torch.float64, torch.float32))
    dev = _dev()
    x_d, gout_d, params_d = x.to(dev), gout.to(dev), [_t(p) for p in params]
    with torch.no_grad(), GM.guarded("functional") as guard:
        grads = UF._epilogue_gradients(x_d, x_d, True)
        UF._combine_backward_fused(x_d, x_d, UF._epilogue(*params_d, 1e-5, True, True), gout_d, None, grads, _t(tile_list))
        guard.check()
        assert len(guard.records) >= 7
    listed = at.to(dev)
    off = torch.ones(rows, dtype=torch.bool, device=dev)
    off[listed] = False
    for name, grad, w, a in zip(("d_input", "d_update"), grads[:2], want[2:4], aten[2:4]):
        assert not GM.has_poison(grad) and not bool(grad[off].view(torch.int32).any()), name + " outside the listed tiles is not +0"
        _held(grad[listed], w, a, name + " at the listed tiles", floor=1e-6)
    for name, grad, w, a in zip(("d_weight", "d_bias", "d_ln_weight", "d_ln_bias"), grads[2:], want[4:], aten[4:]):
        _held(grad.view(w.shape), w, a, name + " from the listed tiles", floor=1e-6)


# ==================================================================================================== weight gradients
def test_weight_gradients_take_a_third_pass():
    """``weight_grad_kernel`` and ``weight_grad_blocks_kernel``: one wave per edge over at most 8 192 workgroups of 4 -- more than
    65 573 edges are two passes and a ragged third.  (The rotate forms are held past one pass by the ``wrap`` cases of
    tests/test_rotate_edge_grad_gpu.py; no default test took these two past 32 768 edges.)  ``F = 64``, sum and max, grid
    operands: the fp64 definition of tests/test_exact_grid_gpu.py, entry for entry, per block on that block's columns alone."""
    import exact_grid as XG
    import test_exact_grid_gpu as EG
    from ultra_torchdrug_amd import functional as UF
    name = "caps_edges"
    EG.GRAPHS[name] = (dict(n_edge=65_700, unique=True), 9000, 5, 64, True)
    csr = EG._csr(name)
    per_trip = CAPS["weight_grad"]
    assert trips(csr.n_edges, per_trip) >= 3 and csr.n_edges % per_trip % 4 != 0, csr.n_edges
    g = EG._graph(name)
    relation, x, grad = EG._inputs(name)
    for s in ("add", "max"):
        want = EG._definition(name, s, "mul")
        assert np.abs(want[3][2 * per_trip:]).max() > 0 and np.abs(want[3][per_trip:2 * per_trip]).max() > 0
        out = UF.rspmm_forward(csr, _t(relation), _t(x), s, "mul")
        assert EG._same(out, want[0])
        d_w = MB.run_guarded(lambda rl, xi, o, gr: UF.rspmm_backward_weight(csr, rl, xi, o, gr, s, "mul"), _t(relation), _t(x), out, _t(grad),
                             what="rspmm_backward_weight " + s)
        assert d_w.shape == (csr.n_edges,) and EG._same(d_w, want[3]), s
        blocks = MB.run_guarded(lambda rl, xi, o, gr: UF.rspmm_backward_weight_blocks(csr, rl, xi, o, gr, s, "mul", 32), _t(relation), _t(x),
                                out, _t(grad), what="rspmm_backward_weight_blocks " + s)
        per_block = np.stack([XG.definition(g["dst"], g["src"], g["rel"], g["w"], relation[:, c:c + 32], x[:, c:c + 32], grad[:, c:c + 32],
                                            9000, s, "mul")[3] for c in (0, 32)])
        assert blocks.shape == (2, csr.n_edges) and EG._same(blocks, per_block), s

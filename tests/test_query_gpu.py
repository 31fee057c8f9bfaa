"""MI355X: logical queries on the device -- ``ultra_set_boundary_f32`` against the numpy restatement of its contract
(tests/query_definition.py) bit for bit on both store widths, captured into a hipGraph, ``TransferNBFNet.project`` against the
fp64 ATen definition, column independence, and the 14 query structures against the hand evaluator on the device's own tensors.

The untrained models give nearly flat memberships, so the cuts are ``max_sources`` (a row's own K-th value) or floors taken from
the rows themselves, and every test with a cut asserts ``0 < kept < N``."""
import numpy as np
import pytest
import torch

from query_definition import SET_PROJECTIONS, SHAPES, first_hop, hand_answers, query_ids, set_boundary_numpy, special_members
from sampled_graphs import small_task, wide_graph
from topk_definition import same_bits

pytestmark = pytest.mark.gpu


def _dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _check_kernel(member, query, floor, stride_pad=0, misalign=False):
    """``functional.set_boundary`` on device copies of the host tensors against the numpy definition: boundary bits and counts.
    ``stride_pad``: the memberships are a view of a matrix that many columns wider; ``misalign``: the query vectors start 4
    bytes past a 16-byte boundary (the 4-byte stores)."""
    from ultra_torchdrug_amd import functional as UF
    dev = _dev()
    n_query, n_node = member.shape
    dim = query.shape[1]
    wide = torch.full((n_query, n_node + stride_pad), 0.75, device=dev)
    wide[:, :n_node] = member.to(dev)
    member_d = wide[:, :n_node]
    if misalign:
        flat = torch.zeros(n_query * dim + 4, device=dev)
        query_d = flat[1:1 + n_query * dim].view(n_query, dim)
        query_d.copy_(query.to(dev))
        assert query_d.data_ptr() % 16 == 4 and query_d.is_contiguous()
    else:
        query_d = query.to(dev)
    floor_d = None if floor is None else floor.to(dev)
    want, want_count = set_boundary_numpy(member.numpy(), query.numpy(), None if floor is None else floor.numpy())
    got, count = UF.set_boundary(member_d, query_d, floor_d, with_count=True)
    assert got.dtype == torch.float32 and tuple(got.shape) == want.shape and count.dtype == torch.int32
    what = (n_query, n_node, dim, floor is None, stride_pad, misalign)
    assert np.array_equal(count.cpu().numpy(), want_count), what
    assert same_bits(got.cpu().numpy(), want), what
    alone = UF.set_boundary(member_d, query_d, floor_d)
    assert torch.equal(alone.view(torch.int32), got.view(torch.int32)), what
    return want_count


@pytest.mark.parametrize("dim", [64, 6])
@pytest.mark.parametrize("n_node", [1, 63, 64, 65, 1031])
def test_kernel_equals_the_numpy_definition_bit_for_bit(n_node, dim):
    for n_query in (1, 3, 16, 33):
        member, query, floor = special_members(n_query, n_node, seed=100 * n_node + n_query, dim=dim)
        for f in (None, floor):
            for pad in (0, 5):
                kept = _check_kernel(member, query, f, stride_pad=pad)
        if n_node >= 63:
            assert 0 < kept[0] < n_node and (n_query < 3 or kept[2] == 0)          # the floor cuts, and row 2 is empty
    if dim == 64:                                                                   # the 4-byte stores at the 16-byte width
        member, query, floor = special_members(3, n_node, seed=n_node, dim=dim)
        _check_kernel(member, query, floor, misalign=True)


@pytest.mark.parametrize("n_query,dim", [(2, 64), (33, 6)])
def test_kernel_on_a_long_row(n_query, dim):
    """70 001 nodes: 1 094 tiles and a last tile of 49 nodes; with 33 queries 3 282 work items, more than the grid holds, so
    blocks take several items."""
    member, query, floor = special_members(n_query, 70_001, seed=7, dim=dim)
    kept = _check_kernel(member, query, floor, stride_pad=3)
    assert 0 < kept[0] < 70_001
    _check_kernel(member, query, None)


def test_set_boundary_captured_into_a_hipgraph():
    from ultra_torchdrug_amd import functional as UF
    dev = _dev()
    first, query, floor = special_members(5, 1031, seed=1, dim=64)
    second = special_members(5, 1031, seed=2, dim=64)[0]
    third = second.flip(1).contiguous()
    static, query_d, floor_d = first.to(dev), query.to(dev), floor.to(dev)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        UF.set_boundary(static, query_d, floor_d, with_count=True)               # warm-up: the outputs enter the allocator's cache
    torch.cuda.current_stream().wait_stream(side)
    captured = torch.cuda.CUDAGraph()
    with torch.cuda.graph(captured, stream=side):
        boundary, count = UF.set_boundary(static, query_d, floor_d, with_count=True)
    for member in (first, second, third):
        static.copy_(member.to(dev))
        captured.replay()
        torch.cuda.synchronize()
        want, want_count = set_boundary_numpy(member.numpy(), query.numpy(), floor.numpy())
        assert np.array_equal(count.cpu().numpy(), want_count) and same_bits(boundary.cpu().numpy(), want)
        eager = UF.set_boundary(member.to(dev), query_d, floor_d, with_count=True)
        assert torch.equal(eager[1], count) and torch.equal(eager[0].view(torch.int32), boundary.view(torch.int32))


# ------------------------------------------------------------------------------------------------ model level
@pytest.fixture(scope="module")
def wide64():
    """The 64-wide two-layer model on ``wide_graph()``: the fused epilogue and the fused all-entity score head."""
    from ultra_torchdrug_amd.task import build_ultra
    graph = wide_graph()
    torch.manual_seed(5)
    task = build_ultra(graph.num_relation, hidden_dims=(64,) * 2, rel_layers=2, num_negative=8, full_batch_eval=True)
    task.preprocess(graph)
    return task.eval().to(_dev())


@pytest.fixture(scope="module")
def small16():
    return small_task(wide_graph()).to(_dev())


def _bars(mine, aten, truth, what):
    scale = float(truth.abs().max())
    e_hip, e_aten = float((mine.double() - truth).abs().max()), float((aten.double() - truth).abs().max())
    print("%s: HIP %.3g, ATen fp32 %.3g away from the fp64 definition (scale %.3g)" % (what, e_hip, e_aten, scale))
    assert e_hip <= 4 * e_aten + 1e-5 * scale, (what, e_hip, e_aten, scale)
    assert e_hip <= 2e-4 * scale, (what, e_hip, scale)


def test_project_is_within_rounding_of_the_fp64_definition(wide64):
    from aten_definition import aten_definition
    task, dev = wide64, _dev()
    anchors, relations = (x.to(dev) for x in query_ids("2p", 4, 300, 10, seed=3))
    rel = relations[:, 1]
    with torch.no_grad():
        member = first_hop(task, anchors[:, 0], relations[:, 0])
        floor = torch.topk(member, 16, dim=1).values[:, -1].contiguous()
        kept = (member >= floor[:, None]).sum(1)
        assert bool(((kept > 0) & (kept < 300)).all()), kept.tolist()

        def run(member, floor):
            return task.model.project(task.fact_graph, task.relation_representations(rel % 5), member, rel, floor)

        mine, count = run(member, floor)
        assert torch.equal(count.long(), kept) and mine.dtype == torch.float32 and mine.shape == (4, 300)
        with aten_definition(task):
            aten = run(member, floor)[0]
        with aten_definition(task, double=True):
            truth, count64 = run(member, floor)
            assert truth.dtype == torch.float64 and torch.equal(count64.long(), kept)
        _bars(mine, aten, truth, "project of cut sets")

        # one-hot members of weight 1.0: the fp64 predict of the same queries
        anchor = anchors[:, 0]
        onehot = torch.zeros(4, 300, device=dev)
        onehot[torch.arange(4, device=dev), anchor] = 1.0
        mine, count = run(onehot, None)
        assert count.tolist() == [1] * 4
        head = rel >= 5
        zero = torch.zeros_like(anchor)
        batch = torch.stack([torch.where(head, zero, anchor), torch.where(head, anchor, zero), rel % 5], dim=1)
        pick = (torch.arange(4, device=dev), head.long())
        with aten_definition(task):
            aten = task.predict(batch)[pick]
        with aten_definition(task, double=True):
            truth = task.predict(batch)[pick]
            assert truth.dtype == torch.float64
            # in fp64 the two are one computation (0.0 on the host); the device's scatter sums add in any order
            assert float((run(onehot, None)[0] - truth).abs().max()) <= 1e-12 * float(truth.abs().max())
        _bars(mine, aten, truth, "project of one-hot sets against predict")
        single = task.model.score_all_entities(task.fact_graph, task.relation_representations(rel % 5), anchor, rel)
        print("one-hot project against score_all_entities on the device: max |difference| %.3g"
              % float((mine - single).abs().max()))


def test_sets_are_independent_columns(wide64):
    from ultra_torchdrug_amd import engine
    task, dev = wide64, _dev()
    anchors, relations = (x.to(dev) for x in query_ids("3p", 5, 300, 10, seed=11))
    member = first_hop(task, anchors[:, 0], relations[:, 0])
    together = task.project(member, relations[:, 1], max_sources=20)
    assert together.shape == (5, 300) and together.dtype == torch.float32
    for q in range(5):
        alone = task.project(member[q:q + 1], relations[q:q + 1, 1], max_sources=20)
        assert torch.equal(alone[0], together[q]), q
    got = engine.answer_query(task, "3p", anchors, relations, k=10, batch_size=2, max_sources=20)
    chunks = [task.answer_query("3p", anchors[i:i + 2], relations[i:i + 2], k=10, max_sources=20) for i in range(0, 5, 2)]
    assert got[0].shape == (5, 10) and torch.equal(got[0], torch.cat([c[0] for c in chunks]))
    assert torch.equal(got[1], torch.cat([c[1] for c in chunks]))
    whole = task.answer_query("3p", anchors, relations, k=10, max_sources=20)
    assert torch.equal(whole[0], got[0]) and torch.equal(whole[1], got[1])


def _recorded_counts(task, monkeypatch):
    seen = []
    inner = task.model.project

    def project(*args, **kwargs):
        score, count = inner(*args, **kwargs)
        seen.append(count.clone())
        return score, count

    monkeypatch.setattr(task.model, "project", project)
    return seen


@pytest.mark.parametrize("width", [64, 16])
@pytest.mark.parametrize("name", list(SHAPES))
def test_whole_queries_equal_the_hand_evaluator(wide64, small16, name, width, monkeypatch):
    task, dev = (wide64 if width == 64 else small16), _dev()
    anchors, relations = (x.to(dev) for x in query_ids(name, 3, 300, 10, seed=len(name) + 17 * list(SHAPES).index(name)))
    seen = _recorded_counts(task, monkeypatch)
    entities, membership = task.answer_query(name, anchors, relations, k=10, max_sources=12)
    assert len(seen) == SET_PROJECTIONS[name]
    assert all(bool(((c > 0) & (c < 300)).all()) for c in seen), [c.tolist() for c in seen]
    want_entities, want_membership = hand_answers(task, name, anchors, relations, 10, max_sources=12)
    assert entities.dtype == torch.int64 and membership.dtype == torch.float32 and entities.shape == membership.shape == (3, 10)
    assert entities.device == want_entities.device
    assert torch.equal(entities, want_entities) and torch.equal(membership, want_membership)
    assert (entities >= 0).all() and (membership > 0).all()


def test_an_empty_set_has_no_answers_on_the_device(wide64):
    task, dev = wide64, _dev()
    anchors, relations = (x.to(dev) for x in query_ids("2p", 3, 300, 10, seed=5))
    member = first_hop(task, anchors[:, 0], relations[:, 0]).clone()
    member[1] = member[1] * 0.5
    threshold = float(member[1].max()) + 1e-3
    assert float(member[0].max()) > threshold and float(member[2].max()) > threshold
    out = task.project(member, relations[:, 1], threshold=threshold)
    assert not out[1].any() and (out[0] > 0).all() and (out[2] > 0).all()
    entities, membership = task.answer_query("2p", anchors, relations, k=10, threshold=0.999)
    assert (entities == -1).all() and not membership.any()


def test_refusals_raise_before_any_launch(wide64):
    from ultra_torchdrug_amd import functional as UF
    task, dev = wide64, _dev()
    member, query, floor = (x.to(dev) for x in special_members(4, 70, seed=2, dim=8))
    UF.set_boundary(member, query, floor)
    wide = torch.zeros(4, 140, device=dev)
    for bad in (dict(member=member.double()), dict(query=query.double()), dict(member=member[0]), dict(query=query[:3]),
                dict(member=wide[:, ::2]), dict(member=wide.reshape(-1).as_strided((4, 70), (35, 1))), dict(floor=floor[:3]),
                dict(floor=floor.double()), dict(member=member[:, :0]), dict(query=query[:, :0]), dict(query=query.cpu()),
                dict(floor=floor.cpu()), dict(member=member[:0], query=query[:0], floor=None)):
        with pytest.raises(RuntimeError):
            UF.set_boundary(**dict(dict(member=member, query=query, floor=floor), **bad))
    anchors, relations = (x.to(dev) for x in query_ids("2p", 2, 300, 10, seed=1))
    for bad in (0, 129):
        with pytest.raises(ValueError):
            task.answer_query("2p", anchors, relations, max_sources=bad)
    with pytest.raises(ValueError):
        task.answer_query("2p", anchors, relations + 10)
    with pytest.raises(ValueError):
        task.answer_query((("e", ("r",)),), anchors, relations)
    # the C entry itself: sizes and null pointers
    from ultra_torchdrug_amd import _lib
    out = torch.empty(70, 4, 8, device=dev)
    good = [member, 4, 70, 70, floor, query, 8, out, None]
    _lib.launch(dev, "ultra_set_boundary_f32", *good)
    for at, value in ((1, 0), (2, 0), (6, 0), (3, 69), (0, None), (5, None), (7, None)):
        args = list(good)
        args[at] = value
        with pytest.raises(RuntimeError, match="shape"):
            _lib.launch(dev, "ultra_set_boundary_f32", *args)
    torch.cuda.synchronize()

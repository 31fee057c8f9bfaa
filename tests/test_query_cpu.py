"""Logical queries without a GPU: the structure parser, ``functional.dense_set_boundary`` against the numpy restatement of the
boundary contract (tests/query_definition.py), ``task.project`` / ``task.answer_query`` / ``engine.answer_query`` on a small
model against the hand evaluator, and the binding's surface.

The untrained test model gives nearly flat memberships (every ``p`` of ``small_task(wide_graph())`` lies between 0.76 and 0.80),
so a fixed threshold keeps everything or nothing: the cuts used here are ``max_sources`` (the row's own K-th value) and, for the
empty-set rule, a threshold above the row's maximum; every test with a cut asserts ``0 < kept < N``."""
import numpy as np
import pytest
import torch

from query_definition import SET_PROJECTIONS, SHAPES, hand_answers, query_ids, set_boundary_numpy, special_members
from sampled_graphs import small_task, wide_graph
from topk_definition import same_bits

P1, P2, N1 = ("e", ("r",)), ("e", ("r", "r")), ("e", ("r", "n"))
TUPLES = {"1p": P1, "2p": P2, "3p": ("e", ("r", "r", "r")), "2i": (P1, P1), "3i": (P1, P1, P1), "ip": ((P1, P1), ("r",)),
          "pi": (P2, P1), "2u": (P1, P1, ("u",)), "up": ((P1, P1, ("u",)), ("r",)), "2in": (P1, N1), "3in": (P1, P1, N1),
          "inp": ((P1, N1), ("r",)), "pin": (P2, N1), "pni": (("e", ("r", "r", "n")), P1)}


@pytest.fixture(scope="module")
def small():
    return small_task(wide_graph())


def test_parser_takes_the_14_structures_and_rejects_malformed_tuples():
    from ultra_torchdrug_amd.task import QUERY_STRUCTURES, parse_query_structure
    assert list(QUERY_STRUCTURES) == list(TUPLES) == list(SHAPES) and len(TUPLES) == 14
    for name, spelled in TUPLES.items():
        assert QUERY_STRUCTURES[name] == spelled, name
        by_name, by_tuple = parse_query_structure(name), parse_query_structure(spelled)
        assert by_name == by_tuple and by_name[1:] == SHAPES[name], name
    assert parse_query_structure("ip")[0] == ("ops", ("i", [("e", ("r",)), ("e", ("r",))]), ("r",))
    assert parse_query_structure("2u")[0][0] == "u" and parse_query_structure("pni")[0][1][0] == ("e", ("r", "r", "n"))
    # beyond the 14: ops with a complement behind a union of three
    assert parse_query_structure(((P1, P2, N1, ("u",)), ("r", "n")))[1:] == (3, 5)
    for bad in ("4p", (), ("e",), ("e", ()), ("e", ("n",)), ("e", ("r", "x")), ("e", "r"), ("x", ("r",)), (P1,), (P1, ("u",)),
                (P1, ("r",)), ((P1, P1), ()), (P1, P1, ("u", "u")), (P1, "e"), ["e", ("r",)], (P1, 3), ("e", ("r",), ("r",)), None):
        with pytest.raises(ValueError):
            parse_query_structure(bad)


@pytest.mark.parametrize("n_query,n_node,dim", [(1, 1, 6), (3, 65, 64), (5, 300, 16), (2, 1031, 6)])
def test_dense_set_boundary_equals_the_numpy_definition(n_query, n_node, dim):
    from ultra_torchdrug_amd import functional as UF
    member, query, floor = special_members(n_query, n_node, seed=n_node, dim=dim)
    for f in (None, floor):
        want, want_count = set_boundary_numpy(member.numpy(), query.numpy(), None if f is None else f.numpy())
        got, count = UF.set_boundary(member, query, f, with_count=True)                  # CPU tensors: the dense twin
        assert got.dtype == torch.float32 and got.shape == (n_node, n_query, dim) and count.dtype == torch.int32
        assert same_bits(got.numpy(), want) and np.array_equal(count.numpy(), want_count), (n_query, n_node, dim, f is None)
        assert same_bits(UF.dense_set_boundary(member, query, f).numpy(), want)
        # row 0 of the query holds inf and NaN: the rows that are not kept are +0.0 bits all the same
        gone = ~(member[0] > 0) if f is None else ~((member[0] > 0) & (member[0] >= f[0]))
        assert gone.any() and not got[gone, 0].view(torch.int32).any()
    if n_node >= 65:
        kept = set_boundary_numpy(member.numpy(), query.numpy(), floor.numpy())[1]
        assert 0 < kept[0] < n_node and (n_query < 3 or kept[2] == 0)
        ties = int((member[0] == floor[0]).sum())
        assert ties > 1 and ties == int(((member[0] >= floor[0]).sum() - (member[0] > floor[0]).sum()))       # all kept
    # in the dtype of the query: the fp64 definition
    assert UF.dense_set_boundary(member, query.double(), floor).dtype == torch.float64


def test_one_hot_member_of_weight_one_is_bellmanfords_own_boundary(small):
    from ultra_torchdrug_amd import functional as UF
    task, model = small, small.model
    h = torch.tensor([11, 0, 299, 11])
    r = torch.tensor([1, 7, 4, 9])
    with torch.no_grad():
        rel = task.relation_representations(r % 5)
        model.query = rel[0]
        for conv in model.layers:
            conv.relation = rel[0]
        graph = model._undirected(task.fact_graph)
        model.bellmanford(graph, h, r, want_feature=False)
        want, query = graph.boundary.clone(), graph.query.clone()
        assert graph.boundary_sparse is not None
        member = torch.zeros(4, 300)
        member[torch.arange(4), h] = 1.0
        assert same_bits(UF.set_boundary(member, query).numpy(), want.numpy())
        _, count = model.project(task.fact_graph, rel, member, r)
        assert same_bits(graph.boundary.numpy(), want.numpy()) and graph.boundary_sparse is None and count.tolist() == [1] * 4


def _recorded_counts(task, monkeypatch):
    """Every ``model.project`` call of the task appends its per-query kept counts here."""
    seen = []
    inner = task.model.project

    def project(*args, **kwargs):
        score, count = inner(*args, **kwargs)
        seen.append(count.clone())
        return score, count

    monkeypatch.setattr(task.model, "project", project)
    return seen


@pytest.mark.parametrize("name", list(SHAPES))
def test_answer_query_equals_the_hand_evaluator(small, name, monkeypatch):
    task = small
    anchors, relations = query_ids(name, 3, 300, 10, seed=len(name) + 17 * list(SHAPES).index(name))
    seen = _recorded_counts(task, monkeypatch)
    entities, membership = task.answer_query(name, anchors, relations, k=10, max_sources=12)
    assert len(seen) == SET_PROJECTIONS[name]
    assert all(bool(((c > 0) & (c < 300)).all()) for c in seen), [c.tolist() for c in seen]      # the cut cuts: not vacuous
    want_entities, want_membership = hand_answers(task, name, anchors, relations, 10, max_sources=12)
    assert entities.dtype == torch.int64 and membership.dtype == torch.float32 and entities.shape == membership.shape == (3, 10)
    assert torch.equal(entities, want_entities) and same_bits(membership.numpy(), want_membership.numpy())
    assert (entities >= 0).all() and (membership > 0).all() and (membership[:, :-1] >= membership[:, 1:]).all()
    # the tuple form is the same query
    again = task.answer_query(TUPLES[name], anchors, relations, k=10, max_sources=12)
    assert torch.equal(again[0], entities) and torch.equal(again[1], membership)


def test_1p_memberships_are_the_sigmoid_of_predict(small):
    task = small
    anchor = torch.tensor([11, 9, 299, 42])
    rel = torch.tensor([1, 3, 4, 0])
    with torch.no_grad():
        tails = torch.sigmoid(task.predict(torch.stack([anchor, torch.zeros_like(anchor), rel], dim=1))[:, 0])
        heads = torch.sigmoid(task.predict(torch.stack([torch.zeros_like(anchor), anchor, rel], dim=1))[:, 1])
    for want, relations in ((tails, rel), (heads, rel + 5)):
        entities, membership = task.answer_query("1p", anchor[:, None], relations[:, None], k=128)
        assert same_bits(membership.numpy(), want.gather(1, entities).numpy())
        order = torch.sort(want, dim=1, descending=True, stable=True).indices[:, :128]
        assert torch.equal(entities, order)
    assert 0.7 < float(tails.min()) and float(tails.max()) < 0.85           # the flat memberships the module docstring speaks of


def test_an_empty_set_has_no_answers(small, monkeypatch):
    task = small
    anchors, relations = query_ids("2p", 3, 300, 10, seed=5)
    from query_definition import first_hop
    p = first_hop(task, anchors[:, 0], relations[:, 0])
    # a threshold above row 1's maximum but inside the other rows' range is not guaranteed to exist on flat memberships: cut
    # row 1 alone by handing `project` a member matrix whose row 1 lies below the threshold
    member = p.clone()
    member[1] = member[1] * 0.5
    threshold = float(member[1].max()) + 1e-3
    seen = _recorded_counts(task, monkeypatch)
    out = task.project(member, relations[:, 1], threshold=threshold)
    kept = seen[-1].tolist()
    assert kept[1] == 0 and 0 < kept[0] <= 300 and 0 < kept[2] <= 300
    assert not out[1].any() and (out[0] > 0).all() and (out[2] > 0).all()
    # rows are columns of the kernels: the other rows do not notice
    alone = task.project(member[[0, 2]], relations[[0, 2], 1], threshold=threshold)
    assert alone.shape == (2, 300) and float((alone - out[[0, 2]]).abs().max()) < 1e-5
    # a whole query: above every membership, the intermediate set is empty and nothing is listed
    entities, membership = task.answer_query("2p", anchors, relations, k=10, threshold=0.99)
    assert (entities == -1).all() and not membership.any()
    assert all(c == 0 for c in seen[-1].tolist())
    # ... and the complement of nothing is everything, at membership 1
    entities, membership = task.answer_query((("e", ("r", "r", "n")), ("e", ("r",))), torch.cat([anchors, anchors], 1)[:, :2],
                                             torch.cat([relations, relations[:, :1]], 1), k=3, threshold=0.99)
    assert (entities >= 0).all() and (membership > 0.7).all()


def test_cut_arguments_are_checked(small):
    from ultra_torchdrug_amd import engine
    task = small
    anchors, relations = query_ids("2p", 2, 300, 10, seed=1)
    member = torch.full((2, 300), 0.5)
    for bad in (0, 129, -1):
        with pytest.raises(ValueError):
            task.project(member, relations[:, 0], max_sources=bad)
        with pytest.raises(ValueError):
            task.answer_query("2p", anchors, relations, max_sources=bad)
        with pytest.raises(ValueError):
            engine.answer_query(task, "2p", anchors, relations, max_sources=bad)
    task.project(member, relations[:, 0], max_sources=1)
    task.project(member, relations[:, 0], max_sources=128)
    for bad in (dict(anchors=anchors[:, :0]), dict(relations=relations[:, :1]), dict(anchors=anchors.int()),
                dict(anchors=torch.tensor([[300], [0]])), dict(relations=torch.tensor([[0, 10], [0, 0]])),
                dict(relations=torch.tensor([[0, -1], [0, 0]])), dict(k=0), dict(k=129)):
        with pytest.raises(ValueError):
            task.answer_query(**dict(dict(structure="2p", anchors=anchors, relations=relations), **bad))
    with pytest.raises(ValueError):
        task.project(member[:, :299], relations[:, 0])
    with pytest.raises(ValueError):
        task.project(member, torch.tensor([0, 10]))
    with pytest.raises(TypeError):
        engine.answer_query(task, "2p", anchors, relations, cutoff=1)


def test_engine_answer_query_in_chunks_equals_task_answer_query_chunk_by_chunk(small):
    from ultra_torchdrug_amd import engine
    task = small
    for name in ("3p", "pin"):
        anchors, relations = query_ids(name, 5, 300, 10, seed=23)
        got = engine.answer_query(task, name, anchors, relations, k=7, batch_size=2, max_sources=9)
        chunks = [task.answer_query(name, anchors[i:i + 2], relations[i:i + 2], k=7, max_sources=9) for i in range(0, 5, 2)]
        assert got[0].shape == (5, 7) and torch.equal(got[0], torch.cat([c[0] for c in chunks]))
        assert same_bits(got[1].numpy(), torch.cat([c[1] for c in chunks]).numpy())
    empty = engine.answer_query(task, "2i", torch.zeros(0, 2, dtype=torch.long), torch.zeros(0, 2, dtype=torch.long), k=4)
    assert empty[0].shape == empty[1].shape == (0, 4)


def test_project_is_within_rounding_of_the_fp64_definition(small):
    """The CPU route against the ATen definition in fp64, by the bars of tests/test_reference_definition_gpu.py."""
    from aten_definition import aten_definition
    from query_definition import first_hop
    task = small
    anchors, relations = query_ids("2p", 4, 300, 10, seed=3)
    member = first_hop(task, anchors[:, 0], relations[:, 0])
    cut = dict(max_sources=16)
    with torch.no_grad():
        floor = torch.topk(member, 16, dim=1).values[:, -1]
        kept = (member >= floor[:, None]).sum(1)
        assert bool(((kept > 0) & (kept < 300)).all())
        rel = task.relation_representations(relations[:, 1] % 5)
        mine = task.model.project(task.fact_graph, rel, member, relations[:, 1], floor)[0].double()
        with aten_definition(task):
            aten = task.model.project(task.fact_graph, task.relation_representations(relations[:, 1] % 5), member,
                                      relations[:, 1], floor)[0].double()
        with aten_definition(task, double=True):
            truth = task.model.project(task.fact_graph, task.relation_representations(relations[:, 1] % 5), member,
                                       relations[:, 1], floor)[0]
            assert truth.dtype == torch.float64
            same = task.project(member, relations[:, 1], **cut)
            # (fp64 scatter sums add in an order that depends on the thread count: a few ulps of 2.2e-16, not bits)
            assert same.dtype == torch.float64 and float((same - torch.sigmoid(truth)).abs().max()) <= 1e-12
            # a one-hot member of weight 1.0 is the query predict answers: in fp64 the two are one computation
            anchor, rel_q = anchors[:, 0], relations[:, 1]
            onehot = torch.zeros(4, 300)
            onehot[torch.arange(4), anchor] = 1.0
            head, zero = rel_q >= 5, torch.zeros_like(anchor)
            batch = torch.stack([torch.where(head, zero, anchor), torch.where(head, anchor, zero), rel_q % 5], dim=1)
            single = task.predict(batch)[torch.arange(4), head.long()]
            hot = task.model.project(task.fact_graph, task.relation_representations(rel_q % 5), onehot, rel_q)[0]
            assert single.dtype == hot.dtype == torch.float64
            assert float((hot - single).abs().max()) <= 1e-12 * float(single.abs().max())
    scale = float(truth.abs().max())
    e_mine, e_aten = float((mine - truth).abs().max()), float((aten - truth).abs().max())
    print("project vs fp64: route %.3g, ATen fp32 %.3g, scale %.3g" % (e_mine, e_aten, scale))
    assert e_mine <= 4 * e_aten + 1e-5 * scale and e_mine <= 2e-4 * scale


def test_binding_lists_the_entry_and_keeps_the_abi():
    from ultra_torchdrug_amd import _lib, backend, functional as UF
    assert "ultra_set_boundary_f32" in _lib.EXPORTS and _lib.ABI_VERSION == 8
    assert backend.get().set_boundary is UF.set_boundary and callable(backend.get().dense_set_boundary)


def test_set_boundary_refuses_bad_arguments():
    from ultra_torchdrug_amd import functional as UF
    member, query, floor = special_members(4, 70, seed=2, dim=8)
    UF.set_boundary(member, query, floor)
    wide = torch.zeros(4, 140)
    assert UF.set_boundary(wide[:, :70], query).shape == (70, 4, 8)                     # strided rows are fine
    for bad in (dict(member=member.double()), dict(query=query.double()), dict(member=member[0]), dict(query=query[:3]),
                dict(member=wide[:, ::2]), dict(member=wide.reshape(-1).as_strided((4, 70), (35, 1))), dict(floor=floor[:3]),
                dict(floor=floor.double()), dict(member=member[:, :0]), dict(query=query[:, :0]),
                dict(member=member[:0], query=query[:0], floor=None)):
        with pytest.raises(RuntimeError):
            UF.set_boundary(**dict(dict(member=member, query=query, floor=floor), **bad))

"""GPU tests of the one-hop edge removal (``remove_one_hop=True``, ``ultra/model.py:57-74``): ``ultra_pair_removal``
(csrc/sampler.inc) as an operator on a crafted graph, in a training step of the model, and in captured steps.

Bars: the weights the kernel writes are exact work -- every plan must EQUAL what the reference formulation gives
(``easy_edge_mask`` = ``graph.match`` with a wildcard relation, then ``reweighted``), and so must the rspmm results and a
whole training step on the two routes; against a graph from which the edges are really dropped the plans differ, hence the
order of the fp32 additions, and the bar is that of tests/test_frontier_sampler_gpu.py for the same comparison."""
import contextlib
import copy

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

N_NODE, N_REL = 257, 140


def _dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def _t(a):
    return torch.from_numpy(np.asarray(a)).to(_dev())


def _crafted_triples(triplicate):
    """~3 000 seeded random triples over 257 nodes and 140 base relations, plus
    - a hub pair (3, 200) under all 140 relations in both directions: 280 parallel edges per ordered pair once the inverses are
      added -- more than a wave and more than a 256-thread block;
    - (0, 256) under relations {0, 139}, one direction: the first and the last row of every plan, the first and last relation;
    - self loops (5, 5, 7) and (5, 5, 8);
    - ``triplicate``: one triple listed three times (coalesced into one edge of weight 3);
    - nothing between 10 and 11."""
    rng = np.random.default_rng(140)
    rand = np.stack([rng.integers(0, N_NODE, 3000), rng.integers(0, N_NODE, 3000), rng.integers(0, N_REL, 3000)], axis=1)
    rand = np.unique(rand, axis=0)
    rand = rand[~(((rand[:, 0] == 10) & (rand[:, 1] == 11)) | ((rand[:, 0] == 11) & (rand[:, 1] == 10)))]
    rels = np.arange(N_REL)
    hub = np.concatenate([np.stack([np.full(N_REL, 3), np.full(N_REL, 200), rels], axis=1),
                          np.stack([np.full(N_REL, 200), np.full(N_REL, 3), rels], axis=1)])
    fixed = np.array([[0, 256, 0], [0, 256, 139], [5, 5, 7], [5, 5, 8], [20, 21, 4]])
    triples = np.unique(np.concatenate([rand, hub, fixed]), axis=0)           # every triple once ...
    if triplicate:
        triples = np.concatenate([triples, [[20, 21, 4], [20, 21, 4]]])       # ... but this one
    return rng.permutation(triples).astype(np.int64)


def _patterns(triples, empty):
    """(3, 200) twice and (200, 3) once, the other crafted pairs, the unconnected (10, 11) and random pairs that are no edges."""
    if empty:
        return np.zeros((2, 0), dtype=np.int64)
    rng = np.random.default_rng(7)
    connected = set(map(tuple, triples[:, :2])) | set(map(tuple, triples[:, 1::-1]))
    cand = rng.integers(0, N_NODE, (400, 2))
    free = np.array([p for p in cand if tuple(p) not in connected][:300])
    assert len(free) == 300
    listed = np.array([[3, 200], [0, 256], [5, 5], [3, 200], [20, 21], [10, 11], [200, 3]])
    return rng.permutation(np.concatenate([listed, free])).T.copy()


@pytest.fixture(scope="module")
def crafted():
    """The crafted graphs, each with its graph with inverse edges (built once; the tests leave them unchanged)."""
    from ultra_torchdrug_amd.graph import Graph
    from ultra_torchdrug_amd.model import TransferNBFNet
    rng = np.random.default_rng(3)
    out = {}
    for case in ("unit", "unit_distinct", "weighted"):
        triples = _crafted_triples(triplicate=case != "unit_distinct")
        # weights on the grid k / 256, k in [1, 1024]: positive, and the three copies of the listed triple add up to the same
        # float in every order (the coalescing kernel and index_add_ need not agree on one)
        weight = _t((rng.integers(1, 1025, len(triples)) / 256.0).astype(np.float32)) if case == "weighted" else None
        graph = Graph(_t(triples), weight, num_node=N_NODE, num_relation=N_REL)
        out[case] = (triples, graph, graph.undirected(add_inverse=True))
    out["model"] = TransferNBFNet(64, [64], num_relation=N_REL, message_func="distmult", aggregate_func="sum",
                                  remove_one_hop=True)
    return out


@pytest.mark.parametrize("empty", [False, True], ids=["listed", "empty"])
@pytest.mark.parametrize("case", ["unit", "unit_distinct", "weighted"])
def test_pair_removal_equals_mask_and_reweight_path(crafted, case, empty):
    """``Graph.without_pairs`` (one native call) against ``easy_edge_mask`` + ``reweighted``: the weights of all three plans, the
    marked words where the plans carry them, and forward, d_relation and d_input of the rspmm; then against a graph built
    without those edges.  ``unit``: the listed triple makes one coalesced weight 3, so the weights route; ``unit_distinct``:
    every weight is 1 and the packed words leave bit 31 free, so the marks route; ``weighted``: the weights route."""
    from ultra_torchdrug_amd import functional as UF
    from ultra_torchdrug_amd.graph import Graph
    dev = _dev()
    triples, graph, und = crafted[case]
    h, t = (_t(x) for x in _patterns(triples, empty))
    if empty:
        keep = torch.ones(graph.num_edge, dtype=torch.bool, device=dev)
    else:
        keep = crafted["model"].easy_edge_mask(graph, h, t, torch.zeros_like(h))
        gone = graph.edge_list[~keep]
        assert int(((gone[:, 0] == 3) & (gone[:, 1] == 200)).sum()) == N_REL == int(((gone[:, 0] == 200) & (gone[:, 1] == 3)).sum())
        assert len(gone) >= 2 * N_REL + 2 + 2 + 1
    want_graph = und.reweighted(und.edge_weight * keep.repeat_interleave(2))
    got_graph = UF.remove_pairs(und, h, t)
    E = und.relcsr.n_edges
    marked_plans = 0
    for plan in ("fwd", "by_src", "by_rel"):
        a, b, base = getattr(got_graph.relcsr, plan), getattr(want_graph.relcsr, plan), getattr(und.relcsr, plan)
        assert torch.equal(a.weight[:E], b.weight[:E]), plan
        assert torch.equal(a.weight[E:], torch.ones_like(a.weight[E:])), plan
        assert a.chunks.data_ptr() == base.chunks.data_ptr()                   # plans shared, not rebuilt
        if a.packed_dead is not None:
            marked_plans += 1
            assert a.struct.packed_dead == a.packed_dead.data_ptr()
            assert torch.equal((a.packed_dead[:E].long() & 0x80000000) != 0, a.weight[:E] == 0), plan
            assert torch.equal(a.packed_dead.long() & 0x7fffffff, base.packed.long() & 0xffffffff), plan
    assert marked_plans == (3 if case == "unit_distinct" else 0)
    if not empty:
        assert int((got_graph.relcsr.fwd.weight[:E] == 0).sum()) == 2 * int((~keep).sum()) - (4 if case != "unit_distinct" else 0)
    F = 128
    gen = torch.Generator(device=dev).manual_seed(2)
    relation = torch.randn(2 * N_REL, F, device=dev, generator=gen).requires_grad_()
    x = torch.randn(N_NODE, F, device=dev, generator=gen).requires_grad_()
    grad = torch.randn(N_NODE, F, device=dev, generator=gen)
    dropped = und.edge_list[keep.repeat_interleave(2)]
    outs = []
    for g in (got_graph, want_graph, Graph(dropped, und.edge_weight[keep.repeat_interleave(2)], N_NODE, 2 * N_REL)):
        relation.grad = x.grad = None
        out = UF.generalized_rspmm(g.relcsr, relation, x)
        out.backward(grad)
        outs.append((out.detach(), relation.grad.clone(), x.grad.clone()))
    for a, b in zip(outs[0], outs[1]):
        assert torch.equal(a, b)
    for a, b in zip(outs[0], outs[2]):                  # really removing the edges: another plan, hence another
        torch.testing.assert_close(a, b, rtol=1e-4, atol=1e-4)     # chunk / piece structure and order of fp32 additions


def test_pair_removal_ignores_ids_outside_the_graph(crafted):
    """An id outside ``[0, N)`` -- negative, N itself, beyond 2^31 (where an int32 cast would alias node 3) -- matches nothing and
    writes nothing: the same arrays as without those pairs."""
    from ultra_torchdrug_amd import functional as UF
    triples, graph, und = crafted["unit_distinct"]
    h, t = (_t(x) for x in _patterns(triples, False))
    hub = torch.tensor([3, 200], device=_dev())
    away = ~(torch.isin(h, hub) | torch.isin(t, hub))                       # the hub pair stays: an aliased id would remove it
    h, t = h[away], t[away]
    extra_h = torch.tensor([-1, N_NODE, 2 ** 32 + 3, 3, 200, -200], device=_dev())
    extra_t = torch.tensor([200, 3, 200, 2 ** 32 + 200, -3, -3], device=_dev())
    want, got = UF.remove_pairs(und, h, t), UF.remove_pairs(und, torch.cat([extra_h, h]), torch.cat([extra_t, t]))
    E = und.relcsr.n_edges
    assert 0 < int((want.relcsr.fwd.weight[:E] == 0).sum()) < 2 * N_REL
    for plan in ("fwd", "by_src", "by_rel"):
        assert torch.equal(getattr(got.relcsr, plan).weight, getattr(want.relcsr, plan).weight), plan
        assert torch.equal(getattr(got.relcsr, plan).packed_dead, getattr(want.relcsr, plan).packed_dead), plan


# ------------------------------------------------------------------------------------------------ model
def _tiny_task(seed=1024, **kwargs):
    from ultra_torchdrug_amd.data import synthetic_triples
    from ultra_torchdrug_amd.graph import Graph
    from ultra_torchdrug_amd.task import build_ultra
    triples, n, r = synthetic_triples("S-tiny", seed)
    torch.manual_seed(seed)
    task = build_ultra(r, num_negative=16, **kwargs)
    task.preprocess(Graph(torch.from_numpy(triples), num_node=n, num_relation=r))
    return task.to(_dev()).train(), triples


def _step(task, batch, negatives):
    task.zero_grad(set_to_none=True)
    task._static_negative = negatives
    try:
        loss, _ = task(batch)
        loss.backward()
    finally:
        task._static_negative = None
    grads = {k: p.grad.detach().clone() for k, p in task.named_parameters() if p.grad is not None}
    task.zero_grad(set_to_none=True)
    return loss.detach().clone(), grads


@contextlib.contextmanager
def _mask_route(model):
    """The route every ``remove_one_hop`` model took before the native one: ``_removal_by_zero_weight`` declines ``sums_only``."""
    model._removal_by_zero_weight = lambda sums_only=False: not sums_only
    try:
        yield
    finally:
        del model._removal_by_zero_weight


@contextlib.contextmanager
def _definition(task, double=False):
    """``aten_definition`` for a ``remove_one_hop`` model.  That backend accepts no tensor, so the model takes the mask route and
    hands the layers ``graph.reweighted(...)`` -- a graph made for the kernels, with ``requires_grad`` off; the definition needs
    the reference's switch to ``message`` + ``aggregate`` (``ultra/layer.py:299``) on it as on the graph it was made from."""
    from aten_definition import aten_definition
    from ultra_torchdrug_amd.graph import Graph
    real = Graph.reweighted

    def reweighted(self, edge_weight):
        out = real(self, edge_weight)
        out.requires_grad = self.requires_grad
        return out

    Graph.reweighted = reweighted
    try:
        with aten_definition(task, double=double):
            yield
    finally:
        Graph.reweighted = real


def test_one_hop_step_on_the_native_route_equals_the_mask_route_and_the_definition(monkeypatch):
    """S-tiny, B = 8, 16 strict negatives: loss and every parameter gradient of a training step whose edges go by
    ``ultra_pair_removal`` EQUAL those of the mask route, and are as close to the fp64 ATen definition (mask route on
    materialised messages, no kernel of the package) as the fp32 definition is -- the yardstick of
    tests/test_reference_definition_gpu.py."""
    from ultra_torchdrug_amd import functional as UF
    task, triples = _tiny_task(remove_one_hop=True)
    batch = _t(triples[:8])
    torch.manual_seed(5)
    negatives = task._strict_negative(*batch.t())
    assert negatives.shape == (8, 16)
    calls = []
    real = UF.remove_pairs
    monkeypatch.setattr(UF, "remove_pairs", lambda *a: calls.append(1) or real(*a))
    loss_hip, g_hip = _step(task, batch, negatives)
    assert calls == [1]                                                     # the native route ran ...
    with _mask_route(task.model):
        loss_mask, g_mask = _step(task, batch, negatives)
    assert calls == [1]                                                     # ... and the mask route did not use it
    assert torch.equal(loss_hip, loss_mask)
    assert g_hip.keys() == g_mask.keys() and len(g_hip) >= 6 * 8 + 4 + 6 * 5
    for k in g_hip:
        assert torch.equal(g_hip[k], g_mask[k]), k

    with _definition(task):
        loss_aten, g_aten = _step(task, batch, negatives)
    with _definition(task, double=True):
        loss_true, g_true = _step(task, batch, negatives)
    assert calls == [1] and loss_true.dtype == torch.float64
    assert all(p.dtype == torch.float32 for p in task.parameters())
    assert g_hip.keys() == g_aten.keys() == g_true.keys()
    loss_hip, loss_aten, loss_true = float(loss_hip), float(loss_aten), float(loss_true)
    print("loss: HIP %.9g, ATen-fp32 %.9g, fp64 %.12g" % (loss_hip, loss_aten, loss_true))
    assert abs(loss_hip - loss_true) <= 4 * abs(loss_aten - loss_true) + 1e-5 * abs(loss_true)
    worst = {}
    for k in g_true:
        s = g_true[k].abs().max().item() + 1e-12
        e_hip = (g_hip[k].double() - g_true[k]).abs().max().item()
        e_aten = (g_aten[k].double() - g_true[k]).abs().max().item()
        worst[k] = (e_hip / s, e_aten / s)
        assert e_hip <= 4 * e_aten + 5e-4 * s, "%s: HIP %.3g vs ATen-fp32 %.3g away from fp64 (scale %.3g)" % (k, e_hip, e_aten, s)
    print("one-hop step vs fp64 definition: worst relative gradient error HIP %.2e, ATen-fp32 %.2e"
          % (max(v[0] for v in worst.values()), max(v[1] for v in worst.values())))


# ------------------------------------------------------------------------------------------------ captured steps
def test_graphed_train_step_captures_the_one_hop_removal():
    """``GraphedTrainStep`` takes a ``remove_one_hop`` model: three replays give the losses, and leave the parameters, of
    ``engine.train_step`` on a deep copy fed the negatives the graph drew."""
    from ultra_torchdrug_amd import engine
    task, triples = _tiny_task(remove_one_hop=True)
    twin = copy.deepcopy(task)
    batches = [_t(triples[i:i + 8]) for i in (0, 8, 16, 24)]
    opt_g = torch.optim.AdamW(twin.parameters(), lr=1e-3)
    step = engine.GraphedTrainStep(twin, opt_g, batches[0])
    losses_g, negs = [], []
    for b in batches[1:]:
        losses_g.append(step(b)[0].item())
        negs.append(step.last_negatives.clone())
    opt_e = torch.optim.AdamW(task.parameters(), lr=1e-3)
    losses_e = []
    for b, neg in zip(batches[1:], negs):
        task._static_negative = neg                    # the graph drew its own negatives: replay them eagerly
        losses_e.append(engine.train_step(task, opt_e, b)[0].item())
    task._static_negative = None
    assert losses_g == losses_e
    for (k, a), (_, b) in zip(task.named_parameters(), twin.named_parameters()):
        assert torch.equal(a, b), k
    assert not torch.equal(negs[0], negs[1]) and not torch.equal(negs[1], negs[2])      # the captured RNG advances between replays


def test_multi_graph_graphed_steps_capture_the_one_hop_removal():
    """``GraphedMultiGraphTrainStep`` over two S-tiny contexts with different seeds: both are captured, and one step on each
    equals its eager twin."""
    from ultra_torchdrug_amd import engine
    from ultra_torchdrug_amd.data import synthetic_triples
    from ultra_torchdrug_amd.graph import Graph
    from ultra_torchdrug_amd.task import build_ultra
    dev = _dev()
    torch.manual_seed(1024)
    task = build_ultra(6, num_negative=16, remove_one_hop=True)
    facts = {}
    for name, seed in (("a", 1024), ("b", 77)):
        tr, n, r = synthetic_triples("S-tiny", seed)
        facts[name] = tr
        task.add_context(name, Graph(torch.from_numpy(tr), num_node=n, num_relation=r))
    assert not np.array_equal(facts["a"], facts["b"])
    task.to(dev).train()
    twin = copy.deepcopy(task)
    opt_g = torch.optim.AdamW(twin.parameters(), lr=1e-3)
    graphed = engine.GraphedMultiGraphTrainStep(twin, opt_g, 8)
    assert set(graphed.modes) == {"a", "b"}
    opt_e = torch.optim.AdamW(task.parameters(), lr=1e-3)
    for name in ("b", "a"):
        batch = (_t(facts[name][40:48]), name)
        loss_g, _ = graphed(batch)
        task._static_negative = graphed.steps[name].last_negatives.clone()
        loss_e, _ = engine.train_step(task, opt_e, batch)
        task._static_negative = None
        assert loss_g.item() == loss_e.item(), name
    for (k, a), (_, b) in zip(task.named_parameters(), twin.named_parameters()):
        assert torch.equal(a, b), k


# ------------------------------------------------------------------------------------------------ aggregates that stay eager
@pytest.mark.parametrize("aggregate_func", ["mean", "max"])
def test_other_aggregates_keep_the_mask_route_and_eager_steps(aggregate_func, monkeypatch):
    """A ``mean`` / ``max`` model with ``remove_one_hop=True`` is refused by ``GraphedTrainStep`` and never reaches
    ``remove_pairs``; its eager step is the mask route: ``easy_edge_mask`` and then, for ``mean``, exactly the weights
    ``edge_weight * keep`` on the graph with inverse edges, for ``max`` the graph without the masked edges."""
    from ultra_torchdrug_amd import engine, functional as UF
    from ultra_torchdrug_amd.data import synthetic_triples
    from ultra_torchdrug_amd.graph import Graph
    from ultra_torchdrug_amd.model import TransferNBFNet
    from ultra_torchdrug_amd.rel_model import RelationModelList
    from ultra_torchdrug_amd.task import KnowledgeGraphCompletion
    dev = _dev()
    triples, n, r = synthetic_triples("S-tiny", 1024)
    torch.manual_seed(1024)
    model = TransferNBFNet(input_dim=64, hidden_dims=[64] * 2, num_relation=r, message_func="distmult",
                           aggregate_func=aggregate_func, short_cut=True, layer_norm=True, project=True, mod=True,
                           remove_one_hop=True)
    rel_models = RelationModelList(num_rel_models=1, num_relation=2 * r,
                                   rel_model=dict(class_str="RelNBFNet", input_dim=64, input_type="ones", num_layers=2, hidden=64))
    task = KnowledgeGraphCompletion(model, rel_models, criterion="bce", num_negative=16, strict_negative=True,
                                    adversarial_temperature=1.0, sample_weight=False, full_batch_eval=True)
    task.preprocess(Graph(torch.from_numpy(triples), num_node=n, num_relation=r))
    task.to(dev).train()
    batch = _t(triples[:8])
    optimizer = torch.optim.AdamW(task.parameters(), lr=1e-3)
    with pytest.raises(ValueError, match="summed messages"):
        engine.GraphedTrainStep(task, optimizer, batch)

    def unreachable(*args):
        raise AssertionError("remove_pairs reached by a %s model" % aggregate_func)

    monkeypatch.setattr(UF, "remove_pairs", unreachable)
    seen = {}
    real_mask, real_reweighted, real_edge_mask = model.easy_edge_mask, Graph.reweighted, Graph.edge_mask

    def easy_edge_mask(graph, h, t, rel=None):
        seen["keep"] = real_mask(graph, h, t, rel)
        return seen["keep"]

    def reweighted(self, edge_weight):
        seen.setdefault("weight", []).append(edge_weight.clone())
        return real_reweighted(self, edge_weight)

    def edge_mask(self, index):
        seen.setdefault("edge_mask", []).append(index.clone())
        return real_edge_mask(self, index)

    monkeypatch.setattr(model, "easy_edge_mask", easy_edge_mask)
    monkeypatch.setattr(Graph, "reweighted", reweighted)
    monkeypatch.setattr(Graph, "edge_mask", edge_mask)
    torch.manual_seed(5)
    negatives = task._strict_negative(*batch.t())
    loss, grads = _step(task, batch, negatives)
    keep = seen["keep"]
    assert int((~keep).sum()) > len(batch)                                  # the pairs, not only the 8 triples
    if aggregate_func == "mean":
        und = task.model._undirected(task.fact_graph)
        assert len(seen["weight"]) == 1 and "edge_mask" not in seen
        assert torch.equal(seen["weight"][0], und.edge_weight * keep.repeat_interleave(2))
    else:
        assert len(seen["edge_mask"]) == 1 and torch.equal(seen["edge_mask"][0], keep) and "weight" not in seen
    assert torch.isfinite(loss) and grads
    again, grads_again = _step(task, batch, negatives)                      # the same step once more: the same numbers
    assert torch.equal(loss, again)
    for k in grads:
        assert torch.equal(grads[k], grads_again[k]), k

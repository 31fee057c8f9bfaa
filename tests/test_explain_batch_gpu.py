"""Batched explanations on the MI355X: the per-query-block edge-weight gradients against the single entries (bit for bit) and the
fp64 definition, the 2-D ``edge_weight`` through autograd, the batched beam-search step against its CPU key and B single HIP
calls, ``edge_gradients_batch`` against the fp64 materialised definition, ``visualize_batch`` / ``task.explain`` /
``engine.explain`` against the single-triple calls, the memory of a batch, and the three new entries between guard bands."""
import pytest
import torch

from explain_restatement import beam_inputs, coalesced_csr
from test_explain_batch_cpu import assert_batch_equals_singles, batch_case

pytestmark = pytest.mark.gpu

SHAPES = [(1, 64), (3, 64), (16, 64), (3, 32), (2, 192)]          # (B, block)
ROTATE_SHAPES = [(1, 64), (3, 64), (16, 64), (1, 6), (3, 6), (2, 192)]
EDGES = [0, 1, 6001]                                               # 6001 edges: the last workgroup of four waves holds one
N, R = 500, 9
_plans = {}


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    import ultra_torchdrug_amd as U
    U.require_library()
    return torch.device("cuda:0")


def _bits(t):
    return t.contiguous().view(torch.int32)


def _plan(E, weighted, dev):
    """A graph of exactly ``E`` distinct triples over ``N`` nodes and ``R`` relations; weights with zeros and negatives."""
    from ultra_torchdrug_amd import RelCSR
    key = (E, weighted)
    if key not in _plans:
        g = torch.Generator().manual_seed(5 + E)
        ids = torch.randperm(N * N * R, generator=g)[:E]
        dst, src, rel = (ids // (N * R)).to(dev), ((ids // R) % N).to(dev), (ids % R).to(dev)
        w = None
        if weighted:
            w = torch.randn(E, generator=g)
            w[::7] = 0
            w = w.to(dev)
        csr = RelCSR(dst, src, rel, w, N, N, R)
        assert csr.n_edges == E and (E == 0 or bool(csr.unit_weight) == (not weighted))
        _plans[key] = csr
    return _plans[key]


def _operands(F, dev, seed=0):
    g = torch.Generator(device=dev).manual_seed(100 + F + seed)
    return tuple(torch.randn(rows, F, device=dev, generator=g) for rows in (R, N, N))


@pytest.mark.parametrize("weighted", [True, False])
@pytest.mark.parametrize("mul", ["mul", "add"])
@pytest.mark.parametrize("sum", ["add", "min", "max"])
def test_blocks_operator_equals_the_single_entry_on_each_block(sum, mul, weighted):
    """Slice ``[b]`` of ``rspmm_backward_weight_blocks`` carries the bits of ``rspmm_backward_weight`` on a contiguous copy of
    block ``b``'s columns; ``output`` is the real forward result, so that the min / max masks select."""
    from ultra_torchdrug_amd import functional
    dev = _dev()
    for E in EDGES:
        csr = _plan(E, weighted, dev)
        for B, block in SHAPES:
            F = B * block
            relation, x, grad = _operands(F, dev)
            out = functional.rspmm_forward(csr, relation, x, sum, mul) if E else torch.zeros_like(x)
            got = functional.rspmm_backward_weight_blocks(csr, relation, x, out, grad, sum, mul, block)
            assert got.shape == (B, E) and got.dtype == torch.float32
            for b in range(B):
                blk = slice(b * block, (b + 1) * block)
                want = functional.rspmm_backward_weight(csr, *(a[:, blk].contiguous() for a in (relation, x, out, grad)), sum, mul)
                assert torch.equal(_bits(got[b]), _bits(want)), (E, B, block, b)
            if E > 1 and sum != "add":                             # the masks select: not the unmasked sums
                assert not torch.equal(got, functional.rspmm_backward_weight_blocks(csr, relation, x, None, grad, "add", mul, block))


@pytest.mark.parametrize("weighted", [True, False])
@pytest.mark.parametrize("sum", ["add", "min", "max"])
def test_rotate_blocks_operator_equals_the_single_entry_on_each_block(sum, weighted):
    """The same for rotate messages: block 64 and 6 (one block per half wave, the tree from 16) and 192 (96 pairs per block: whole
    waves, two trips, the tree from 32)."""
    from ultra_torchdrug_amd import functional
    dev = _dev()
    for E in EDGES:
        csr = _plan(E, weighted, dev)
        for B, block in ROTATE_SHAPES:
            F = B * block
            relation, x, grad = _operands(F, dev, seed=1)
            out = functional.rotate_rspmm_forward(csr, relation, x, sum, block) if E else torch.zeros_like(x)
            got = functional.rotate_rspmm_backward_weight_blocks(csr, relation, x, out, grad, sum, block)
            assert got.shape == (B, E) and got.dtype == torch.float32
            for b in range(B):
                blk = slice(b * block, (b + 1) * block)
                want = functional.rotate_rspmm_backward_weight(csr, *(a[:, blk].contiguous() for a in (relation, x, out, grad)),
                                                               sum, block)
                assert torch.equal(_bits(got[b]), _bits(want)), (E, B, block, b)


def _blocks_definition(csr, w, relation, x, grad_out, B, sum, mul, dtype):
    """d(weights) per query block from the scatter definition in ``dtype``: a ``(B, E)`` leaf, row ``b`` weighing block ``b``."""
    n, F = x.shape
    wd = w.detach().to(dtype).expand(B, -1).clone().requires_grad_()
    a, b = relation.to(dtype)[csr.rel_id], x.to(dtype)[csr.src]
    msg = wd.t().repeat_interleave(F // B, dim=1) * (a * b if mul == "mul" else a + b)
    reduce = {"add": "sum", "min": "amin", "max": "amax"}[sum]
    o = torch.zeros(n, F, dtype=dtype, device=x.device).scatter_reduce(0, csr.dst.view(-1, 1).expand(-1, F), msg, reduce,
                                                                       include_self=False)
    return torch.autograd.grad(o, wd, grad_out.to(dtype))[0]


@pytest.mark.parametrize("sum,mul", [("add", "mul"), ("max", "add")])
def test_blocks_operator_matches_the_fp64_definition(sum, mul):
    """Every ``[b][e]`` against the fp64 scatter definition, by the project's bound: at most 4 x the fp32 ATen definition's own
    distance + 5e-4 of the gradient's scale."""
    from ultra_torchdrug_amd import functional
    dev = _dev()
    B, block = 3, 32
    csr = _plan(6001, False, dev)
    relation, x, grad = _operands(B * block, dev, seed=2)
    g = torch.Generator(device=dev).manual_seed(3)
    w = torch.rand(csr.n_edges, device=dev, generator=g) + 0.5
    weighted = csr.with_coalesced_weights(w)
    out = functional.rspmm_forward(weighted, relation, x, sum, mul)
    got = functional.rspmm_backward_weight_blocks(weighted, relation, x, out, grad, sum, mul, block)
    truth = _blocks_definition(csr, w, relation, x, grad, B, sum, mul, torch.float64)
    aten = _blocks_definition(csr, w, relation, x, grad, B, sum, mul, torch.float32)
    s = truth.abs().max().item()
    e_hip, e_aten = (got.double() - truth).abs().max().item(), (aten.double() - truth).abs().max().item()
    print("blocks %s %s: e_hip %.3g e_aten %.3g scale %.3g" % (sum, mul, e_hip, e_aten, s))
    assert s > 0 and e_hip <= 4 * e_aten + 5e-4 * s, (e_hip, e_aten, s)


@pytest.mark.parametrize("route", ["rspmm_add", "rspmm_max", "sum_plus", "rotate"])
def test_two_dimensional_edge_weight_through_autograd(route):
    """``edge_weight`` of shape ``(B, E)`` with equal rows: the forward is the 1-D form's, the gradient is ``(B, E)``, for sums its
    sum over ``B`` is the 1-D gradient (held to the fp64 definition by the project's bound), and ``d_relation`` / ``d_input`` do
    not change by a bit."""
    from ultra_torchdrug_amd import functional
    dev = _dev()
    B, block = 3, 32
    F = B * block
    csr = _plan(6001, False, dev)
    relation, x, grad = _operands(F, dev, seed=3)
    g = torch.Generator(device=dev).manual_seed(4)
    w = torch.rand(csr.n_edges, device=dev, generator=g) + 0.5
    add_rows = torch.randn(N, F, device=dev, generator=g)
    call = {"rspmm_add": lambda r, i, ew: functional.generalized_rspmm(csr, r, i, sum="add", mul="mul", edge_weight=ew),
            "rspmm_max": lambda r, i, ew: functional.generalized_rspmm(csr, r, i, sum="max", mul="add", edge_weight=ew),
            "sum_plus": lambda r, i, ew: functional.rspmm_sum_plus(csr, r, i, add_rows, mul="mul", edge_weight=ew),
            "rotate": lambda r, i, ew: functional.rotate_rspmm(csr, r, i, "add", block, edge_weight=ew)}[route]
    results = []
    for leaf in (w.clone().requires_grad_(), w.expand(B, -1).clone().requires_grad_()):
        rel_l, x_l = relation.clone().requires_grad_(), x.clone().requires_grad_()
        out = call(rel_l, x_l, leaf)
        results.append((out.detach(),) + torch.autograd.grad(out, (leaf, rel_l, x_l), grad))
    (out1, dw1, drel1, dx1), (out2, dw2, drel2, dx2) = results
    assert torch.equal(_bits(out1), _bits(out2))
    assert dw1.shape == (csr.n_edges,) and dw2.shape == (B, csr.n_edges) and dw2.dtype == torch.float32
    assert torch.equal(_bits(drel1), _bits(drel2)) and torch.equal(_bits(dx1), _bits(dx2))
    if route in ("rspmm_add", "sum_plus"):
        truth = _blocks_definition(csr, w, relation, x, grad, 1, "add", "mul", torch.float64)[0]
        aten = _blocks_definition(csr, w, relation, x, grad, 1, "add", "mul", torch.float32)[0]
        s = truth.abs().max().item()
        e_hip, e_aten = (dw2.double().sum(0) - truth).abs().max().item(), (aten.double() - truth).abs().max().item()
        print("%s: e_hip %.3g e_aten %.3g scale %.3g" % (route, e_hip, e_aten, s))
        assert e_hip <= 4 * e_aten + 5e-4 * s, (e_hip, e_aten, s)
        assert (dw1.double() - truth).abs().max().item() <= 4 * e_aten + 5e-4 * s
    with pytest.raises(RuntimeError, match="edge_weight"):
        call(relation, x, w.expand(5, -1).clone())                 # 5 does not divide F = 96 (rotate: 5 * 32 != F)


def _hip_batch(row_ptr, src, grads, beams, tails, dev):
    from ultra_torchdrug_amd import functional
    return functional.beam_search_step_batch(*(a.to(dev) for a in (row_ptr, src, grads, beams, tails)))


@pytest.mark.parametrize("K", [1, 10, 32])
@pytest.mark.parametrize("B", [1, 2, 5])
def test_hip_batch_operator_equals_the_cpu_key_and_single_hip_calls(B, K):
    from ultra_torchdrug_amd import functional
    dev = _dev()
    row_ptr, src, grads, beams, tails = batch_case(B, K)
    cpu = functional.beam_search_step_batch(row_ptr, src, grads, beams, tails)
    hip = _hip_batch(row_ptr, src, grads, beams, tails, dev)
    for name, a, b in zip(("distance", "back_edge", "back_rank"), hip, cpu):
        assert a.is_cuda and a.dtype == b.dtype and torch.equal(a.cpu(), b), name
    assert_batch_equals_singles(hip, row_ptr.to(dev), src.to(dev), grads.to(dev), beams.to(dev), tails, functional.beam_search_step)
    with pytest.raises(RuntimeError, match="tail"):
        _hip_batch(row_ptr, src, grads, beams, torch.full_like(tails, 300), dev)


def test_hip_batch_operator_on_a_large_graph_with_a_hub_row():
    """200 000 nodes, one row of 20 000 in-edges, B = 3, K = 10: 16-lane groups, three of them on the hub row at once."""
    from ultra_torchdrug_amd import functional
    dev = _dev()
    n, B, K = 200_000, 3, 10
    row_ptr, src = coalesced_csr(7, n, 600_000, 20, hub_row=123_456, hub_edges=20_000)
    assert int(row_ptr[123_457] - row_ptr[123_456]) >= 19_000 and src.numel() // n < 24
    beams, grads = zip(*[beam_inputs(8 + b, n, K, src.numel(), empty=0.2) for b in range(B)])
    beams, grads = torch.stack(beams), torch.stack(grads)
    tails = torch.tensor([42, 123_456, 42], dtype=torch.int32)
    cpu = functional.beam_search_step_batch(row_ptr, src, grads, beams, tails)
    hip = _hip_batch(row_ptr, src, grads, beams, tails, dev)
    for name, a, b in zip(("distance", "back_edge", "back_rank"), hip, cpu):
        assert torch.equal(a.cpu(), b), name
    assert_batch_equals_singles(hip, row_ptr.to(dev), src.to(dev), grads.to(dev), beams.to(dev), tails, functional.beam_search_step)
    assert torch.isfinite(hip[0][:, 123_456]).all()


def _graph_and_model(aggregate, message, layers=3, seed=11, n_query=1):
    """The 2000-node, 12000-edge, 12-relation models of tests/test_explain_gpu.py, with ``n_query`` rows of relation
    representations."""
    from ultra_torchdrug_amd.data import synthetic_triples
    from ultra_torchdrug_amd.graph import Graph
    from ultra_torchdrug_amd.model import TransferNBFNet
    dev = _dev()
    triples, n, r = synthetic_triples((2000, 12000, 12), seed)
    torch.manual_seed(seed)
    model = TransferNBFNet(input_dim=64, hidden_dims=[64] * layers, num_relation=r, message_func=message,
                           aggregate_func=aggregate, short_cut=True, layer_norm=True, project=True, mod=True).to(dev)
    graph = Graph(torch.from_numpy(triples).to(dev), num_node=n, num_relation=r)
    gen = torch.Generator(device=dev).manual_seed(seed)
    rel = torch.randn(n_query, 2 * r, 64, device=dev, generator=gen)
    return model, graph, triples, rel


def _ids(triples, rows):
    return tuple([int(triples[i][c]) for i in rows] for c in range(3))


def _record_leaves(monkeypatch):
    """Shapes of the leaves ``bellmanford(separate_grad="native")`` hands its layers from here on, and their routes."""
    from ultra_torchdrug_amd.model import TransferNBFNet
    seen = []
    original = TransferNBFNet._edge_grad_graph

    def spy(*args, **kwargs):
        step = original(*args, **kwargs)
        seen.append((bool(step.edge_grad_coalesced), tuple(step.edge_grad_leaf.shape)))
        return step

    monkeypatch.setattr(TransferNBFNet, "_edge_grad_graph", staticmethod(spy))
    return seen


@pytest.mark.parametrize("aggregate,message", [("sum", "distmult"), ("sum", "transe"), ("sum", "rotate"), ("mean", "distmult")])
def test_batched_edge_gradients_match_the_fp64_definition(aggregate, message, monkeypatch):
    """B = 5 (two triples share a head, one is listed twice): one native forward / backward with ``(B, E)`` leaves; every query's
    gradients lie within 4 x the fp32 materialised definition's own distance from the fp64 materialised definition of that
    triple + 5e-4 of its scale, per layer.  No parameter gradient."""
    from aten_definition import AtenDefinition
    from ultra_torchdrug_amd import backend
    B = 5
    model, graph, triples, rel = _graph_and_model(aggregate, message, n_query=B)
    h, t, r = _ids(triples, (3, 4, 5, 6, 3))
    h[1] = h[0]
    E = model._undirected(graph).relcsr.n_edges
    seen = _record_leaves(monkeypatch)
    native = model.edge_gradients_batch(graph, [rel], h, t, r)
    assert seen == [(True, (B, E))] * 3, seen
    assert len(native) == 3 and all(g.shape == (B, E) and g.dtype == torch.float32 for g in native)
    for b in range(B):
        one = ([rel[b:b + 1]], [h[b]], [t[b]], [r[b]])
        with backend.use(AtenDefinition()):
            aten = model.edge_gradients(graph, *one)
            model.double()
            try:
                truth = model.edge_gradients(graph, [rel[b:b + 1].double()], *one[1:])
            finally:
                model.float()
        for layer, (g, a, w) in enumerate(zip(native, aten, truth)):
            s = w.abs().max().item() + 1e-30
            e_native, e_aten = (g[b].double() - w).abs().max().item(), (a.double() - w).abs().max().item()
            print("%s %s query %d layer %d: native %.3g aten %.3g scale %.3g" % (aggregate, message, b, layer, e_native, e_aten, s))
            assert e_native <= 4 * e_aten + 5e-4 * s, "query %d layer %d: native %.3g vs fp32 definition %.3g (scale %.3g)" % (
                b, layer, e_native, e_aten, s)
            assert w.abs().max() > 0
    assert all(p.grad is None for p in model.parameters())


@pytest.mark.parametrize("aggregate,message", [("sum", "distmult"), ("sum", "rotate"), ("mean", "transe"), ("max", "distmult")])
def test_a_batch_of_one_is_the_single_triple_call(aggregate, message):
    model, graph, triples, rel = _graph_and_model(aggregate, message)
    h, t, r = _ids(triples, (3,))
    batch = model.edge_gradients_batch(graph, [rel], h, t, r)
    single = model.edge_gradients(graph, [rel], h, t, r)
    assert len(batch) == len(single) == 3
    for a, b in zip(batch, single):
        assert a.shape == (1,) + tuple(b.shape) and torch.equal(_bits(a[0]), _bits(b))
    model.num_beam, model.path_topk = 10, 10
    assert model.visualize_batch(graph, [rel], h, t, r) == [model.visualize(graph, [rel], h, t, r)]


def test_max_stack_takes_the_native_route_in_a_batch(monkeypatch):
    B = 4
    model, graph, triples, rel = _graph_and_model("max", "transe", n_query=B)
    h, t, r = _ids(triples, range(3, 3 + B))
    E = model._undirected(graph).relcsr.n_edges
    seen = _record_leaves(monkeypatch)
    grads = model.edge_gradients_batch(graph, [rel], h, t, r)
    assert seen == [(True, (B, E))] * 3
    assert all(g.shape == (B, E) and torch.isfinite(g).all() for g in grads)
    results = model.visualize_batch(graph, [rel], h, t, r)
    assert len(results) == B
    for (paths, weights), hb, tb in zip(results, h, t):
        assert len(paths) == len(weights) and all(p[0][0] == hb and p[-1][1] == tb for p in paths)


def test_pna_stack_falls_back_to_single_triple_calls(monkeypatch):
    model, graph, triples, rel = _graph_and_model("pna", "distmult", n_query=2)
    h, t, r = _ids(triples, (3, 4))
    seen = _record_leaves(monkeypatch)
    grads = model.edge_gradients_batch(graph, [rel], h, t, r)
    assert seen and all(not coalesced and len(shape) == 1 for coalesced, shape in seen)
    # (the values are compared exactly on the CPU: on the device the materialised route scatters with atomics, whose order --
    # and so the last bits -- differs from run to run)
    E = model._undirected(graph).relcsr.n_edges
    assert len(grads) == 3 and all(g.shape == (2, E) and torch.isfinite(g).all() and g.abs().max() > 0 for g in grads)


def test_visualize_batch_equals_the_cpu_operator_fed_its_gradients():
    """4 layers, B = 4, 10 beams: the whole batch on the device == the CPU key of the batched operator and the host-side assembly
    fed the device's own batched gradients, exactly; a second call returns the same; no parameter gradient."""
    from types import SimpleNamespace
    from ultra_torchdrug_amd import functional
    from ultra_torchdrug_amd.model import TransferNBFNet
    B = 4
    model, graph, triples, rel = _graph_and_model("sum", "distmult", layers=4, n_query=B)
    model.num_beam, model.path_topk = 10, 10
    csr = model._undirected(graph).relcsr
    row_ptr, src, _, _ = (a.cpu() if a is not None else None for a in csr.csr_arrays)
    host_csr = SimpleNamespace(src=csr.src.cpu(), dst=csr.dst.cpu(), rel_id=csr.rel_id.cpu())
    h, t, r = _ids(triples, range(B))
    results = model.visualize_batch(graph, [rel], h, t, r)
    assert model.visualize_batch(graph, [rel], h, t, r) == results
    grads = model.edge_gradients_batch(graph, [rel], h, t, r)
    rows, tails = torch.arange(B), torch.tensor(t)
    beams = torch.full((B, graph.num_node, 10), float("-inf"))
    beams[rows, torch.tensor(h), 0] = 0
    steps = []
    for g in grads:
        beams, back_edge, back_rank = functional.beam_search_step_batch(row_ptr, src, g.cpu(), beams, tails.to(torch.int32))
        steps.append((beams[rows, tails], back_edge, back_rank))
    want = TransferNBFNet._assemble_paths_batch(host_csr, steps, tails, 10)
    assert results == want
    assert len(results) == B and sum(len(p) for p, _ in results) > 0
    for (paths, weights), hb, tb in zip(results, h, t):
        assert all(p[0][0] == hb and p[-1][1] == tb for p in paths) and list(weights) == sorted(weights, reverse=True)
    assert all(p.grad is None for p in model.parameters())


def test_task_and_engine_explain_on_the_device():
    """``task.explain(head=True)`` on chunks of one == ``task.visualize(head=True)``; ``engine.explain`` over 7 triples in chunks of
    3: 7 results in order, each chunk equal to ``task.explain`` of its rows; no parameter gradient."""
    from ultra_torchdrug_amd import engine
    from ultra_torchdrug_amd.data import synthetic_triples
    from ultra_torchdrug_amd.graph import Graph
    from ultra_torchdrug_amd.task import build_ultra
    dev = _dev()
    triples, n, r = synthetic_triples((2000, 12000, 12), 11)
    torch.manual_seed(11)
    task = build_ultra(r, hidden_dims=(64,) * 3, rel_layers=2).to(dev)
    task.preprocess(Graph(torch.from_numpy(triples).to(dev), None, n, r))
    task.eval()
    task.model.path_topk = 6
    rows = torch.from_numpy(triples[:7]).to(dev)
    for i in range(3):
        assert task.explain(rows[i:i + 1], head=True) == [task.visualize(rows[i], head=True)]
        assert task.explain(rows[i:i + 1]) == [task.visualize(rows[i])]
    results = engine.explain(task, rows, batch_size=3)
    assert len(results) == 7
    for c in range(0, 7, 3):
        assert results[c:c + 3] == task.explain(rows[c:c + 3])
    assert sum(len(p) for p, _ in results) > 0
    for (paths, _), row in zip(results, rows.tolist()):
        assert all(p[0][0] == row[0] and p[-1][1] == row[1] for p in paths)
    assert all(p.grad is None for p in task.parameters())
    assert not task.training


def test_a_batch_materialises_less_than_one_batched_message_tensor():
    """S-fb15k237 shape, the shipped 6 x 64d model, B = 4: the peak memory of visualize_batch above the model's baseline stays
    under B x E x 64 x 4 bytes -- one batched (E, B, D) fp32 message tensor."""
    from ultra_torchdrug_amd.data import synthetic_kg
    from ultra_torchdrug_amd.model import TransferNBFNet
    dev = _dev()
    B = 4
    graph = synthetic_kg("S-fb15k237", device=dev)
    torch.manual_seed(0)
    model = TransferNBFNet(input_dim=64, hidden_dims=[64] * 6, num_relation=graph.num_relation, message_func="distmult",
                           aggregate_func="sum", short_cut=True, layer_norm=True, project=True, mod=True).to(dev)
    rel = torch.randn(B, 2 * graph.num_relation, 64, device=dev)
    csr = model._undirected(graph).relcsr
    _ = csr.csr_arrays, csr.fwd, csr.by_src, csr.by_rel
    h, t, r = (graph.edge_list[:B, c] for c in range(3))
    model.visualize_batch(graph, [rel], h, t, r)            # warm: every lazily built index exists
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    results = model.visualize_batch(graph, [rel], h, t, r)
    torch.cuda.synchronize()
    extra = torch.cuda.max_memory_allocated() - base
    print("visualize_batch B = %d: peak %d bytes above the baseline, bound %d" % (B, extra, B * csr.n_edges * 64 * 4))
    assert extra < B * csr.n_edges * 64 * 4, (extra, B * csr.n_edges * 64 * 4)
    assert sum(len(p) for p, _ in results) > 0


def _hub_last(dev, weighted):
    """200 nodes, 1203 distinct triples (no multiple of 4) of which 300 enter the LAST row, the hub."""
    from ultra_torchdrug_amd import RelCSR
    n, n_rel, E, hub = 200, 5, 1203, 300
    g = torch.Generator().manual_seed(17)
    ids = torch.randperm((n - 1) * n * n_rel, generator=g)[:E - hub]             # rows 0 .. n - 2
    into_hub = torch.randperm(n * n_rel, generator=g)[:hub]                      # distinct (src, rel) pairs of row n - 1
    dst = torch.cat([ids // (n * n_rel), torch.full((hub,), n - 1)])
    src = torch.cat([(ids // n_rel) % n, into_hub // n_rel])
    rel = torch.cat([ids % n_rel, into_hub % n_rel])
    w = torch.randn(E, generator=g).to(dev) if weighted else None
    return RelCSR(dst.to(dev), src.to(dev), rel.to(dev), w, n, n, n_rel), n, n_rel


@pytest.mark.parametrize("weighted", [True, False])
def test_blocks_entries_stay_within_their_bounds(weighted):
    """Both blocks entries at their tail shapes (E no multiple of 4, block 32, B = 3, the hub in the last row) between poisoned,
    guard-banded allocations: the bands intact, the same bits as the plain call, no poison left in ``d_weight``."""
    from test_memory_bounds_gpu import run_guarded
    from ultra_torchdrug_amd import functional as UF
    dev = _dev()
    csr, n, n_rel = _hub_last(dev, weighted)
    E = csr.n_edges
    assert E == 1203 and E % 4 != 0 and int((csr.dst == n - 1).sum()) == 300
    B, block = 3, 32
    g = torch.Generator(device=dev).manual_seed(9)
    relation, x, grad = (torch.randn(rows, B * block, device=dev, generator=g) for rows in (n_rel, n, n))
    for sum in ("add", "max"):
        out = UF.rspmm_forward(csr, relation, x, sum, "mul")
        got = run_guarded(lambda rl, xi, o, gr: UF.rspmm_backward_weight_blocks(csr, rl, xi, o, gr, sum, "mul", block),
                          relation, x, out, grad, widest_row=4 * B * block, what="rspmm_backward_weight_blocks " + sum)
        assert got.shape == (B, E)
        out = UF.rotate_rspmm_forward(csr, relation, x, sum, block)
        got = run_guarded(lambda rl, xi, o, gr: UF.rotate_rspmm_backward_weight_blocks(csr, rl, xi, o, gr, sum, block),
                          relation, x, out, grad, widest_row=4 * B * block, what="rotate_rspmm_backward_weight_blocks " + sum)
        assert got.shape == (B, E)


@pytest.mark.parametrize("K", [1, 32])
def test_batched_beam_step_stays_within_its_bounds(K):
    """The batched step with the hub in the LAST row, B = 3, E no multiple of 4: ``row_ptr`` / ``src`` / ``tails`` between zero
    bands, ``edge_grad`` / ``input`` between NaN bands (finite inputs: any NaN in the result is an over-read), the bands intact
    afterwards, and the result equal to the unbanded call and to the CPU key.  (The outputs are ``at::empty`` in C++: unguarded,
    as those of the single step.)"""
    from test_memory_bounds_gpu import run_guarded
    from ultra_torchdrug_amd import functional as UF
    dev = _dev()
    n, B = 203, 3
    row_ptr, src = coalesced_csr(31, n, 1500, 4, hub_row=n - 1, hub_edges=400, self_loops=10)
    E = src.numel()
    assert E % 4 != 0 and int(row_ptr[n] - row_ptr[n - 1]) >= 300
    beams, grads = zip(*[beam_inputs(40 + b + K, n, K, E, empty=0.1) for b in range(B)])
    beams, grads = torch.stack(beams), torch.stack(grads)
    assert bool(torch.isfinite(grads).all()) and not bool(torch.isnan(beams).any())
    tails = torch.tensor([int(src[0]), n - 1, int(src[0])], dtype=torch.int32)
    twin = UF.beam_search_step_batch(row_ptr, src, grads, beams, tails)
    got = run_guarded(lambda rp, s, g, b, t: list(UF.beam_search_step_batch(rp, s, g, b, t)), row_ptr.to(dev), src.to(dev),
                      grads.to(dev), beams.to(dev), tails.to(dev), what="beam_search_step_batch")
    for name, a, b in zip(("distance", "back_edge", "back_rank"), got, twin):
        assert a.is_cuda and a.dtype == b.dtype and not bool(torch.isnan(a).any()) if a.dtype == torch.float32 else a.is_cuda
        assert torch.equal(a.cpu(), b), name

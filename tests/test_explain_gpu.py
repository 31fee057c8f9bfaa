"""TransferNBFNet.visualize on the MI355X: the HIP beam-search step against its CPU twin and the restatement (bit for bit), the native
per-layer edge gradients against the fp64 materialised definition, the whole explanation against the CPU operator fed the GPU's
own gradients, and the memory the native route needs."""
import pytest
import torch

from explain_restatement import beam_inputs, beam_step, coalesced_csr

pytestmark = pytest.mark.gpu


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    import ultra_torchdrug_amd as U
    U.require_library()
    return torch.device("cuda:0")


def _op(*args):
    from ultra_torchdrug_amd import functional
    return functional.beam_search_step(*args)


def _three_way(row_ptr, src, grad, beams, tail, dev):
    """HIP == CPU == restatement, every output, bit for bit."""
    cpu = _op(row_ptr, src, grad, beams, tail)
    hip = _op(row_ptr.to(dev), src.to(dev), grad.to(dev), beams.to(dev), tail)
    torch.cuda.synchronize()
    want = beam_step(row_ptr.to(dev), src.to(dev), grad.to(dev), beams.to(dev), tail)
    for name, a, b, c in zip(("distance", "back_edge", "back_rank"), hip, cpu, want):
        assert a.is_cuda and a.dtype == b.dtype
        assert torch.equal(a.cpu(), b), name
        assert torch.equal(c.cpu(), b), name
    return hip


@pytest.mark.parametrize("K", [1, 3, 10, 32])
def test_hip_operator_equals_cpu_operator_and_restatement(K):
    """The CPU test's cases (duplicates, isolated nodes, self-loops, a row of more than 64 K candidates, near-equal values, exact
    ties, non-finite gradients, tails with and without out-edges) on the device, one graph at least per group width (the lanes
    per row follow the mean in-degree: 64 from 48 on, 32 from 24 on, else 16)."""
    dev = _dev()
    cases = [coalesced_csr(1, 200, 3000, 5, isolated=20, self_loops=50, duplicates=300),
             coalesced_csr(2, 3000, 4000 + 300 * K, 3, hub_row=7, hub_edges=300 * K + 300, duplicates=50),
             coalesced_csr(5, 5000, 200000, 7, isolated=100),
             # 403 rows: the last block of four 64-lane groups is ragged
             coalesced_csr(9, 403, 40000, 11, isolated=15, hub_row=5, hub_edges=1500, self_loops=40, duplicates=200)]
    lanes = (16, 16, 32, 64)
    for i, (row_ptr, src) in enumerate(cases):
        n = row_ptr.numel() - 1
        mean = src.numel() // n
        assert {16: mean < 24, 32: 24 <= mean < 48, 64: mean >= 48}[lanes[i]], (i, mean)
        beams, grad = beam_inputs(10 + i, n, K, src.numel(), empty=0.1)
        if i in (0, 3):
            grad[::17] = float("nan")
            grad[3::19] = float("inf")
        deg_in = row_ptr[1:] - row_ptr[:-1]
        for tail in (int(src[0]), int(deg_in.argmax()), n - 1):
            _three_way(row_ptr, src, grad, beams, tail, dev)


def test_hip_operator_on_a_two_million_node_graph_with_a_hub_row():
    """2 M nodes, 6 M edges, one row of 60 000 in-edges (the Zipf heads of S-fb15k237 reach tens of thousands); only 16-lane
    groups run here (mean degree 3), the hub row is walked by one of them."""
    dev = _dev()
    n = 2_000_000
    row_ptr, src = coalesced_csr(7, n, 6_000_000, 20, hub_row=123_456, hub_edges=60_000)
    assert int(row_ptr[123_457] - row_ptr[123_456]) > 50_000
    assert src.numel() // n < 24
    beams, grad = beam_inputs(8, n, 10, src.numel(), empty=0.2)
    hip = _three_way(row_ptr, src, grad, beams, 42, dev)
    assert torch.isfinite(hip[0][123_456]).all()


def _graph_and_model(aggregate, message, layers=3, seed=11):
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
    rel = torch.randn(1, 2 * r, 64, device=dev, generator=gen)
    return model, graph, triples, rel


@pytest.mark.parametrize("aggregate", ["sum"])
@pytest.mark.parametrize("message", ["distmult", "transe"])
def test_native_edge_gradients_match_the_fp64_definition(aggregate, message):
    """Per layer, the native route's coalesced edge gradients against the materialised definition in fp64 (the truth): within
    4 x the fp32 materialised route's own distance from it + 5e-4 of the gradient's scale.  Max-aggregated stacks are held to
    the definition at the operator (test below), not here: every node a query has not reached yet holds the SAME row, so a max
    layer's messages tie structurally, and the rspmm backward feeds every tied edge in full (torchdrug's rspmm convention,
    include/ultra_rspmm.h) where ATen's scatter amax splits the gradient -- a measured 0.6 % of the scale in the first layer of a
    3-layer DistMult / max stack ("Explaining a prediction")."""
    from aten_definition import AtenDefinition
    from ultra_torchdrug_amd import backend
    model, graph, triples, rel = _graph_and_model(aggregate, message)
    h, t, r = (int(x) for x in triples[3])
    native = model.edge_gradients(graph, [rel], [h], [t], [r])
    und = model._undirected(graph)
    assert all(g.shape == (und.relcsr.n_edges,) and g.dtype == torch.float32 for g in native)
    with backend.use(AtenDefinition()):
        aten = model.edge_gradients(graph, [rel], [h], [t], [r])
        model.double()
        try:
            truth = model.edge_gradients(graph, [rel.double()], [h], [t], [r])
        finally:
            model.float()
    assert truth[0].dtype == torch.float64
    assert all(p.grad is None for p in model.parameters())
    for layer, (g, a, w) in enumerate(zip(native, aten, truth)):
        s = w.abs().max().item() + 1e-30
        e_native, e_aten = (g.double() - w).abs().max().item(), (a.double() - w).abs().max().item()
        assert e_native <= 4 * e_aten + 5e-4 * s, "layer %d: native %.3g vs fp32 definition %.3g (scale %.3g)" % (
            layer, e_native, e_aten, s)
        assert w.abs().max() > 0


@pytest.mark.parametrize("sum", ["add", "min", "max"])
@pytest.mark.parametrize("mul", ["mul", "add"])
def test_rspmm_edge_weight_gradient_matches_the_fp64_definition(sum, mul):
    """``generalized_rspmm(edge_weight=...)``: forward as with the weights in the adjacency, d(edge_weight) against the scatter
    definition in fp64, for every sum / mul pair (min included: no layer aggregates with it)."""
    from ultra_torchdrug_amd import RelCSR, functional
    dev = _dev()
    g = torch.Generator(device=dev).manual_seed(3)
    n, E, R, F = 500, 6000, 9, 32
    dst, src, rel = (torch.randint(0, m, (E,), device=dev, generator=g) for m in (n, n, R))
    csr = RelCSR(dst, src, rel, None, n, n, R)
    relation = torch.randn(R, F, device=dev, generator=g)
    x = torch.randn(n, F, device=dev, generator=g)
    w = (torch.rand(csr.n_edges, device=dev, generator=g) + 0.5).requires_grad_()
    grad_out = torch.randn(n, F, device=dev, generator=g)
    out = functional.generalized_rspmm(csr, relation, x, sum=sum, mul=mul, edge_weight=w)
    want_out = functional.generalized_rspmm(csr.with_coalesced_weights(w.detach()), relation, x, sum=sum, mul=mul)
    assert torch.equal(out, want_out)
    (d_w,) = torch.autograd.grad(out, w, grad_out)

    def definition(dtype):
        wd = w.detach().to(dtype).requires_grad_()
        a, b = relation.to(dtype)[csr.rel_id], x.to(dtype)[csr.src]
        msg = wd.unsqueeze(-1) * (a * b if mul == "mul" else a + b)
        reduce = {"add": "sum", "min": "amin", "max": "amax"}[sum]
        o = torch.zeros(n, F, dtype=dtype, device=dev).scatter_reduce(0, csr.dst.view(-1, 1).expand(-1, F), msg, reduce,
                                                                      include_self=False)
        return torch.autograd.grad(o, wd, grad_out.to(dtype))[0]

    truth, aten = definition(torch.float64), definition(torch.float32)
    s = truth.abs().max().item()
    e_hip, e_aten = (d_w.double() - truth).abs().max().item(), (aten.double() - truth).abs().max().item()
    assert e_hip <= 4 * e_aten + 5e-4 * s, (e_hip, e_aten, s)


def test_max_stack_takes_the_native_route():
    """A max-aggregated stack explains on the native route too: coalesced leaves on every layer, finite gradients, paths found."""
    model, graph, triples, rel = _graph_and_model("max", "transe")
    h, t, r = (int(x) for x in triples[3])
    grads = model.edge_gradients(graph, [rel], [h], [t], [r])
    assert all(g.shape == (model._undirected(graph).relcsr.n_edges,) and torch.isfinite(g).all() for g in grads)
    paths, weights = model.visualize(graph, [rel], [h], [t], [r])
    assert len(paths) == len(weights) and all(p[0][0] == h and p[-1][1] == t for p in paths)


def test_visualize_on_the_gpu_equals_the_cpu_operator_fed_its_gradients():
    """The whole explanation on the device == the CPU operator (and host-side assembly) fed the device's own edge gradients,
    exactly; a second call returns the same; parameters keep no gradient."""
    from types import SimpleNamespace
    from ultra_torchdrug_amd import functional
    from ultra_torchdrug_amd.model import TransferNBFNet
    model, graph, triples, rel = _graph_and_model("sum", "distmult", layers=4)
    model.num_beam, model.path_topk = 10, 10
    und = model._undirected(graph)
    csr = und.relcsr
    row_ptr, src, _, _ = (a.cpu() if a is not None else None for a in csr.csr_arrays)
    host_csr = SimpleNamespace(src=csr.src.cpu(), dst=csr.dst.cpu(), rel_id=csr.rel_id.cpu())
    seen = 0
    for i in range(4):
        h, t, r = (int(x) for x in triples[i])
        paths, weights = model.visualize(graph, [rel], [h], [t], [r])
        again = model.visualize(graph, [rel], [h], [t], [r])
        assert (paths, weights) == again
        grads = model.edge_gradients(graph, [rel], [h], [t], [r])
        beams = torch.full((graph.num_node, 10), float("-inf"))
        beams[h, 0] = 0
        steps = []
        for g in grads:
            beams, back_edge, back_rank = functional.beam_search_step(row_ptr, src, g.cpu(), beams, t)
            steps.append((beams[t], back_edge, back_rank))
        want = TransferNBFNet._assemble_paths(host_csr, steps, t, 10)
        assert (paths, weights) == want
        seen += len(paths)
    assert seen > 0
    assert all(p.grad is None for p in model.parameters())


def test_native_route_materialises_no_edge_message_tensor():
    """S-fb15k237 shape, the shipped 6 x 64d model, B = 1: the peak memory of visualize above the model's baseline stays under
    E x 64 x 4 bytes -- one (E, D) fp32 message tensor, which the materialised route needs per layer."""
    from ultra_torchdrug_amd.data import synthetic_kg
    from ultra_torchdrug_amd.model import TransferNBFNet
    dev = _dev()
    graph = synthetic_kg("S-fb15k237", device=dev)
    torch.manual_seed(0)
    model = TransferNBFNet(input_dim=64, hidden_dims=[64] * 6, num_relation=graph.num_relation, message_func="distmult",
                           aggregate_func="sum", short_cut=True, layer_norm=True, project=True, mod=True).to(dev)
    rel = torch.randn(1, 2 * graph.num_relation, 64, device=dev)
    und = model._undirected(graph)
    csr = und.relcsr
    _ = csr.csr_arrays, csr.fwd, csr.by_src, csr.by_rel
    h, t, r = (int(x) for x in graph.edge_list[0])
    model.visualize(graph, [rel], [h], [t], [r])            # warm: every lazily built index exists
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    paths, weights = model.visualize(graph, [rel], [h], [t], [r])
    torch.cuda.synchronize()
    extra = torch.cuda.max_memory_allocated() - base
    assert extra < csr.n_edges * 64 * 4, (extra, csr.n_edges * 64 * 4)
    assert len(paths) > 0

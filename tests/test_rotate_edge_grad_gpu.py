"""Edge-weight gradients of rotate and mean layers on the MI355X: ``rotate_rspmm(edge_weight=)`` and its gradient
(``rotate_weight_grad_kernel``, csrc/rotate.inc) against the fp64 definition on every launch form, both bindings, the layer
stacks of ``TransferNBFNet.edge_gradients`` that now take the native route (rotate with sum / max, mean on unit-weight graphs)
against the fp64 materialised definition, the memory ``visualize`` needs on a rotate model, and the whole explanation against
the CPU beam search fed the device's gradients.

Launch forms of the kernel: one edge per wave (more than 32 pairs; 1, 2 and 9 pair tiles, blocks that straddle a tile), two edges
per wave (at most 32 pairs: F = 2 and the explain shape F = 64), unit-weight and weighted plans, and for both forms an edge
count beyond one pass of the 8192-block grid (32 768 waves)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import rotate_restatement as RR
from graphs import random_graph

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (F, block): one pair on two lanes' worth of a wave | the explain shape, two edges per wave | one full pair tile, one edge per
# wave | 12 pairs per block: blocks straddle the pair tiles, the second tile partial | 9 pair tiles
SHAPES = [(2, 2), (64, 64), (128, 64), (192, 24), (1152, 64)]
# name -> (graph kwargs, nodes, relations, F, block, unit weights).  "wrap*": more edges than one pass of the grid has waves
# (one edge per wave at F = 128: > 32 768 edges; two per wave at F = 64: > 65 536 edges)
GRAPHS = {
    "unit": (dict(n_edge=4000, unique=True), 300, 7, 192, 24, True),
    "unit_two_per_wave": (dict(n_edge=4003, unique=True), 300, 7, 64, 64, True),
    "wrap": (dict(n_edge=40000), 2000, 7, 128, 64, False),
    "wrap_two_per_wave": (dict(n_edge=70000), 2000, 7, 64, 64, False),
    "duplicates_isolated": (dict(n_edge=4000, skew=True, isolated=40), 300, 7, 64, 64, False),
}
for _F, _block in SHAPES:
    GRAPHS["F%d_block%d" % (_F, _block)] = (dict(n_edge=4000), 300, 7, _F, _block, False)


def _dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import ultra_torchdrug_amd as U
    U.require_library()
    return torch.device("cuda:0")


def _case(name, dev):
    """The operands of one operator case, seeded: ``(csr, relation, x, w, grad_out)`` on ``dev`` (``w`` in forward-plan order)."""
    from ultra_torchdrug_amd import RelCSR
    kw, n, r, F, block, unit = GRAPHS[name]
    g = random_graph(seed=len(name) + 17, n_node=n, n_rel=r, **kw)
    t = lambda a: torch.from_numpy(a).to(dev)
    csr = RelCSR(t(g["dst"]), t(g["src"]), t(g["rel"]), None, n, n, r)
    gen = torch.Generator().manual_seed(len(name))
    relation, x, grad_out = (torch.randn(rows, F, generator=gen).to(dev) for rows in (r, n, n))
    w = torch.ones(csr.n_edges) if unit else torch.rand(csr.n_edges, generator=gen) + 0.5
    return csr, relation, x, w.to(dev), grad_out


def _definition(csr, relation, x, w, grad_out, block, sum, dtype):
    """``d_w`` from the definition in ``dtype``: ``w`` times the complex product (the expression of
    ``rotate_restatement.messages``), ``scatter_reduce`` over the destinations, ``autograd.grad`` with respect to ``w``."""
    E, F, n = csr.n_edges, x.shape[1], csr.shape[0]
    wd = w.detach().to(dtype).requires_grad_()
    xs = x.to(dtype)[csr.src].view(E, F // block, 2, block // 2)
    rs = relation.to(dtype)[csr.rel_id].view(E, F // block, 2, block // 2)
    re = xs[:, :, 0] * rs[:, :, 0] - xs[:, :, 1] * rs[:, :, 1]
    im = xs[:, :, 0] * rs[:, :, 1] + xs[:, :, 1] * rs[:, :, 0]
    m = torch.stack([re, im], dim=2).reshape(E, F) * wd.unsqueeze(-1)
    reduce = {"add": "sum", "min": "amin", "max": "amax"}[sum]
    out = torch.zeros(n, F, dtype=dtype, device=x.device).scatter_reduce(0, csr.dst.view(-1, 1).expand(-1, F), m, reduce,
                                                                         include_self=False)
    return torch.autograd.grad(out, wd, grad_out.to(dtype))[0], m.detach()


def _unambiguous(csr, relation, x, w, grad_out, block, sum):
    """``grad_out`` with the cells zeroed whose two best fp64 messages lie within 4e-6 (``rotate_restatement.ambiguous_cells``:
    fp32 may select the other edge there); at most 0.1 % of the cells of non-empty rows, the cap of the rotate parity tests."""
    if sum == "add":
        return grad_out
    dst, src, rel = (a.cpu().numpy() for a in (csr.dst, csr.src, csr.rel_id))
    n = csr.shape[0]
    ambiguous = RR.ambiguous_cells(dst, src, rel, w.cpu().numpy(), relation.cpu(), x.cpu(), n, block, sum)
    cells = int((np.bincount(dst, minlength=n) > 0).sum()) * x.shape[1]
    print("%s: %d ambiguous cells of %d" % (sum, int(ambiguous.sum()), cells))
    assert int(ambiguous.sum()) <= 1e-3 * cells
    return grad_out * (~ambiguous).to(grad_out.device)


def _operator_d_w(name, sum, dev):
    """``(d_w, csr, relation, x, w, grad_out)`` of one case through ``rotate_rspmm(edge_weight=)``, the forward checked."""
    from ultra_torchdrug_amd import functional
    csr, relation, x, w, grad_out = _case(name, dev)
    block = GRAPHS[name][4]
    grad_out = _unambiguous(csr, relation, x, w, grad_out, block, sum)
    leaf = w.clone().requires_grad_()
    out = functional.rotate_rspmm(csr, relation, x, sum, block, edge_weight=leaf)
    with torch.no_grad():
        want_out = functional.rotate_rspmm(csr.with_coalesced_weights(w), relation, x, sum, block)
    assert torch.equal(out, want_out)
    (d_w,) = torch.autograd.grad(out, leaf, grad_out)
    return d_w, csr, relation, x, w, grad_out


@pytest.mark.parametrize("name", list(GRAPHS))
@pytest.mark.parametrize("sum", ["add", "min", "max"])
def test_rotate_edge_weight_gradient_matches_the_fp64_definition(name, sum):
    """``rotate_rspmm(edge_weight=w)``: the forward equals the operator over ``csr.with_coalesced_weights(w)`` bit for bit, and
    ``d_w`` is held to the fp64 definition by the project's bound: its distance at most 4 x the fp32 ATen definition's own + 5e-4
    of the gradient's scale.  Every entry of ``d_w`` is compared, so an entry the kernel left unwritten would show; two runs
    agree bit for bit; on unit-weight plans the kernel without a weight array gives the same bits as the one that multiplies by 1.
    Measured on an MI355X: ``e_hip`` between 0.7 and 1.8 x ``e_aten`` in every case (both a few 1e-7 of the scale)."""
    from ultra_torchdrug_amd import functional
    dev = _dev()
    kw, n, r, F, block, unit = GRAPHS[name]
    d_w, csr, relation, x, w, grad_out = _operator_d_w(name, sum, dev)
    n_pairs = F // 2
    if name.startswith("wrap"):
        assert csr.n_edges > (65536 if n_pairs <= 32 else 32768)
    if name in ("unit_two_per_wave", "F64_block64", "F2_block2"):
        assert n_pairs <= 32 and csr.n_edges % 2 == 1   # two edges per wave: the last wave holds one
    if name == "duplicates_isolated":
        assert csr.n_edges < kw["n_edge"] and (torch.bincount(csr.dst, minlength=n) == 0).any() and not csr.unit_weight
    assert d_w.shape == (csr.n_edges,) and d_w.dtype == torch.float32 and torch.isfinite(d_w).all()
    truth, m64 = _definition(csr, relation, x, w, grad_out, block, sum, torch.float64)
    aten, _ = _definition(csr, relation, x, w, grad_out, block, sum, torch.float32)
    # the definition above IS the restatement's message expression
    want_m = RR.messages(csr.src.cpu().numpy(), csr.rel_id.cpu().numpy(), w.cpu().numpy(), relation.cpu(), x.cpu(), block)
    assert torch.equal(m64.cpu(), want_m)
    s = truth.abs().max().item()
    e_hip, e_aten = (d_w.double() - truth).abs().max().item(), (aten.double() - truth).abs().max().item()
    print("%s %s: e_hip %.3g e_aten %.3g scale %.3g" % (name, sum, e_hip, e_aten, s))
    assert s > 0
    assert e_hip <= 4 * e_aten + 5e-4 * s, (e_hip, e_aten, s)
    out = functional.rotate_rspmm_forward(csr.with_coalesced_weights(w), relation, x, sum, block)
    again = functional.rotate_rspmm_backward_weight(csr.with_coalesced_weights(w), relation, x, out, grad_out, sum, block)
    assert torch.equal(again, d_w)
    if unit:
        assert csr.unit_weight and csr.fwd.weight is None
        plain = functional.rotate_rspmm_backward_weight(csr, relation, x, functional.rotate_rspmm_forward(csr, relation, x, sum, block),
                                                        grad_out, sum, block)
        assert torch.equal(plain, d_w)


def test_masked_out_edges_receive_an_exact_zero():
    """Under max an edge that wins no component receives exactly 0: its entry is written, not left over."""
    dev = _dev()
    d_w, csr, relation, x, w, grad_out = _operator_d_w("F2_block2", "max", dev)
    _, m = _definition(csr, relation, x, w, grad_out, 2, "max", torch.float64)
    best = torch.full((csr.shape[0], 2), float("-inf"), dtype=torch.float64, device=dev).scatter_reduce(
        0, csr.dst.view(-1, 1).expand(-1, 2), m, "amax")
    loser = (m < best[csr.dst] - 1e-3 * best[csr.dst].abs()).all(dim=1)
    assert loser.sum() > 100
    assert (d_w[loser] == 0).all()


def _child(path):
    """Runs in a fresh process (``ULTRA_BINDING`` chosen by the parent): the ``d_w`` of two cases, saved to ``path``."""
    dev = _dev()
    res = []
    for name, sum in (("F192_block24", "max"), ("F64_block64", "add"), ("unit", "min")):
        res.append(_operator_d_w(name, sum, dev)[0].cpu())
    torch.save(res, path)


def test_ctypes_binding_gives_the_same_bits(tmp_path):
    from ultra_torchdrug_amd import _torch_ext
    outs = {}
    for binding in ("torch", "ctypes"):
        env = dict(os.environ, ULTRA_BINDING=binding)
        path = str(tmp_path / ("%s.pt" % binding))
        code = ("import sys; sys.path[:0] = [sys.argv[1], sys.argv[1] + '/tests']; import test_rotate_edge_grad_gpu as T; "
                "T._child(sys.argv[2])")
        proc = subprocess.run([sys.executable, "-c", code, ROOT, path], env=env, timeout=300, capture_output=True, text=True)
        assert proc.returncode == 0, proc.stderr[-3000:]
        outs[binding] = torch.load(path)
    assert len(outs["torch"]) == len(outs["ctypes"]) == 3
    for a, b in zip(outs["torch"], outs["ctypes"]):
        assert torch.equal(a, b)
    if _torch_ext.binding() == "torch":                # ... and this process, on the extension, agrees with both
        dev = _dev()
        assert torch.equal(_operator_d_w("F64_block64", "add", dev)[0].cpu(), outs["ctypes"][1])


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


def _record_routes(monkeypatch):
    """``edge_grad_coalesced`` of every step graph ``bellmanford(separate_grad="native")`` builds from here on."""
    from ultra_torchdrug_amd.model import TransferNBFNet
    seen = []
    original = TransferNBFNet._edge_grad_graph

    def spy(graph, conv, query, boundary):
        step = original(graph, conv, query, boundary)
        seen.append(bool(step.edge_grad_coalesced))
        return step

    monkeypatch.setattr(TransferNBFNet, "_edge_grad_graph", staticmethod(spy))
    return seen


@pytest.mark.parametrize("aggregate,message", [("sum", "rotate"), ("mean", "rotate"), ("mean", "distmult")])
def test_stack_edge_gradients_take_the_native_route_and_match_fp64(aggregate, message, monkeypatch):
    """3 x 64d stacks: every layer's step graph carries a coalesced leaf (the native route), the gradients are fp32 in
    coalesced order and lie within 4 x the fp32 materialised definition's own distance from the fp64 materialised definition +
    5e-4 of the gradient's scale; no parameter receives a gradient.  The graph's coalesced weights are all 1, which the mean
    stacks need: ``degree_out + 1`` is then the count ``scatter(..., "mean")`` divides by."""
    from aten_definition import AtenDefinition
    from ultra_torchdrug_amd import backend
    model, graph, triples, rel = _graph_and_model(aggregate, message)
    h, t, r = (int(x) for x in triples[3])
    und = model._undirected(graph)
    assert und.relcsr.unit_weight
    seen = _record_routes(monkeypatch)
    native = model.edge_gradients(graph, [rel], [h], [t], [r])
    assert seen == [True] * 3, seen
    assert all(g.shape == (und.relcsr.n_edges,) and g.dtype == torch.float32 for g in native)
    del seen[:]
    with backend.use(AtenDefinition()):
        aten = model.edge_gradients(graph, [rel], [h], [t], [r])
        model.double()
        try:
            truth = model.edge_gradients(graph, [rel.double()], [h], [t], [r])
        finally:
            model.float()
    assert seen == [False] * 6
    assert truth[0].dtype == torch.float64
    assert all(p.grad is None for p in model.parameters())
    for layer, (g, a, w) in enumerate(zip(native, aten, truth)):
        s = w.abs().max().item() + 1e-30
        e_native, e_aten = (g.double() - w).abs().max().item(), (a.double() - w).abs().max().item()
        print("%s %s layer %d: native %.3g aten %.3g scale %.3g" % (aggregate, message, layer, e_native, e_aten, s))
        assert e_native <= 4 * e_aten + 5e-4 * s, "layer %d: native %.3g vs fp32 definition %.3g (scale %.3g)" % (
            layer, e_native, e_aten, s)
        assert w.abs().max() > 0


def test_rotate_max_stack_takes_the_native_route(monkeypatch):
    """Max over rotate messages: structural ties make a stack-level fp64 comparison meaningless ("Explaining a
    prediction"; the operator is held to fp64 above), so: the native route on every layer, finite gradients, paths h -> t."""
    model, graph, triples, rel = _graph_and_model("max", "rotate")
    h, t, r = (int(x) for x in triples[3])
    seen = _record_routes(monkeypatch)
    grads = model.edge_gradients(graph, [rel], [h], [t], [r])
    assert seen == [True] * 3, seen
    assert all(g.shape == (model._undirected(graph).relcsr.n_edges,) and torch.isfinite(g).all() for g in grads)
    paths, weights = model.visualize(graph, [rel], [h], [t], [r])
    assert len(paths) == len(weights) and all(p[0][0] == h and p[-1][1] == t for p in paths)


@pytest.mark.parametrize("message", ["rotate", "distmult"])
def test_mean_stack_on_a_weighted_graph_stays_materialised(message, monkeypatch):
    """With weights other than 1 the native divisor (the weighted degree) is not the count ``scatter(..., "mean")`` divides by:
    the mean layers keep the materialised route."""
    model, graph, triples, rel = _graph_and_model("mean", message)
    gen = torch.Generator(device=graph.device).manual_seed(1)
    weighted = graph.reweighted(torch.rand(graph.edge_weight.shape, device=graph.device, generator=gen) + 0.5)
    h, t, r = (int(x) for x in triples[3])
    seen = _record_routes(monkeypatch)
    grads = model.edge_gradients(weighted, [rel], [h], [t], [r])
    assert seen == [False] * 3, seen
    assert all(torch.isfinite(g).all() for g in grads)


def test_rotate_visualize_materialises_no_edge_message_tensor():
    """S-fb15k237 shape, a 6 x 64d rotate / sum model, B = 1: the peak memory of visualize above the model's baseline stays under
    E x 64 x 4 bytes -- ONE (E, D) fp32 message tensor, of which the materialised rotate route holds several per layer."""
    from ultra_torchdrug_amd.data import synthetic_kg
    from ultra_torchdrug_amd.model import TransferNBFNet
    dev = _dev()
    graph = synthetic_kg("S-fb15k237", device=dev)
    torch.manual_seed(0)
    model = TransferNBFNet(input_dim=64, hidden_dims=[64] * 6, num_relation=graph.num_relation, message_func="rotate",
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
    print("peak above baseline %d bytes, one message tensor %d bytes" % (extra, csr.n_edges * 64 * 4))
    assert extra < csr.n_edges * 64 * 4, (extra, csr.n_edges * 64 * 4)
    assert len(paths) > 0


def test_rotate_visualize_equals_the_cpu_operator_fed_its_gradients():
    """The whole explanation of a rotate / sum stack on the device == the CPU beam search (and host-side assembly) fed the
    device's own edge gradients, exactly; a second call returns the same; parameters keep no gradient."""
    from types import SimpleNamespace
    from ultra_torchdrug_amd import functional
    from ultra_torchdrug_amd.model import TransferNBFNet
    model, graph, triples, rel = _graph_and_model("sum", "rotate", layers=4)
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

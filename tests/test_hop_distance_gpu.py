"""MI355X: hop distances on the device -- the bit-parallel BFS of ``csrc/hop_distance.hip`` through both bindings, polled and
with the fixed number of levels, captured into a hipGraph, on a Zipf graph, and the task / engine / model layers over it.  Held to
the CPU key and to the definitions of tests/hop_definition.py exactly (int32, ``torch.equal``)."""
import numpy as np
import pytest
import torch

from graphs import kg_graph
from hop_definition import (graph_of, iteration_form, path_graph, queue_form, random_edges, small_graphs, star_with_rows)
from sampled_graphs import small_task, wide_graph

pytestmark = pytest.mark.gpu


def _dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def _device_runs(graph, sources, num_iters, monkeypatch, targets=None):
    """The device operator every way it can be reached: the dispatcher op, the C ABI polled, the C ABI with a fixed number of
    levels.  ``graph`` lives on the device."""
    from ultra_torchdrug_amd import functional as UF
    dev = _dev()
    sources = torch.as_tensor(np.asarray(sources), dtype=torch.long).to(dev)
    targets = None if targets is None else targets.to(dev)
    runs = {"torch": UF.hop_distance(graph.relcsr, sources, num_iters, targets),
            "torch fixed": UF.hop_distance(graph.relcsr, sources, num_iters, targets, poll=False)}
    monkeypatch.setenv("ULTRA_BINDING", "ctypes")
    runs["ctypes"] = UF.hop_distance(graph.relcsr, sources, num_iters, targets)
    runs["ctypes poll"] = UF.hop_distance(graph.relcsr, sources, num_iters, targets, poll=True)
    runs["ctypes fixed"] = UF.hop_distance(graph.relcsr, sources, num_iters, targets, poll=False)
    monkeypatch.delenv("ULTRA_BINDING")
    return runs


@pytest.fixture(scope="module")
def cases():
    """Every graph of tests/test_hop_distance_cpu.py: name -> (n, node_in, node_out, weight, sources, num_iters, definition)."""
    out = {}
    for name, (n, node_in, node_out, sources) in small_graphs().items():
        for num_iters in (100, 2, 0):
            out["%s/%d" % (name, num_iters)] = (n, node_in, node_out, None, sources, num_iters,
                                                iteration_form(n, node_in, node_out, sources, num_iters).numpy())
    n, node_in, node_out = path_graph(130)
    for num_iters in (100, 1, 0):
        out["path/%d" % num_iters] = (n, node_in, node_out, None, [0, 3, 129], num_iters,
                                      iteration_form(n, node_in, node_out, [0, 3, 129], num_iters).numpy())
    for group in (16, 32, 64):
        n, node_in, node_out = star_with_rows(group)
        sources = [0, 6, 7, int(node_in[5000]), n - 1, 6]
        out["star%d" % group] = (n, node_in, node_out, None, sources, 100, queue_form(n, node_in, node_out, sources))
        out["star%d/3" % group] = (n, node_in, node_out, None, sources, 3, iteration_form(n, node_in, node_out, sources, 3).numpy())
    for n in (1000, 1031):
        node_in, node_out = random_edges(n, 3 * n, seed=n)
        rng = np.random.default_rng(n + 1)
        sources = rng.integers(0, n, 129)
        sources[1] = sources[0]
        sources[128] = sources[64]
        want = queue_form(n, node_in, node_out, sources)
        for n_source in (1, 63, 64, 65, 129):
            out["random%d/%d" % (n, n_source)] = (n, node_in, node_out, None, sources[:n_source], 100, want[:, :n_source])
        if n == 1031:
            weight = np.random.default_rng(5).choice(np.array([0.0, 0.5, 1.0], dtype=np.float32), size=len(node_in), p=[0.4, 0.3, 0.3])
            keep = weight != 0
            out["zero weights"] = (n, node_in, node_out, weight, sources[:70], 100,
                                   queue_form(n, node_in[keep], node_out[keep], sources[:70]))
    return out


def test_device_equals_cpu_key_and_definition_every_way(cases, monkeypatch):
    from ultra_torchdrug_amd import _lib
    graphs = {}
    groups = set()
    for name, (n, node_in, node_out, weight, sources, num_iters, want) in cases.items():
        key = (n, len(node_in), weight is not None)
        if key not in graphs:
            host = graph_of(n, node_in, node_out, weight)
            graphs[key] = (host, host.to(_dev()))
        host, graph = graphs[key]
        cpu = host.hop_distance(sources, num_iters)
        assert np.array_equal(cpu.numpy(), want), name
        for how, got in _device_runs(graph, sources, num_iters, monkeypatch).items():
            assert got.dtype == torch.int32 and got.is_cuda and torch.equal(got.cpu(), cpu), (name, how)
        row_ptr, src, _, w = graph.relcsr.csr_arrays
        assert weight is None or w is not None                        # (merged duplicates also make a weight array)
        mean = src.numel() // n
        groups.add(64 if mean >= 48 else 32 if mean >= 24 else 16)
    assert groups == {16, 32, 64}                                     # every lane-group size of the level kernel ran
    assert _lib.ABI_VERSION == 8


def test_reweighted_and_removed_edges_on_the_device(cases, monkeypatch):
    n, node_in, node_out, weight, sources, _, want = cases["zero weights"]
    dev = _dev()
    graph = graph_of(n, node_in, node_out).to(dev)
    got = graph.reweighted(_t(weight).to(dev)).hop_distance(_t(sources).to(dev))
    assert np.array_equal(got.cpu().numpy(), want)
    # Graph.without_triples on a graph with inverse edges: its csr_arrays carry the zeros (the removal is a device launch, so
    # this case has no CPU twin)
    base = np.random.default_rng(9)
    h, t, r = base.integers(0, 400, 1500), base.integers(0, 400, 1500), base.integers(0, 3, 1500)
    fact = graph_of(400, h, t, n_rel=3, rel=r)
    und = fact.undirected(add_inverse=True).to(dev)
    gone = np.arange(0, 1500, 3)
    cut = und.without_triples(_t(h[gone]).to(dev), _t(t[gone]).to(dev), _t(r[gone]).to(dev), 3)
    assert cut.relcsr.csr_arrays[3] is not None and int((cut.relcsr.csr_arrays[3] == 0).sum()) > 0
    triple = set(zip(h[gone].tolist(), t[gone].tolist(), r[gone].tolist()))
    keep = np.array([(a, b, c) not in triple for a, b, c in zip(h.tolist(), t.tolist(), r.tolist())])
    node_in, node_out = np.concatenate([h[keep], t[keep]]), np.concatenate([t[keep], h[keep]])
    sources = np.arange(0, 400, 5)
    want = queue_form(400, node_in, node_out, sources)
    for how, got in _device_runs(cut, sources, 100, monkeypatch).items():
        assert np.array_equal(got.cpu().numpy(), want), how
    assert not np.array_equal(und.hop_distance(_t(sources).to(dev)).cpu().numpy(), want)


@pytest.mark.parametrize("per_source", [1, 7])
def test_targets_form_on_the_device(cases, monkeypatch, per_source):
    n, node_in, node_out, _, sources, _, want = cases["random1000/129"]
    graph = graph_of(n, node_in, node_out).to(_dev())
    rng = np.random.default_rng(per_source)
    targets = rng.integers(0, n, (129, per_source))
    targets[:, 0] = sources
    v, b = np.argwhere(want == n)[0]
    targets[b, per_source - 1] = v
    gathered = np.take_along_axis(want.T, targets, axis=1)
    for how, got in _device_runs(graph, sources, 100, monkeypatch, _t(targets)).items():
        assert got.shape == (129, per_source) and np.array_equal(got.cpu().numpy(), gathered), how
    capped = np.where(gathered <= 3, gathered, n)
    for how, got in _device_runs(graph, sources, 3, monkeypatch, _t(targets)).items():
        assert np.array_equal(got.cpu().numpy(), capped), how


@pytest.mark.parametrize("binding", ["torch", "ctypes"])
def test_captured_into_a_hipgraph(cases, monkeypatch, binding):
    from ultra_torchdrug_amd import functional as UF
    dev = _dev()
    n, node_in, node_out, _, sources, _, _ = cases["random1031/129"]
    want = queue_form(n, node_in, node_out, sources, 6)
    graph = graph_of(n, node_in, node_out).to(dev)
    monkeypatch.setenv("ULTRA_BINDING", binding)
    first, second = _t(sources[:70]).to(dev), _t(sources[59:129]).to(dev)
    targets = _t(np.random.default_rng(1).integers(0, n, (70, 5))).to(dev)
    static = first.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        UF.hop_distance(graph.relcsr, static, 6)                       # warm-up: the CSR arrays and the workspace exist
        UF.hop_distance(graph.relcsr, static, 6, targets)
    torch.cuda.current_stream().wait_stream(side)
    captured = torch.cuda.CUDAGraph()
    with torch.cuda.graph(captured, stream=side):
        matrix = UF.hop_distance(graph.relcsr, static, 6)
        pairs = UF.hop_distance(graph.relcsr, static, 6, targets)
    for start, fresh in ((0, first), (59, second)):
        static.copy_(fresh)
        captured.replay()
        torch.cuda.synchronize()
        assert np.array_equal(matrix.cpu().numpy(), want[:, start:start + 70]), start
        assert torch.equal(matrix, UF.hop_distance(graph.relcsr, fresh, 6)), start
        assert torch.equal(pairs, matrix.t().gather(1, targets)), start


@pytest.fixture(scope="module")
def zipf():
    """3 000 nodes, 10 000 Zipf triples with their inverses (20 000 edges): 130 sources once through the queue BFS."""
    g = kg_graph(21, 3000, 10000, 5)
    sources = np.random.default_rng(2).integers(0, 3000, 130)
    return {"graph": graph_of(3000, g["src"], g["dst"], n_rel=10, rel=g["rel"]), "sources": sources,
            "want": queue_form(3000, g["src"], g["dst"], sources)}


@pytest.mark.parametrize("n_source", [64, 130])
def test_zipf_graph_matrix_and_targets(zipf, monkeypatch, n_source):
    graph, sources, want = zipf["graph"].to(_dev()), zipf["sources"][:n_source], zipf["want"][:, :n_source]
    assert int(want.max()) == 3000 and int(np.bincount(zipf["graph"].edge_list[:, 1].numpy()).max()) > 500      # hubs, unreachable nodes
    targets = np.random.default_rng(n_source).integers(0, 3000, (n_source, 9))
    for how, got in _device_runs(graph, sources, 100, monkeypatch).items():
        assert np.array_equal(got.cpu().numpy(), want), how
    for how, got in _device_runs(graph, sources, 100, monkeypatch, _t(targets)).items():
        assert np.array_equal(got.cpu().numpy(), np.take_along_axis(want.T, targets, axis=1)), how


def test_bad_arguments_raise_on_the_device():
    from ultra_torchdrug_amd import functional as UF
    dev = _dev()
    n, node_in, node_out, _ = small_graphs()["two_components"]
    row_ptr, src, _, w = graph_of(n, node_in, node_out).to(dev).relcsr.csr_arrays
    sources = torch.tensor([0, 5], device=dev)
    UF.hop_distance((row_ptr, src, w), sources)
    with pytest.raises(ValueError):
        UF.hop_distance((row_ptr, src, w), sources, num_iters=-1)
    for poll in (None, False):                                         # the dispatcher op and the C ABI path
        for bad in (torch.tensor([0, n], device=dev), torch.tensor([-1, 0], device=dev)):
            with pytest.raises(RuntimeError):
                UF.hop_distance((row_ptr, src, w), bad, poll=poll)
            with pytest.raises(RuntimeError):
                UF.hop_distance((row_ptr, src, w), sources, targets=bad[:, None], poll=poll)
        with pytest.raises(RuntimeError):
            UF.hop_distance((row_ptr.long(), src.long(), w), sources, poll=poll)
        with pytest.raises(RuntimeError):
            UF.hop_distance((row_ptr, src, w), sources.cpu(), poll=poll)          # mixed devices
        with pytest.raises(RuntimeError):
            UF.hop_distance((row_ptr.flip(0), src, w), sources, poll=poll)
    with pytest.raises(RuntimeError):
        UF.hop_distance((row_ptr.cpu(), src.cpu(), None), sources)


def test_task_and_engine_on_a_codexs_sized_graph():
    """2 034 nodes, Zipf triples: ``task.hop_distance`` and ``evaluate_by_distance`` on the device against the CPU task."""
    from ultra_torchdrug_amd import engine
    from ultra_torchdrug_amd.data import synthetic_kg
    from ultra_torchdrug_amd.graph import Graph
    dev = _dev()
    full = synthetic_kg("S-codexs")
    graph = Graph(full.edge_list[::8].contiguous(), None, full.num_node, full.num_relation)      # sparse enough for real depth
    task = small_task(graph)
    g = torch.Generator().manual_seed(8)
    triples = torch.cat([graph.edge_list[torch.randint(0, graph.num_edge, (12,), generator=g)],
                         torch.stack([torch.randint(0, 2034, (36,), generator=g), torch.randint(0, 2034, (36,), generator=g),
                                      torch.randint(0, graph.num_relation, (36,), generator=g)], dim=1)])
    cpu_distance = {k: task.hop_distance(triples, num_iters=k) for k in (100, 2)}
    cpu_buckets, _, _ = engine.evaluate_by_distance(task, triples, batch_size=8)
    assert len(set(cpu_distance[100].tolist())) >= 4                  # several distances occur
    task = task.to(dev)
    for k, want in cpu_distance.items():
        assert torch.equal(task.hop_distance(triples.to(dev), num_iters=k).cpu(), want), k
    by_distance, distance, ranking = engine.evaluate_by_distance(task, triples, batch_size=8)
    assert torch.equal(distance.cpu(), cpu_distance[2])
    assert set(by_distance) == set(cpu_buckets) and "beyond" in by_distance
    assert {k: v["count"] for k, v in by_distance.items()} == {k: v["count"] for k, v in cpu_buckets.items()}
    plain = engine.evaluate(task, triples, batch_size=8)
    assert torch.equal(plain[1], ranking)
    for name, bucket in by_distance.items():
        mask = (distance > 2) if name == "beyond" else (distance == name)
        for key, value in task.evaluate(ranking[mask]).items():
            assert torch.equal(bucket[key], value), (name, key)
    # answers with hops on the device == the CPU definition at the device's own entities
    anchor, relation = triples[:9, 0].to(dev), triples[:9, 2].to(dev)
    entities, scores, hops = task.answer(anchor, relation, k=10, with_hops=True)
    again = engine.answer(task, anchor, relation, k=10, batch_size=2, with_hops=True)
    e = graph.edge_list.numpy()
    table = queue_form(2034, np.concatenate([e[:, 0], e[:, 1]]), np.concatenate([e[:, 1], e[:, 0]]), anchor.cpu().numpy(), 2)
    assert np.array_equal(hops.cpu().numpy(), table[entities.cpu().numpy(), np.arange(9)[:, None]])
    assert torch.equal(again[0], entities) and torch.equal(again[2], hops)
    plain = task.answer(anchor, relation, k=10)
    assert len(plain) == 2 and torch.equal(plain[0], entities) and torch.equal(plain[1], scores)


def test_models_return_the_reference_layout_on_the_device():
    from ultra_torchdrug_amd.model import TransferNBFNet
    from ultra_torchdrug_amd.rel_model import RelNBFNet
    dev = _dev()
    task = small_task(wide_graph())
    rel_graph = task.rel_graphs[0]
    e = rel_graph.edge_list.numpy()
    n = rel_graph.num_node
    every = task.rel_models[0]._get_shortest_distance(rel_graph.to(dev), num_iters=3)
    assert every.shape == (n, n) and every.dtype == torch.int32 and every.is_cuda
    assert torch.equal(every.cpu(), iteration_form(n, e[:, 0], e[:, 1], list(range(n)), 3))
    assert isinstance(task.rel_models[0], RelNBFNet) and isinstance(task.model, TransferNBFNet)
    n2, node_in, node_out, sources = small_graphs()["two_components"]
    got = task.model._get_shortest_distance(graph_of(n2, node_in, node_out).to(dev), torch.tensor(sources, device=dev))
    assert got.shape == (n2, len(sources)) and got.dtype == torch.int32
    assert torch.equal(got.cpu(), iteration_form(n2, node_in, node_out, sources))

"""TransferNBFNet.visualize on the CPU (``--gpus null``): the beam-search step's CPU operator against the pure-torch restatement of
its documented semantics (tests/explain_restatement.py), a hand-computed case, and the whole explanation on a tiny model."""
import json
import os

import pytest
import torch

from explain_restatement import beam_inputs, beam_step, coalesced_csr, csr_of

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "explain_handcomputed.json")


def _op(*args):
    from ultra_torchdrug_amd import functional
    return functional.beam_search_step(*args)


def _tail_with_both_directions(row_ptr, src):
    """A node that has in-edges and out-edges."""
    deg_in = (row_ptr[1:] - row_ptr[:-1]).long()
    has_out = torch.zeros_like(deg_in, dtype=torch.bool)
    has_out[src.long()] = True
    return int(((deg_in > 0) & has_out).nonzero()[0])


@pytest.mark.parametrize("K", [1, 3, 10, 32])
def test_cpu_operator_equals_the_restatement(K):
    """Random graphs with duplicate triples, isolated nodes and self-loops; a row with more than 64 K candidates; near-equal and
    exactly tied values; a tail with in- and out-edges and one without out-edges; a dense graph (mean in-degree above 48, the
    one the GPU test runs on 64 lanes per row) with non-finite gradients."""
    cases = [coalesced_csr(1, 200, 3000, 5, isolated=20, self_loops=50, duplicates=300),
             coalesced_csr(2, 3000, 4000 + 300 * K, 3, hub_row=7, hub_edges=300 * K + 300, duplicates=50),
             coalesced_csr(9, 403, 40000, 11, isolated=15, hub_row=5, hub_edges=1500, self_loops=40, duplicates=200)]
    for i, (row_ptr, src) in enumerate(cases):
        n = row_ptr.numel() - 1
        beams, grad = beam_inputs(10 + (3 if i == 2 else i), n, K, src.numel(), empty=0.1)     # the GPU test's seeds
        if i == 2:
            assert src.numel() // n >= 48
            grad[::17] = float("nan")
            grad[3::19] = float("inf")
        for tail in (_tail_with_both_directions(row_ptr, src), n - 1):
            got = _op(row_ptr, src, grad, beams, tail)
            want = beam_step(row_ptr, src, grad, beams, tail)
            for name, a, b in zip(("distance", "back_edge", "back_rank"), got, want):
                assert a.dtype == b.dtype and torch.equal(a, b), (i, tail, name)
            if i == 1:
                hub_src = src[int(row_ptr[7]):int(row_ptr[8])].long()
                assert int(torch.isfinite(beams[hub_src]).sum()) > 64 * K        # candidates of the hub row
                assert torch.isfinite(got[0][7]).sum() == K          # the hub row fills every slot


def test_cpu_operator_on_non_finite_gradients_and_empty_graphs():
    """NaN / inf gradients are not candidates; a graph without edges gives empty slots everywhere."""
    row_ptr, src = coalesced_csr(3, 50, 400, 2)
    beams, grad = beam_inputs(4, 50, 4, src.numel())
    grad[::7] = float("nan")
    grad[3::11] = float("inf")
    grad[5::13] = float("-inf")
    got = _op(row_ptr, src, grad, beams, 0)
    want = beam_step(row_ptr, src, grad, beams, 0)
    assert all(torch.equal(a, b) for a, b in zip(got, want))
    assert torch.isfinite(got[0][got[1] >= 0]).all()
    empty = _op(torch.zeros(6, dtype=torch.int32), torch.zeros(0, dtype=torch.int32), torch.zeros(0), torch.zeros(5, 3), 1)
    assert (empty[0] == float("-inf")).all() and (empty[1] == -1).all() and (empty[2] == -1).all()


def test_cpu_operator_refuses_bad_arguments():
    row_ptr, src = csr_of([1, 2, 2], [0, 0, 1], 3)
    grad = torch.zeros(3)
    for K in (0, 33):
        with pytest.raises(ValueError):
            _op(row_ptr, src, grad, torch.zeros(3, K), 0)
    from ultra_torchdrug_amd import _torch_ext
    with pytest.raises(ValueError):                  # the operator itself refuses too (not only the Python wrapper)
        _torch_ext.load().beam_search_step(row_ptr, src, grad, torch.zeros(3, 33), 0)
    with pytest.raises(RuntimeError, match="malformed"):
        _op(row_ptr, torch.tensor([0, 5, 1], dtype=torch.int32), grad, torch.zeros(3, 2), 0)
    with pytest.raises(RuntimeError, match="malformed"):
        _op(torch.tensor([0, 2, 1, 3], dtype=torch.int32), src, grad, torch.zeros(3, 2), 0)
    with pytest.raises(RuntimeError, match="tail"):
        _op(row_ptr, src, grad, torch.zeros(3, 2), 3)


def test_hand_computed_case():
    """tests/golden/explain_handcomputed.json: three layers of the search and the assembled paths, worked out by hand."""
    from types import SimpleNamespace
    from ultra_torchdrug_amd.model import TransferNBFNet
    case = json.load(open(GOLDEN))
    edges = torch.tensor(case["edges"])
    row_ptr = torch.tensor(case["row_ptr"], dtype=torch.int32)
    src = edges[:, 0].to(torch.int32)
    n, K, t = case["n_node"], case["num_beam"], case["tail"]
    beams = torch.full((n, K), float("-inf"))
    beams[case["head"], 0] = 0
    steps = []
    for grad, want in zip(case["edge_grad"], case["tail_rows"]):
        grad = torch.tensor(grad, dtype=torch.float32)
        want_full = beam_step(row_ptr, src, grad, beams, t)
        beams, back_edge, back_rank = _op(row_ptr, src, grad, beams, t)
        assert all(torch.equal(a, b) for a, b in zip((beams, back_edge, back_rank), want_full))
        dist = [float("-inf") if v is None else v for v in want["distance"]]
        assert beams[t].tolist() == dist and back_edge[t].tolist() == want["back_edge"] and back_rank[t].tolist() == want["back_rank"]
        steps.append((beams[t], back_edge, back_rank))
    csr = SimpleNamespace(src=edges[:, 0], dst=edges[:, 1], rel_id=edges[:, 2])
    paths, weights = TransferNBFNet._assemble_paths(csr, steps, t, case["path_topk"])
    assert [[list(e) for e in p] for p in paths] == case["paths"]
    assert list(weights) == case["weights"]


def _tiny_task(aggregate="sum", seed=0):
    from ultra_torchdrug_amd.graph import Graph
    from ultra_torchdrug_amd.task import build_ultra
    torch.manual_seed(seed)
    n, R, T = 40, 3, 160
    g = torch.Generator().manual_seed(seed)
    triples = torch.stack([torch.randint(0, n, (T,), generator=g), torch.randint(0, n, (T,), generator=g),
                           torch.randint(0, R, (T,), generator=g)], 1)
    triples = torch.cat([triples, triples[:5]])                       # duplicate triples
    task = build_ultra(R, hidden_dims=(64,) * 3, rel_layers=2)
    for conv in task.model.layers:
        conv.aggregate_func = aggregate
    task.preprocess(Graph(triples, None, n, R))
    return task.eval(), triples


@pytest.mark.parametrize("aggregate", ["sum", "max", "mean"])
def test_visualize_end_to_end_on_cpu(aggregate):
    """Every path is connected, runs from h to t over triples of the graph with inverse edges; each weight is the f32 sum of the
    path's autograd edge gradients (first hop first, as the layers chain it) over its length, exactly; sorted, at most
    path_topk; no parameter gradient, the module's mode unchanged."""
    task, triples = _tiny_task(aggregate)
    model = task.model
    model.path_topk = 6
    R = task.fact_graph.num_relation
    und = model._undirected(task.fact_graph)
    csr = und.relcsr
    edge_ids = {(int(s), int(d), int(r)): e for e, (s, d, r) in enumerate(zip(csr.src, csr.dst, csr.rel_id))}
    found = 0
    for i in range(6):
        h, t, r = (int(x) for x in triples[i])
        paths, weights = task.visualize(triples[i])
        with torch.no_grad():
            rel = task.relation_representations(torch.tensor([r]))
        grads = model.edge_gradients(task.fact_graph, rel, [h], [t], [r])
        assert len(paths) == len(weights) <= model.path_topk
        assert list(weights) == sorted(weights, reverse=True)
        assert list(zip(weights, paths)) == sorted(zip(weights, paths), reverse=True)
        for path, weight in zip(paths, weights):
            assert path[0][0] == h and path[-1][1] == t
            assert all(a[1] == b[0] for a, b in zip(path, path[1:]))
            assert all(0 <= e[2] < 2 * R and e in edge_ids for e in path)
            total = torch.zeros((), dtype=torch.float32)
            for layer, hop in enumerate(path):
                total = total + grads[layer][edge_ids[hop]].float()
            assert weight == float(total) / len(path)
        found += len(paths)
        head_paths, _ = task.visualize(triples[i], head=True)
        assert all(p[0][0] == t and p[-1][1] == h for p in head_paths)
    assert found > 0
    assert all(p.grad is None for p in task.parameters())
    assert not task.training and not model.training


def test_visualize_refuses_batches_and_beam_counts():
    task, triples = _tiny_task()
    model = task.model
    with torch.no_grad():
        rel = task.relation_representations(triples[:2, 2])
    with pytest.raises(ValueError):
        model.visualize(task.fact_graph, rel, triples[:2, 0], triples[:2, 1], triples[:2, 2])
    for k in (0, 33):
        model.num_beam = k
        with pytest.raises(ValueError):
            task.visualize(triples[0])
    model.num_beam = 32
    task.visualize(triples[0])
    with pytest.raises(ValueError):
        task.visualize(triples[:2])


def test_native_separate_grad_leaves_the_materialised_route_alone():
    """``separate_grad=True`` keeps its graphs (no leaf weights); ``"native"`` on CPU tensors gives every layer a leaf weight
    per original edge on the materialised route."""
    task, triples = _tiny_task()
    model = task.model
    with torch.no_grad():
        rel = task.relation_representations(triples[:1, 2])
    model.query = rel[0]
    for conv in model.layers:
        conv.relation = rel[0]
    und = model._undirected(task.fact_graph)
    h, r = triples[:1, 0], triples[:1, 2]
    old = model.bellmanford(und, h, r, separate_grad=True)["step_graphs"]
    assert all(g.requires_grad and not g.edge_weight.requires_grad and not hasattr(g, "edge_grad_leaf") for g in old)
    with torch.enable_grad():
        new = model.bellmanford(und, h, r, separate_grad="native")["step_graphs"]
    assert all(g.edge_grad_leaf.requires_grad and not g.edge_grad_coalesced and g.edge_grad_leaf.shape == (und.num_edge,)
               for g in new)

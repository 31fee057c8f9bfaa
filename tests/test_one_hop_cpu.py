"""CPU: the one-hop edge removal (``remove_one_hop=True``, ``ultra/model.py:57-74``) above the kernel -- the host branch of
``functional.remove_pairs`` against the reference formulation (``easy_edge_mask`` = ``graph.match`` with a wildcard relation, then
``reweighted``), the binding row of the native entry and the ``remove_one_hop`` keyword of ``build_ultra``."""
import numpy as np
import torch


def _t(a):
    return torch.from_numpy(np.asarray(a))


def _mask_route(model, graph, h, t, r):
    """What ``TransferNBFNet.forward`` does on the mask route: the graph with inverse edges, weight 0 at the masked edges."""
    keep = model.easy_edge_mask(graph, h, t, r)
    und = graph.undirected(add_inverse=True)
    return und, und.reweighted(und.edge_weight * keep.repeat_interleave(2)), keep


def test_remove_pairs_on_a_host_graph_equals_the_mask_route():
    """S-tiny, 8 positives and 4 more columns whose tails are neighbours of the head through some OTHER relation than the
    positive's: the pairs remove strictly more than the triples do, and the host branch of ``functional.remove_pairs`` gives the
    weights of ``easy_edge_mask`` + ``reweighted``."""
    from ultra_torchdrug_amd import functional as UF
    from ultra_torchdrug_amd.data import synthetic_triples
    from ultra_torchdrug_amd.graph import Graph
    from ultra_torchdrug_amd.task import build_ultra
    triples, n, r = synthetic_triples("S-tiny", 1024)
    assert (n, r) == (300, 6)
    graph = Graph(_t(triples), num_node=n, num_relation=r)
    model = build_ultra(r, remove_one_hop=True).model
    pos = _t(triples[:8])
    cols = []
    for hh, tt, rr in triples[:8]:
        # neighbours in either direction (the rule matches both orders); a head with fewer than four lists them again
        out = triples[(triples[:, 0] == hh) & (triples[:, 2] != rr) & (triples[:, 1] != tt)][:, 1]
        inn = triples[(triples[:, 1] == hh) & (triples[:, 2] != rr) & (triples[:, 0] != tt)][:, 0]
        other = np.unique(np.concatenate([out, inn]))
        assert len(other) >= 2
        cols.append(np.resize(other, 4))
    h = pos[:, 0:1].repeat(1, 5)
    t = torch.cat([pos[:, 1:2], _t(np.stack(cols))], dim=1)
    rel = pos[:, 2:3].repeat(1, 5)

    # the 8 positive pairs alone: more edges than the 8 triples themselves
    by_triple = build_ultra(r).model.easy_edge_mask(graph, pos[:, 0:1], pos[:, 1:2], pos[:, 2:3])
    by_pair = model.easy_edge_mask(graph, pos[:, 0:1], pos[:, 1:2], pos[:, 2:3])
    print("edges removed by the 8 triples: %d, by their 8 pairs: %d" % (int((~by_triple).sum()), int((~by_pair).sum())))
    assert int((~by_triple).sum()) == 8
    assert int((~by_pair).sum()) > int((~by_triple).sum())
    assert not (by_pair & ~by_triple).any()                              # a superset of the triples' edges

    und, want, keep = _mask_route(model, graph, h, t, rel)
    assert int((~keep).sum()) > int((~by_pair).sum())                    # the neighbour columns remove edges of their own
    got = UF.remove_pairs(und, h, t)
    assert got.edge_list.data_ptr() == und.edge_list.data_ptr()
    assert torch.equal(got.edge_weight, want.edge_weight)
    assert int((got.edge_weight == 0).sum()) == 2 * int((~keep).sum())
    for plan in ("fwd", "by_src", "by_rel"):
        assert torch.equal(getattr(got.relcsr, plan).weight, getattr(want.relcsr, plan).weight), plan


def test_remove_pairs_special_cases_on_a_host_graph():
    """A pair nothing connects, a pair listed twice and in both orders, a self-loop pair, parallel edges under several relations in
    both directions and ids outside ``[0, N)``: against a plain loop over the edge list."""
    from ultra_torchdrug_amd import functional as UF
    from ultra_torchdrug_amd.graph import Graph
    edges = np.array([[0, 1, 0], [0, 1, 2], [1, 0, 1], [1, 2, 0], [2, 2, 1], [2, 2, 2], [3, 4, 0], [4, 3, 0], [0, 4, 1], [0, 1, 0]])
    graph = Graph(_t(edges), num_node=5, num_relation=3)
    und = graph.undirected(add_inverse=True)
    h = torch.tensor([0, 1, 0, 2, 1, 4, -1, 5, 2 ** 31 + 3, 0])
    t = torch.tensor([1, 0, 1, 2, 3, 3, 1, 0, 4, 2 ** 32 + 1])
    got = UF.remove_pairs(und, h, t)
    pairs = {(0, 1), (1, 0), (2, 2), (1, 3), (3, 1), (4, 3), (3, 4)}
    want = torch.tensor([0.0 if (int(a), int(b)) in pairs else 1.0 for a, b, _ in und.edge_list])
    assert torch.equal(got.edge_weight, want)
    assert int((want == 0).sum()) == 2 * 8                   # (0, 1) x 3 incl. the duplicate, (1, 0), two self loops, (3, 4), (4, 3)
    none = UF.remove_pairs(und, h[:0], t[:0])
    assert torch.equal(none.edge_weight, und.edge_weight)


def test_pair_removal_entry_is_bound():
    """The native entry has a row in the signature table (the header / ``nm -D`` / prototype tests of test_host_logic.py then cover
    it) and the operator is part of the backend."""
    from ultra_torchdrug_amd import _lib, backend, functional
    assert "ultra_pair_removal" in _lib.SIGNATURES and "ultra_pair_removal" in _lib.EXPORTS
    restype, argtypes = _lib.SIGNATURES["ultra_pair_removal"]
    assert restype is _lib.i32 and len(argtypes) == 15 and argtypes[:3] == [_lib.seg] * 3
    assert hasattr(_lib.load(), "ultra_pair_removal")
    assert backend.get() is functional and callable(backend.get().remove_pairs)


def test_build_ultra_forwards_remove_one_hop():
    from ultra_torchdrug_amd.task import build_ultra
    assert build_ultra(4, remove_one_hop=True).model.remove_one_hop is True
    assert build_ultra(4).model.remove_one_hop is False
    task = build_ultra(4, remove_one_hop=True, num_negative=7)           # the other keywords still reach the task
    assert task.num_negative == 7 and task.model.remove_one_hop is True

"""Batched explanations on the CPU (``--gpus null``): ``beam_search_step_batch``'s CPU key against ``beam_search_step`` per query,
``TransferNBFNet.visualize_batch`` / ``edge_gradients_batch`` on CPU tensors (the documented fallback: B single-triple calls)
against the single-triple calls, and the three new C entries in the header and the ctypes signature table."""
import ctypes
import os
import re

import pytest
import torch

from explain_restatement import beam_inputs, coalesced_csr, csr_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = ("ultra_rspmm_backward_weight_blocks_f32", "ultra_rspmm_rotate_backward_weight_blocks_f32",
               "ultra_beam_search_step_batch_f32")


def batch_case(B, K, n=300, seed=0):
    """One graph (a hub row of at least 200 in-edges, trailing rows without edges), per query its own beams (20 % empty rows)
    and gradients (a NaN and an inf in each), and tails of which two are shared when B > 1: ``(row_ptr, src, grad (B, E), beams
    (B, n, K), tails int32 (B,))`` on the CPU."""
    row_ptr, src = coalesced_csr(21 + seed, n, 2400, 4, isolated=25, hub_row=11, hub_edges=260, self_loops=20, duplicates=60)
    assert int(row_ptr[12] - row_ptr[11]) >= 200 and int(row_ptr[n] - row_ptr[n - 20]) == 0
    E = src.numel()
    beams, grads = zip(*[beam_inputs(100 * seed + 7 * b + K, n, K, E, empty=0.2) for b in range(B)])
    beams, grads = torch.stack(beams), torch.stack(grads)
    grads[:, 5::41] = float("nan")
    grads[:, 9::53] = float("inf")
    tails = torch.tensor([int(src[3 + 17 * b]) for b in range(B)], dtype=torch.int32)
    if B > 1:
        tails[-1] = tails[0]                          # two queries share a tail
    return row_ptr, src, grads, beams, tails


def assert_batch_equals_singles(got, row_ptr, src, grads, beams, tails, single):
    for b in range(beams.shape[0]):
        want = single(row_ptr, src, grads[b], beams[b], int(tails[b]))
        for name, a, w in zip(("distance", "back_edge", "back_rank"), got, want):
            assert a[b].dtype == w.dtype and torch.equal(a[b].cpu(), w.cpu()), (b, name)


@pytest.mark.parametrize("K", [1, 10, 32])
@pytest.mark.parametrize("B", [1, 2, 5])
def test_cpu_batch_operator_equals_the_single_step_per_query(B, K):
    from ultra_torchdrug_amd import functional
    row_ptr, src, grads, beams, tails = batch_case(B, K)
    got = functional.beam_search_step_batch(row_ptr, src, grads, beams, tails)
    assert all(tuple(a.shape) == (B, 300, K) for a in got)
    assert_batch_equals_singles(got, row_ptr, src, grads, beams, tails, functional.beam_search_step)
    assert int((got[1] >= 0).sum()) > 0


def test_cpu_batch_operator_refuses_bad_arguments():
    from ultra_torchdrug_amd import _torch_ext, functional
    row_ptr, src = csr_of([1, 2, 2], [0, 0, 1], 3)
    op = functional.beam_search_step_batch
    tails = torch.zeros(2, dtype=torch.int32)
    with pytest.raises(ValueError):                                                   # B = 0
        op(row_ptr, src, torch.zeros(0, 3), torch.zeros(0, 3, 2), torch.zeros(0, dtype=torch.int32))
    with pytest.raises(ValueError):                                                   # K = 33
        op(row_ptr, src, torch.zeros(2, 3), torch.zeros(2, 3, 33), tails)
    raw = _torch_ext.load().beam_search_step_batch                                    # the operator itself refuses too
    with pytest.raises(ValueError):
        raw(row_ptr, src, torch.zeros(0, 3), torch.zeros(0, 3, 2), torch.zeros(0, dtype=torch.int32))
    with pytest.raises(ValueError):
        raw(row_ptr, src, torch.zeros(2, 3), torch.zeros(2, 3, 33), tails)
    with pytest.raises(RuntimeError, match="tail"):                                   # a tail equal to n
        op(row_ptr, src, torch.zeros(2, 3), torch.zeros(2, 3, 2), torch.tensor([0, 3], dtype=torch.int32))
    with pytest.raises(RuntimeError, match="tail"):
        op(row_ptr, src, torch.zeros(2, 3), torch.zeros(2, 3, 2), torch.tensor([-1, 0], dtype=torch.int32))
    for grads, beams, t in ((torch.zeros(3, 3), torch.zeros(2, 3, 2), tails),         # mismatched leading dimensions
                            (torch.zeros(2, 3), torch.zeros(2, 3, 2), torch.zeros(3, dtype=torch.int32)),
                            (torch.zeros(2, 3), torch.zeros(3, 3, 2), tails)):
        with pytest.raises(RuntimeError, match="expected"):
            op(row_ptr, src, grads, beams, t)
    with pytest.raises(RuntimeError, match="malformed"):
        op(row_ptr, torch.tensor([0, 5, 1], dtype=torch.int32), torch.zeros(2, 3), torch.zeros(2, 3, 2), tails)
    ok = op(row_ptr, src, torch.zeros(2, 3), torch.zeros(2, 3, 2), tails)
    assert tuple(ok[0].shape) == (2, 3, 2)


def _tiny_task(aggregate="sum", seed=0):
    """The tiny task of tests/test_explain_cpu.py, with one node that no edge touches."""
    from ultra_torchdrug_amd.graph import Graph
    from ultra_torchdrug_amd.task import build_ultra
    torch.manual_seed(seed)
    n, R, T = 40, 3, 160
    g = torch.Generator().manual_seed(seed)
    triples = torch.stack([torch.randint(0, n, (T,), generator=g), torch.randint(0, n, (T,), generator=g),
                           torch.randint(0, R, (T,), generator=g)], 1)
    triples = torch.cat([triples, triples[:5]])                       # duplicate triples
    task = build_ultra(R, hidden_dims=(64,) * 3, rel_layers=2)
    if aggregate == "pna":                                            # (its epilogue is 13 inputs wide: built as such)
        from ultra_torchdrug_amd.model import TransferNBFNet
        task.model = TransferNBFNet(input_dim=64, hidden_dims=[64] * 3, num_relation=R, message_func="distmult",
                                    aggregate_func="pna", short_cut=True, layer_norm=True, project=True, mod=True)
    else:
        for conv in task.model.layers:
            conv.aggregate_func = aggregate
    task.preprocess(Graph(triples, None, n + 1, R))                   # node n: unreachable
    return task.eval(), triples, n


def _four_triples(triples, unreachable):
    """Two with the same head, one whose tail is unreachable, one duplicate."""
    a = triples[0].clone()
    same_head = torch.stack([a[0], triples[1][1], triples[1][2]])
    lost = torch.stack([triples[2][0], torch.tensor(unreachable), triples[2][2]])
    return torch.stack([a, same_head, lost, a])


@pytest.mark.parametrize("aggregate", ["sum", "pna"])
def test_cpu_model_route_equals_the_single_triple_calls(aggregate):
    """On CPU tensors (and for a ``pna`` stack anywhere) the batch calls take the documented fallback: the same numbers as B
    single-triple calls, exactly; no parameter gradient, the module's mode unchanged."""
    task, triples, unreachable = _tiny_task(aggregate)
    model = task.model
    model.path_topk = 6
    four = _four_triples(triples, unreachable)
    h, t, r = four.unbind(-1)
    with torch.no_grad():
        rel = task.relation_representations(r)
    singles = [model.visualize(task.fact_graph, [x[b:b + 1] for x in rel], h[b:b + 1], t[b:b + 1], r[b:b + 1]) for b in range(4)]
    batch = model.visualize_batch(task.fact_graph, rel, h, t, r)
    assert isinstance(batch, list) and batch == singles
    assert batch[2] == ((), ()) and batch[0] == batch[3] and sum(len(p) for p, _ in batch) > 0
    grads = model.edge_gradients_batch(task.fact_graph, rel, h, t, r)
    want = [model.edge_gradients(task.fact_graph, [x[b:b + 1] for x in rel], h[b:b + 1], t[b:b + 1], r[b:b + 1]) for b in range(4)]
    assert len(grads) == len(model.layers)
    for i, g in enumerate(grads):
        assert g.shape == (4, model._undirected(task.fact_graph).relcsr.n_edges)
        assert torch.equal(g, torch.stack([w[i] for w in want]))
    assert all(p.grad is None for p in task.parameters())
    assert not task.training and not model.training


def test_cpu_task_and_engine_explain():
    """``task.explain`` == ``task.visualize`` per row (both sides); ``engine.explain`` chunks, keeps the order and validates."""
    from ultra_torchdrug_amd import engine
    task, triples, _ = _tiny_task()
    task.model.path_topk = 5
    rows = triples[:7]
    for head in (False, True):
        want = [task.visualize(row, head=head) for row in rows]
        assert task.explain(rows, head=head) == want
        assert engine.explain(task, rows, batch_size=3, head=head) == want
    assert engine.explain(task, rows[:0]) == []
    with pytest.raises(ValueError):
        engine.explain(task, torch.tensor([[0, 1, 99]]))
    with pytest.raises(ValueError):
        engine.explain(task, rows, batch_size=0)
    with pytest.raises(ValueError):
        task.explain(rows[0])
    with pytest.raises(IndexError):
        task.model.edge_gradients_batch(task.fact_graph, task.relation_representations(rows[:2, 2]), [0, 400], [1, 2], [0, 1])


def test_new_entries_are_declared_exported_and_bound():
    """The header declares the three entries, the ctypes table carries them with the header's argument counts, and the ABI
    version has not moved (the plan struct is untouched)."""
    from ultra_torchdrug_amd import _lib, _torch_ext
    header = open(os.path.join(ROOT, "include", "ultra_rspmm.h")).read()
    assert int(re.search(r"#define ULTRA_RSPMM_ABI_VERSION (\d+)", header).group(1)) == 8 == _lib.ABI_VERSION
    for name in NEW_ENTRIES:
        proto = re.search(r"\bint %s\(([^;]*)\);" % name, header)
        assert proto is not None, name
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == proto.group(1).count(",") + 1, name
        assert hasattr(_lib.load(), name)
    assert "beam_search_step_batch" in _torch_ext.OPS


def test_c_abi_refuses_before_any_device_work():
    """No GPU involved: foreign plans, bad shapes, unknown ops and NULL operands are refused first; a plan without edges is
    ULTRA_OK."""
    from ultra_torchdrug_amd import _lib
    lib = _lib.load()
    OK, BAD_OP, BAD_SHAPE, NULL, ABI = 0, 1, 2, 3, 7
    seg = _lib.UltraSegments()
    foreign = _lib.UltraSegments()
    foreign.abi_version = 7
    one_edge = _lib.UltraSegments()
    one_edge.n_rows = one_edge.n_edges = 1
    blocks = lambda F, block, sum_op, mul_op, s=seg: lib.ultra_rspmm_backward_weight_blocks_f32(
        ctypes.byref(s), None, None, None, None, None, 1, F, block, sum_op, mul_op, None)
    rotate = lambda F, block, sum_op, s=seg: lib.ultra_rspmm_rotate_backward_weight_blocks_f32(
        ctypes.byref(s), None, None, None, None, None, 1, F, block, sum_op, None)
    assert blocks(192, 64, 0, 0) == OK and rotate(192, 64, 2) == OK                    # empty plans: nothing to do
    assert blocks(0, 64, 0, 0) == blocks(64, 0, 0, 0) == blocks(96, 64, 0, 0) == blocks(64, -64, 0, 0) == BAD_SHAPE
    assert rotate(0, 64, 0) == rotate(64, 0, 0) == rotate(96, 64, 0) == rotate(42, 7, 0) == BAD_SHAPE
    assert blocks(64, 64, 3, 0) == blocks(64, 64, 0, 2) == blocks(64, 64, -1, 0) == rotate(64, 64, 3) == BAD_OP
    assert blocks(64, 64, 0, 0, foreign) == rotate(64, 64, 0, foreign) == ABI
    assert blocks(96, 64, 0, 0, foreign) == ABI                                          # the fence comes first
    assert blocks(64, 64, 0, 0, one_edge) == rotate(64, 64, 0, one_edge) == NULL
    beam = lambda n_node, n_edges, n_query, K: lib.ultra_beam_search_step_batch_f32(None, None, None, None, None, n_node, n_edges,
                                                                                    n_query, K, None, None, None, None)
    assert beam(5, 0, 1, 0) == beam(5, 0, 1, 33) == beam(5, 0, 0, 4) == beam(-1, 0, 1, 4) == beam(5, 0, 65536, 4) == BAD_SHAPE
    assert beam(0, 0, 2, 4) == OK                                                        # no rows: nothing to do
    assert beam(5, 0, 2, 4) == NULL

"""Training through logical queries without a GPU: the numpy restatements of the two new backwards
(tests/query_grad_definition.py) against ``torch.autograd`` in fp64, ``project_train`` / ``query_loss`` on CPU tensors against the
fp64 ATen definition and ``torch.autograd.gradcheck``, the binding's table rows, the negative sampler, and the refusals of the
C entries, which come before any launch and therefore need no device."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from query_definition import query_ids
from query_grad_definition import (grid_head_case, grid_set_case, keep_mask, score_backward_numpy,
                                   set_boundary_backward_numpy)
from sampled_graphs import ring_graph, small_task, wide_graph


def _finite_set_case(n_query, n_node, dim, seed):
    """The grid case with its planted non-finite values replaced: the torch expression multiplies by zero where the device
    entry selects."""
    member, query, floor, d_boundary = grid_set_case(n_query, n_node, dim, seed)
    query[~np.isfinite(query)] = 0.5
    d_boundary[~np.isfinite(d_boundary)] = -1.25
    return member, query, floor, d_boundary


@pytest.mark.parametrize("n_query,n_node,dim,use_floor", [(1, 1, 6, True), (3, 65, 64, True), (16, 257, 6, False), (5, 63, 8, True)])
def test_set_boundary_definition_is_autograd_of_the_dense_expression(n_query, n_node, dim, use_floor):
    """On finite inputs ``torch.where``'s own backward IS the definition (``functional.dense_set_boundary``'s docstring)."""
    from ultra_torchdrug_amd import functional as UF
    member, query, floor, d_boundary = _finite_set_case(n_query, n_node, dim, seed=n_node)
    floor = floor if use_floor else None
    m = torch.from_numpy(member).double().requires_grad_()
    q = torch.from_numpy(query).double().requires_grad_()
    f = None if floor is None else torch.from_numpy(floor)
    boundary, count = UF.dense_set_boundary(m, q, f, with_count=True)
    assert boundary.dtype == torch.float64 and np.array_equal(count.numpy(), keep_mask(member, floor).sum(axis=1))
    d_m, d_q = torch.autograd.grad(boundary, [m, q], torch.from_numpy(d_boundary).double())
    want_member, want_query = set_boundary_backward_numpy(d_boundary, member, floor, query)
    assert np.array_equal(d_m.numpy(), want_member) and np.array_equal(d_q.numpy(), want_query)          # exact on the grid
    # fp32 CPU tensors take the same expression through functional.set_boundary: the same numbers, still exact
    m32 = torch.from_numpy(member).requires_grad_()
    q32 = torch.from_numpy(query).requires_grad_()
    UF.set_boundary(m32, q32, f).backward(torch.from_numpy(d_boundary))
    assert np.array_equal(m32.grad.numpy().astype(np.float64), want_member)
    assert np.array_equal(q32.grad.numpy().astype(np.float64), want_query)


@pytest.mark.parametrize("n_node,batch", [(1, 1), (33, 3), (257, 16)])
def test_score_head_definition_is_autograd_of_the_aten_head(n_node, batch):
    case = grid_head_case(n_node, batch, seed=n_node, zero_rows=n_node > 5)
    leaves = [torch.from_numpy(a).double().requires_grad_() for a in case[:6]]
    h, q, w1, b1, w2, b2 = leaves
    x = torch.cat([h, q.unsqueeze(0).expand(n_node, -1, -1)], dim=-1)
    score = F.linear(F.relu(F.linear(x, w1, b1)), w2.view(1, 128), b2).squeeze(-1).t()
    got = torch.autograd.grad(score, leaves, torch.from_numpy(case[6]).double())
    want = score_backward_numpy(*case[:5], case[6])
    for g, w in zip(got, want):
        scale = np.abs(w).max() + 1e-300
        assert np.abs(g.numpy().reshape(w.shape) - w).max() <= 1e-12 * scale


def test_the_binding_has_rows_for_both_entries():
    from ultra_torchdrug_amd import _lib
    for name, n_args in (("ultra_set_boundary_backward_f32", 13), ("ultra_set_boundary_backward_workspace", 3),
                         ("ultra_score_backward_f32", 18), ("ultra_score_backward_workspace", 2)):
        assert name in _lib.SIGNATURES and name in _lib.EXPORTS
        assert len(_lib.SIGNATURES[name][1]) == n_args
        assert hasattr(_lib.load(), name)
    assert _lib.SIGNATURES["ultra_set_boundary_backward_workspace"][0] is ctypes.c_size_t
    assert _lib.SIGNATURES["ultra_score_backward_workspace"][0] is ctypes.c_size_t


def test_the_entries_refuse_before_any_launch():
    """Shapes, null pointers and workspaces are checked first: these calls never reach the device (there is none here)."""
    from ultra_torchdrug_amd import _lib
    from ultra_torchdrug_amd import functional as UF
    lib = _lib.load()
    size = int(lib.ultra_set_boundary_backward_workspace(4, 70, 8))
    assert size > 0 and size % 4 == 0
    assert lib.ultra_set_boundary_backward_workspace(0, 70, 8) == 0 and lib.ultra_set_boundary_backward_workspace(4, 70, 0) == 0
    p = 4096                                                        # a non-null address that is never dereferenced on the host
    good = [p, p, 4, 70, 70, p, p, 8, p, p, p, size, None]
    for at, value, status in ((2, 0, 2), (3, 0, 2), (7, 0, 2), (4, 69, 2), (7, 2048, 2), (0, None, 3), (1, None, 3),
                              (6, None, 3), (8, None, 3), (10, None, 3), (11, size - 4, 4)):
        args = list(good)
        args[at] = value
        assert lib.ultra_set_boundary_backward_f32(*args) == status, (at, value)
    good = [p, p, p, p, p, p, 33, p, p, p, p, p, p, p, 1 << 30, 33, 3, None]
    for at, value, status in ((15, 0, 2), (16, 0, 2), (16, 65536, 2), (6, 32, 2), (0, None, 3), (1, None, 3), (2, None, 3), (3, None, 3),
                              (4, None, 3), (5, None, 3), (13, None, 3), (0, p + 4, 2)):
        args = list(good)
        args[at] = value
        assert lib.ultra_score_backward_f32(*args) == status, (at, value)
    assert lib.ultra_score_backward_workspace(0, 3) == 0 and lib.ultra_score_backward_workspace(33, 65536) == 0
    # the Python entries: CPU tensors have no kernel behind them
    member, query, floor, d_boundary = (torch.from_numpy(a) for a in _finite_set_case(3, 9, 4, 1))
    with pytest.raises(RuntimeError):
        UF.set_boundary_backward(d_boundary, member, query, floor)
    hidden, q, w1, b1, w2, b2, grad = (torch.from_numpy(a) for a in grid_head_case(5, 2, seed=1))
    with pytest.raises(RuntimeError):
        UF.score_all_backward(hidden, q, w1, b1, w2, grad)
    with pytest.raises(RuntimeError):
        UF.score_all_entities(hidden.requires_grad_(), q, w1, b1, w2, b2)


def test_sample_query_negatives():
    from ultra_torchdrug_amd import data
    g = torch.Generator().manual_seed(5)
    answers = torch.rand(7, 50, generator=g) < 0.6
    answers[3] = True
    answers[3, 41] = False                                           # one non-answer: every draw is that entity
    answers[4] = False
    first = data.sample_query_negatives(answers, 64, torch.Generator().manual_seed(9))
    again = data.sample_query_negatives(answers, 64, torch.Generator().manual_seed(9))
    other = data.sample_query_negatives(answers, 64, torch.Generator().manual_seed(10))
    assert first.dtype == torch.int64 and first.shape == (7, 64) and torch.equal(first, again) and not torch.equal(first, other)
    assert int(first.min()) >= 0 and int(first.max()) < 50
    assert not answers.gather(1, first).any()
    assert (first[3] == 41).all()
    assert len(set(first[4].tolist())) > 20                          # uniform over 50 entities, with replacement
    for q in range(7):                                               # every non-answer can be drawn
        free = set((~answers[q]).nonzero().flatten().tolist())
        many = data.sample_query_negatives(answers[q:q + 1], 2000, torch.Generator().manual_seed(q))
        assert set(many[0].tolist()) == free
    with pytest.raises(ValueError):
        data.sample_query_negatives(torch.ones(2, 5, dtype=torch.bool), 3)
    with pytest.raises(ValueError):
        data.sample_query_negatives(answers.float(), 3)
    with pytest.raises(ValueError):
        data.sample_query_negatives(answers, 0)


# ------------------------------------------------------------------------------------------------ model, task, engine on the CPU
@pytest.fixture(scope="module")
def cpu16():
    return small_task(wide_graph())


def _loss_inputs(name, seed, n_node=300, n_rel2=10):
    anchors, relations = query_ids(name, 3, n_node, n_rel2, seed=seed)
    g = torch.Generator().manual_seed(seed + 1)
    return anchors, relations, torch.randint(0, n_node, (3,), generator=g), torch.randint(0, n_node, (3, 5), generator=g)


def _gradients(task, loss):
    named = list(task.named_parameters())
    grads = torch.autograd.grad(loss, [p for _, p in named], allow_unused=True)
    return {n: g.detach().double() for (n, _), g in zip(named, grads) if g is not None}


@pytest.mark.parametrize("name", ["2p", "2i", "ip", "2in", "2u"])
def test_query_loss_on_the_cpu_against_the_fp64_definition(cpu16, name):
    from aten_definition import aten_definition
    task = cpu16
    inputs = _loss_inputs(name, seed=len(name))

    def run():
        with torch.enable_grad():
            loss = task.query_loss(name, *inputs)
            return loss.detach(), _gradients(task, loss)

    mine, g_mine = run()
    with aten_definition(task):
        aten, g_aten = run()
    with aten_definition(task, double=True):
        truth, g_true = run()
        assert truth.dtype == torch.float64
    assert mine.dim() == 0 and mine.dtype == torch.float32
    e_mine, e_aten = abs(float(mine) - float(truth)), abs(float(aten) - float(truth))
    assert e_mine <= 4 * e_aten + 1e-5 * abs(float(truth)), (e_mine, e_aten)
    assert set(g_mine) == set(g_true) and len(g_true) > 10
    for key in g_true:
        scale = float(g_true[key].abs().max()) + 1e-12
        e_mine, e_aten = float((g_mine[key] - g_true[key]).abs().max()), float((g_aten[key] - g_true[key]).abs().max())
        assert e_mine <= 4 * e_aten + 5e-4 * scale, (key, e_mine, e_aten, scale)
    # the definition of the loss itself, from the memberships
    with torch.no_grad():
        tree, anchors, relations = task.query_inputs(name, inputs[0], inputs[1])
        p = task.query_memberships(tree, anchors, relations, differentiable=True)
        frozen = task.query_memberships(tree, anchors, relations)
        assert float((p - frozen).abs().max()) <= 1e-5                          # the one-hot first hop is the single-source route
        pos = -torch.log(p.gather(1, inputs[2][:, None])).clamp(max=100).squeeze(1)
        neg = -torch.log(1 - p.gather(1, inputs[3])).clamp(max=100).mean(dim=1)
        assert abs(float((0.5 * (pos + neg)).mean()) - float(mine)) <= 1e-6 * abs(float(mine))


def test_cuts_are_masks_and_an_empty_set_gives_no_gradient(cpu16):
    task = cpu16
    anchors, relations, positives, negatives = _loss_inputs("2p", seed=4)
    with torch.enable_grad():
        cut = task.query_loss("2p", anchors, relations, positives, negatives, max_sources=12)
        g_cut = _gradients(task, cut)
        empty = task.query_loss("2p", anchors, relations, positives, negatives, threshold=0.9999)
        g_empty = torch.autograd.grad(empty, list(task.parameters()), allow_unused=True)
    assert any(float(g.abs().max()) > 0 for g in g_cut.values())
    # every intermediate set is empty: zero rows, BCE(0, 1) clamps at 100 and BCE(0, 0) is 0
    assert abs(float(empty.detach()) - 50.0) <= 1e-4
    assert all(g is None or not g.any() for g in g_empty)
    for bad in (dict(positives=positives[:2]), dict(negatives=negatives[:, :0]), dict(positives=positives.int()),
                dict(negatives=negatives + 300), dict(positives=positives - 300)):
        with pytest.raises(ValueError):
            task.query_loss("2p", **dict(dict(anchors=anchors, relations=relations, positives=positives, negatives=negatives), **bad))
    with pytest.raises(ValueError):
        task.query_loss("2p", anchors, relations, positives, negatives, max_sources=0)


def test_project_train_gradcheck_in_fp64_on_a_6_wide_model():
    from aten_definition import aten_definition
    from ultra_torchdrug_amd.task import build_ultra
    graph = ring_graph()
    torch.manual_seed(3)
    task = build_ultra(graph.num_relation, hidden_dims=(6,) * 2, input_dim=6, rel_hidden=6, rel_layers=2, num_negative=4,
                       full_batch_eval=True)
    task.preprocess(graph)
    task.eval()
    rel = torch.tensor([1, 4])
    g = torch.Generator().manual_seed(2)
    member = (torch.randint(8, 17, (2, 64), generator=g).double() / 16)
    member[:, ::3] = 0.125                                           # below the floor, and a finite difference keeps them there
    floor = torch.full((2,), 0.3)
    with aten_definition(task, double=True):
        reps = [r.detach() for r in task.relation_representations(rel % 3)]

        def logits(m, *relation):
            return task.model.project_train(task.fact_graph, list(relation), m, rel, floor)[0]

        assert torch.autograd.gradcheck(logits, (member.requires_grad_(), *[r.requires_grad_() for r in reps]), eps=1e-6,
                                        atol=1e-6, rtol=1e-4, nondet_tol=1e-9)
        with torch.no_grad():                                        # without grad project_train IS project
            a = task.model.project_train(task.fact_graph, reps, member.detach(), rel, floor)
            b = task.model.project(task.fact_graph, reps, member.detach(), rel, floor)
            assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_ten_training_steps_lower_the_loss_on_the_cpu():
    from ultra_torchdrug_amd import engine
    from ultra_torchdrug_amd import data
    task = small_task(wide_graph()).train()              # a task of its own: the steps change the weights
    # a batch as training makes one: grounded queries, their targets as positives, negatives among the non-answers
    g = torch.Generator().manual_seed(33)
    anchors, relations, targets = data.sample_queries(task.message_graph(), "2p", 8, g)
    answers = task.query_answers("2p", anchors, relations, graph="filter")
    assert bool(answers.gather(1, targets[:, None]).all())
    inputs = (anchors, relations, targets, data.sample_query_negatives(answers, 16, g))
    with torch.no_grad():
        start = float(task.query_loss("2p", *inputs))
    optimizer = torch.optim.Adam(task.parameters(), lr=5e-3)
    first, metric = engine.train_query_step(task, optimizer, "2p", *inputs)
    assert abs(float(first) - start) <= 1e-5 * abs(start) and not first.requires_grad
    assert list(metric) == ["query binary cross entropy"]
    for _ in range(9):
        engine.train_query_step(task, optimizer, "2p", *inputs)
    with torch.no_grad():
        end = float(task.query_loss("2p", *inputs))
    assert end < start, (start, end)
    assert task.training

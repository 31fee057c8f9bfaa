"""MI355X: training through logical queries.

Kernel A, ``ultra_set_boundary_backward_f32``: inputs on the dyadic grid of tests/exact_grid.py, where every product and every
partial sum is exact in fp32, so the result EQUALS the numpy definition (tests/query_grad_definition.py) entry for entry.
Kernel B, ``ultra_score_backward_f32``: grid inputs again (no ReLU side can differ between fp32 and fp64), each gradient held to
the project's operator bar against the fp64 definition with ATen-fp32 autograd as the yardstick.  Then what the launches touch
(guard-banded allocations; one case past 2^32 bytes per entry), and the model, task and engine levels against the fp64 ATen
definition (tests/aten_definition.py)."""
import collections

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from query_definition import query_ids
from query_grad_definition import (grid_head_case, grid_set_case, keep_mask, score_backward_numpy,
                                   set_boundary_backward_numpy)
from sampled_graphs import small_task, wide_graph

pytestmark = pytest.mark.gpu

HEAD_NAMES = ("d_hidden", "d_query", "d_w1", "d_b1", "d_w2", "d_b2")


def _dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _bits(t):
    return t.contiguous().view(torch.int32)


def _bars(mine, aten, truth, what):
    """The operator bar of tests/test_query_gpu.py."""
    scale = float(truth.abs().max())
    e_hip, e_aten = float((mine.double() - truth).abs().max()), float((aten.double() - truth).abs().max())
    print("%s: HIP %.3g, ATen fp32 %.3g away from the fp64 definition (scale %.3g)" % (what, e_hip, e_aten, scale))
    assert e_hip <= 4 * e_aten + 1e-5 * scale, (what, e_hip, e_aten, scale)
    assert e_hip <= 2e-4 * scale, (what, e_hip, scale)


def _gradient_bar(mine, aten, truth, what):
    """The bar tests/test_reference_definition_gpu.py gives stack gradients: a pre-activation within fp32 rounding of zero may
    land on the other side of a ReLU than in fp64, hence the floor of 5e-4 of the gradient's scale."""
    scale = float(truth.abs().max()) + 1e-12
    e_hip, e_aten = float((mine.double() - truth).abs().max()), float((aten.double() - truth).abs().max())
    print("%s: HIP %.3g, ATen fp32 %.3g away from fp64 (scale %.3g)" % (what, e_hip, e_aten, scale))
    assert e_hip <= 4 * e_aten + 5e-4 * scale, (what, e_hip, e_aten, scale)


# ------------------------------------------------------------------------------------------------ kernel A
def _check_set(n_query, n_node, dim, seed, use_floor, pad=0, with_query=True):
    """``functional.set_boundary_backward`` on device copies against the numpy definition, no tolerance; the kept counts."""
    from ultra_torchdrug_amd import functional as UF
    dev = _dev()
    member, query, floor, d_boundary = grid_set_case(n_query, n_node, dim, seed)
    if not use_floor:
        floor = None
    wide = torch.full((n_query, n_node + pad), 0.75, device=dev)
    wide[:, :n_node] = torch.from_numpy(member).to(dev)
    member_d = wide[:, :n_node]
    query_d, grad_d = torch.from_numpy(query).to(dev), torch.from_numpy(d_boundary).to(dev)
    floor_d = None if floor is None else torch.from_numpy(floor).to(dev)
    want_member, want_query = set_boundary_backward_numpy(d_boundary, member, floor, query)
    d_member, d_query = UF.set_boundary_backward(grad_d, member_d, query_d, floor_d, want_query=with_query)
    what = (n_query, n_node, dim, use_floor, pad, with_query)
    assert d_member.dtype == torch.float32 and tuple(d_member.shape) == (n_query, n_node) and d_member.is_contiguous(), what
    assert np.array_equal(d_member.cpu().numpy().astype(np.float64), want_member), what
    keep = keep_mask(member, floor)
    assert not _bits(d_member).cpu().numpy()[~keep].any(), what                      # +0.0 BITS where nothing is kept
    if with_query:
        assert d_query.dtype == torch.float32 and tuple(d_query.shape) == (n_query, dim), what
        assert np.array_equal(d_query.cpu().numpy().astype(np.float64), want_query), what
    else:
        assert d_query is None
    again = UF.set_boundary_backward(grad_d, member_d, query_d, floor_d, want_query=with_query)
    assert torch.equal(_bits(again[0]), _bits(d_member)), what
    assert not with_query or torch.equal(_bits(again[1]), _bits(d_query)), what
    return keep.sum(axis=1)


@pytest.mark.parametrize("dim", [64, 6])
@pytest.mark.parametrize("n_node", [1, 63, 64, 65, 1031])
def test_set_boundary_backward_equals_the_definition_exactly(n_node, dim):
    for n_query in (1, 3, 16, 33):
        seed = 1000 * n_node + 10 * n_query + dim
        for use_floor in (False, True):
            for pad in (0, 5):
                kept = _check_set(n_query, n_node, dim, seed, use_floor, pad=pad)
        if n_node >= 63:
            assert 0 < kept[0] < n_node and (n_query < 2 or 0 < kept[1] < n_node)      # both floors cut
            assert n_query < 3 or kept[2] == 0                                         # and row 2 keeps nothing
        _check_set(n_query, n_node, dim, seed, True, with_query=False)


@pytest.mark.parametrize("n_query,dim", [(2, 64), (33, 6)])
def test_set_boundary_backward_on_a_long_row(n_query, dim):
    """70 001 nodes: terms of size at most 4 in units of 1/16, 70 001 * 4 * 16 < 2^24, still exact."""
    kept = _check_set(n_query, 70_001, dim, 7, True, pad=3)
    assert 0 < kept[0] < 70_001
    _check_set(n_query, 70_001, dim, 8, False)


def test_set_boundary_backward_captured_into_a_hipgraph():
    from ultra_torchdrug_amd import functional as UF
    dev = _dev()
    cases = [grid_set_case(5, 1031, 64, seed) for seed in (1, 2, 3)]
    member, query, floor, d_boundary = (torch.from_numpy(a).to(dev) for a in cases[0])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        UF.set_boundary_backward(d_boundary, member, query, floor)                   # warm-up: the outputs enter the allocator's cache
    torch.cuda.current_stream().wait_stream(side)
    captured = torch.cuda.CUDAGraph()
    with torch.cuda.graph(captured, stream=side):
        d_member, d_query = UF.set_boundary_backward(d_boundary, member, query, floor)
    for case in cases:
        for static, new in zip((member, query, floor, d_boundary), case):
            static.copy_(torch.from_numpy(new).to(dev))
        captured.replay()
        torch.cuda.synchronize()
        want_member, want_query = set_boundary_backward_numpy(case[3], case[0], case[2], case[1])
        assert np.array_equal(d_member.cpu().numpy().astype(np.float64), want_member)
        assert np.array_equal(d_query.cpu().numpy().astype(np.float64), want_query)


def test_set_boundary_backward_through_autograd():
    from ultra_torchdrug_amd import functional as UF
    dev = _dev()
    for n_query, n_node, dim, use_floor in ((3, 65, 64, True), (16, 1031, 6, False)):
        member, query, floor, d_boundary = grid_set_case(n_query, n_node, dim, 11)
        floor = floor if use_floor else None
        member_d = torch.from_numpy(member).to(dev).requires_grad_()
        query_d = torch.from_numpy(query).to(dev).requires_grad_()
        floor_d = None if floor is None else torch.from_numpy(floor).to(dev)
        plain = UF.set_boundary(member_d.detach(), query_d.detach(), floor_d, with_count=True)
        boundary, count = UF.set_boundary(member_d, query_d, floor_d, with_count=True)
        assert boundary.requires_grad and not count.requires_grad
        assert torch.equal(_bits(boundary), _bits(plain[0])) and torch.equal(count, plain[1])      # today's launch, today's bits
        boundary.backward(torch.from_numpy(d_boundary).to(dev))
        want_member, want_query = set_boundary_backward_numpy(d_boundary, member, floor, query)
        assert np.array_equal(member_d.grad.cpu().numpy().astype(np.float64), want_member)
        assert np.array_equal(query_d.grad.cpu().numpy().astype(np.float64), want_query)
        with torch.no_grad():
            assert not UF.set_boundary(member_d, query_d, floor_d).requires_grad


# ------------------------------------------------------------------------------------------------ kernel B
def _head_tensors(case):
    return [torch.from_numpy(a).to(_dev()) for a in case]


def _aten_head(hidden, query, w1, b1, w2, b2, grad):
    """ATen-fp32 autograd of the materialised head: ``cat``, two ``F.linear``, relu."""
    leaves = [t.detach().clone().requires_grad_() for t in (hidden, query, w1, b1, w2, b2)]
    h, q, a1, c1, a2, c2 = leaves
    x = torch.cat([h, q.unsqueeze(0).expand(h.shape[0], -1, -1)], dim=-1)
    score = F.linear(F.relu(F.linear(x, a1, c1)), a2.view(1, 128), c2).squeeze(-1).t()
    return torch.autograd.grad(score, leaves, grad)


@pytest.fixture(scope="module")
def head_cases():
    """``{(N, B): (host case, fp64 definition)}``, computed once."""
    out = {}
    for n_node in (1, 31, 32, 33, 1031):
        for batch in (1, 3, 16):
            case = grid_head_case(n_node, batch, seed=100 * n_node + batch, zero_rows=n_node > 5)
            out[n_node, batch] = (case, score_backward_numpy(*case[:5], case[6]))
    return out


@pytest.mark.parametrize("batch", [1, 3, 16])
@pytest.mark.parametrize("n_node", [1, 31, 32, 33, 1031])
def test_score_backward_is_within_rounding_of_the_fp64_definition(head_cases, n_node, batch):
    from ultra_torchdrug_amd import functional as UF
    dev = _dev()
    case, truth = head_cases[n_node, batch]
    hidden, query, w1, b1, w2, b2, grad = _head_tensors(case)
    wide = torch.full((batch, n_node + 3), float("nan"), device=dev)              # a strided grad: rows of a wider matrix
    wide[:, :n_node] = grad
    mine = UF.score_all_backward(hidden, query, w1, b1, w2, wide[:, :n_node])
    aten = _aten_head(hidden, query, w1, b1, w2, b2, grad)
    for name, m, a, t in zip(HEAD_NAMES, mine, aten, truth):
        assert m.dtype == torch.float32 and m.numel() == t.size
        _bars(m.reshape(-1).cpu(), a.reshape(-1).cpu(), torch.from_numpy(t).reshape(-1), "%s at (N, B) = (%d, %d)" % (name, n_node, batch))
    zero = (grad == 0).all(dim=0)                                                  # entities whose grad is zero for every query
    assert n_node <= 5 or bool(zero.any())
    assert not mine[0][zero].any()
    contiguous = UF.score_all_backward(hidden, query, w1, b1, w2, grad)            # the same call: the same bits
    for m, c in zip(mine, contiguous):
        assert torch.equal(_bits(m), _bits(c))
    for skip in range(6):                                                          # each nullable output skipped once
        want = tuple(i != skip for i in range(6))
        part = UF.score_all_backward(hidden, query, w1, b1, w2, grad, want)
        assert part[skip] is None
        assert all(torch.equal(_bits(p), _bits(m)) for i, (p, m) in enumerate(zip(part, mine)) if i != skip), skip


@pytest.mark.parametrize("n_node,batch,lo,hi", [(1031, 16, 37, 1000), (1031, 3, 1000, 1031), (33, 1, 1, 2), (1031, 16, 0, 513)])
def test_score_backward_rows_do_not_depend_on_their_place(head_cases, n_node, batch, lo, hi):
    from ultra_torchdrug_amd import functional as UF
    hidden, query, w1, b1, w2, _, grad = _head_tensors(head_cases[n_node, batch][0])
    want = (True, False, False, False, False, False)
    whole = UF.score_all_backward(hidden, query, w1, b1, w2, grad, want)[0]
    part = UF.score_all_backward(hidden[lo:hi], query, w1, b1, w2, grad[:, lo:hi], want)[0]
    assert tuple(part.shape) == (hi - lo, batch, 64)
    assert torch.equal(_bits(part), _bits(whole[lo:hi]))


@pytest.mark.parametrize("n_node,batch", [(1031, 16), (33, 3)])
def test_score_backward_agrees_with_score_candidates(head_cases, n_node, batch):
    """``grad`` non-zero in K = 7 columns per query only: the candidate rows' backward computes the same gradients."""
    from ultra_torchdrug_amd import functional as UF
    dev = _dev()
    hidden, query, w1, b1, w2, b2, grad = _head_tensors(head_cases[n_node, batch][0])
    g = torch.Generator().manual_seed(n_node)
    t_index = torch.stack([torch.randperm(n_node, generator=g)[:7] for _ in range(batch)]).to(dev)
    sparse = torch.zeros_like(grad)
    sparse.scatter_(1, t_index, grad.gather(1, t_index))
    mine = UF.score_all_backward(hidden, query, w1, b1, w2, sparse)
    leaves = [t.detach().clone().requires_grad_() for t in (hidden, query, w1, b1, w2.view(1, 128), b2)]
    score = UF.score_candidates(leaves[0], leaves[1], t_index, *leaves[2:])
    cand = torch.autograd.grad(score, leaves, grad.gather(1, t_index))
    aten = _aten_head(hidden, query, w1, b1, w2, b2, sparse)
    for name, m, c, a in zip(HEAD_NAMES, mine, cand, aten):
        _bars(m.reshape(-1).cpu(), a.reshape(-1).cpu(), c.reshape(-1).double().cpu(), name + " against score_candidates")


def test_score_all_entities_through_autograd(head_cases):
    from ultra_torchdrug_amd import functional as UF
    hidden, query, w1, b1, w2, b2, grad = _head_tensors(head_cases[1031, 3][0])
    plain = UF.score_all_entities(hidden, query, w1, b1, w2.view(1, 128), b2)
    leaves = [t.detach().clone().requires_grad_() for t in (hidden, query, w1, b1, w2.view(1, 128), b2)]
    score = UF.score_all_entities(*leaves)
    assert score.requires_grad and torch.equal(_bits(score), _bits(plain))        # inference's launch, inference's bits
    got = torch.autograd.grad(score, leaves, grad)
    direct = UF.score_all_backward(hidden, query, w1, b1, w2, grad)
    for g, d, leaf in zip(got, direct, leaves):
        assert g.shape == leaf.shape and torch.equal(_bits(g).reshape(-1), _bits(d).reshape(-1))
    only = torch.autograd.grad(UF.score_all_entities(leaves[0], *[t.detach() for t in leaves[1:]]), leaves[:1], grad)[0]
    assert torch.equal(_bits(only), _bits(direct[0]))
    with torch.no_grad():
        assert not UF.score_all_entities(*leaves).requires_grad


# ------------------------------------------------------------------------------------------------ what the launches touch
def test_both_backwards_between_guard_bands():
    """The tail shapes between poisoned, guard-banded allocations: every output and workspace is carved between two bands
    and handed out as NaN; a read of an unwritten word or a store past an end shows."""
    from guarded_memory import guarded, has_poison
    from ultra_torchdrug_amd import functional as UF
    dev = _dev()
    for n_query, n_node, dim in ((3, 65, 64), (33, 1031, 6), (16, 63, 64), (1, 1, 6)):
        member, query, floor, d_boundary = grid_set_case(n_query, n_node, dim, 5)
        with guarded(widest_row=4 * n_query * dim) as guard:
            args = [guard.banded(torch.from_numpy(a).to(dev)) for a in (d_boundary, member, query, floor)]
            d_member, d_query = UF.set_boundary_backward(args[0], args[1], args[2], args[3])
            assert not has_poison(d_member) and not has_poison(d_query)
            want_member, want_query = set_boundary_backward_numpy(d_boundary, member, floor, query)
            assert np.array_equal(d_member.cpu().numpy().astype(np.float64), want_member)
            assert np.array_equal(d_query.cpu().numpy().astype(np.float64), want_query)
    for n_node, batch in ((33, 3), (1031, 16), (1, 1), (31, 16)):
        case = grid_head_case(n_node, batch, seed=n_node + batch, zero_rows=False)
        plain = UF.score_all_backward(*_head_tensors(case)[:5], _head_tensors(case)[6])
        with guarded(widest_row=4 * batch * 64) as guard:
            tensors = [guard.banded(t) for t in _head_tensors(case)]
            outs = UF.score_all_backward(*tensors[:5], tensors[6])
            for name, out, want in zip(HEAD_NAMES, outs, plain):
                assert not has_poison(out), name
                assert torch.equal(_bits(out), _bits(want)), name


MARK_ROWS = (2 ** 31 // 4096 - 1, 2 ** 31 // 4096, 0xffff0000 // 4096 - 1, 0xffff0000 // 4096, 2 ** 32 // 4096 - 1, 2 ** 32 // 4096,
             1_048_639)             # entities whose (16 x 64 x 4 = 4096-byte) rows lie next to the 2^31, 0xffff0000 and 2^32 byte marks


def _grid_on_device(shape, generator, lo=-8, hi=9):
    return torch.randint(lo, hi, shape, device=_dev(), generator=generator).float() / 4


def test_set_boundary_backward_past_4_gib():
    """N = 1 048 640, Q = 16, D = 64: d_boundary is 4 GiB + 256 KiB.  Gradient rows at the byte marks and the last row only, so
    that the sums stay exact; a chunked torch evaluation of the definition is the reference."""
    from ultra_torchdrug_amd import functional as UF
    dev = _dev()
    n_node, n_query, dim = 1_048_640, 16, 64
    g = torch.Generator(device=dev).manual_seed(3)
    member = torch.randint(-2, 9, (n_query, n_node), device=dev, generator=g).float() / 4
    query = _grid_on_device((n_query, dim), g)
    floor = torch.full((n_query,), 0.875, device=dev)
    d_boundary = torch.zeros(n_node, n_query, dim, device=dev)
    rows = torch.tensor(MARK_ROWS, device=dev)
    d_boundary[rows] = _grid_on_device((len(MARK_ROWS), n_query, dim), g)
    d_member, d_query = UF.set_boundary_backward(d_boundary, member, query, floor)
    keep = (member > 0) & (member >= floor[:, None])
    kept = keep.sum(dim=1)
    assert bool(((kept > 0) & (kept < n_node)).all())
    want_member = torch.zeros(n_query, n_node, device=dev)
    want_query = torch.zeros(n_query, dim, device=dev)
    for lo in range(0, n_node, 65536):
        hi = min(lo + 65536, n_node)
        k = keep[:, lo:hi].t()
        piece = d_boundary[lo:hi]
        want_member[:, lo:hi] = torch.where(k, (piece * query.unsqueeze(0)).sum(dim=-1), torch.zeros((), device=dev)).t()
        want_query += torch.where(k.unsqueeze(-1), member[:, lo:hi].t().unsqueeze(-1) * piece, torch.zeros((), device=dev)).sum(dim=0)
    assert bool(want_member[:, rows].any()) and bool(want_query.any())
    assert torch.equal(d_member, want_member) and torch.equal(d_query, want_query)
    assert not _bits(d_member)[~keep].any()


def test_score_backward_past_4_gib():
    """N = 1 048 640, B = 16: hidden and d_hidden are 4 GiB + 256 KiB each.  ``grad`` is non-zero at the byte marks and the last
    row; the rows there equal, bit for bit, the rows of calls on slices around the marks, and every other row is zero."""
    from ultra_torchdrug_amd import functional as UF
    dev = _dev()
    n_node, batch = 1_048_640, 16
    g = torch.Generator(device=dev).manual_seed(4)
    hidden = torch.empty(n_node, batch, 64, device=dev)
    for lo in range(0, n_node, 65536):
        hidden[lo:lo + 65536] = _grid_on_device(tuple(hidden[lo:lo + 65536].shape), g)
    query, w1, b1, w2 = (_grid_on_device(s, g) for s in ((batch, 64), (128, 128), (128,), (128,)))
    grad = torch.zeros(batch, n_node, device=dev)
    rows = torch.tensor(MARK_ROWS, device=dev)
    grad[:, rows] = _grid_on_device((batch, len(MARK_ROWS)), g, 1, 9)
    outs = UF.score_all_backward(hidden, query, w1, b1, w2, grad)
    d_hidden = outs[0]
    assert bool((d_hidden[rows].abs().amax(dim=(1, 2)) > 0).all())
    listed = torch.zeros(n_node, dtype=torch.bool, device=dev)
    listed[rows] = True
    for lo in range(0, n_node, 65536):
        assert not d_hidden[lo:lo + 65536][~listed[lo:lo + 65536]].any(), lo
    want = (True, False, False, False, False, False)
    for mark in (2 ** 31 // 4096, 0xffff0000 // 4096, 2 ** 32 // 4096, n_node - 1):
        lo, hi = mark - 40, min(mark + 40, n_node)
        part = UF.score_all_backward(hidden[lo:hi], query, w1, b1, w2, grad[:, lo:hi], want)[0]
        assert torch.equal(_bits(part), _bits(d_hidden[lo:hi])), mark
    # the sums over rows see the rows past the marks too: the same call on the listed rows alone
    small = UF.score_all_backward(hidden[rows].contiguous(), query, w1, b1, w2, grad[:, rows].contiguous())
    for name, whole, few in zip(HEAD_NAMES[1:], outs[1:], small[1:]):
        _bars(whole.reshape(-1).cpu(), few.reshape(-1).cpu(), few.reshape(-1).double().cpu(), name + " past 4 GiB")


# ------------------------------------------------------------------------------------------------ model level
def _wide64_task():
    from ultra_torchdrug_amd.task import build_ultra
    graph = wide_graph()
    torch.manual_seed(5)
    task = build_ultra(graph.num_relation, hidden_dims=(64,) * 2, rel_layers=2, num_negative=8, full_batch_eval=True)
    task.preprocess(graph)
    return task.eval().to(_dev())


@pytest.fixture(scope="module")
def wide64():
    """The 64-wide two-layer model on ``wide_graph()`` (tests/test_query_gpu.py's construction)."""
    return _wide64_task()


@pytest.fixture(scope="module")
def small16():
    return small_task(wide_graph()).to(_dev())


def _explicit_members(n_query, n_node, seed):
    """fp32-exact memberships (multiples of 1/16) and a floor strictly between two of them: the kept set is the same in fp32
    and in fp64 by construction."""
    g = torch.Generator().manual_seed(seed)
    member = torch.randint(0, 17, (n_query, n_node), generator=g).float() / 16
    floor = torch.full((n_query,), 0.40625)                      # between 6/16 and 7/16
    return member.to(_dev()), floor.to(_dev())


def _named_gradients(task, outputs, cotangent, extra):
    names = [n for n, _ in task.named_parameters()]
    wanted = list(extra.values()) + [p for _, p in task.named_parameters()]
    grads = torch.autograd.grad(outputs, wanted, cotangent, allow_unused=True)
    out = {}
    for name, g in zip(list(extra) + names, grads):
        if g is not None:
            out[name] = g.detach().double().cpu()
    return out


@pytest.mark.parametrize("width", [64, 16])
def test_project_train_against_the_fp64_definition(wide64, small16, width):
    from aten_definition import aten_definition
    task, dev = (wide64 if width == 64 else small16), _dev()
    _, relations = (x.to(dev) for x in query_ids("2p", 4, 300, 10, seed=3))
    rel = relations[:, 1]
    member, floor = _explicit_members(4, 300, seed=width)
    kept = ((member > 0) & (member >= floor[:, None])).sum(1)
    kept64 = ((member.double() > 0) & (member.double() >= floor.double()[:, None])).sum(1)
    assert torch.equal(kept, kept64) and bool(((kept > 0) & (kept < 300)).all())
    cotangent = torch.randn(4, 300, generator=torch.Generator().manual_seed(1)).to(dev)

    def run(dtype):
        leaf = member.to(dtype).requires_grad_()
        with torch.enable_grad():
            reps = task.relation_representations(rel % 5)
            logits, count = task.model.project_train(task.fact_graph, reps, leaf, rel, floor)
            assert logits.requires_grad and torch.equal(count.long(), kept)
            extra = {"member": leaf}
            extra.update({"relation representation %d" % i: r for i, r in enumerate(reps)})
            grads = _named_gradients(task, logits, cotangent.to(dtype), extra)
        return logits.detach(), grads

    mine, g_mine = run(torch.float32)
    with torch.no_grad():
        frozen = task.model.project(task.fact_graph, task.relation_representations(rel % 5), member, rel, floor)[0]
    print("project_train against project without grad: max |difference| %.3g" % float((mine - frozen).abs().max()))
    with aten_definition(task):
        aten, g_aten = run(torch.float32)
    with aten_definition(task, double=True):
        truth, g_true = run(torch.float64)
        assert truth.dtype == torch.float64
    _bars(mine, aten, truth, "project_train at %d columns" % width)
    assert set(g_mine) == set(g_true) == set(g_aten) and "member" in g_true and len(g_true) > 10
    for name in g_true:
        _gradient_bar(g_mine[name], g_aten[name], g_true[name], "d %s at %d columns" % (name, width))


def _loss_inputs(name, seed):
    dev = _dev()
    anchors, relations = (x.to(dev) for x in query_ids(name, 3, 300, 10, seed=seed))
    g = torch.Generator().manual_seed(seed + 1)
    return (anchors, relations, torch.randint(0, 300, (3,), generator=g).to(dev), torch.randint(0, 300, (3, 5), generator=g).to(dev))


@pytest.mark.parametrize("width", [64, 16])
@pytest.mark.parametrize("name", ["2p", "2i", "ip", "2in", "2u"])
def test_query_loss_against_the_fp64_definition(wide64, small16, name, width):
    """The default cut: nothing is cut, so no set can differ between the precisions."""
    from aten_definition import aten_definition
    task = wide64 if width == 64 else small16
    inputs = _loss_inputs(name, seed=len(name) + width)

    def run():
        with torch.enable_grad():
            loss = task.query_loss(name, *inputs)
            assert loss.dim() == 0 and loss.requires_grad
            return loss.detach().reshape(1), _named_gradients(task, loss, None, {})

    mine, g_mine = run()
    with aten_definition(task):
        aten, g_aten = run()
    with aten_definition(task, double=True):
        truth, g_true = run()
        assert truth.dtype == torch.float64
    _bars(mine, aten, truth, "query_loss of %s at %d columns" % (name, width))
    assert set(g_mine) == set(g_true) and len(g_true) > 10
    for key in g_true:
        _gradient_bar(g_mine[key], g_aten[key], g_true[key], "d %s of %s at %d columns" % (key, name, width))


class RecordingBackend:
    """The backend in force behind an object that counts the calls of its entry points (predicates pass uncounted), as
    tests/test_reference_architectures_gpu.py does."""

    def __init__(self, inner):
        self._inner = inner
        self.calls = collections.Counter()

    def __getattr__(self, name):
        value = getattr(self._inner, name)
        if not callable(value) or isinstance(value, type) or name == "accepts" or name.endswith("_supported"):
            return value

        def counted(*args, **kwargs):
            self.calls[name] += 1
            return value(*args, **kwargs)

        return counted


def test_the_differentiable_route_of_the_shipped_architecture(wide64):
    from ultra_torchdrug_amd import backend
    task = wide64
    inputs = _loss_inputs("2p", seed=9)
    proxy = RecordingBackend(backend.get())
    with backend.use(proxy), torch.enable_grad():
        task.query_loss("2p", *inputs).backward()
    task.zero_grad(set_to_none=True)
    print("differentiable 2p:", dict(proxy.calls))
    assert proxy.calls["set_boundary"] == 2 and proxy.calls["score_all_entities"] == 2      # the first hop is a one-hot set
    # two projections, each through the two entity layers and the two layers of the relation stack (which trains on sum_layer too)
    assert proxy.calls["sum_layer"] == 2 * (len(task.model.layers) + 2)
    assert proxy.calls["score_candidates"] == 0 and proxy.calls["rspmm_frontier"] == 0
    assert proxy.calls["candidate_tiles"] == 0 and proxy.calls["first_layer_forward"] == 0


def test_inference_is_untouched_by_a_training_backward(wide64):
    task, dev = wide64, _dev()
    anchors, relations, positives, negatives = _loss_inputs("2p", seed=21)
    mode = task.training
    before = task.answer_query("2p", anchors, relations, k=10, max_sources=12)
    with torch.enable_grad():
        task.query_loss("2p", anchors, relations, positives, negatives, max_sources=12).backward()
    assert any(p.grad is not None and bool(p.grad.abs().sum() > 0) for p in task.parameters())
    task.zero_grad(set_to_none=True)
    after = task.answer_query("2p", anchors, relations, k=10, max_sources=12)
    assert task.training == mode
    assert torch.equal(before[0], after[0]) and torch.equal(_bits(before[1]), _bits(after[1]))


def test_ten_training_steps_lower_the_loss_and_the_guard_raises():
    from ultra_torchdrug_amd import engine
    from ultra_torchdrug_amd import data
    task = _wide64_task().train()                                # a task of its own: the steps change the weights
    # a batch as training makes one: grounded queries, their targets as positives, negatives among the non-answers
    g = torch.Generator().manual_seed(33)
    anchors, relations, targets = data.sample_queries(task.message_graph(), "2p", 8, g)
    answers = task.query_answers("2p", anchors, relations, graph="filter")
    assert bool(answers.gather(1, targets.to(answers.device)[:, None]).all())
    inputs = (anchors, relations, targets, data.sample_query_negatives(answers, 16, g))
    with torch.no_grad():
        start = float(task.query_loss("2p", *inputs))
    optimizer = torch.optim.Adam(task.parameters(), lr=5e-3)
    guard = engine.FiniteGuard(task)
    losses = [float(engine.train_query_step(task, optimizer, "2p", *inputs, guard=guard)[0]) for _ in range(10)]
    with torch.no_grad():
        end = float(task.query_loss("2p", *inputs))
    print("2p batch: loss %.5f before, %.5f after ten Adam steps (%s)" % (start, end, ", ".join("%.4f" % x for x in losses)))
    assert abs(losses[0] - start) <= 1e-5 * abs(start) and end < start
    with torch.no_grad():
        task.model.mlp.layers[0].weight[3, 5] = float("nan")
    with pytest.raises(engine.NonFiniteError) as caught:
        engine.train_query_step(task, optimizer, "2p", *inputs, guard=guard)
    assert caught.value.kind == "parameter" and caught.value.name == "model.mlp.layers.0.weight"


def test_refusals_raise_before_any_launch():
    from ultra_torchdrug_amd import _lib
    from ultra_torchdrug_amd import functional as UF
    dev = _dev()
    member, query, floor, d_boundary = (torch.from_numpy(a).to(dev) for a in grid_set_case(4, 70, 8, 2))
    UF.set_boundary_backward(d_boundary, member, query, floor)
    wide = torch.zeros(4, 140, device=dev)
    for bad in (dict(member=member.double()), dict(query=query[:3]), dict(d_boundary=d_boundary[:, :3]), dict(member=wide[:, ::2]),
                dict(floor=floor[:3]), dict(d_boundary=d_boundary.cpu()), dict(d_boundary=d_boundary.double())):
        with pytest.raises(RuntimeError):
            UF.set_boundary_backward(**dict(dict(d_boundary=d_boundary, member=member, query=query, floor=floor), **bad))
    d_member, d_query = torch.empty(4, 70, device=dev), torch.empty(4, 8, device=dev)
    bytes_a = int(_lib.load().ultra_set_boundary_backward_workspace(4, 70, 8))
    ws = torch.empty(bytes_a // 4, device=dev)
    good = [d_boundary, member, 4, 70, 70, floor, query, 8, d_member, d_query, ws, bytes_a]
    _lib.launch(dev, "ultra_set_boundary_backward_f32", *good)
    for at, value, word in ((2, 0, "shape"), (3, 0, "shape"), (7, 0, "shape"), (4, 69, "shape"), (7, 2048, "shape"), (0, None, "null"),
                            (1, None, "null"), (6, None, "null"), (8, None, "null"), (10, None, "null"), (11, bytes_a - 4, "workspace")):
        args = list(good)
        args[at] = value
        with pytest.raises(RuntimeError, match="(?i)" + word):
            _lib.launch(dev, "ultra_set_boundary_backward_f32", *args)
    hidden, q, w1, b1, w2, _, grad = _head_tensors(grid_head_case(33, 3, seed=1))
    for bad in (dict(hidden=hidden[:, :, :32]), dict(query=q[:2]), dict(grad=grad[:, :30]), dict(w1=w1[:64]), dict(grad=grad.cpu()),
                dict(hidden=hidden.double())):
        with pytest.raises(RuntimeError):
            UF.score_all_backward(**dict(dict(hidden=hidden, query=q, w1=w1, b1=b1, w2=w2, grad=grad), **bad))
    bytes_b = int(_lib.load().ultra_score_backward_workspace(33, 3))
    ws = torch.empty(bytes_b // 4, device=dev)
    outs = [torch.empty(s, device=dev) for s in ((33, 3, 64), (3, 64), (128, 128), (128,), (128,), (1,))]
    good = [hidden, q, w1, b1, w2, grad, 33, *outs, ws, bytes_b, 33, 3]
    _lib.launch(dev, "ultra_score_backward_f32", *good)
    for at, value, word in ((15, 0, "shape"), (16, 0, "shape"), (16, 65536, "shape"), (6, 32, "shape"), (0, None, "null"), (1, None, "null"),
                            (2, None, "null"), (3, None, "null"), (4, None, "null"), (5, None, "null"), (13, None, "null"),
                            (14, bytes_b - 4, "workspace")):
        args = list(good)
        args[at] = value
        with pytest.raises(RuntimeError, match="(?i)" + word):
            _lib.launch(dev, "ultra_score_backward_f32", *args)
    torch.cuda.synchronize()

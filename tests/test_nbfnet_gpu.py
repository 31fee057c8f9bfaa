"""MI355X: ``NeuralBellmanFordNetwork`` on the device.

(a) The operator ``ultra_query_tables_f32`` / ``ultra_query_tables_backward_f32`` (``csrc/query_tables.hip``) against the plain fp64
    definition of ``tests/nbfnet_definition.py``: on dyadic-grid inputs, where every partial sum in any order is exactly
    representable (``exact_grid.assert_exact`` holds the precondition per shape), entry for entry with no tolerance; on normal
    inputs within the forward-error bound of a length-``n`` fp32 sum, ``n * 2^-24 * sum|terms|``; the same bits on every call, under
    capture and replay, and through both bindings; between poisoned, guard-banded allocations; every host status.
(b) The model on the HIP path held to the four recorded cases of the reference (``tests/nbfnet_cases.py``): ``max|X - T| <= 4 *
    ref_dev + floor * scale`` with the floors of ``test_reference_architectures_gpu.py``; which entry points each case reaches.
(c) The fused inference sequence of ``score_all_entities`` against the layer-by-layer route of a child process
    (``ULTRA_FAST_INFERENCE=0``), bit for bit, eagerly and under ``engine.GraphedPredict``.
(d) A task from ``task.build_nbfnet``: predict / evaluate, eager and captured training steps, answers, explanations; a graph
    without relations."""
import collections
import copy
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import nbfnet_cases as NC
import nbfnet_definition as ND
import reference_fixture as RF
from exact_grid import assert_exact, grid
from guarded_memory import guarded, has_poison

pytestmark = pytest.mark.gpu

FLOORS = {"hidden": 8e-7, "scores": 1.1e-6, "scores_all": 1.4e-6, "gradient": 2.4e-6}
HERE = os.path.dirname(os.path.abspath(__file__))
EPS = 2.0 ** -24


def _dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def _UF():
    from ultra_torchdrug_amd import functional
    return functional


def _to(arrays, dev):
    return [None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in arrays]


# ------------------------------------------------------------------------------------------------ (a) the operator
# (n_rel, batch, dims of the layers, K, which gradients are NULL)
SHAPES = [
    (1, 1, (64,), 64, ()),
    (2, 3, (32,), 32, ()),
    (22, 16, (16,) * 6, 64, ()),
    (22, 64, (64,) * 8, 64, ()),                # d_query: 8 x 22 x 64 terms per entry
    (22, 65, (6,), 6, ()),                      # the scalar route, a second block of queries holding one query
    (3, 65, (6, 6), 6, (1,)),                   # ... a NULL gradient at the end
    (474, 16, (64,) * 6, 64, (2,)),             # the headline vocabulary; a NULL gradient in the middle
    (22, 3, (64, 32, 6, 16), 64, (1, 3)),       # layers of mixed width; NULL in the middle and at the end
    (5, 33, (8,), 100, ()),                     # K above one chunk of 64 columns, 16-byte loads
    (5, 4, (7,), 70, ()),                       # ... 4-byte loads
]
SHAPE_IDS = ["r%d-b%d-d%s-k%d" % (s[0], s[1], "x".join(map(str, sorted(set(s[2])))) + "n%d" % len(s[2]), s[3]) for s in SHAPES]


def _operands(shape, draw):
    n_rel, batch, dims, K, null = shape
    query = draw((batch, K))
    weights = [draw((n_rel * d, K)) for d in dims]
    biases = [draw((n_rel * d,)) for d in dims]
    grads = [None if l in null else draw((n_rel, batch * d)) for l, d in enumerate(dims)]
    return query, weights, biases, grads


def _exact_operands(shape):
    """Operands on a dyadic grid fine enough that every sum of the shape is exact (``assert_exact``): values ``k / 4`` with
    ``|k| <= lim``; ``lim`` halves until the largest sum of |terms| -- that of ``d_query`` -- stays below ``2^24`` units."""
    n_rel = shape[0]
    for lim in (8, 4, 2, 1):
        rng = np.random.default_rng(shape[0] * 1000 + shape[1] * 10 + len(shape[2]))
        query, weights, biases, grads = _operands(shape, lambda s: grid(rng, s, q=4, lim=lim))
        sums = ND.tables(query, weights, biases, n_rel, absolute=True) + [x for part in ND.gradients(
            query, weights, grads, n_rel, absolute=True)[:2] for x in part] + [ND.gradients(query, weights, grads, n_rel, absolute=True)[2]]
        try:
            for s in sums:
                assert_exact(s, 2.0 ** -4)
        except AssertionError:
            continue
        return query, weights, biases, grads
    raise AssertionError("no grid makes %s exact" % (shape,))


def _run_operator(query, weights, biases, grads, n_rel, dev, query_view=False):
    UF = _UF()
    q, = _to([query], dev)
    if query_view:                              # a strided column view: rows 3 floats... apart, 16-byte alignment lost
        wide = torch.full((q.shape[0], q.shape[1] + 7), float("nan"), device=dev)
        wide[:, 3:3 + q.shape[1]] = q
        q = wide[:, 3:3 + q.shape[1]]
        assert not q.is_contiguous() or q.shape[0] == 1
    w, b, g = _to(weights, dev), _to(biases, dev), _to(grads, dev)
    out = UF.query_tables_forward(q, w, b, n_rel)
    d_w, d_b, d_q = UF.query_tables_backward(q, w, g, n_rel)
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in out], [t.cpu().numpy() for t in d_w], [t.cpu().numpy() for t in d_b], d_q.cpu().numpy()


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_operator_equals_the_definition_on_exact_grids(shape):
    n_rel = shape[0]
    query, weights, biases, grads = _exact_operands(shape)
    want_out = ND.tables(query, weights, biases, n_rel)
    want_w, want_b, want_q = ND.gradients(query, weights, grads, n_rel)
    for view in (False, True):
        out, d_w, d_b, d_q = _run_operator(query, weights, biases, grads, n_rel, _dev(), query_view=view)
        for l in range(len(weights)):
            assert out[l].shape == want_out[l].shape and np.array_equal(out[l].astype(np.float64), want_out[l]), ("out", l, view)
            assert np.array_equal(d_w[l].astype(np.float64), want_w[l]), ("d_w", l, view)
            assert np.array_equal(d_b[l].astype(np.float64), want_b[l]), ("d_bias", l, view)
        assert np.array_equal(d_q.astype(np.float64), want_q), ("d_query", view)
    assert any(np.abs(o).max() > 0 for o in want_out) and np.abs(want_q).max() > 0


NORMAL = [SHAPES[i] for i in (1, 3, 5, 6, 7, 9)]


@pytest.mark.parametrize("shape", NORMAL, ids=[SHAPE_IDS[i] for i in (1, 3, 5, 6, 7, 9)])
def test_operator_on_normal_inputs_within_the_summation_bound(shape):
    """``|fp32 - fp64| <= n * 2^-24 * sum|terms|`` per entry, ``n`` the number of terms of the entry's sum: ``K + 1`` (forward),
    ``batch`` (``d_w``, ``d_bias``), ``sum_l n_rel * D_l`` over the layers with a gradient (``d_query``).  Two calls: equal bits."""
    n_rel, batch, dims, K, null = shape
    rng = np.random.default_rng(7 + n_rel)
    query, weights, biases, grads = _operands(shape, lambda s: rng.standard_normal(s).astype(np.float32))
    first = _run_operator(query, weights, biases, grads, n_rel, _dev())
    again = _run_operator(query, weights, biases, grads, n_rel, _dev())
    flat = lambda run: run[0] + run[1] + run[2] + [run[3]]
    for a, b in zip(flat(first), flat(again)):
        assert np.array_equal(a.view(np.int32), b.view(np.int32))
    # the strided, unaligned query view against the contiguous call: the routes share one order, so the bits are equal
    view = _run_operator(query, weights, biases, grads, n_rel, _dev(), query_view=True)
    for a, b in zip(flat(first), flat(view)):
        assert np.array_equal(a.view(np.int32), b.view(np.int32))
    want = ND.tables(query, weights, biases, n_rel), *ND.gradients(query, weights, grads, n_rel)
    mass = ND.tables(query, weights, biases, n_rel, absolute=True), *ND.gradients(query, weights, grads, n_rel, absolute=True)
    n_query_terms = sum(n_rel * d for l, d in enumerate(dims) if l not in null)
    for l in range(len(dims)):
        assert (np.abs(first[0][l] - want[0][l]) <= (K + 1) * EPS * mass[0][l]).all(), ("out", l)
        assert (np.abs(first[1][l] - want[1][l]) <= batch * EPS * mass[1][l]).all(), ("d_w", l)
        assert (np.abs(first[2][l] - want[2][l]) <= batch * EPS * mass[2][l]).all(), ("d_bias", l)
    assert (np.abs(first[3] - want[3]) <= n_query_terms * EPS * mass[3]).all()


def _fma32(a, b, acc):
    """``fmaf(a, b, acc)`` on float32 arrays: the product of two float32 is exact in float64, the sum is rounded to float64 and
    then to float32.  The two roundings equal the single one unless the float64 sum sits exactly half way between two float32
    values; such a case is refused here instead of guessed."""
    s = a.astype(np.float64) * b.astype(np.float64) + acc.astype(np.float64)
    assert not ((s.view(np.int64) & ((1 << 29) - 1)) == (1 << 28)).any(), "a half-way case: change the seed"
    return s.astype(np.float32)


@pytest.mark.parametrize("shape,offset", [((3, 5, (6, 8), 12, ()), 0), ((3, 5, (6, 8), 12, ()), 1), ((2, 35, (4,), 100, ()), 0),
                                          ((2, 3, (5,), 70, ()), 1)], ids=["k12-wide", "k12-narrow", "k100-wide", "k70-narrow"])
def test_operator_keeps_the_documented_order(shape, offset):
    """The header's order, held bit for bit on normal inputs against a sequential fp32 restatement: the forward is ONE ``fmaf``
    chain from the bias with ``k`` ascending; ``d_w`` one from ``+0.0`` with ``b`` ascending; ``d_bias`` plain adds, ``b``
    ascending.  ``offset`` 1 puts every weight 4 bytes off a 16-byte boundary (the 4-byte route), 0 leaves them aligned."""
    UF, dev = _UF(), _dev()
    n_rel, batch, dims, K, _ = shape
    rng = np.random.default_rng(17 + K + offset)
    query, weights, biases, grads = _operands(shape, lambda s: rng.standard_normal(s).astype(np.float32))
    q, = _to([query], dev)
    b, g = _to(biases, dev), _to(grads, dev)
    w = []
    for a in weights:                                   # contiguous (rows, K) tensors at a chosen byte offset
        flat = torch.empty(a.size + 4, device=dev)
        part = flat[offset:offset + a.size].view(a.shape)
        part.copy_(torch.from_numpy(a))
        assert part.is_contiguous() and (part.data_ptr() % 16 == 0) == (offset == 0)
        w.append(part)
    out = UF.query_tables_forward(q, w, b, n_rel)
    d_w, d_b, _ = UF.query_tables_backward(q, w, g, n_rel)
    torch.cuda.synchronize()
    for l, D in enumerate(dims):
        acc = np.repeat(biases[l][None, :], batch, axis=0)                     # [b, j]
        for k in range(K):
            acc = _fma32(weights[l][None, :, k], query[:, k, None], acc)
        want = acc.reshape(batch, n_rel, D).transpose(1, 0, 2).reshape(n_rel, batch * D)
        assert np.array_equal(out[l].cpu().numpy().view(np.int32), want.view(np.int32)), ("out", l)
        rows = grads[l].reshape(n_rel, batch, D).transpose(0, 2, 1).reshape(n_rel * D, batch)      # [j, b]
        dw, db = np.zeros((n_rel * D, K), dtype=np.float32), np.zeros(n_rel * D, dtype=np.float32)
        for i in range(batch):
            dw = _fma32(rows[:, i, None], query[None, i, :], dw)
            db = (db + rows[:, i]).astype(np.float32)
        assert np.array_equal(d_w[l].cpu().numpy().view(np.int32), dw.view(np.int32)), ("d_w", l)
        assert np.array_equal(d_b[l].cpu().numpy().view(np.int32), db.view(np.int32)), ("d_bias", l)


def test_unused_tables_reach_the_backward_as_null():
    """The autograd node does not materialise the gradient of a table nothing read: the backward call gets ``None`` for it (the
    C entry's NULL path), and the gradients equal those of the twin, whose unused layer gets none either."""
    UF, dev = _UF(), _dev()
    n_rel, batch, D, K = 5, 4, 8, 8
    gen = torch.Generator(device=dev).manual_seed(3)
    leaf = lambda *s: torch.randn(*s, device=dev, generator=gen).requires_grad_()
    q, w, b = leaf(batch, K), [leaf(n_rel * D, K) for _ in range(3)], [leaf(n_rel * D) for _ in range(3)]
    seen = []
    plain = UF.query_tables_backward

    def spy(query, weights, grads, n_rel):
        seen.append([x is None for x in grads])
        return plain(query, weights, grads, n_rel)
    UF.query_tables_backward = spy
    try:
        tables = UF.query_tables(q, w, b, n_rel)
        (tables[0].sum() + 2 * tables[2].sum()).backward()
    finally:
        UF.query_tables_backward = plain
    assert seen == [[False, True, False]]
    assert not bool(w[1].grad.any()) and not bool(b[1].grad.any())
    assert torch.allclose(b[0].grad, torch.full_like(b[0], batch)) and torch.allclose(b[2].grad, torch.full_like(b[2], 2 * batch))
    want = (w[0].detach().sum(0) + 2 * w[2].detach().sum(0)).expand(batch, K)
    assert torch.allclose(q.grad, want, rtol=1e-5, atol=1e-5)


def test_operator_captured_and_through_both_bindings(monkeypatch):
    """Capture plus two replays give the eager bits; the ctypes binding gives the torch extension's."""
    UF, dev = _UF(), _dev()
    shape = (22, 16, (64, 64, 32), 64, (1,))
    rng = np.random.default_rng(5)
    query, weights, biases, grads = _operands(shape, lambda s: rng.standard_normal(s).astype(np.float32))
    q, = _to([query], dev)
    w, b, g = _to(weights, dev), _to(biases, dev), _to(grads, dev)

    def call():
        out = UF.query_tables_forward(q, w, b, 22)
        d_w, d_b, d_q = UF.query_tables_backward(q, w, g, 22)
        return out + d_w + d_b + [d_q]
    monkeypatch.setenv("ULTRA_BINDING", "torch")
    eager = [t.clone() for t in call()]
    monkeypatch.setenv("ULTRA_BINDING", "ctypes")
    plain = call()
    for a, c in zip(eager, plain):
        assert torch.equal(a.view(torch.int32), c.view(torch.int32))
    for binding in ("torch", "ctypes"):
        monkeypatch.setenv("ULTRA_BINDING", binding)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            call()                                  # warm-up: the outputs enter the allocator's cache
        torch.cuda.current_stream().wait_stream(side)
        captured = torch.cuda.CUDAGraph()
        with torch.cuda.graph(captured, stream=side):
            static = call()
        for _ in range(2):
            for t in static:
                t.fill_(float("nan"))
            captured.replay()
            torch.cuda.synchronize()
            for a, c in zip(eager, static):
                assert torch.equal(a.view(torch.int32), c.view(torch.int32)), binding
    # the dispatcher operators by their names
    monkeypatch.setenv("ULTRA_BINDING", "torch")
    tables = torch.ops.ultra_mi.query_tables(q, w, b, 22)
    back = torch.ops.ultra_mi.query_tables_backward(q, w, g, 22)
    for a, c in zip(eager, list(tables) + list(back)):
        assert torch.equal(a.view(torch.int32), c.view(torch.int32))


@pytest.mark.parametrize("shape", [(1, 1, (64,), 64, ()), (3, 65, (6, 6), 6, (0,)), (474, 33, (64, 64), 64, ())],
                         ids=["r1-b1", "r3-b65-d6", "r474-b33-d64"])
def test_operator_between_guard_bands(shape, monkeypatch):
    """Forward and backward between poisoned, guard-banded allocations (``ULTRA_BINDING=ctypes``: the outputs and the workspace
    are allocated in ``functional.py``): no band is touched, no output keeps a poisoned entry, the values are the unguarded run's."""
    monkeypatch.setenv("ULTRA_BINDING", "ctypes")
    UF, dev = _UF(), _dev()
    n_rel = shape[0]
    rng = np.random.default_rng(11)
    query, weights, biases, grads = _operands(shape, lambda s: rng.standard_normal(s).astype(np.float32))
    want = _run_operator(query, weights, biases, grads, n_rel, dev)
    with guarded("functional", widest_row=4 * shape[1] * max(shape[2])) as guard:
        q = guard.banded(torch.from_numpy(query).to(dev))
        w = [guard.banded(t) for t in _to(weights, dev)]
        b = [guard.banded(t) for t in _to(biases, dev)]
        g = [None if t is None else guard.banded(t) for t in _to(grads, dev)]
        out = UF.query_tables_forward(q, w, b, n_rel)
        d_w, d_b, d_q = UF.query_tables_backward(q, w, g, n_rel)
        torch.cuda.synchronize()
        got = out + d_w + d_b + [d_q]
        assert not any(has_poison(t) for t in got)
        got = [t.cpu().numpy() for t in got]
    for a, c in zip(want[0] + want[1] + want[2] + [want[3]], got):
        assert np.array_equal(a.view(np.int32), c.view(np.int32))


def test_host_statuses_leave_the_outputs_untouched():
    """Every refusal happens before any launch: the poisoned outputs keep every bit."""
    from ultra_torchdrug_amd import _lib
    from ultra_torchdrug_amd.functional import _pointer_array
    dev = _dev()
    lib = _lib.load()
    n_rel, batch, D, K = 3, 5, 8, 8
    query = torch.randn(batch, K, device=dev)
    w = [torch.randn(n_rel * D, K, device=dev) for _ in range(2)]
    b = [torch.randn(n_rel * D, device=dev) for _ in range(2)]
    g = [torch.randn(n_rel, batch * D, device=dev) for _ in range(2)]
    poison = float("nan")
    outs = [torch.full((n_rel, batch * D), poison, device=dev) for _ in range(2)]
    d_w = [torch.full_like(t, poison) for t in w]
    d_b = [torch.full_like(t, poison) for t in b]
    d_q = torch.full((batch, K), poison, device=dev)
    dims = (ctypes.c_int64 * 2)(D, D)
    nine = (ctypes.c_int64 * 9)(*[D] * 9)
    need = int(lib.ultra_query_tables_backward_workspace(2, batch, n_rel, dims, K))
    assert need == 2 * batch * K * 4                       # one partial block per layer at this size
    ws = torch.full((need // 4,), poison, device=dev)
    missing = [w[0], None]

    def fwd(**kw):
        a = dict(query=query, stride=K, w=_pointer_array(w), b=_pointer_array(b), out=_pointer_array(outs), dims=dims, n=2,
                 batch=batch, n_rel=n_rel, K=K)
        a.update(kw)
        return [a[k] for k in ("query", "stride", "w", "b", "out", "dims", "n", "batch", "n_rel", "K")]

    def bwd(**kw):
        a = dict(query=query, stride=K, w=_pointer_array(w), g=_pointer_array(g), d_w=_pointer_array(d_w), d_b=_pointer_array(d_b),
                 d_q=d_q, ws=ws, ws_bytes=need, dims=dims, n=2, batch=batch, n_rel=n_rel, K=K)
        a.update(kw)
        return [a[k] for k in ("query", "stride", "w", "g", "d_w", "d_b", "d_q", "ws", "ws_bytes", "dims", "n", "batch", "n_rel", "K")]

    shape_cases = [dict(n=0), dict(n=9, dims=nine), dict(K=0), dict(batch=-1), dict(n_rel=-1), dict(stride=K - 1),
                   dict(dims=(ctypes.c_int64 * 2)(D, 0))]
    for kw in shape_cases:
        with pytest.raises(RuntimeError, match="bad shape"):
            _lib.launch(dev, "ultra_query_tables_f32", *fwd(**kw))
        with pytest.raises(RuntimeError, match="bad shape"):
            _lib.launch(dev, "ultra_query_tables_backward_f32", *bwd(**kw))
        assert lib.ultra_query_tables_backward_workspace(kw.get("n", 2), kw.get("batch", batch), kw.get("n_rel", n_rel),
                                                         kw.get("dims", dims), kw.get("K", K)) == 0 or "stride" in kw
    for kw in (dict(query=None), dict(w=None), dict(b=None), dict(out=None), dict(dims=None), dict(w=_pointer_array(missing)),
               dict(b=_pointer_array(missing)), dict(out=_pointer_array(missing))):
        with pytest.raises(RuntimeError, match="NULL"):
            _lib.launch(dev, "ultra_query_tables_f32", *fwd(**kw))
    for kw in (dict(query=None), dict(w=None), dict(g=None), dict(d_w=None), dict(d_b=None), dict(d_q=None), dict(ws=None),
               dict(w=_pointer_array(missing)), dict(d_w=_pointer_array(missing)), dict(d_b=_pointer_array(missing))):
        with pytest.raises(RuntimeError, match="NULL"):
            _lib.launch(dev, "ultra_query_tables_backward_f32", *bwd(**kw))
    with pytest.raises(RuntimeError, match="workspace"):
        _lib.launch(dev, "ultra_query_tables_backward_f32", *bwd(ws_bytes=need - 4))
    # an empty batch or vocabulary: ULTRA_OK, nothing launched
    _lib.launch(dev, "ultra_query_tables_f32", *fwd(batch=0))
    _lib.launch(dev, "ultra_query_tables_f32", *fwd(n_rel=0))
    _lib.launch(dev, "ultra_query_tables_backward_f32", *bwd(batch=0))
    _lib.launch(dev, "ultra_query_tables_backward_f32", *bwd(n_rel=0))
    torch.cuda.synchronize()
    for t in outs + d_w + d_b + [d_q, ws]:
        assert bool(torch.isnan(t).all())
    # the Python entry refuses before the C entry does
    UF = _UF()
    for bad in (dict(query=query.double()), dict(query=query[0]), dict(weights=[w[0][:, :4]]), dict(weights=w * 5, biases=b * 5),
                dict(biases=[b[0][:3], b[1]]), dict(weights=[w[0][:5], w[1]])):
        args = dict(query=query, weights=w, biases=b)
        args.update(bad)
        with pytest.raises(RuntimeError):
            UF.query_tables_forward(args["query"], args["weights"], args["biases"], n_rel)
    _lib.launch(dev, "ultra_query_tables_f32", *fwd())
    _lib.launch(dev, "ultra_query_tables_backward_f32", *bwd())
    torch.cuda.synchronize()
    assert not any(bool(torch.isnan(t).any()) for t in outs + d_w + d_b + [d_q])


def test_autograd_node_against_the_twin_in_fp64():
    """``functional.query_tables`` in fp32 (one autograd node, one backward call) against ``dense_query_tables`` in fp64 at
    ``n_rel = 4, batch = 3, D = K = 8``: values and all three kinds of gradient within the fp32 summation bound."""
    UF, dev = _UF(), _dev()
    n_rel, batch, D, K = 4, 3, 8, 8
    rng = np.random.default_rng(2)
    query = rng.standard_normal((batch, K)).astype(np.float32)
    weights = [rng.standard_normal((n_rel * D, K)).astype(np.float32) for _ in range(2)]
    biases = [rng.standard_normal(n_rel * D).astype(np.float32) for _ in range(2)]
    upstream = [rng.standard_normal((n_rel, batch * D)).astype(np.float32) for _ in range(2)]

    def run(dtype, fn, device):
        leaf = lambda a: torch.from_numpy(a).to(device=device, dtype=dtype).requires_grad_()
        q, w, b = leaf(query), [leaf(a) for a in weights], [leaf(a) for a in biases]
        out = fn(q, w, b, n_rel)
        torch.autograd.backward(out, [torch.from_numpy(u).to(device=device, dtype=dtype) for u in upstream])
        return [t.detach().double().cpu().numpy() for t in list(out) + [x.grad for x in w + b] + [q.grad]]
    got = run(torch.float32, UF.query_tables, dev)
    want = run(torch.float64, UF.dense_query_tables, torch.device("cpu"))
    mass = ND.tables(query, weights, biases, n_rel, absolute=True)
    mw, mb, mq = ND.gradients(query, weights, upstream, n_rel, absolute=True)
    terms = [K + 1] * 2 + [batch] * 4 + [2 * n_rel * D]
    for a, c, m, n in zip(got, want, mass + mw + mb + [mq], terms):
        assert a.shape == c.shape and (np.abs(a - c) <= n * EPS * m.reshape(a.shape)).all()


# ------------------------------------------------------------------------------------------------ (b) the recorded cases
class RecordingBackend:
    """The backend in force behind an object that counts the calls of its entry points."""

    def __init__(self, inner):
        self._inner = inner
        self.calls = collections.Counter()

    def __getattr__(self, name):
        value = getattr(self._inner, name)
        if not callable(value) or name == "accepts" or name.endswith("_supported"):
            return value

        def counted(*args, **kwargs):
            self.calls[name] += 1
            return value(*args, **kwargs)
        return counted


_RUNS = {}


def hip_runs(name):
    if name not in _RUNS:
        from ultra_torchdrug_amd import backend
        got, calls = {}, {}
        for mode in ("eval", "train") if name in NC.TRAINED else ("eval",):
            proxy = RecordingBackend(backend.get())
            with backend.use(proxy):
                out = NC.run(name, _dev(), torch.float32, mode)
            torch.cuda.synchronize()
            got.update({k: v.detach().double().cpu().numpy() for k, v in out.items()})
            calls[mode] = proxy.calls
        _RUNS[name] = (got, calls)
    return _RUNS[name]


def _group(key):
    if "/train/d_" in key:
        return "gradient"
    if key.endswith("/scores_all"):
        return "scores_all"
    return "scores" if key.endswith("scores") else "hidden"


@pytest.mark.parametrize("name", list(NC.CASES))
def test_hip_path_equals_the_recording(name):
    got, _ = hip_runs(name)
    want = sorted(k for k in NC.stats()["tensors"] if k.startswith(name + "/"))
    assert sorted(got) == want
    for key in want:
        err, scale, ref_dev = NC.deviation(key, got[key])
        floor = FLOORS[_group(key)]
        print("%-10s %-52s %.3e of scale (reference's own %.3e)" % (_group(key), key, err / scale, ref_dev / scale))
        assert err <= 4 * ref_dev + floor * scale, (key, err, ref_dev, scale, floor)


def test_routes():
    """Which entry points each case reaches on the device: the tables of every ``dependent`` stack come from ``query_tables``
    (one call per Bellman-Ford), ``shipped64`` takes the sparse first layer and the fused score head, ``paper32`` the one-walk PNA
    statistics; ``independent16`` (``dependent=False``) and no other case builds its tables per layer."""
    calls = {name: hip_runs(name)[1] for name in NC.CASES}
    for name, modes in calls.items():
        for mode, seen in modes.items():
            print(name, mode, dict(seen))
    shipped = calls["shipped64"]["eval"]
    # two forwards per eval run: the 4 x 9 batch, then the four queries over all entities
    assert shipped["query_tables"] == 2 and shipped["rspmm_frontier"] == 2 and shipped["score_all_entities"] == 1
    assert shipped["score_candidates"] == 1 and shipped["combine"] == 2 * NC.LAYERS and not shipped["relation_project"]
    train = calls["shipped64"]["train"]
    assert train["query_tables"] == 1 and train["sum_layer"] == NC.LAYERS and train["remove_triples"] == 1
    paper = calls["paper32"]["eval"]
    assert paper["query_tables"] == 2 and paper["pna_statistics"] == 2 * NC.LAYERS and not paper["rspmm_frontier"]
    assert not paper["pna_combine_forward"] and not paper["score_all_entities"]            # 32 wide: the epilogues are ATen
    assert not calls["independent16"]["eval"]["query_tables"] and not calls["independent16"]["train"]["query_tables"]
    assert calls["independent16"]["eval"]["rspmm_forward"] == 2 * NC.LAYERS
    homogeneous = calls["homogeneous16"]
    assert homogeneous["eval"]["query_tables"] == 1 and homogeneous["train"]["query_tables"] == 1
    assert not homogeneous["train"]["remove_triples"]


def test_switch_selects_the_per_layer_tables(monkeypatch):
    """``functional.QUERY_TABLES = False`` (``ULTRA_QUERY_TABLES=0``): every layer builds its own table; the scores move by
    rounding only."""
    from ultra_torchdrug_amd import backend
    UF = _UF()
    on = hip_runs("shipped64")[0]["shipped64/scores"]
    monkeypatch.setattr(UF, "QUERY_TABLES", False)
    proxy = RecordingBackend(backend.get())
    with backend.use(proxy):
        off = NC.run("shipped64", _dev(), torch.float32, "eval")["shipped64/scores"].double().cpu().numpy()
    assert not proxy.calls["query_tables"]
    assert np.abs(on - off).max() <= 1e-5 * np.abs(on).max()


# ------------------------------------------------------------------------------------------------ (c) the fused sequence
@pytest.fixture(scope="module")
def layerwise_scores(tmp_path_factory):
    """The scores of the layer-by-layer route, from ONE child process for all cases."""
    path = str(tmp_path_factory.mktemp("nbfnet") / "layerwise.npz")
    env = dict(os.environ, ULTRA_FAST_INFERENCE="0")
    done = subprocess.run([sys.executable, os.path.join(HERE, "nbfnet_fast_child.py"), path], env=env, capture_output=True, text=True,
                          timeout=300)
    assert done.returncode == 0, done.stdout + done.stderr
    with np.load(path) as data:
        return {k: data[k] for k in data.files}


@pytest.mark.parametrize("name", ["shipped", "plain"])
def test_fast_sequence_equals_the_layerwise_route(name, layerwise_scores):
    from nbfnet_fast_child import fast_case
    from ultra_torchdrug_amd import backend
    UF = _UF()
    assert UF.FAST_INFERENCE
    model, graph, h, r = fast_case(name, _dev())
    proxy = RecordingBackend(backend.get())
    with backend.use(proxy), torch.no_grad():
        fast = model.score_all_entities(graph, h, r)
        same = model.score_all_entities(graph, [], h, r)
    torch.cuda.synchronize()
    # (the fused sequence asks the sparse first layer first; the layers never go through ``layer.forward``)
    assert proxy.calls["query_tables"] == 2 and proxy.calls["first_layer_forward"] == 2 and not proxy.calls["combine"], dict(proxy.calls)
    want = torch.from_numpy(layerwise_scores[name]).to(fast.device)
    assert fast.shape == want.shape == (len(h), graph.num_node)
    assert torch.equal(fast, want) and torch.equal(same, want)


def _wide_task(name="shipped", **kwargs):
    from nbfnet_fast_child import FAST_CASES
    from sampled_graphs import wide_batch, wide_graph
    from ultra_torchdrug_amd.task import build_nbfnet
    graph = wide_graph()
    torch.manual_seed(31 + list(FAST_CASES).index(name))
    options = dict(num_negative=8, full_batch_eval=True)
    options.update(kwargs)
    task = build_nbfnet(graph.num_relation, 64, (64,) * 6, **FAST_CASES[name], **options)
    task.preprocess(graph)
    return task.eval().to(_dev()), wide_batch(graph).to(_dev())


def test_fast_sequence_under_graphed_predict(layerwise_scores):
    """``task.predict`` (both sides stacked: the queries of the child's case) eagerly and replayed as one hipGraph."""
    from ultra_torchdrug_amd import engine
    task, batch = _wide_task("shipped")
    with torch.no_grad():
        eager = task.predict(batch)
    want = torch.from_numpy(layerwise_scores["shipped"]).to(eager.device)
    want = want.view(2, len(batch), -1).transpose(0, 1)
    assert torch.equal(eager, want)
    graphed = engine.GraphedPredict(task, batch)
    for rows in (batch, batch.flip(0)):
        got = graphed(rows).clone()
        with torch.no_grad():
            assert torch.equal(got, task.predict(rows))
    assert torch.equal(graphed(batch), want)


# ------------------------------------------------------------------------------------------------ (d) the task
def test_task_predicts_evaluates_and_answers():
    from ultra_torchdrug_amd import engine
    task, batch = _wide_task("shipped")
    with torch.no_grad():
        pred = task.predict(batch)
        ranks = task.rank_batch(batch)
        assert pred.shape == (len(batch), 2, 300) and torch.equal(ranks, task.get_ranking(pred, task.target(batch)))
    metric, ranking = engine.evaluate(task, batch, batch_size=8)
    assert torch.equal(ranking, ranks) and abs(float(metric["mrr"]) - float((1 / ranks.double()).mean())) < 1e-6
    # answers against the dense definition: the filtered scores sorted by (score descending, entity ascending)
    entities, scores = task.answer(batch[:, 0], batch[:, 2], k=7)
    mask, _ = task.target(batch)
    for q in range(len(batch)):
        row = pred[q, 0].clone()
        row[~mask[q, 0]] = float("-inf")
        order = sorted(range(300), key=lambda v: (-float(row[v]), v))[:7]
        assert entities[q].tolist() == order and torch.equal(scores[q], row[order])
    again = engine.answer(task, batch[:, 0], batch[:, 2], k=7)
    assert torch.equal(again[0], entities) and torch.equal(again[1], scores)


def test_task_explains_with_paths_of_the_graph():
    task, batch = _wide_task("shipped")
    und = task.model._undirected(task.fact_graph)
    edges = set(map(tuple, und.edge_list.tolist()))
    found = task.explain(batch[:2])
    assert len(found) == 2
    for (paths, weights), (h, t, r) in zip(found, batch[:2].tolist()):
        assert len(paths) == len(weights) >= 1
        for path in paths:
            assert path[0][0] == h and path[-1][1] == t and all(edge in edges for edge in path)
            assert all(a[1] == b[0] for a, b in zip(path, path[1:]))
    paths, weights = task.visualize(batch[0])
    assert len(paths) == len(weights) >= 1 and all(edge in edges for path in paths for edge in path)


def test_captured_training_steps_equal_eager_steps():
    """An eager ``train_step`` runs; three replays of a captured ``GraphedTrainStep`` (one graph, no reducer) take the three eager
    steps from the same state: equal losses, equal parameters, bit for bit."""
    from ultra_torchdrug_amd import engine
    task, _ = _wide_task("shipped", num_negative=16)
    task.train()
    triples = task.fact_graph.edge_list
    twin = copy.deepcopy(task)
    batches = [triples[i:i + 8].contiguous() for i in (0, 8, 16, 24)]
    opt_e = torch.optim.AdamW(task.parameters(), lr=1e-3)
    losses_e = []
    for b in batches[1:]:
        torch.manual_seed(int(b[0, 0]))
        losses_e.append(engine.train_step(task, opt_e, b)[0].item())
    assert all(np.isfinite(losses_e))
    opt_g = torch.optim.AdamW(twin.parameters(), lr=1e-3)
    step = engine.GraphedTrainStep(twin, opt_g, batches[0])
    assert step.mode == "single"
    losses_g = []
    for b in batches[1:]:
        torch.manual_seed(int(b[0, 0]))
        losses_g.append(step(b)[0].item())
    assert losses_g == losses_e
    for (k, a), (_, b) in zip(task.named_parameters(), twin.named_parameters()):
        assert torch.equal(a, b), k
    moved = [k for (k, a), (_, b) in zip(task.named_parameters(), _wide_task("shipped")[0].named_parameters()) if not torch.equal(a, b)]
    assert "model.query.weight" in moved and "model.layers.0.relation_linear.weight" in moved


def test_homogeneous_graph_trains_and_predicts():
    """``num_relation=None`` on a 200-node graph without relations: scores of the shape of 1-D ``h``, a training step that moves
    the parameters, and ``predict``-like scoring of every node as the tail of four heads."""
    from ultra_torchdrug_amd import NeuralBellmanFordNetwork
    from ultra_torchdrug_amd.graph import Graph
    dev = _dev()
    rng = np.random.default_rng(4)
    edges = np.unique(rng.integers(0, 200, size=(1500, 2)), axis=0)
    graph = Graph(torch.from_numpy(edges).to(dev), None, 200, None)
    torch.manual_seed(8)
    model = NeuralBellmanFordNetwork(16, [16] * 3, None, message_func="distmult", aggregate_func="sum", short_cut=True,
                                     layer_norm=True).to(dev)
    pairs = torch.from_numpy(edges[:12]).to(dev)
    optimizer = torch.optim.AdamW(model.parameters(), lr=1e-2)
    before = model.query.weight.detach().clone()
    model.train()
    score = model(graph, pairs[:, 0], pairs[:, 1], all_loss=torch.zeros((), device=dev))
    assert score.shape == (12,)
    torch.nn.functional.binary_cross_entropy_with_logits(score, torch.ones_like(score)).backward()
    optimizer.step()
    assert not torch.equal(before, model.query.weight) and model.layers[0].relation_linear.weight.grad.abs().max() > 0
    model.eval()
    heads = pairs[:4, 0].repeat_interleave(200)
    tails = torch.arange(200, device=dev).repeat(4)
    with torch.no_grad():
        every = model(graph, heads, tails)
        some = model(graph, pairs[:4, 0], pairs[:4, 1])
    assert every.shape == (800,) and bool(torch.isfinite(every).all())
    rows = torch.arange(4, device=dev) * 200 + pairs[:4, 1]
    assert torch.allclose(every[rows], some, rtol=1e-5, atol=1e-6)

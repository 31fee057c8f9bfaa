"""What the launches TOUCH: every kernel family at its edge shapes under the guard of tests/guarded_memory.py.

Every case runs the same call twice -- plainly, and inside ``guarded`` with its tensor inputs copied by ``banded`` (NaN bands
around floats, zero bands around integers) -- and asserts

  (a) the guarded result carries the bits of the unguarded one (int32 / int64 views);
  (b) the guarded result agrees with the family's INDEPENDENT reference: the oracle where the family is pinned to it bit for
      bit, the fp64 ATen / numpy definition at the tolerance the family's own test uses, integers exactly -- (a) alone cannot
      fail when both runs are wrong in the same way;
  (c) ``check()``: every band of every allocation the wrappers made, and of every input, still holds its pattern;
  (d) no poison payload is left in a tensor the call documents as fully written.

and, where the library records its launches (the plan runs of every rspmm and rotate call, ``_lib.launch_records``; class
``Launches`` below), the kernel that ran: family and kind, the ``x_lds`` / ``act`` / ``dead`` form where a case is about it, the
same records in both runs, and NO record from the entries that launch outside the plan launchers.  The epilogue, score-head and
integer entries have one kernel each per knob value and no launch record: there the knob IS the selection (as in
tests/test_combine_paired_gpu.py and tests/test_row_per_lane_gpu.py).

Shapes are the smallest that reach the tail and boundary code: 1, 33 and 32 * 24 + 5 rows of 64 floats for the 32-row tiles
of the epilogues (one short tile; a full tile + one row; several tiles per wave in one workgroup + a tail).  The widest row any
case stores is 256 columns of fp32 = 1 KiB, so the default band of 64 KiB holds 64 such rows (guarded_memory's docstring).
"""
import contextlib
import os

import numpy as np
import pytest
import torch

import guarded_memory as GM
from guarded_memory import guarded  # the context manager: cases choose their modules and bands
from guarded_memory import guarded_fixture  # noqa: F401  (registers the fixture ``guarded``; a test that names it gets the default guard)
import test_combine_paired_gpu as CP
import test_row_per_lane_gpu as RPL
from graphs import random_graph
from oracle_ops import OracleFunctional

pytestmark = pytest.mark.gpu

ROWS = [1, 33, 32 * 24 + 5]


def _dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


@contextlib.contextmanager
def _knob(bits):
    import ultra_torchdrug_amd as U
    lib = U.require_library()
    lib.ultra_rspmm_force_general_path(bits)
    try:
        yield
    finally:
        lib.ultra_rspmm_force_general_path(0)


def _flat(result):
    """The tensors of a result (a tensor, ``None``, or nested tuples / lists of them), in order."""
    if result is None:
        return []
    if isinstance(result, torch.Tensor):
        return [result]
    out = []
    for r in result:
        out += _flat(r)
    return out


def _bits(t):
    t = t.detach().contiguous()
    if t.dtype in (torch.float32, torch.float64):
        return t.view(torch.int32 if t.dtype == torch.float32 else torch.int64)
    return t


def assert_same_bits(got, want, what=""):
    got, want = _flat(got), _flat(want)
    assert len(got) == len(want), what
    for k, (g, w) in enumerate(zip(got, want)):
        assert g.shape == w.shape and g.dtype == w.dtype, (what, k, g.shape, w.shape)
        assert torch.equal(_bits(g), _bits(w)), "%s: output %d under the guard differs from the unguarded run" % (what, k)


def assert_no_poison(result, what=""):
    for k, t in enumerate(_flat(result)):
        if t.dtype in (torch.float32, torch.float64):
            assert not GM.has_poison(t), "%s: output %d still holds the poison of an unwritten allocation" % (what, k)


def run_guarded(fn, *args, modules=(), widest_row=1024, what="", defined=None):
    """``fn(*args)`` plainly and under the guard with every tensor argument ``banded``; asserts (a), (c), (d) and returns the
    guarded result for (b).  ``defined(result)``: the part of the result the call documents as written (default: all of it)."""
    defined = defined or (lambda r: r)
    with torch.no_grad():
        plain = fn(*[a.clone() if isinstance(a, torch.Tensor) else a for a in args])    # (a call may overwrite an operand)
        torch.cuda.synchronize()
    with guarded(*modules, widest_row=widest_row) as guard:
        inputs = [guard.banded(a) if isinstance(a, torch.Tensor) else a for a in args]
        with torch.no_grad():
            got = fn(*inputs)
        guard.check()                                                                   # (c), and once more when the guard closes
        assert guard.records, what
    assert_same_bits(defined(got), defined(plain), what)                                # (a)
    assert_no_poison(defined(got), what)                                                # (d)
    return got


class Launches:
    """The library's launch records (``_lib.launch_records``: per thread, the plan runs of rspmm and rotate calls) around single
    calls, collected over the plain and the guarded run of a case: ``call(fn, *args)`` clears the ring, calls and keeps the
    records; ``check(*wants)`` asserts that both runs recorded the same (all fields but the running ``seq``) and, per call, the
    expected number of records with the expected fields (``wants[i]``: one dict per record of call ``i``)."""

    def __init__(self):
        self.calls = []

    def call(self, fn, *args, **kwargs):
        from ultra_torchdrug_amd import _lib
        _lib.launch_records_clear()
        out = fn(*args, **kwargs)
        count, rows = _lib.launch_records()
        self.calls.append((count, [{k: v for k, v in row.items() if k != "seq"} for row in rows]))
        return out

    def check(self, *wants):
        assert len(self.calls) == 2 * len(wants), (len(self.calls), len(wants))
        plain, guarded_run = self.calls[:len(wants)], self.calls[len(wants):]
        assert plain == guarded_run, "the guarded run launched other kernels than the plain run"
        for i, ((count, rows), want) in enumerate(zip(guarded_run, wants)):
            assert count == len(rows) == len(want), (i, count, rows)
            for row, fields in zip(rows, want):
                assert row["status"] == 0 and {k: row[k] for k in fields} == fields, (i, fields, row)
        del self.calls[:]


def _close(got, want, what, rel=2e-5, floor=1e-6):
    """The bar of the epilogue backward tests: ``rel`` of the gradient's largest entry (tests/test_rspmm_gpu.py)."""
    want = want.double().cpu()
    scale = want.abs().max().item() + 1e-12
    err = (got.detach().double().cpu() - want).abs().max().item()
    assert err <= rel * scale + floor, "%s: err %.3g vs scale %.3g" % (what, err, scale)


# ==================================================================================================== the mechanism on the device
def test_a_device_write_into_either_band_is_named():
    """Detection without a faulty kernel: a torch indexing write one element before and one element after a device body."""
    dev = _dev()
    guard = GM.Guard()
    body = guard.carve((33, 64), torch.float32, dev)
    other = guard.carve((7,), torch.int32, dev)
    assert body.is_cuda and bool(torch.isnan(body).all()) and bool((other == -1).all())
    guard.check()
    raw = guard.records[0].buffer
    before = torch.tensor([guard.band - 4, guard.band - 3, guard.band - 2, guard.band - 1], device=dev)
    keep = raw[before].clone()
    raw[before] = torch.zeros(4, dtype=torch.uint8, device=dev)
    with pytest.raises(GM.BandDamage, match=r"leading band of allocation \(33, 64\) torch.float32 .*test_memory_bounds_gpu.py:\d+.* offset -4 "):
        guard.check()
    raw[before] = keep
    guard.check()
    after = torch.tensor([guard.band + 33 * 64 * 4], device=dev)
    raw[after] = torch.zeros(1, dtype=torch.uint8, device=dev)
    with pytest.raises(GM.BandDamage, match=r"trailing band of allocation \(33, 64\) .* offset %d " % (33 * 64 * 4)) as err:
        guard.check()
    assert "(7,)" not in str(err.value)


def test_a_float_body_left_unwritten_is_reported():
    """(d) without a faulty kernel: an output of which one row was never stored still carries the payload."""
    from ultra_torchdrug_amd import functional as UF
    dev = _dev()
    with guarded() as guard:
        out = UF.torch.empty(33, 64, dtype=torch.float32, device=dev)
        assert isinstance(UF.torch, GM.TorchProxy) and len(guard.records) == 1
        out[:32] = 1.0                                                   # a "kernel" that forgets the tail tile's only row
    assert GM.has_poison(out) and not GM.has_poison(out[:32])
    with pytest.raises(AssertionError, match="poison"):
        assert_no_poison((out,), "tail row")
    out[32] = 2.0
    assert_no_poison((out,))


def test_the_guard_refuses_to_start_inside_a_capture():
    dev = _dev()
    x = torch.zeros(4, device=dev)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            x.add_(1)
            with pytest.raises(RuntimeError, match="capturing"):
                with guarded():
                    pass
    torch.cuda.current_stream().wait_stream(side)


# ==================================================================================================== epilogue family
@pytest.mark.parametrize("alias", [False, True], ids=["separate_out", "out_is_update"])
@pytest.mark.parametrize("knob", [0, 256, 512, 512 | 2048])
@pytest.mark.parametrize("rows", ROWS)
def test_combine_forward(rows, knob, alias):
    """``ultra_combine_forward_f32`` in each of its forms against the oracle's C restatement, bit for bit (the bar of
    tests/test_combine_paired_gpu.py, whose operands and memoised oracle results this uses)."""
    from ultra_torchdrug_amd import functional as UF
    x, u, w, b, gamma, beta = CP._on_device(rows, "normal")

    def call(x, u, w, b, gamma, beta):
        with _knob(knob):
            out = UF.combine_forward(x, u, w, b, gamma, beta, 1e-5, True, True, reuse_update=alias)
            assert (out.data_ptr() == u.data_ptr()) == alias
            return out

    got = run_guarded(call, x, u, w, b, gamma, beta, what="combine_forward")           # (both runs work on copies of their own)
    assert np.array_equal(got.cpu().numpy(), CP._oracle(rows, "normal", True, True, True).numpy())


_combine_memo = {}


def _combine_reference(rows, ln, relu, shortcut):
    """fp64 autograd of the reference's chain cat -> Linear -> LayerNorm -> relu (+ input) on the operands of
    test_combine_paired_gpu: ``(out, gout, [d_input, d_update, d_weight, d_bias, d_gamma, d_beta])``.  Rows with a
    pre-activation within 1e-4 of 0 get a zero output gradient (tests/test_rspmm_gpu.py: relu is not differentiable there)."""
    key = (rows, ln, relu, shortcut)
    if key not in _combine_memo:
        leaves = [t.double().requires_grad_() for t in CP._operands(rows, "normal")]
        x, u, w, b, gamma, beta = leaves
        gout = torch.randn(rows, 64, generator=torch.Generator().manual_seed(rows))
        ref = torch.nn.functional.linear(torch.cat([x, u], dim=-1), w, b)
        if ln:
            ref = torch.nn.functional.layer_norm(ref, (64,), gamma, beta, 1e-5)
        if relu:
            gout[(ref.detach().abs() < 1e-4).any(dim=1)] = 0.0
            ref = torch.relu(ref)
        if shortcut:
            ref = ref + x
        ref.backward(gout.double())
        _combine_memo[key] = (ref.detach(), gout, [t.grad for t in (leaves if ln else leaves[:4])])
    return _combine_memo[key]


NAMES = ["d_input", "d_update", "d_weight", "d_bias", "d_ln_weight", "d_ln_bias"]


@pytest.mark.parametrize("mode,keep", [("fused", False), ("split", False), ("fused", True)], ids=["fused", "split", "fused_keep_pre_norm"])
@pytest.mark.parametrize("rows", ROWS)
def test_combine_with_backward(monkeypatch, rows, mode, keep):
    """``functional.combine`` forward + backward (one-pass and three-kernel form, once with the kept pre-norm tensor) against
    fp64 autograd of the reference chain at 2e-5 of each gradient's scale.  The partial slabs of the split form (``dw_p`` /
    ``dbias_p`` / ``dg_p``: ``n_wg`` slabs summed whether or not a workgroup had a tile) are poisoned here."""
    from ultra_torchdrug_amd import functional as UF
    monkeypatch.setenv("ULTRA_COMBINE_BWD", mode)
    monkeypatch.setattr(UF, "KEEP_PRE_NORM", keep)
    want_out, gout, want = _combine_reference(rows, True, True, True)
    ops = CP._on_device(rows, "normal")

    def call(gout, *ops):
        with torch.enable_grad():
            leaves = [t.detach().requires_grad_() for t in ops]
            out = UF.combine(*leaves, 1e-5, True, True)
            out.backward(gout)
        return [out.detach()] + [t.grad for t in leaves]

    got = run_guarded(call, gout.to(_dev()), *ops, what="combine %s" % mode)
    torch.testing.assert_close(got[0].cpu().double(), want_out, rtol=2e-5, atol=2e-5)
    for name, g, w in zip(NAMES, got[1:], want):
        _close(g, w, name)


@pytest.mark.parametrize("rows", ROWS)
def test_epilogue_backward_entries_store_inside_views_of_the_tests_choosing(rows):
    """The C entries themselves (``_lib.launch``), with ``d_input`` / ``d_update`` carved by the test: the one-pass backward's
    stores (its comment: "no store guard", the descriptor's range check drops the tail tile's rows) and ``ultra_combine_dxdu_f32``
    of the split form, held by bands on both sides of exactly ``rows`` rows."""
    from ultra_torchdrug_amd import _lib, functional as UF
    dev = _dev()
    _, gout, want = _combine_reference(rows, True, True, True)
    x, u, w, b, gamma, beta = CP._on_device(rows, "normal")
    with guarded(widest_row=256) as guard:
        xb, ub, gb = guard.banded(x), guard.banded(u), guard.banded(gout.to(dev))
        epilogue = UF._epilogue(w, b, gamma, beta, 1e-5, True, True)
        grads = [guard.carve((rows, 64), torch.float32, dev), guard.carve((rows, 64), torch.float32, dev),
                 guard.carve((64, 128), torch.float32, dev)] + [guard.carve((64,), torch.float32, dev) for _ in range(3)]
        UF._combine_backward_fused(xb, ub, epilogue, gb, None, grads)
        guard.check()
        assert_no_poison(grads, "ultra_combine_backward_fused_f32")
        for name, g, w64 in zip(NAMES, grads, want):
            _close(g.view(w64.shape), w64, name)
        # the split form's activation gradients from a d_z of the test's own: d_input | d_update = d_z . W (+ grad_out)
        d_z = guard.banded(torch.randn(rows, 64, generator=torch.Generator().manual_seed(rows + 1)).to(dev))
        d_in, d_up = guard.carve((rows, 64), torch.float32, dev), guard.carve((rows, 64), torch.float32, dev)
        _lib.launch(dev, "ultra_combine_dxdu_f32", d_z, w, gb, d_in, d_up, rows, 64)
        guard.check()
        assert_no_poison([d_in, d_up], "ultra_combine_dxdu_f32")
        w64, z64 = w.double().cpu(), d_z.double().cpu()
        _close(d_in, z64 @ w64[:, :64] + gb.double().cpu(), "dxdu d_input")
        _close(d_up, z64 @ w64[:, 64:], "dxdu d_update")


@pytest.mark.parametrize("shape", [(64, 64, True), (128, 1, False)], ids=["64_to_64", "128_to_1"])
@pytest.mark.parametrize("rows", ROWS)
def test_linear_forward(oracle, rows, shape):
    from ultra_torchdrug_amd import functional as UF
    k, n, relu = shape
    gen = torch.Generator().manual_seed(rows + k)
    x, w, b = torch.randn(rows, k, generator=gen), torch.randn(n, k, generator=gen) / k ** 0.5, torch.randn(n, generator=gen)
    got = run_guarded(lambda x, w, b: UF.linear_forward(x, w, b, relu=relu), x.to(_dev()), w.to(_dev()), b.to(_dev()), what="linear_forward")
    assert np.array_equal(got.cpu().numpy(), oracle.linear_forward(x.numpy(), w.numpy(), b.numpy(), relu))


@pytest.mark.parametrize("knob", [0, 1024])
@pytest.mark.parametrize("n_node,batch", [(1, 1), (11, 3), (32 * 24 + 5, 1), (37, 3)])
def test_score_all_entities(n_node, batch, knob):
    """Both forms of the score head (rows = nodes x queries: 1, 33, 32 * 24 + 5 and 111) against the oracle, bit for bit."""
    from ultra_torchdrug_amd import functional as UF
    ops = tuple(_t(a) for a in RPL._operands(n_node, batch, "normal"))

    def call(*ops):
        with _knob(knob):
            return UF.score_all_entities(*ops)

    got = run_guarded(call, *ops, what="score_all_entities")
    assert np.array_equal(got.cpu().numpy(), RPL._oracle(n_node, batch, "normal"))


@pytest.mark.parametrize("n_node,batch,per_row", [(1, 1, 1), (11, 3, 33), (200, 5, 160)])
def test_score_candidates_with_backward(n_node, batch, per_row):
    """``ultra_score_rows_*`` against fp64 autograd of the reference chain (oracle_ops.score_candidates: index, cat, two
    Linear) at 2e-5 of each result's scale; ``d_hidden`` is zero outside the candidates' rows and must be written everywhere."""
    from ultra_torchdrug_amd import functional as UF
    hidden, query, w1, b1, w2, b2 = (torch.from_numpy(a) for a in RPL._operands(n_node, batch, "normal"))
    gen = torch.Generator().manual_seed(per_row)
    t_index = torch.randint(0, n_node, (batch, per_row), generator=gen)
    gout = torch.randn(batch, per_row, generator=gen)
    leaves64 = [t.double().requires_grad_() for t in (hidden, query, w1, b1, w2, b2)]
    want = OracleFunctional.score_candidates(leaves64[0], leaves64[1], t_index, *leaves64[2:])
    want.backward(gout.double())

    def call(gout, t_index, *ops):
        with torch.enable_grad():
            leaves = [t.detach().requires_grad_() for t in ops]
            score = UF.score_candidates(leaves[0], leaves[1], t_index, *leaves[2:])
            score.backward(gout)
        return [score.detach()] + [t.grad for t in leaves]

    dev = _dev()
    got = run_guarded(call, gout.to(dev), t_index.to(dev), *(t.to(dev) for t in (hidden, query, w1, b1, w2, b2)), what="score_candidates")
    torch.testing.assert_close(got[0].cpu(), want.detach().float(), rtol=2e-5, atol=2e-5)          # (tests/test_model_gpu.py's bars)
    for name, g, leaf in zip(("d_hidden", "d_query", "d_w1", "d_b1", "d_w2", "d_b2"), got[1:], leaves64):
        _close(g, leaf.grad, name, floor=1e-7)


@pytest.mark.parametrize("batch,n_rel,n_layers", [(1, 1, 2), (3, 11, 1), (5, 155, 3)])
def test_relation_project_with_backward(batch, n_rel, n_layers):
    """Rows = batch x relations: 1, 33, 775.  Forward against the oracle's documented order (bit for bit, through
    ``OracleFunctional.relation_project``), the one-launch backward against fp64 autograd of the reference chain at 2e-5."""
    from ultra_torchdrug_amd import functional as UF
    gen = torch.Generator().manual_seed(batch * 1000 + n_rel)
    relation = torch.randn(batch, n_rel, 64, generator=gen)
    flat = []
    for _ in range(n_layers):
        flat += [torch.randn(64, 64, generator=gen) * 0.2, torch.randn(64, generator=gen) * 0.1,
                 torch.randn(64, 64, generator=gen) * 0.2, torch.randn(64, generator=gen) * 0.1]
    table_grads = [torch.randn(n_rel, batch * 64, generator=gen) for _ in range(n_layers)]
    group = lambda ts: [tuple(ts[4 * l:4 * l + 4]) for l in range(n_layers)]
    with torch.no_grad():
        want_tables = OracleFunctional(None).relation_project(relation, group(flat))
    x64 = relation.double().requires_grad_()
    w64 = [t.double().requires_grad_() for t in flat]
    tables64 = OracleFunctional.relation_project_train(x64, group(w64))
    sum((t * g.double()).sum() for t, g in zip(tables64, table_grads)).backward()

    def call(relation, *rest):
        grads, ws = rest[:n_layers], rest[n_layers:]
        plain = UF.relation_project(relation, group(ws))
        twice = UF.relation_project(relation, group(ws), repeat=2)
        with torch.enable_grad():
            x = relation.detach().requires_grad_()
            leaves = [t.detach().requires_grad_() for t in ws]
            tables = UF.relation_project_train(x, group(leaves))
            sum((t * g).sum() for t, g in zip(tables, grads)).backward()
        return [plain, twice, [t.detach() for t in tables], x.grad, [t.grad for t in leaves]]

    dev = _dev()
    plain, twice, tables, d_x, d_w = run_guarded(call, relation.to(dev), *(t.to(dev) for t in table_grads + flat), what="relation_project")
    for p, tw, tr, want in zip(plain, twice, tables, want_tables):
        assert np.array_equal(p.cpu().numpy(), want.numpy()) and torch.equal(tr, p) and torch.equal(tw, torch.cat([p, p], dim=1))
    _close(d_x, x64.grad, "d_relation", floor=0.0)
    for k, (g, leaf) in enumerate(zip(d_w, w64)):
        _close(g, leaf.grad, "d_w[%d]" % k, floor=0.0)


@pytest.mark.parametrize("numel,repeat", [(1, 0), (33 * 64, 3), ((32 * 24 + 5) * 64, 0), (1 << 18, 5)])
def test_statistics(numel, repeat):
    """``ultra_statistics_f32`` (per-block fp64 partials, then one block) against ``Tensor.norm / mean / std`` in fp64, at the
    1e-5 relative bar of tests/test_model_gpu.py's statistics test; 2^18 + 1 elements for more than one block of partials."""
    from ultra_torchdrug_amd import functional as UF
    gen = torch.Generator().manual_seed(numel)
    values = torch.randn(numel + (numel > 1000), generator=gen) * 2 + 0.5
    extra = torch.randn(7, 64, generator=gen) if repeat else None
    dev = _dev()
    got = run_guarded(lambda v, e: UF.statistics(v, e, repeat), values.to(dev), None if extra is None else extra.to(dev), what="statistics")
    flat = values.double() if extra is None else torch.cat([values.double(), extra.double().reshape(1, -1).expand(repeat, -1).reshape(-1)])
    want = torch.stack([flat.norm(), flat.mean(), flat.std() if flat.numel() > 1 else torch.tensor(float("nan"), dtype=torch.float64)])
    torch.testing.assert_close(got.cpu(), want.float(), rtol=1e-5, atol=1e-6, equal_nan=True)


@pytest.mark.parametrize("rows,cols,temperature", [(1, 2, 1.0), (33, 33, 0.5), (65, 257, 0.0)])
def test_bce_adversarial_loss(rows, cols, temperature):
    """Loss and gradient in one launch against the reference's ATen chain (oracle_ops.bce_adversarial_loss) in fp64."""
    from ultra_torchdrug_amd import functional as UF
    gen = torch.Generator().manual_seed(rows * cols)
    pred = torch.randn(rows, cols, generator=gen) * 3
    gout = torch.randn(rows, generator=gen)
    p64 = pred.double().requires_grad_()
    want = OracleFunctional.bce_adversarial_loss(p64, temperature)
    want.backward(gout.double())

    def call(pred, gout):
        with torch.enable_grad():
            p = pred.detach().requires_grad_()
            loss = UF.bce_adversarial_loss(p, temperature)
            loss.backward(gout)
        return loss.detach(), p.grad

    loss, grad = run_guarded(call, pred.to(_dev()), gout.to(_dev()), what="bce_adversarial_loss")
    torch.testing.assert_close(loss.cpu(), want.detach().float(), rtol=2e-6, atol=2e-6)           # (the bars of tests/test_model_gpu.py)
    torch.testing.assert_close(grad.cpu(), p64.grad.float(), rtol=1e-5, atol=1e-7)


# ==================================================================================================== rspmm family (ULTRA_BINDING=ctypes)
# With the ctypes binding every operand of these entries is allocated in functional.py (through the dispatcher the outputs are
# at::empty in csrc/torch_ext.cpp, which no proxy sees).  The RelCSR is built INSIDE the guard, by both plan builders: its
# packed words, chunk and long-row tables, builder scratch, weights and slack words are poisoned and banded too.
SUMS, MULS = ("add", "min", "max"), ("mul", "add")
DENSE, ROWGROUP, QUAD, PACKED, GENERAL, ROTATE = 0, 1, 2, 3, 4, 5
FWD, DX, DREL = 0, 1, 2
# name: (graph of tests/test_rspmm_gpu.py's CASES or keywords, nodes, relations, F, RelCSR options, knob values)
PLANS = {
    "isolated_and_ragged_F": ("isolated_and_ragged_F", {}, [0, 1, 4]),                      # F = 100: a ragged last column tile
    "skewed_hub": ("skewed_hub", {}, [0, 2, 32]),                                           # F = 192; the hub row is split (fix-up)
    "hub_split": ((dict(n_edge=30000, skew=True, hub_row=5, hub_edges=4000), 900, 14, 64), dict(chunk_edges=16, piece_len=64), [0]),
    "wide_ids": ("isolated_and_ragged_F", dict(wide_ids=True), [0, 8, 16]),                 # no split row: one row per lane group
    "wide_ids_hub": ("skewed_hub", dict(wide_ids=True), [0]),                               # split rows: the big-graph packed kernel
}
_rspmm_memo = {}


def _plan_case(name, oracle):
    """Graph, operands (numpy) and every oracle result of a plan case, computed once."""
    if name in _rspmm_memo:
        return _rspmm_memo[name]
    import zlib
    import test_rspmm_gpu as RS
    graph, opts, _ = PLANS[name]
    kw, n, r, F = RS.CASES[graph] if isinstance(graph, str) else graph
    g = random_graph(seed=zlib.crc32(name.encode()) % 1000, n_node=n, n_rel=r, **dict(kw, unique=True))
    rng = np.random.default_rng(len(name))
    f32 = lambda *shape: rng.standard_normal(shape).astype(np.float32)
    relation, x, grad, add, base = f32(r, F), f32(n, F), f32(n, F), f32(n, F), f32(n, F)
    n_query = 5 if F == 100 else F // 64
    b_node = rng.integers(0, n, n_query).astype(np.int32)
    b_node[0] = 5                                                                          # (the hub row of the hub graphs)
    b_value = f32(n_query, F // n_query)
    opts = dict(opts, piece_len=opts.get("piece_len", 128))          # (128: what a graph of this size gets by default; the oracle needs it)
    piece = opts["piece_len"]
    csr_o = oracle.coalesce_csr(g["dst"], g["src"], g["rel"], g["w"], n, n, r)
    want = {}
    for s in SUMS:
        for m in MULS:
            out = oracle.rspmm_forward(csr_o, relation, x, s, m, piece=piece)
            d_rel, d_x = oracle.rspmm_backward(csr_o, relation, x, out, grad, s, m, piece=piece)
            want[s, m] = (out, d_x, d_rel)
    dense = OracleFunctional._dense_boundary((torch.from_numpy(b_node), torch.from_numpy(b_value)), n).numpy()
    out_seq = oracle.rspmm_forward(csr_o, relation, x, "add", "mul", piece=0)
    _, _, d_w = oracle.rspmm_backward(csr_o, relation, x, out_seq, grad, "add", "mul", need_weight_grad=True)
    case = dict(g=g, n=n, r=r, F=F, opts=opts, piece=piece, relation=relation, x=x, grad=grad, add=add, base=base, b_node=b_node,
                b_value=b_value, want=want, dense=dense, d_w=d_w, csr_o=csr_o)
    _rspmm_memo[name] = case
    return case


def _forward_family(big, n_long_rows, knob):
    """The family ``plan_path()`` (csrc/plan_path.h) gives a FORWARD over these plans -- packed words present, the relation tile
    in LDS, F a multiple of 4, every pointer 256-byte aligned: bit 0 forces the general kernel; plans with the node ids outside
    the word run one row per lane group unless a row is split or bit 3 is set, then packed_kernel; the others run quad_kernel
    unless bit 2 asks for packed_kernel."""
    if knob & 1:
        return GENERAL
    if big:
        return ROWGROUP if (n_long_rows == 0 and not knob & 8) else PACKED
    return PACKED if knob & 4 else QUAD


@pytest.mark.parametrize("name,knob", [(name, knob) for name in PLANS for knob in PLANS[name][2]])
def test_rspmm_forward_backward_and_both_plan_builders(oracle, monkeypatch, name, knob):
    """``rspmm_forward`` (six operator pairs, dense and sparse boundary epilogue), ``rspmm_backward`` (six pairs, and accumulated
    into a given gradient) and ``rspmm_backward_weight`` over plans built inside the guard by the native and by the torch
    builder: the oracle in the kernels' order, bit for bit (tests/test_rspmm_gpu.py); the weight gradient at that file's 1e-4."""
    from ultra_torchdrug_amd import RelCSR, _lib, functional as UF
    monkeypatch.setenv("ULTRA_BINDING", "ctypes")
    c = _plan_case(name, oracle)
    n, r, F, g = c["n"], c["r"], c["F"], c["g"]
    records = []

    def call(dst, src, rel, relation, x, grad, add, base, b_node, b_value):
        csr = RelCSR(dst, src, rel, None, n, n, r, **c["opts"])
        assert csr.piece_len == c["piece"] and csr.fwd.builder == os.environ["ULTRA_RELCSR_BUILDER"]
        shape = (csr.fwd.packed_src_shift == 32, int(csr.fwd.long_rows.shape[0]))
        outs, recs = [], []
        with _knob(knob):
            for s in SUMS:
                for m in MULS:
                    _lib.launch_records_clear()
                    out = UF.rspmm_forward(csr, relation, x, s, m)
                    recs.append(_lib.launch_records())
                    _lib.launch_records_clear()
                    d_x, d_rel = UF.rspmm_backward(csr, relation, x, out, grad, s, m)
                    recs.append(_lib.launch_records())
                    outs += [out, d_x, d_rel]
            outs.append(UF.rspmm_forward(csr, relation, x, "add", "mul", add_rows=add))
            outs.append(UF.rspmm_forward(csr, relation, x, "max", "mul", add_rows=add))
            outs.append(UF.rspmm_forward(csr, relation, x, "add", "mul", boundary=(b_node, b_value)))
            acc = base.clone()
            d_acc, _ = UF.rspmm_backward(csr, relation, x, None, grad, "add", "mul", need_relation=False, d_input_add=acc)
            assert d_acc.data_ptr() == acc.data_ptr()
            outs.append(d_acc)
            outs.append(UF.rspmm_backward_weight(csr, relation, x, outs[0], grad, "add", "mul"))
        records.append((shape, recs))
        return outs

    args = [_t(g[k]) for k in ("dst", "src", "rel")] + [_t(c[k]) for k in ("relation", "x", "grad", "add", "base", "b_node", "b_value")]
    results = {}
    for builder in ("native", "torch"):
        monkeypatch.setenv("ULTRA_RELCSR_BUILDER", builder)
        del records[:]
        got = results[builder] = [t.cpu().numpy() for t in run_guarded(call, *args, modules=("functional", "relcsr"), widest_row=4 * F,
                                                                       what="%s %s" % (name, builder))]
        # the kernels that ran: the same in both runs, and the family plan_path.h gives this plan under this knob
        (shape, plain_recs), (shape_g, guarded_recs) = records
        assert shape == shape_g and shape[0] == bool(c["opts"].get("wide_ids"))
        strip = lambda recs: [(count, [{k: v for k, v in rec.items() if k != "seq"} for rec in rows]) for count, rows in recs]
        assert strip(plain_recs) == strip(guarded_recs)
        for k, (count, rows) in enumerate(guarded_recs):
            forward = k % 2 == 0
            assert count == len(rows) == (1 if forward else 2) and all(rec["status"] == 0 for rec in rows), (k, count, rows)
            if forward:
                assert rows[0]["kind"] == FWD and rows[0]["family"] == _forward_family(shape[0], shape[1], knob), (k, rows[0])
                if rows[0]["family"] == QUAD and knob & 2:
                    assert rows[0]["x_lds"] == 0
            else:
                assert [rec["kind"] for rec in rows] == [DX, DREL]
        k = 0
        for s in SUMS:
            for m in MULS:
                for what, want in zip(("forward", "d_input", "d_relation"), c["want"][s, m]):
                    assert np.array_equal(got[k], want), "%s %s %s/%s differs from the oracle" % (name, what, s, m)
                    k += 1
        out_add, out_max = c["want"]["add", "mul"][0], c["want"]["max", "mul"][0]
        assert np.array_equal(got[k], out_add + c["add"]) and np.array_equal(got[k + 1], np.maximum(out_max, c["add"]))
        assert np.array_equal(got[k + 2], out_add + c["dense"])
        assert np.array_equal(got[k + 3], c["base"] + c["want"]["add", "mul"][1])
        np.testing.assert_allclose(got[k + 4], c["d_w"], rtol=1e-4, atol=1e-4)
    for a, b in zip(results["native"], results["torch"]):
        assert np.array_equal(a.view(np.int32), b.view(np.int32)), "the two plan builders' plans give different results"


@pytest.mark.parametrize("name", ["skewed_hub", "hub_split"])
def test_first_layer_and_masked_backward_entries(oracle, monkeypatch, name):
    """The entries that visit part of the graph: ``rspmm_frontier``, ``rspmm_backward`` under destination bitmaps
    (``candidate_rows``) and under the boundary nodes, ``rspmm_drelation_boundary`` and ``rspmm_backward_boundary_rows``, on a
    plan with split rows, F = 192 and 64.  References: the oracle on the dense operands the promises describe -- bit for bit
    (tests/test_rspmm_gpu.py, tests/test_frontier_sampler_gpu.py) -- and for the boundary rows, whose kernel sums a node's
    out-edges in its own order, the oracle's ``d_input`` rows at 2e-5 (tests/test_model_gpu.py)."""
    from ultra_torchdrug_amd import RelCSR, functional as UF
    monkeypatch.setenv("ULTRA_BINDING", "ctypes")
    c = _plan_case(name, oracle)
    n, r, F, g, csr_o, piece = c["n"], c["r"], c["F"], c["g"], c["csr_o"], c["piece"]
    Q = F // 64
    rng = np.random.default_rng(Q)
    t_index = rng.integers(0, n, (Q, 9))
    t_index[:, 0] = 5
    member = np.zeros((n, Q), dtype=bool)
    member[t_index, np.arange(Q)[:, None]] = True
    sparse_grad = (c["grad"].reshape(n, Q, 64) * member[:, :, None]).reshape(n, F)
    dense = c["dense"]                                                                 # zero outside row b_node[q] of block q
    out_s = oracle.rspmm_forward(csr_o, c["relation"], c["x"], "add", "mul", piece=piece)
    want_drel_s, want_dx_s = oracle.rspmm_backward(csr_o, c["relation"], c["x"], out_s, sparse_grad, "add", "mul", piece=piece)
    out_b = oracle.rspmm_forward(csr_o, c["relation"], dense, "add", "mul", piece=piece)
    want_drel_b, _ = oracle.rspmm_backward(csr_o, c["relation"], dense, out_b, c["grad"], "add", "mul", piece=piece)
    want_dx = c["want"]["add", "mul"][1]
    launches = Launches()

    def call(dst, src, rel, relation, x, grad, sparse_grad, dense, base, b_node, b_value, t_index):
        csr = RelCSR(dst, src, rel, None, n, n, r, **c["opts"])
        assert csr.fwd.long_rows.shape[0] > 0
        bits = UF.candidate_rows(t_index, n)
        frontier = launches.call(UF.rspmm_frontier, csr, relation, (b_node, b_value))
        masked = []
        for knob in (0, 2):                       # as the plan decides, and with the gathered matrix kept out of LDS (see below)
            with _knob(knob):
                masked += launches.call(UF.rspmm_backward, csr, relation, x, None, sparse_grad, "add", "mul", active_dst=bits)
                masked.append(launches.call(UF.rspmm_backward, csr, relation, dense, None, grad, "add", "mul", need_input=False,
                                            active_src=b_node)[1])
        drel_bb = launches.call(UF.rspmm_drelation_boundary, csr, dense, grad, b_node)
        rows = launches.call(UF.rspmm_backward_boundary_rows, csr, relation, grad, b_node, base.clone(), "mul")
        return [bits, frontier, drel_bb, rows] + masked

    args = [_t(g[k]) for k in ("dst", "src", "rel")] + [_t(a) for a in (c["relation"], c["x"], c["grad"], sparse_grad, dense, c["base"],
                                                                         c["b_node"], c["b_value"], t_index)]
    bits, frontier, drel_bb, rows, *masked = (
        t.cpu().numpy() for t in run_guarded(call, *args, modules=("functional", "relcsr"), widest_row=4 * F, what=name))
    # the kernels that ran.  The masked backward runs its plans through quad_kernel (packed words, node ids inside them: the rule
    # of _forward_family).  plan_path.h gives d_relation its ACT form -- 2 under destination bitmaps, 3 under the boundary nodes
    # -- only where the gathered matrix is NOT staged in LDS (var 0); a matrix that fits beside the relation tile (156 KiB: 256 B
    # per gathered row and, for d_input, per relation) is staged and the masks are not consulted (x_lds 1, act 0).  So every call
    # runs twice: as the plan decides, and under knob bit 1, which keeps the matrix out of LDS and so reaches the ACT kernels on
    # these small graphs too.  d_input under bitmaps keeps ACT 0 (tests/test_rspmm_gpu.py).  The frontier, boundary-relation
    # and boundary-rows entries are launches of their own outside the plan launchers (csrc/frontier.inc,
    # csrc/first_layer_train.inc) and keep no record: none may appear.
    room = 156 * 1024
    staged_dx, staged_drel = (n + r) * 256 <= room, n * 256 <= room
    assert staged_drel == (name == "skewed_hub")                       # (both forms are reached as the plan's own decision)
    wants = [[]]
    for knob in (0, 2):
        x_dx, x_drel = int(staged_dx and not knob), int(staged_drel and not knob)
        q = lambda kind, x_lds, act: dict(family=QUAD, kind=kind, x_lds=x_lds, act=act, dead=0, unit_w=1)
        wants += [[q(DX, x_dx, 0), q(DREL, x_drel, 0 if x_drel else 2)], [q(DREL, x_drel, 0 if x_drel else 3)]]
    launches.check(*wants, [], [])
    words = bits.astype(np.int64) & 0xffffffff
    unpacked = ((words[:, :, None] >> np.arange(32)) & 1).astype(bool).reshape(Q, -1)[:, :n]
    assert np.array_equal(unpacked, member.T)
    assert np.array_equal(frontier, out_b + dense)
    for dx_s, drel_s, drel_b in (masked[:3], masked[3:]):
        assert np.array_equal(dx_s, want_dx_s) and np.array_equal(drel_s, want_drel_s) and np.array_equal(drel_b, want_drel_b)
    assert np.array_equal(drel_bb, want_drel_b)
    picked = (c["b_node"].astype(np.int64), np.arange(Q))
    got_rows, base3 = rows.reshape(n, Q, 64), c["base"].reshape(n, Q, 64)
    np.testing.assert_allclose(got_rows[picked] - base3[picked], want_dx.reshape(n, Q, 64)[picked], rtol=2e-5, atol=2e-5)
    others = got_rows.copy()
    others[picked] = base3[picked]
    assert np.array_equal(others.view(np.int32), base3.view(np.int32)), "a row other than (b_node[q], q) changed"


@pytest.mark.parametrize("weights", [False, True], ids=["unit_weights", "weights"])
def test_rotate_trio(monkeypatch, weights):
    """``rotate_rspmm_forward`` / ``_backward`` / ``_backward_weight`` (sum aggregation, rows split into pieces of 64, F = 192 with
    blocks of 64) against the fp64 restatement of tests/rotate_restatement.py, entry by entry within 1e-6 of the sum of the
    |terms| of that entry (the bar of tests/test_rotate_gpu.py)."""
    import rotate_restatement as RR
    from ultra_torchdrug_amd import RelCSR, functional as UF
    monkeypatch.setenv("ULTRA_BINDING", "ctypes")
    n, r, F, block = 300, 9, 192, 64
    g = random_graph(seed=7, n_node=n, n_edge=5000, n_rel=r, weights=weights, hub_row=3, hub_edges=300, hub_src=5, hub_rel=1)
    gen = torch.Generator().manual_seed(5)
    relation, x, grad = torch.randn(r, F, generator=gen), torch.randn(n, F, generator=gen), torch.randn(n, F, generator=gen)
    dst, src, rel, w = RR.coalesce(g["dst"], g["src"], g["rel"], g["w"], n, r)
    rel64, x64 = relation.double().requires_grad_(), x.double().requires_grad_()
    want = RR.rotate_rspmm(dst, src, rel, w, rel64, x64, n, block, "add")
    want.backward(grad.double())
    scale = RR.abs_scale(dst, src, rel, w, relation, x, n, block)
    bound_x, bound_rel = RR.grad_abs_scale(dst, src, rel, w, relation, x, grad, block, None)
    ones = np.ones(len(dst))
    unit = RR.messages(src, rel, ones, relation, x, block)                             # (E, F) fp64: the messages without weights
    g_rows = grad.double()[torch.as_tensor(dst)]
    want_w = (unit * g_rows).sum(1)
    bound_w = (RR._edge_abs_scale(src, rel, ones, relation, x, block) * g_rows.abs()).sum(1)
    launches, unit_w = Launches(), []

    def call(dst_t, src_t, rel_t, w_t, relation, x, grad):
        csr = RelCSR(dst_t, src_t, rel_t, w_t, n, n, r, piece_len=64)
        assert csr.fwd.n_pieces > 0 and csr.by_src.n_pieces > 0 and csr.by_rel.n_pieces > 0 and csr.n_edges == len(dst)
        unit_w.append(int(csr.fwd.weight is None))
        out = launches.call(UF.rotate_rspmm_forward, csr, relation, x, "add", block)
        d_x, d_rel = launches.call(UF.rotate_rspmm_backward, csr, relation, x, None, grad, "add", block)
        d_w = launches.call(UF.rotate_rspmm_backward_weight, csr, relation, x, None, grad, "add", block)
        return [out, d_x, d_rel, d_w]

    dev = _dev()
    got = run_guarded(call, _t(g["dst"]), _t(g["src"]), _t(g["rel"]), None if g["w"] is None else _t(g["w"]), relation.to(dev), x.to(dev),
                      grad.to(dev), modules=("functional", "relcsr"), widest_row=4 * F, what="rotate")
    # the ROTATE family's records (csrc/rotate.inc: rotate_segment_kernel per plan; the weight gradient is a kernel of its own
    # outside that launcher and keeps no record)
    rot = lambda kind: dict(family=ROTATE, kind=kind, sum=0, unit_w=unit_w[-1])
    assert unit_w == [unit_w[0]] * 2 and (unit_w[0] == 0 or not weights)
    launches.check([rot(FWD)], [rot(DX), rot(DREL)], [])
    for what, a, truth, bound in zip(("forward", "d_input", "d_relation", "d_weight"), got,
                                     (want.detach(), x64.grad, rel64.grad, want_w), (scale, bound_x, bound_rel, bound_w)):
        err = (a.cpu().double() - truth).abs()
        assert bound.max() > 0
        assert (err <= 1e-6 * bound + 1e-30).all(), "%s: max err / yardstick %.3g" % (what, (err / (bound + 1e-24)).max().item())


# ==================================================================================================== integer and selection family
RANK_SLICE = 32768          # kRankSlice of csrc/sampler.inc: candidates per workgroup of the sliced kernels


def _ranking_case(n_cand, seed):
    """Scores with exact ties inside a WIDER matrix whose padding columns are NaN, sorted completion keys, and the dense mask
    the reference side works from (True = unfiltered): ``(wide, pred, target, anchor, rel, keys, mask)`` on the host."""
    from sampled_graphs import tied_scores
    rows, n_rel, pad = 4, 3, 5
    gen = torch.Generator().manual_seed(seed)
    pred = tied_scores(rows, n_cand, seed=seed)[:, 0].contiguous()
    wide = torch.full((rows, n_cand + pad), float("nan"))
    wide[:, :n_cand] = pred
    anchor = torch.randint(0, n_cand, (rows,), generator=gen)
    rel = torch.arange(rows) % n_rel                                       # (the first three queries differ in their relation)
    target = torch.randint(0, n_cand, (rows,), generator=gen)
    mask = torch.ones(rows, n_cand, dtype=torch.bool)
    for q, count in enumerate((0, 40, min(n_cand, 700), 1)):               # no completion, some, many (first and last entity), one
        mask[q, torch.randperm(n_cand, generator=gen)[:count]] = False
    if n_cand > 1:
        mask[2, 0] = mask[2, n_cand - 1] = False
    anchor[3], rel[3] = anchor[1], rel[1]                                  # two queries share their completions
    mask[3] = mask[1]
    q_idx, other = (~mask[:3]).nonzero(as_tuple=True)
    noise = torch.randint(0, n_cand, (50, 3), generator=gen)               # completions of queries nobody asks
    keys = torch.cat([(anchor[q_idx] * n_rel + rel[q_idx]) * n_cand + other,
                      ((noise[:, 0] + n_cand) * n_rel + noise[:, 1] % n_rel) * n_cand + noise[:, 2]])
    clash = (anchor[:3].unsqueeze(1) == anchor[:3].unsqueeze(0)) & (rel[:3].unsqueeze(1) == rel[:3].unsqueeze(0))
    assert int(clash.sum()) == 3, "the seeded queries must be distinct"
    return wide, pred, target, anchor, rel, torch.unique(keys), mask


@pytest.mark.parametrize("n_cand", [1, 257, 2 * RANK_SLICE - 1, 2 * RANK_SLICE, 2 * RANK_SLICE + 1])
def test_rank_count_and_sampling_kernels(n_cand):
    """``filtered_rank`` (filter lists), ``filtered_rank_keys``, ``filter_counts``, ``strict_negatives`` and ``sampled_rank_keys``
    one below, at and one above the row length from which the rank comes from the sliced kernels (2 x 32768), on scores that
    are a view of a wider matrix with NaN padding columns.  References: the oracle's rank over the dense mask, the mask's row
    sums, ``task.py:102-118`` restated over the mask (oracle_ops) and the dense sampled protocol -- integers, exactly."""
    from oracle import oracle as O
    from ultra_torchdrug_amd import functional as UF
    from ultra_torchdrug_amd.task import dense_sampled_ranks
    wide, pred, target, anchor, rel, keys, mask = _ranking_case(n_cand, seed=n_cand % 1000)
    rows, n_rel = pred.shape[0], 3
    gen = torch.Generator().manual_seed(n_cand)
    rand = torch.rand(rows, 7, generator=gen)
    rand[:, 0], rand[:, 1] = 0.0, float(np.nextafter(np.float32(1), np.float32(0)))
    counts = (~mask).sum(1)
    filt_ptr = torch.cat([torch.zeros(1, dtype=torch.long), counts.cumsum(0)]).to(torch.int32)
    filt_node = (~mask).nonzero(as_tuple=True)[1].to(torch.int32)
    want_rank = torch.from_numpy(O.filtered_rank(pred.numpy(), mask.numpy(), target.numpy()))
    want_free = torch.from_numpy(O.filtered_rank(pred.numpy(), np.ones_like(mask.numpy()), target.numpy()))
    has_free = mask.any(1)
    want_neg = OracleFunctional.strict_negatives(keys, anchor[has_free], rel[has_free], n_rel, n_cand, rand[has_free])
    want_sampled = dense_sampled_ranks(pred, target, mask, rand)

    def call(wide, target, anchor, rel, keys, rand, filt_ptr, filt_node):
        view = wide[:, :n_cand]
        assert view.stride(0) == n_cand + 5
        return [UF.filtered_rank(view, target, filt_ptr, filt_node), UF.filtered_rank(view, target),
                UF.filtered_rank_keys(view, target, keys, anchor, rel, n_rel, n_node=n_cand),
                UF.filtered_rank_keys(view, target, None, anchor, rel, n_rel),
                UF.filter_counts(keys, anchor, rel, n_rel, n_cand), UF.filter_counts(None, anchor, rel, n_rel, n_cand),
                UF.strict_negatives(keys, anchor[has_free.to(anchor.device)], rel[has_free.to(anchor.device)], n_rel, n_cand,
                                    rand[has_free.to(anchor.device)].contiguous()),
                UF.sampled_rank_keys(view, target, keys, anchor, rel, n_rel, rand, n_node=n_cand, return_samples=True)]

    got = run_guarded(call, *(t.to(_dev()) for t in (wide, target, anchor, rel, keys, rand, filt_ptr, filt_node)), what="ranking")
    lists, free, by_keys, free_keys, n_free, n_all, negatives, sampled = got
    assert torch.equal(lists.cpu(), want_rank) and torch.equal(by_keys.cpu(), want_rank)
    assert torch.equal(free.cpu(), want_free) and torch.equal(free_keys.cpu(), want_free)
    assert torch.equal(n_free.cpu(), mask.sum(1)) and n_all.tolist() == [n_cand] * rows
    assert torch.equal(negatives.cpu(), want_neg)
    for g, w in zip(sampled, want_sampled):
        assert g.dtype == torch.int64 and torch.equal(g.cpu(), w)


@pytest.mark.parametrize("k", [1, 128])
@pytest.mark.parametrize("n_cand", [1, 257, RANK_SLICE - 1, RANK_SLICE, RANK_SLICE + 1])
def test_topk_keys(n_cand, k):
    """``ultra_topk_keys`` one below, at and one above the row length from which it runs per slice with a workspace (32768),
    k = 1 and 128, NaN / infinite / signed-zero scores, a strided view with NaN padding: the numpy restatement of
    tests/topk_definition.py, values bit for bit and indices exactly."""
    from topk_definition import same_bits, special_scores, topk_rows
    from ultra_torchdrug_amd import functional as UF
    wide, _, _, anchor, rel, keys, mask = _ranking_case(n_cand, seed=n_cand % 1000 + 1)
    pred = special_scores(4, n_cand, seed=n_cand)[:, 1].contiguous() if n_cand > 300 else wide[:, :n_cand].contiguous()
    wide[:, :n_cand] = pred
    known = [np.flatnonzero(~mask[q].numpy()) for q in range(4)]
    want_index, want_value = topk_rows(pred.numpy(), k, known)
    free_index, free_value = topk_rows(pred.numpy(), k, None)

    def call(wide, anchor, rel, keys):
        view = wide[:, :n_cand]
        return [UF.topk_keys(view, k, keys, anchor, rel, 3, n_node=n_cand), UF.topk_keys(view, k, None, anchor, rel, 3)]

    (value, index), (value_f, index_f) = run_guarded(call, *(t.to(_dev()) for t in (wide, anchor, rel, keys)), what="topk_keys")
    assert np.array_equal(index.cpu().numpy(), want_index) and same_bits(value.cpu().numpy(), want_value)
    assert np.array_equal(index_f.cpu().numpy(), free_index) and same_bits(value_f.cpu().numpy(), free_value)


@pytest.mark.parametrize("n_query,n_node,dim", [(1, 1, 1), (3, 257, 64), (5, 1025, 16)])
def test_set_boundary_with_count(n_query, n_node, dim):
    """``ultra_set_boundary_f32`` with its counts, memberships a strided view with NaN padding: tests/query_definition.py's numpy
    definition, bit for bit."""
    from query_definition import set_boundary_numpy, special_members
    from topk_definition import same_bits
    from ultra_torchdrug_amd import functional as UF
    if n_node > 64:
        member, query, floor = special_members(n_query, n_node, seed=n_node, dim=dim)
    else:
        member, query, floor = torch.tensor([[0.5]]), torch.tensor([[-2.0]]), torch.tensor([0.25])
    wide = torch.full((n_query, n_node + 3), float("nan"))
    wide[:, :n_node] = member
    want_b, want_c = set_boundary_numpy(member.numpy(), query.numpy(), floor.numpy())
    want_b0, want_c0 = set_boundary_numpy(member.numpy(), query.numpy(), None)

    def call(wide, query, floor):
        return [UF.set_boundary(wide[:, :n_node], query, floor, with_count=True), UF.set_boundary(wide[:, :n_node], query, None, with_count=True)]

    (b, c), (b0, c0) = run_guarded(call, wide.to(_dev()), query.to(_dev()), floor.to(_dev()), what="set_boundary")
    assert same_bits(b.cpu().numpy(), want_b) and np.array_equal(c.cpu().numpy(), want_c) and c.dtype == torch.int32
    assert same_bits(b0.cpu().numpy(), want_b0) and np.array_equal(c0.cpu().numpy(), want_c0)


@pytest.mark.parametrize("n_source", [1, 64, 65])
def test_hop_distance(monkeypatch, n_source):
    """The multi-source BFS (blocks of 64 sources: one block, a full block, a block and one) through the C ABI, matrix and
    ``targets`` form, polled and with a fixed level count, the graph and its CSR built inside the guard: the queue BFS of
    tests/hop_definition.py, exactly."""
    from hop_definition import graph_of, queue_form, random_edges
    from ultra_torchdrug_amd import functional as UF
    monkeypatch.setenv("ULTRA_BINDING", "ctypes")
    n = 1031
    node_in, node_out = random_edges(n, 3 * n, seed=n)
    rng = np.random.default_rng(n_source)
    sources = rng.integers(0, n, n_source)
    targets = rng.integers(0, n, (n_source, 7))
    want = queue_form(n, node_in, node_out, sources)
    want_pairs = want[targets, np.arange(n_source)[:, None]]

    def call(sources, targets):
        graph = graph_of(n, node_in, node_out).to(_dev())
        return [UF.hop_distance(graph.relcsr, sources), UF.hop_distance(graph.relcsr, sources, targets=targets),
                UF.hop_distance(graph.relcsr, sources, poll=False), UF.hop_distance(graph.relcsr, sources, targets=targets, poll=False)]

    got = run_guarded(call, _t(sources), _t(targets), modules=("functional", "relcsr", "graph"), what="hop_distance")
    for matrix, pairs in (got[:2], got[2:]):
        assert matrix.dtype == torch.int32 and np.array_equal(matrix.cpu().numpy(), want)
        assert np.array_equal(pairs.cpu().numpy(), want_pairs)


@pytest.mark.parametrize("K", [1, 10, 32])
@pytest.mark.parametrize("graph", ["lanes16", "lanes64_ragged"])
def test_beam_search_step_inputs(graph, K):
    """``beam_search_step`` has no route past the dispatcher: ``functional.beam_search_step`` always calls ``torch.ops.ultra_mi``,
    whose three outputs are ``at::empty`` in csrc/torch_ext.cpp.  The OUTPUTS are therefore unguarded here -- no bands, no poison.
    The input side is held: ``row_ptr`` / ``src`` between zero bands, ``edge_grad`` / ``input`` between NaN bands (a gradient or
    a beam read past its end would enter the top-K as NaN), the bands checked afterwards, and the result equal bit for bit to the
    unbanded call, to the operator's CPU twin and to the restatement of tests/explain_restatement.py (the three-way bar of
    tests/test_explain_gpu.py, on two of its graphs: 16 lanes per row, and 64 lanes with a ragged last block of 403 rows, a hub
    row, self loops and isolated nodes; finite gradients, so that any NaN is an over-read)."""
    from explain_restatement import beam_inputs, beam_step, coalesced_csr
    from ultra_torchdrug_amd import functional as UF
    if graph == "lanes16":
        row_ptr, src = coalesced_csr(1, 200, 3000, 5, isolated=20, self_loops=50, duplicates=300)
    else:
        row_ptr, src = coalesced_csr(9, 403, 40000, 11, isolated=15, hub_row=5, hub_edges=1500, self_loops=40, duplicates=200)
    n = row_ptr.numel() - 1
    assert (src.numel() // n >= 48) == (graph != "lanes16")
    beams, grad = beam_inputs(10 + K, n, K, src.numel(), empty=0.1)
    assert bool(torch.isfinite(grad).all()) and not bool(torch.isnan(beams).any())
    dev = _dev()
    for tail in (int(src[0]), int((row_ptr[1:] - row_ptr[:-1]).argmax()), n - 1):
        twin = UF.beam_search_step(row_ptr, src, grad, beams, tail)
        want = beam_step(row_ptr, src, grad, beams, tail)
        got = run_guarded(lambda rp, s, g, b: list(UF.beam_search_step(rp, s, g, b, tail)), row_ptr.to(dev), src.to(dev), grad.to(dev),
                          beams.to(dev), what="beam_search_step")
        for name, a, b, c in zip(("distance", "back_edge", "back_rank"), got, twin, want):
            assert a.is_cuda and a.dtype == b.dtype and not bool(torch.isnan(a).any()) if a.dtype == torch.float32 else a.is_cuda
            assert torch.equal(a.cpu(), b) and torch.equal(c, b), name


@pytest.mark.parametrize("n_node,n_query,per_row", [(1, 1, 1), (33, 3, 11), (5000, 6, 40)])
def test_candidate_tiles_and_rows(n_node, n_query, per_row):
    """``ultra_candidate_tiles`` against the distinct tiles in numpy (ascending, -1 padding) and ``ultra_node_bitmap``
    (``candidate_rows``) against the membership matrix, exactly."""
    from ultra_torchdrug_amd import functional as UF
    gen = torch.Generator().manual_seed(n_node)
    t_index = torch.randint(0, n_node, (n_query, per_row), generator=gen)
    if per_row > 9:
        t_index[-1, 5] = t_index[-1, 9]
    distinct = np.unique((t_index.numpy() * n_query + np.arange(n_query)[:, None]).reshape(-1) // 32)
    want_tiles = np.full(t_index.numel(), -1, dtype=np.int32)
    want_tiles[:len(distinct)] = distinct
    member = np.zeros((n_query, n_node), dtype=bool)
    member[np.arange(n_query)[:, None], t_index.numpy()] = True

    def call(t_index):
        n_for_tiles = max(n_node, (t_index.numel() * 8 * 32 + n_query - 1) // n_query)    # (past the density rule: the kernel runs)
        tiles = UF.candidate_tiles(t_index, n_query, n_for_tiles)
        assert tiles is not None
        return [tiles, UF.candidate_rows(t_index, n_node)]

    tiles, bits = run_guarded(call, t_index.to(_dev()), what="candidate tiles / rows")
    assert tiles.dtype == torch.int32 and np.array_equal(tiles.cpu().numpy(), want_tiles)
    words = bits.cpu().numpy().astype(np.int64) & 0xffffffff
    unpacked = ((words[:, :, None] >> np.arange(32)) & 1).astype(bool).reshape(n_query, -1)
    assert np.array_equal(unpacked[:, :n_node], member) and not unpacked[:, n_node:].any()


@pytest.mark.parametrize("n_node,n_rel,n_edge", [(1, 1, 1), (33, 5, 200), (700, 65, 3000)])
def test_relation_graph_blocks(n_node, n_rel, n_edge):
    """``ultra_relation_graph_marks`` against the reference's four incidence products (rel_model.py:99-143) as dense boolean
    matrix products in numpy, exactly."""
    from ultra_torchdrug_amd import functional as UF
    rng = np.random.default_rng(n_edge)
    e = np.stack([rng.integers(0, n_node, n_edge), rng.integers(0, n_node, n_edge), rng.integers(0, n_rel, n_edge)], axis=1)
    heads, tails = np.zeros((n_node, n_rel), dtype=np.int64), np.zeros((n_node, n_rel), dtype=np.int64)
    heads[e[:, 0], e[:, 2]] = 1
    tails[e[:, 1], e[:, 2]] = 1
    want = np.stack([heads.T @ heads, tails.T @ tails, heads.T @ tails, tails.T @ heads]) > 0
    got = run_guarded(lambda e: UF.relation_graph_blocks(e, n_node, n_rel), _t(e.astype(np.int64)), what="relation_graph_blocks")
    assert got.dtype == torch.bool and np.array_equal(got.cpu().numpy(), want)


@pytest.mark.parametrize("n_rel,n_query,n_layers", [(1, 1, 1), (11, 3, 2), (155, 5, 8)])
def test_relation_stack_inputs_and_prepare_queries(n_rel, n_query, n_layers):
    """Two copy kernels against the torch expressions their docstrings name (``stack / expand / reshape``, ``ones``, ``cat``,
    an index), bit for bit; ``rel_rep`` goes in as the transposed view the relation stack returns."""
    from ultra_torchdrug_amd import functional as UF
    gen = torch.Generator().manual_seed(n_rel)
    weights = [torch.randn(n_rel, 64, generator=gen) for _ in range(n_layers)]
    h_index = torch.randint(0, n_rel, (n_query,), generator=gen)
    want_tables = torch.stack(weights).unsqueeze(2).expand(-1, -1, n_query, -1).reshape(n_layers, n_rel, n_query * 64)
    n_base = (n_rel + 1) // 2
    batch = torch.stack([torch.randint(0, 50, (n_query,), generator=gen), torch.randint(0, 50, (n_query,), generator=gen),
                         torch.randint(0, n_base, (n_query,), generator=gen)], dim=1)
    rel_rep = torch.randn(2 * n_base, n_query, 64, generator=gen)                    # (R, B, 64): read as its (B, R, 64) transpose
    want_anchor = torch.cat([batch[:, 0], batch[:, 1]])
    want_rel = torch.cat([batch[:, 2], batch[:, 2] + n_base])
    want_query = torch.cat([rel_rep.transpose(0, 1)] * 2)[torch.arange(2 * n_query), want_rel]

    def call(h_index, batch, rel_rep, *weights):
        view = rel_rep.transpose(0, 1)
        assert not view.is_contiguous() or n_query == 1 or n_base * 2 == 1
        return [UF.relation_stack_inputs(list(weights), h_index), UF.prepare_queries(batch, view, n_base)]

    dev = _dev()
    (tables, ones, node32), (anchor, anchor32, relation, query) = run_guarded(
        call, h_index.to(dev), batch.to(dev), rel_rep.to(dev), *(w.to(dev) for w in weights), what="relation_stack_inputs / prepare_queries")
    assert torch.equal(tables.cpu(), want_tables) and torch.equal(ones.cpu(), torch.ones(n_query, 64))
    assert node32.dtype == torch.int32 and torch.equal(node32.cpu().long(), h_index)
    assert torch.equal(anchor.cpu(), want_anchor) and torch.equal(anchor32.cpu().long(), want_anchor) and anchor32.dtype == torch.int32
    assert torch.equal(relation.cpu(), want_rel) and torch.equal(query.cpu(), want_query)


def test_nonfinite_scan_stops_at_the_last_element(guarded):
    """Tensors of 1, chunk - 1, chunk + 1 (and exactly chunk) elements between NaN bands: a scan that reads one element past a
    tensor trips falsely, one that stops short misses the last element (second pass: a NaN planted there must trip)."""
    import ultra_torchdrug_amd as U
    from ultra_torchdrug_amd import functional as UF
    chunk = int(U.require_library().ultra_nonfinite_scan_chunk())
    dev = _dev()
    sizes = [1, chunk - 1, chunk, chunk + 1]
    guard = guarded                                  # (the fixture: the default guard around the test, checked when it returns)
    assert isinstance(guard, GM.Guard) and isinstance(UF.torch, GM.TorchProxy)
    tensors = [guard.banded(torch.full((n,), 1.5, device=dev)) for n in sizes]
    for t, rec in zip(tensors, guard.records):
        assert bool(torch.isnan(rec.buffer[guard.band + rec.nbytes:].view(torch.float32)[0]))      # (the very next element is NaN)
    record = UF.nonfinite_record(dev)
    UF.nonfinite_scan(tensors, record, first_index=3)
    UF.nonfinite_scan([t[1:] for t in tensors[1:]], record)                      # views that start at any element
    assert record.tolist() == [0, -1, -1, UF.GUARD_CLEAN], "the scan read past the end of a tensor"
    for k, t in enumerate(tensors):
        record = UF.nonfinite_record(dev)
        t[-1] = float("inf")
        UF.nonfinite_scan(tensors, record, first_index=3)
        assert record.tolist() == [0, -1, -1, 3 + k], "the scan missed the last element of tensor %d" % k
        t[-1] = 1.5


# ==================================================================================================== per-step removal
@pytest.mark.parametrize("route", ["marks", "weights"])
def test_per_step_removal_built_inside_the_guard(oracle, monkeypatch, route):
    """``RelCSR.with_removed_edges`` (``ultra_edge_removal_marks`` / ``_weights``) and ``with_removed_pairs``
    (``ultra_pair_removal``) on a unit-weight graph with inverse edges, the plans and the ``E + PACK_SLACK`` weight and word
    arrays built inside the guard; a forward and a backward over the resulting plans against the oracle on the same graph with
    weight 0 at the removed edges, bit for bit (the weighted kernels' bar, tests/test_rspmm_gpu.py)."""
    from ultra_torchdrug_amd import RelCSR, functional as UF, relcsr
    monkeypatch.setenv("ULTRA_BINDING", "ctypes")
    monkeypatch.setattr(relcsr, "DEAD_EDGE_WORDS", route == "marks")
    n, r, F = 300, 6, 128
    g = random_graph(seed=3, n_node=n, n_edge=2500, n_rel=r)
    base = np.unique(np.stack([g["dst"], g["src"], g["rel"]]), axis=1)
    base = base[:, base[2] < r // 2]
    both = np.unique(np.concatenate([base, np.stack([base[1], base[0], base[2] + r // 2])], axis=1), axis=1)
    dst, src, rel = both
    rng = np.random.default_rng(4)
    pick = rng.choice(np.flatnonzero(rel < r // 2), 30, replace=False)
    h = np.concatenate([src[pick], rng.integers(0, n, 20)])                      # real edges and patterns that are none
    t = np.concatenate([dst[pick], rng.integers(0, n, 20)])
    rr = np.concatenate([rel[pick], rng.integers(0, r // 2, 20)])
    key = lambda a, b, c: (a * n + b) * r + c
    gone = np.concatenate([key(h, t, rr), key(t, h, rr + r // 2)])
    keep_edges = (~np.isin(key(src, dst, rel), gone)).astype(np.float32)
    keep_pairs = (~np.isin(src * n + dst, np.concatenate([h * n + t, t * n + h]))).astype(np.float32)
    assert 0 < (keep_edges == 0).sum() <= 60 and (keep_pairs == 0).sum() >= (keep_edges == 0).sum()
    f32 = lambda *shape: rng.standard_normal(shape).astype(np.float32)
    relation, x, grad = f32(r, F), f32(n, F), f32(n, F)
    want = []
    for keep in (keep_edges, keep_pairs):
        csr_o = oracle.coalesce_csr(dst, src, rel, keep, n, n, r)
        out = oracle.rspmm_forward(csr_o, relation, x, "add", "mul", piece=128)
        d_rel, d_x = oracle.rspmm_backward(csr_o, relation, x, out, grad, "add", "mul", piece=128)
        want += [out, d_x, d_rel]
    launches = Launches()

    def call(dst, src, rel, h, t, rr, relation, x, grad):
        csr = RelCSR(dst, src, rel, None, n, n, r, piece_len=128)
        assert csr.unit_weight
        outs = []
        for cut in (csr.with_removed_edges(h, t, rr, r // 2), csr.with_removed_pairs(h, t)):
            assert (cut.fwd.packed_dead is not None) == (route == "marks")
            for knob in (0, 2):                   # as the plan decides, and with the gathered matrix kept out of LDS (see below)
                with _knob(knob):
                    out = launches.call(UF.rspmm_forward, cut, relation, x, "add", "mul")
                    d_x, d_rel = launches.call(UF.rspmm_backward, cut, relation, x, None, grad, "add", "mul")
                outs += [out, d_x, d_rel]
            outs.append(cut.weight.clone())
        return outs

    got = run_guarded(call, *(_t(a) for a in (dst, src, rel, h, t, rr, relation, x, grad)), modules=("functional", "relcsr"),
                      widest_row=4 * F, what="removal %s" % route)
    # the kernels that ran: quad_kernel for all three plans.  plan_path.h takes the marked words (the unit-weight DEAD form) only
    # where the gathered matrix is not staged in LDS (var 0); these 300 rows fit, so the plan's own decision is the staged,
    # weighted form on either route, and knob bit 1 (matrix out of LDS) reaches the DEAD kernels on the marks route
    # (tests/test_rspmm_gpu.py's removal test states the same fields on a graph too big to stage).
    assert (n + r) * 256 <= 156 * 1024
    dead = int(route == "marks")
    staged = lambda kind: dict(family=QUAD, kind=kind, x_lds=1, dead=0, unit_w=0, act=0)
    plain = lambda kind: dict(family=QUAD, kind=kind, x_lds=0, dead=dead, unit_w=dead, act=0)
    launches.check(*([[staged(FWD)], [staged(DX), staged(DREL)], [plain(FWD)], [plain(DX), plain(DREL)]] * 2))
    got = [a.cpu().numpy() for a in got]
    order = np.lexsort((rel, src, dst))                                          # the coalesced order of the plans: (dst, src, rel)
    for k, keep in enumerate((keep_edges, keep_pairs)):
        assert np.array_equal(got[7 * k + 6], keep[order]), "the removal's weights"
        for what, a, b in zip(("forward", "d_input", "d_relation") * 2, got[7 * k:7 * k + 6], want[3 * k:3 * k + 3] * 2):
            assert np.array_equal(a, b), (k, what)


# ==================================================================================================== one whole step
def test_one_training_step_and_one_predict_under_the_guard():
    """Task, plans, negatives, forward, loss, backward and an eager ``predict`` with EVERY product module allocating through the
    guard: loss, gradients and scores are finite and EQUAL the unguarded run's (same kernels on the same data: the bar
    ``test_graphed_train_step_equals_eager_train_step`` of tests/test_model_gpu.py sets between two ways of running a step)."""
    import test_model_gpu as TM
    dev = _dev()

    def run():
        task, triples = TM._build((5000, 20000, 7))
        task.num_negative = 32
        task.to(dev).train()
        batch = torch.from_numpy(triples[:16]).to(dev)
        torch.manual_seed(3)
        loss, _ = task(batch)
        loss.backward()
        grads = {k: p.grad.detach().clone() for k, p in task.named_parameters() if p.grad is not None}
        task.eval()
        with torch.no_grad():
            scores = task.predict(batch[:8])
        return loss.detach(), grads, scores

    want_loss, want, want_scores = run()
    torch.cuda.synchronize()
    with guarded(*GM.ALL_MODULES, widest_row=32 * 64 * 4) as guard:
        loss, got, scores = run()
        guard.check()
        assert len(guard.records) > 100
    assert bool(torch.isfinite(loss)) and torch.equal(loss, want_loss)
    assert got.keys() == want.keys() and len(got) > 20
    for k in want:
        assert bool(torch.isfinite(got[k]).all()), k
        assert torch.equal(got[k], want[k]), "%s: max |diff| %.3g" % (k, (got[k] - want[k]).abs().max().item())
    assert bool(torch.isfinite(scores).all()) and torch.equal(scores, want_scores)
    assert_no_poison([loss, scores] + list(got.values()), "whole step")


# ==================================================================================================== fused layers
def _oracle_layer(oracle, g, n, r, piece, relation, x3, boundary, params, relu, shortcut, weights=None):
    """One layer on the host from the oracle's pieces: rspmm (``piece``: 0 = every row sequentially), + the dense boundary,
    the epilogue's C restatement.  ``x3`` ``(N, Q, 64)``; returns ``(update, out)`` as ``(N, Q, 64)`` numpy arrays."""
    n_query = x3.shape[1]
    csr_o = oracle.coalesce_csr(g["dst"], g["src"], g["rel"], weights, n, n, r)
    update = oracle.rspmm_forward(csr_o, relation, x3.reshape(n, -1), "add", "mul", piece=piece)
    if boundary is not None:
        update = update + OracleFunctional._dense_boundary((torch.from_numpy(boundary[0]), torch.from_numpy(boundary[1])), n).numpy()
    w, b, gamma, beta = params
    out = oracle.combine_forward(x3.reshape(-1, 64), update.reshape(-1, 64), w, b, gamma, beta, 1e-5, relu, shortcut)
    return update.reshape(n, n_query, 64), out.reshape(n, n_query, 64)


def _layer_operands(seed, n, r, n_query, layer_norm=True):
    rng = np.random.default_rng(seed)
    f32 = lambda *shape, s=1.0: (s * rng.standard_normal(shape)).astype(np.float32)
    x = f32(n, n_query, 64)
    relation = f32(r, 64 * n_query)
    b_node = rng.integers(0, n, n_query).astype(np.int32)
    b_node[0] = min(7, n - 1)
    b_value = f32(n_query, 64)
    params = (f32(64, 128, s=0.1), f32(64, s=0.1), (1 + f32(64, s=0.1)) if layer_norm else None, f32(64, s=0.1) if layer_norm else None)
    head = (f32(n_query, 64), f32(128, 128, s=0.1), f32(128, s=0.1), f32(1, 128, s=0.1), f32(1))
    return x, relation, b_node, b_value, params, head


@pytest.mark.parametrize("case", ["g16_three_nodes", "g16_three_queries", "g32_rel_part"])
def test_layer_forward_and_layer_score_forward(oracle, case):
    """``ultra_layer_forward_f32`` and ``ultra_layer_score_forward_f32`` on graphs of tests/test_layer_fused_gpu.py (3 rows: less
    than one batch of four iterations; lane groups of 16 and of 32 with part of the relation rows in LDS; an empty row, rows of
    several windows), the plan built inside the guard.  The entries are documented as the bits of rspmm + epilogue (+ score
    head), each of which is pinned to the oracle: here the oracle's chain directly, bit for bit (row-per-group plans never
    split a row: ``piece = 0``)."""
    import test_layer_fused_gpu as LF
    from oracle import oracle as O
    from ultra_torchdrug_amd import RelCSR, functional as UF
    n, e, r, n_query, knob, _ = LF.CASES[case]
    g = random_graph(seed=len(case), n_node=n, n_edge=e, n_rel=r)
    if n > 60:
        g["dst"][:40] = 7
        g["dst"][40:60] = n - 1
    keep = g["dst"] != (11 if n > 60 else 1)
    g = {k: (None if v is None else v[keep]) for k, v in g.items()}
    x, relation, b_node, b_value, params, head = _layer_operands(len(case), n, r, n_query)
    _, want = _oracle_layer(oracle, g, n, r, 0, relation, x, (b_node, b_value), params, True, True)
    want_score = O.score_head_forward(want, *head)

    def call(dst, src, rel, relation, x, b_node, b_value, w, b, gamma, beta, *head):
        csr = RelCSR(dst, src, rel, None, n, n, r, wide_ids=True, piece_len=512)
        assert csr.fwd.row_ptr is not None and csr.fwd.n_pieces == 0
        with _knob(knob):
            out = UF.layer_forward(csr, relation, x, (b_node, b_value), w, b, gamma, beta, 1e-5, True, True)
            score = UF.layer_score_forward(csr, relation, x, (b_node, b_value), w, b, gamma, beta, 1e-5, True, True, *head)
        assert out is not None and score is not None, "the fused entries declined a row-per-group plan"
        return [out, score]

    args = [_t(g[k]) for k in ("dst", "src", "rel")] + [_t(a) for a in (relation, x, b_node, b_value, *params, *head)]
    out, score = run_guarded(call, *args, modules=("functional", "relcsr"), widest_row=256 * n_query, what=case)
    assert np.array_equal(out.cpu().numpy(), want), "layer_forward differs from the oracle's chain"
    assert np.array_equal(score.cpu().numpy(), want_score), "layer_score_forward differs from the oracle's chain"


@pytest.mark.parametrize("layer_norm,relu,shortcut", [(True, True, True), (False, True, False)])
def test_sparse_first_layer_forward_and_its_training_form(oracle, monkeypatch, layer_norm, relu, shortcut):
    """``ultra_first_layer_sparse_f32`` and ``ultra_first_layer_sparse_train_f32`` (row lists sized for the worst head, list
    offsets, the constant row) on the 500-node graph of tests/test_frontier_sampler_gpu.py with an isolated, a repeated and a hub
    head: the oracle's rspmm over the dense boundary + epilogue, bit for bit.  The training form documents ``update`` as
    UNWRITTEN outside the listed rows: it is compared (and searched for poison) at the listed rows only, and the test asserts
    that its other rows DO still hold the poison -- nothing wrote them, and nothing may read them."""
    from ultra_torchdrug_amd import RelCSR, functional as UF
    monkeypatch.setattr(UF, "SPARSE_FIRST_LAYER_MIN_ROWS", 0)
    monkeypatch.setattr(UF, "SPARSE_FIRST_LAYER_TRAIN_MAX_FRACTION", 1.0)
    n, r, Q = 500, 9, 6
    g = random_graph(seed=1, n_node=n, n_edge=6000, n_rel=r, unique=True)
    _, relation, _, b_value, params, _ = _layer_operands(17, n, r, Q, layer_norm)
    deg_out = np.bincount(g["src"], minlength=n)
    b_node = np.array([int(deg_out.argmax()), int(np.flatnonzero(deg_out == 0)[0]) if (deg_out == 0).any() else 1, 0, n - 1, 5, 5], dtype=np.int32)
    dense = OracleFunctional._dense_boundary((torch.from_numpy(b_node), torch.from_numpy(b_value)), n).numpy().reshape(n, Q, 64)
    want_update, want = _oracle_layer(oracle, g, n, r, 128, relation, dense, (b_node, b_value), params, relu, shortcut)
    listed_rows = []

    def call(dst, src, rel, relation, b_node, b_value, w, b, *ln):
        gamma, beta = ln if ln else (None, None)
        csr = RelCSR(dst, src, rel, None, n, n, r, piece_len=128)
        out, row_list, count = UF.first_layer_forward(csr, relation, (b_node, b_value), w, b, gamma, beta, 1e-5, relu, shortcut, want_list=True)
        trained = UF.first_layer_train_forward(csr, relation, (b_node, b_value), w, b, gamma, beta, 1e-5, relu, shortcut)
        assert trained is not None, "the sparse training form declined a shape it should take"
        update, out_t, rows_t, count_t = trained
        rows = rows_t[:int(count_t)]
        rows = rows[rows >= 0].long()
        listed_rows.append(rows)
        listed = torch.sort(row_list[:int(count)][row_list[:int(count)] >= 0]).values
        return [out, out_t, update.view(-1, 64)[rows], torch.sort(rows).values, listed, update]

    args = [_t(g[k]) for k in ("dst", "src", "rel")] + [_t(a) for a in (relation, b_node, b_value, *[p for p in params if p is not None])]
    got = run_guarded(call, *args, modules=("functional", "relcsr"), widest_row=256 * Q, what="sparse first layer", defined=lambda res: res[:5])
    out, out_t, update_rows, rows, listed, update = got
    assert np.array_equal(out.cpu().numpy(), want) and np.array_equal(out_t.cpu().numpy(), want)
    touched = np.flatnonzero((want_update.reshape(-1, 64) != 0).any(1))
    assert set(touched.tolist()) <= set(rows.tolist()) and set(touched.tolist()) <= set(listed.tolist()) and len(rows) < n * Q
    assert np.array_equal(update_rows.cpu().numpy(), want_update.reshape(-1, 64)[listed_rows[-1].cpu().numpy()])
    unlisted = torch.ones(n * Q, dtype=torch.bool, device=update.device)
    unlisted[rows] = False
    left = update.view(-1, 64)[unlisted]
    assert bool((left.view(torch.int32) == GM._signed(GM.POISON_F32, 32)).all()), "a row outside the list was written"


@pytest.mark.parametrize("n,density,n_query", [(90, 1.0, 3), (70, 0.3, 1)])
def test_dense_layer_forward(oracle, n, density, n_query):
    """``ultra_dense_layer_forward_f32`` and the dense rspmm on relation graphs of tests/test_relgraph_dense_gpu.py (90 rows = 5
    tiles of 16 + 10, sources padded to 96), the plan AND its 0/1 matrix with the slack the kernels may read built inside the
    guard: the oracle's chain in the reference order (``piece = 0``), bit for bit."""
    import test_relgraph_dense_gpu as RD
    from ultra_torchdrug_amd import RelCSR, functional as UF
    g = RD._graph(21, n, density)
    x, relation, b_node, b_value, params, _ = _layer_operands(n, n, 4, n_query)
    want_update, want = _oracle_layer(oracle, g, n, 4, 0, relation, x, (b_node, b_value), params, True, True)
    launches = Launches()

    def call(dst, src, rel, relation, x, b_node, b_value, w, b, gamma, beta):
        csr = RelCSR(dst, src, rel, None, n, n, 4)
        assert csr.dense_form and csr.fwd.dense is not None
        update = launches.call(UF.rspmm_forward, csr, relation, x.flatten(1), "add", "mul", boundary=(b_node, b_value))
        out = launches.call(UF.dense_layer_forward, csr, relation, x, (b_node, b_value), w, b, gamma, beta, 1e-5, True, True)
        assert out is not None, "the dense layer declined a plan that carries its dense form"
        return [update, out]

    args = [_t(g[k]) for k in ("dst", "src", "rel")] + [_t(a) for a in (relation, x, b_node, b_value, *params)]
    update, out = run_guarded(call, *args, modules=("functional", "relcsr"), widest_row=256 * n_query, what="dense layer")
    # the rspmm ran in the plan's DENSE form (the record says so and for which call; relgraph_dense.hip picks its own kernels);
    # the one-launch layer is an entry of its own outside the plan launchers and keeps no record
    launches.check([dict(family=DENSE, kind=FWD)], [])
    assert np.array_equal(update.cpu().numpy(), want_update.reshape(n, -1)) and np.array_equal(out.cpu().numpy(), want)


def test_sparse_first_layer_in_training_with_its_epilogue_backward(monkeypatch):
    """``functional.sum_layer`` on the first layer: ``ultra_first_layer_sparse_train_f32`` forward, then
    ``ultra_first_layer_epilogue_backward_f32`` (the listed rows compacted into a poisoned workspace; every other row's share of
    ``d_bias`` / ``d_gamma`` / ``d_beta`` from ``ultra_column_sum_f32``'s per-block partials), ``rspmm_drelation_boundary`` and
    ``rspmm_backward_boundary_rows`` over a ``d_update`` that is written at the listed rows only.  Reference: fp64 autograd of
    the layer written with index_add (the reference's message + aggregate) at 2e-5 of each gradient's scale, the bar of
    tests/test_model_gpu.py's sparse-first-layer test."""
    from ultra_torchdrug_amd import RelCSR, functional as UF
    monkeypatch.setenv("ULTRA_BINDING", "ctypes")
    monkeypatch.setattr(UF, "SPARSE_FIRST_LAYER_MIN_ROWS", 0)
    monkeypatch.setattr(UF, "SPARSE_FIRST_LAYER_TRAIN_MAX_FRACTION", 1.0)
    taken = []
    real = UF.first_layer_train_forward
    monkeypatch.setattr(UF, "first_layer_train_forward", lambda *a, **k: taken.append(real(*a, **k)) or taken[-1])
    n, r, Q = 500, 9, 6
    g = random_graph(seed=1, n_node=n, n_edge=6000, n_rel=r, unique=True)
    _, relation, _, b_value, params, _ = _layer_operands(23, n, r, Q)
    deg_out = np.bincount(g["src"], minlength=n)
    b_node = np.array([int(deg_out.argmax()), 1, 0, n - 1, 5, 5], dtype=np.int64)
    gout = np.random.default_rng(2).standard_normal((n, Q, 64)).astype(np.float32)
    dst, src, rel = (torch.from_numpy(g[k]) for k in ("dst", "src", "rel"))
    leaves64 = [torch.from_numpy(a).double().requires_grad_() for a in (relation, b_value, *params)]
    rel64, bv64, w64, b64, g64, beta64 = leaves64
    dense64 = torch.zeros(n, Q, 64, dtype=torch.float64).index_put((torch.from_numpy(b_node), torch.arange(Q)), bv64, accumulate=True)
    flat = dense64.flatten(1)
    update64 = torch.zeros(n, Q * 64, dtype=torch.float64).index_add(0, dst, rel64[rel] * flat[src]) + flat
    pre = torch.nn.functional.layer_norm(torch.nn.functional.linear(torch.cat([dense64, update64.view(n, Q, 64)], dim=-1), w64, b64),
                                         (64,), g64, beta64, 1e-5)
    gout[(pre.detach().abs() < 1e-4).any(dim=-1).numpy()] = 0.0              # relu is not differentiable at 0 (tests/test_rspmm_gpu.py)
    want_out = torch.relu(pre) + dense64
    want_out.backward(torch.from_numpy(gout).double())

    def call(dst, src, rel, b_node, gout, relation, b_value, *params):
        csr = RelCSR(dst, src, rel, None, n, n, r, piece_len=128)
        with torch.enable_grad():
            leaves = [t.detach().requires_grad_() for t in (relation, b_value, *params)]
            rel_l, bv, w, b, gamma, beta = leaves
            dense = torch.zeros(n, Q, 64, device=bv.device).index_put((b_node, torch.arange(Q, device=bv.device)), bv, accumulate=True)
            out = UF.sum_layer(csr, rel_l, dense, dense, (b_node.to(torch.int32), bv), "mul", w, b, gamma, beta, 1e-5, True, True,
                               input_is_boundary=True)
            out.backward(gout)
        return [out.detach()] + [t.grad for t in leaves]

    args = [_t(g[k]) for k in ("dst", "src", "rel")] + [_t(a) for a in (b_node, gout, relation, b_value, *params)]
    got = run_guarded(call, *args, modules=("functional", "relcsr"), widest_row=256 * Q, what="sparse first layer, training")
    assert len(taken) == 2 and all(t is not None for t in taken), "the layer did not take the sparse training form"
    torch.testing.assert_close(got[0].cpu().double(), want_out.detach(), rtol=2e-5, atol=2e-5)
    for name, grad, leaf in zip(("d_relation", "d_boundary_value", "d_weight", "d_bias", "d_ln_weight", "d_ln_bias"), got[1:], leaves64):
        _close(grad, leaf.grad, name, floor=1e-9)

    # ---- the C entry itself (``_lib.launch``) with d_input / d_update carved by the test, around exactly N * Q rows: the compacted
    # rows are scattered back by row number (``dst[row_list[k]] = src[k]``, csrc/first_layer_train.inc), the one place of this
    # backward where a list slot becomes a store address.  Reference: fp64 autograd of the epilogue alone.  ``d_update`` is
    # documented as written at the LISTED rows only and ``d_input`` as zero elsewhere: both are compared at the listed rows, and
    # the rest is asserted to be what the contract says -- poison still in place, and +0.
    from ultra_torchdrug_amd import _lib
    d64, u64 = dense64.detach().requires_grad_(), update64.detach().view(n, Q, 64).requires_grad_()
    out2 = torch.relu(torch.nn.functional.layer_norm(torch.nn.functional.linear(torch.cat([d64, u64], dim=-1), w64, b64), (64,),
                                                     g64, beta64, 1e-5)) + d64
    want = torch.autograd.grad(out2, [d64, u64, w64, b64, g64, beta64], torch.from_numpy(gout).double())
    dev, rows = _dev(), n * Q
    dst_t, src_t, rel_t, node_t, gout_t, relation_t, value_t, *params_t = args
    with torch.no_grad(), guarded("functional", "relcsr", widest_row=256) as guard:
        csr = RelCSR(dst_t, src_t, rel_t, None, n, n, r, piece_len=128)
        update, _, row_list, list_count = real(csr, relation_t, (node_t.to(torch.int32), value_t), *params_t, 1e-5, True, True)
        dense = torch.zeros(n, Q, 64, device=dev).index_put((node_t, torch.arange(Q, device=dev)), value_t, accumulate=True)
        grads = [guard.carve((rows, 64), torch.float32, dev), guard.carve((rows, 64), torch.float32, dev),
                 guard.carve((64, 128), torch.float32, dev)] + [guard.carve((64,), torch.float32, dev) for _ in range(3)]
        ws = UF.torch.empty(int(_lib.load().ultra_first_layer_epilogue_backward_workspace(0, row_list.numel())) // 4, dtype=torch.float32,
                            device=dev)
        _lib.launch(dev, "ultra_first_layer_epilogue_backward_f32", guard.banded(dense), update, guard.banded(gout_t), row_list, list_count,
                    row_list.numel(), *UF._epilogue(*params_t, 1e-5, True, True), *grads, ws, ws.numel() * 4, rows)
        guard.check()
    listed = row_list[:int(list_count)]
    listed = listed[listed >= 0].long()
    unlisted = torch.ones(rows, dtype=torch.bool, device=dev)
    unlisted[listed] = False
    assert 0 < listed.numel() < rows
    d_input, d_update = grads[0], grads[1]
    _close(d_input[listed], want[0].view(rows, 64)[listed.cpu()], "d_input at the listed rows")
    _close(d_update[listed], want[1].view(rows, 64)[listed.cpu()], "d_update at the listed rows")
    assert not bool(d_input[unlisted].view(torch.int32).any()), "d_input outside the list is not +0"
    assert bool((d_update[unlisted].view(torch.int32) == GM._signed(GM.POISON_F32, 32)).all()), "d_update was written outside the list"
    assert_no_poison([d_input] + grads[2:], "ultra_first_layer_epilogue_backward_f32")
    for name, grad, w in zip(("d_weight", "d_bias", "d_ln_weight", "d_ln_bias"), grads[2:], want[2:]):
        _close(grad.view(w.shape), w, name)

"""The guard of tests/guarded_memory.py itself, on host tensors: layout, poison, detection on either side of a body, the proxy's
coverage of every allocation idiom the product has (by walking its syntax trees), and a host path of the product under it."""
import ast
import math
import os

import pytest
import torch

import guarded_memory as GM
from guarded_memory import guarded  # the context manager
from guarded_memory import guarded_fixture  # noqa: F401  (registers the pytest fixture ``guarded``: the parameter of the tests below)

PACKAGE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), GM.PRODUCT)


def _bits32(t):
    return t.contiguous().view(-1).view(torch.int32).to(torch.int64) & 0xFFFFFFFF


# ---------------------------------------------------------------------------------------------------- carve
@pytest.mark.parametrize("shape,dtype", [((5, 64), torch.float32), ((3, 7, 64), torch.float32), ((1,), torch.float64), ((), torch.float32),
                                         ((33,), torch.int32), ((9, 3), torch.int64), ((17,), torch.uint8), ((0, 4), torch.int64),
                                         ((4,), torch.bool)])
def test_carve_layout_and_poison(shape, dtype):
    guard = GM.Guard()
    body = guard.carve(shape, dtype, "cpu")
    rec = guard.records[-1]
    assert tuple(body.shape) == shape and body.dtype == dtype and body.is_contiguous()
    assert guard.band == 64 * 1024 and rec.buffer.dtype == torch.uint8
    assert rec.buffer.numel() == 2 * guard.band + GM._round_up(body.numel() * body.element_size(), 256)
    if body.numel():
        assert body.data_ptr() - rec.buffer.data_ptr() == guard.band and (body.data_ptr() - rec.buffer.data_ptr()) % 256 == 0
        if dtype == torch.float32:
            assert bool((_bits32(body) == GM.POISON_F32).all()) and bool(torch.isnan(body).all()) and GM.has_poison(body)
        elif dtype == torch.float64:
            assert bool((body.view(-1).view(torch.int64) == GM._signed(GM.POISON_F64, 64)).all()) and bool(torch.isnan(body).all())
        elif dtype == torch.bool:
            assert bool(body.all())
        elif dtype == torch.uint8:
            assert bool((body == 255).all())
        else:
            assert bool((body == -1).all())
    assert bool((rec.buffer[:guard.band] == GM.BAND_BYTE).all())
    assert bool((rec.buffer[guard.band + rec.nbytes:] == GM.BAND_BYTE).all())
    guard.check()


def test_band_defaults_to_32_of_the_widest_rows():
    assert GM.Guard().band == 64 * 1024
    assert GM.Guard(widest_row=256).band == 64 * 1024                  # 32 x 256 B = 8 KiB: the 64 KiB floor holds
    assert GM.Guard(widest_row=4 * 1000 + 4).band == GM._round_up(32 * 4004, 256)
    assert GM.Guard(band=1000).band == 1024


def test_value_allocations_keep_their_values():
    with guarded() as guard:
        proxy = GM.TorchProxy(guard)
        z = proxy.zeros(3, 5, dtype=torch.float32)
        zl = proxy.zeros_like(torch.ones(4, dtype=torch.int64))
        f = proxy.full((2, 3), -1, dtype=torch.long)
        fi = proxy.full((4,), 7)
        ff = proxy.full((), -float("inf"), dtype=torch.float64)
        o = proxy.ones(6, dtype=torch.bool)
        e = proxy.empty((2, 64))
        el = proxy.empty_like(torch.zeros(3, 2).t(), memory_format=torch.contiguous_format)
        assert torch.equal(z, torch.zeros(3, 5)) and torch.equal(zl, torch.zeros(4, dtype=torch.int64))
        assert torch.equal(f, torch.full((2, 3), -1, dtype=torch.long)) and torch.equal(fi, torch.full((4,), 7)) and fi.dtype == torch.int64
        assert ff.shape == () and ff.dtype == torch.float64 and float(ff) == -math.inf
        assert torch.equal(o, torch.ones(6, dtype=torch.bool))
        assert e.shape == (2, 64) and e.dtype == torch.float32 and GM.has_poison(e)
        assert el.shape == (2, 3) and el.is_contiguous() and GM.has_poison(el)
        assert not GM.has_poison(z) and len(guard.records) == 8
        with pytest.raises(TypeError):
            proxy.empty(3, pin_memory=True)                    # an option the proxy does not model is refused, not dropped
        assert proxy.float32 is torch.float32 and proxy.nn is torch.nn


# ---------------------------------------------------------------------------------------------------- detection
def test_check_names_a_write_before_and_after_a_body():
    guard = GM.Guard()
    first = guard.carve((4, 64), torch.float32, "cpu")
    victim = guard.carve((5, 3), torch.float32, "cpu"); line = _line()
    guard.check()
    rec = guard.records[1]
    raw = rec.buffer
    at = torch.tensor([guard.band - 4])
    saved = raw[at].clone()
    raw[at] = torch.tensor([0], dtype=torch.uint8)              # the last byte-quad of the element before the body
    with pytest.raises(GM.BandDamage) as err:
        guard.check()
    text = str(err.value)
    assert "leading band" in text and "(5, 3)" in text and "torch.float32" in text and "offset -4 " in text
    assert "%s:%d" % (__file__, line) in text and "(4, 64)" not in text
    raw[at] = saved
    guard.check()
    after = torch.tensor([guard.band + victim.numel() * 4])
    raw[after] = torch.tensor([0], dtype=torch.uint8)           # the first byte of the element after the body
    with pytest.raises(GM.BandDamage) as err:
        guard.check()
    text = str(err.value)
    assert "trailing band" in text and "(5, 3)" in text and "offset 60 " in text and "%s:%d" % (__file__, line) in text
    raw[after] = torch.tensor([GM.BAND_BYTE], dtype=torch.uint8)
    raw[torch.tensor([raw.numel() - 1])] = torch.tensor([1], dtype=torch.uint8)        # the very last byte of the trailing band
    with pytest.raises(GM.BandDamage, match="offset %d " % (raw.numel() - guard.band - 1)):
        guard.check()
    assert first is not None


def _line():
    import sys
    return sys._getframe(1).f_lineno


def test_banded_inputs_carry_nan_and_zero_bands_and_are_checked():
    guard = GM.Guard()
    x = torch.arange(10, dtype=torch.float32).view(5, 2)
    i = torch.arange(7, dtype=torch.int32)
    bx, bi = guard.banded(x), guard.banded(i)
    assert torch.equal(bx, x) and torch.equal(bi, i) and bx.is_contiguous()
    rx, ri = guard.records
    lead = rx.buffer[:guard.band].view(torch.float32)
    trail = rx.buffer[guard.band + 40:].view(torch.float32)
    assert bool(torch.isnan(lead).all()) and bool(torch.isnan(trail).all()) and not GM.has_poison(lead)
    assert bool((ri.buffer[:guard.band] == 0).all()) and bool((ri.buffer[guard.band + 28:] == 0).all())
    guard.check()
    ri.buffer[torch.tensor([guard.band + 28])] = torch.tensor([9], dtype=torch.uint8)
    with pytest.raises(GM.BandDamage, match=r"input \(7,\) torch.int32 .* offset 28 "):
        guard.check()
    assert torch.equal(guard.banded(torch.ones(3), fill=2.0), torch.ones(3))


def test_guarded_restores_the_modules_and_checks_on_exit():
    from ultra_torchdrug_amd import functional, relcsr, model
    functional._sparse_cache["stale"] = None
    with guarded() as guard:
        assert isinstance(functional.torch, GM.TorchProxy) and isinstance(relcsr.torch, GM.TorchProxy) and model.torch is torch
        assert not functional._sparse_cache
        body = guard.carve((3,), torch.float32, "cpu")
    assert functional.torch is torch and relcsr.torch is torch
    with pytest.raises(GM.BandDamage):
        with guarded("model") as guard:
            assert isinstance(model.torch, GM.TorchProxy) and functional.torch is torch
            body = guard.carve((3,), torch.float32, "cpu")
            guard.records[0].buffer[torch.tensor([guard.band + 12])] = torch.tensor([0], dtype=torch.uint8)
    assert model.torch is torch and body is not None
    with pytest.raises(ValueError):
        with guarded("data"):
            pass


def test_the_fixture_guards_the_default_modules(guarded):
    from ultra_torchdrug_amd import functional, model, relcsr
    assert isinstance(guarded, GM.Guard) and not guarded.records
    assert isinstance(functional.torch, GM.TorchProxy) and isinstance(relcsr.torch, GM.TorchProxy) and model.torch is torch
    assert functional.torch._guard is guarded
    body = functional.torch.empty(3, 2)
    assert GM.has_poison(body) and len(guarded.records) == 1


@pytest.mark.parametrize("guarded", [("model", "task")], indirect=True)
def test_the_fixture_takes_other_modules_by_indirect_parametrisation(guarded):
    from ultra_torchdrug_amd import functional, model, task
    assert isinstance(model.torch, GM.TorchProxy) and isinstance(task.torch, GM.TorchProxy) and functional.torch is torch


def test_the_fixture_restored_the_modules_when_the_tests_above_returned():
    from ultra_torchdrug_amd import functional, model, relcsr, task
    assert all(m.torch is torch for m in (functional, model, relcsr, task))


# ---------------------------------------------------------------------------------------------------- every idiom of the product
# Allocation calls the proxy does not route, each with its reason; the key is (module, enclosing function, call).
NOT_INTERCEPTED = {
    ("functional", "dense_topk", ".new_zeros"): "host twin of topk_keys: zeros that pad an index list, a tensor method; no kernel writes them",
    ("functional", "dense_set_boundary", ".new_zeros"): "host twin of set_boundary: a 0-dim zero for torch.where; no kernel writes it",
    ("task", "answer", ".new_zeros"): "the (0, k) result of an empty batch of queries: zero elements",
    ("task", "project", ".new_zeros"): "the (0, N) membership of an empty batch: zero elements",
    ("task", "_answer_query_checked", ".new_zeros"): "the (0, k) result of an empty batch: zero elements",
    ("model", "_feature_statistics", ".new_zeros"): "two 0-dim fp64 zeros that torch ops accumulate into; no kernel writes them",
    ("data", "*", "torch.zeros"): "dataset loading on the host; data.py runs no kernel and is not a module the guard proxies",
}
POSITIONAL = {"empty": None, "zeros": None, "ones": None, "full": 2, "empty_like": 1, "zeros_like": 1}
KEYWORDS = {"dtype", "device", "memory_format", "requires_grad"}


def _product_calls():
    """``(module, enclosing function, form, call node)`` of every allocation call in the product."""
    found = []
    for name in sorted(os.listdir(PACKAGE)):
        if not name.endswith(".py"):
            continue
        with open(os.path.join(PACKAGE, name)) as handle:
            tree = ast.parse(handle.read())
        parents = {}
        for node in ast.walk(tree):
            for child in ast.iter_child_nodes(node):
                parents[child] = node
        for node in ast.walk(tree):
            if not isinstance(node, ast.Call) or not isinstance(node.func, ast.Attribute):
                continue
            attr = node.func.attr
            on_torch = isinstance(node.func.value, ast.Name) and node.func.value.id == "torch"
            if on_torch and attr in GM.INTERCEPTED:
                form = "torch." + attr
            elif attr in ("new_empty", "new_zeros", "new_full"):
                form = "." + attr
            else:
                continue
            scope = node
            while scope in parents and not isinstance(scope, (ast.FunctionDef, ast.AsyncFunctionDef)):
                scope = parents[scope]
            found.append((name[:-3], scope.name if isinstance(scope, ast.FunctionDef) else "<module>", form, node))
    return found


def test_every_allocation_idiom_of_the_product_is_intercepted_or_listed():
    calls = _product_calls()
    assert len(calls) > 150                                     # the walk found the product
    used = set()
    escaped = []
    for module, scope, form, node in calls:
        key = (module, scope, form) if (module, scope, form) in NOT_INTERCEPTED else (module, "*", form)
        if key in NOT_INTERCEPTED:
            used.add(key)
            continue
        where = "%s.py:%d %s in %s" % (module, node.lineno, form, scope)
        if form.startswith(".") or module not in GM.ALL_MODULES:
            escaped.append(where + ": not a call the proxy sees")
            continue
        name = form[len("torch."):]
        assert hasattr(GM.TorchProxy, name)
        starred = any(isinstance(a, ast.Starred) for a in node.args)           # (sizes as ``*shape`` reach the proxy as varargs)
        if (starred and POSITIONAL[name] is not None) or any(k.arg is None for k in node.keywords):
            escaped.append(where + ": starred arguments")
        elif POSITIONAL[name] is not None and len(node.args) != POSITIONAL[name]:
            escaped.append(where + ": %d positional arguments" % len(node.args))
        elif POSITIONAL[name] is None and not node.args:
            escaped.append(where + ": no size")
        elif {k.arg for k in node.keywords} - KEYWORDS:
            escaped.append(where + ": keywords %s" % sorted({k.arg for k in node.keywords} - KEYWORDS))
    assert not escaped, "allocations that escape the guard:\n" + "\n".join(escaped)
    assert used == set(NOT_INTERCEPTED), "stale entries: %s" % sorted(set(NOT_INTERCEPTED) - used)
    assert all(len(reason) > 20 for reason in NOT_INTERCEPTED.values())


def test_the_proxy_takes_the_sizes_forms_of_the_product():
    """Sizes as varargs, as one tuple / list / torch.Size, empty shapes, tuple sums -- the forms the walk above finds."""
    guard = GM.Guard(band=256)
    proxy = GM.TorchProxy(guard)
    like = torch.zeros(2, 3)
    assert proxy.empty(3, 4).shape == (3, 4) and proxy.empty((3, 4)).shape == (3, 4) and proxy.empty([3]).shape == (3,)
    assert proxy.empty(like.shape).shape == (2, 3) and proxy.empty(tuple(like.shape[:-1]) + (5,)).shape == (2, 5)
    assert proxy.zeros(0, 4, dtype=torch.long).shape == (0, 4) and proxy.empty(0).numel() == 0
    assert proxy.empty(torch.tensor(3).item(), dtype=torch.uint8).shape == (3,)
    assert proxy.full((2,) + (3,), 0.5, device="cpu", dtype=torch.float32).shape == (2, 3)
    assert proxy.empty(2, dtype=torch.float32, device=torch.device("cpu")).device.type == "cpu"
    guard.check()


# ---------------------------------------------------------------------------------------------------- a host path of the product
def test_host_paths_of_the_product_run_unchanged_under_the_guard():
    from ultra_torchdrug_amd import functional as F
    gen = torch.Generator().manual_seed(5)
    member = torch.rand(3, 41, generator=gen) - 0.3
    member[1, 7] = float("nan")
    query = torch.randn(3, 8, generator=gen)
    floor = torch.tensor([0.1, 0.0, 0.5])
    pred = torch.randn(4, 37, generator=gen)
    pred[0, 3] = float("nan")
    pred[2, 5] = pred[2, 9]
    anchor, rel = torch.tensor([0, 1, 2, 3]), torch.tensor([0, 1, 0, 1])
    keys = torch.unique((torch.randint(0, 4, (30,), generator=gen) * 2 + torch.randint(0, 2, (30,), generator=gen)) * 37
                        + torch.randint(0, 37, (30,), generator=gen))
    want_b, want_c = F.dense_set_boundary(member, query, floor, with_count=True)
    want = [F.dense_topk(pred, k, keys, anchor, rel, 2) for k in (1, 40)]
    with guarded() as guard:
        got_b, got_c = F.dense_set_boundary(member, query, floor, with_count=True)
        got_s = F.set_boundary(member, query, floor)
        got = [F.dense_topk(pred, k, keys, anchor, rel, 2) for k in (1, 40)]
        got_t = F.topk_keys(pred, 40, keys, anchor, rel, 2)
        got_f = F.torch.full((3,), 2.0)
        assert len(guard.records) >= 1 and isinstance(F.torch, GM.TorchProxy)
        guard.check()
    assert torch.equal(got_b.view(torch.int32), want_b.view(torch.int32)) and torch.equal(got_c, want_c)
    assert torch.equal(got_s.view(torch.int32), want_b.view(torch.int32)) and torch.equal(got_f, torch.full((3,), 2.0))
    for (gv, gi), (wv, wi) in zip(got + [got_t], want + [want[1]]):
        assert torch.equal(gv.view(torch.int32), wv.view(torch.int32)) and torch.equal(gi, wi)
    assert not GM.has_poison(got_b)

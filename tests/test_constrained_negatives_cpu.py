"""Type-constrained strict negatives without a GPU: the dense torch twin ``functional.dense_constrained_negatives`` against the
plain numpy definition (tests/negative_definition.py) on the cases the device test draws from, against ``mask.nonzero()`` +
``variadic_sample``'s indexing on the mask ``listed & ~known``, the argument checks and the binding tables.  Entities and counts
are integers: nothing is compared with a tolerance."""
import numpy as np
import pytest
import torch

import negative_definition as ND


def _tensors(c):
    from ultra_torchdrug_amd import data
    t = {key: torch.from_numpy(c[key]) for key in ("set_of", "anchor", "rel", "rand", "keys")}
    return t, data.candidate_sets(c["sets"], c["n_node"])


def _twin(c, **kw):
    from ultra_torchdrug_amd import functional as UF
    t, sets = _tensors(c)
    args = dict(keys=t["keys"], anchor=t["anchor"], rel=t["rel"], n_rel=c["n_rel"], n_node=c["n_node"], rand=t["rand"], sets=sets,
                set_of=t["set_of"], min_free=1, return_free=True)
    args.update(kw)
    return UF.dense_constrained_negatives(**args)


@pytest.mark.parametrize("name", list(ND.CASES))
def test_the_dense_twin_equals_the_definition(name):
    c = ND.case(name)
    out, n_free = _twin(c)
    want, count = ND.expected(name)
    assert out.dtype == torch.int64 and n_free.dtype == torch.int64
    assert np.array_equal(out.numpy(), want) and np.array_equal(n_free.numpy(), count)
    if name == "ends":
        assert count.tolist()[:2] == [2, 2]                                       # only the first and the last item are free
        for q in (0, 1):
            assert set(want[q].tolist()) == {int(c["sets"][q][0]), int(c["sets"][q][-1])}


def test_the_dense_twin_falls_back_like_the_definition():
    c = ND.case("edges")
    for min_free in (5, 60, 10 ** 6):
        out, n_free = _twin(c, min_free=min_free)
        want, count = ND.expected("edges", min_free=min_free)
        assert np.array_equal(out.numpy(), want) and np.array_equal(n_free.numpy(), count)
    every, _ = _twin(c, sets=None, set_of=None)
    assert np.array_equal(every.numpy(), ND.expected("edges", with_sets=False)[0])
    assert torch.equal(every, _twin(c, min_free=10 ** 6)[0])                      # every row falls back: the unconstrained draw
    out, n_free = _twin(c, rand=torch.from_numpy(np.array([[np.nan, -0.5, 2.0]] * len(c["set_of"]), dtype=np.float32)))
    want, _ = ND.draw(c["n_node"], c["sets"], c["set_of"], c["known_rows"], np.array([[0.0, 0.0, 1.0]] * len(c["set_of"]), np.float32))
    assert np.array_equal(out.numpy(), want)                                      # NaN and negatives: the first, beyond 1: the last


def test_the_dense_twin_equals_nonzero_and_variadic_sample(monkeypatch):
    """``task.variadic_sample`` draws its own ``rand``; fed the same numbers on the mask ``listed & ~known`` it returns the twin's
    entities (rows without a free entity left out: the reference would index an empty list)."""
    from ultra_torchdrug_amd import task as UT
    c = ND.case("edges")
    t, _ = _tensors(c)
    out, n_free = _twin(c)
    keep = np.flatnonzero(n_free.numpy() > 0)
    mask = torch.zeros(len(keep), c["n_node"], dtype=torch.bool)
    for i, q in enumerate(keep):
        listed = np.arange(c["n_node"]) if c["set_of"][q] == -1 else c["sets"][c["set_of"][q]]
        mask[i, [e for e in listed.tolist() if e not in c["known_rows"][q]]] = True
    # (exactly 1.0 indexes one past a row's end in variadic_sample, which has no clamp: those slots are fed 0.5 and left out)
    inside = t["rand"][keep] < 1
    fed = torch.where(inside, t["rand"][keep], torch.full((), 0.5))
    monkeypatch.setattr(UT.torch, "rand", lambda *shape, **kw: fed)
    got = UT.variadic_sample(mask.nonzero()[:, 1], mask.sum(dim=-1), t["rand"].shape[1])
    monkeypatch.undo()
    assert inside.sum() > 0.8 * inside.numel() and torch.equal(got[inside], out[keep][inside])


def test_arguments_are_checked():
    from ultra_torchdrug_amd import data, functional as UF
    c = ND.case("edges")
    t, sets = _tensors(c)
    args = lambda **kw: {**dict(keys=t["keys"], anchor=t["anchor"], rel=t["rel"], n_rel=c["n_rel"], n_node=c["n_node"], rand=t["rand"],
                                sets=sets, set_of=t["set_of"]), **kw}
    for bad in (dict(min_free=0), dict(n_rel=0), dict(n_node=0), dict(n_node=2 ** 31), dict(rand=t["rand"].double()),
                dict(rand=t["rand"][:, :0]), dict(rand=t["rand"].t()), dict(sets=None), dict(set_of=t["set_of"][:3]),
                dict(anchor=t["anchor"].int()), dict(keys=t["keys"].int()),
                dict(sets=data.candidate_sets(c["sets"], c["n_node"] + 1))):
        with pytest.raises(RuntimeError):
            UF.dense_constrained_negatives(**args(**bad))
        with pytest.raises(RuntimeError):
            UF.constrained_negatives(**args(**bad))
    assert torch.equal(UF.constrained_negatives(**args()), UF.dense_constrained_negatives(**args()))      # CPU tensors: the twin


def test_the_entry_is_bound_three_ways():
    """The header / ``nm -D`` / prototype tests of test_host_logic.py cover the symbol through this row of the table."""
    import ctypes
    from ultra_torchdrug_amd import _lib, _torch_ext, backend, functional as UF
    restype, argtypes = _lib.SIGNATURES["ultra_constrained_negative"]
    assert restype is ctypes.c_int32 or restype is ctypes.c_int
    assert len(argtypes) == 19 and "ultra_constrained_negative" in _lib.EXPORTS
    assert "constrained_negatives" in _torch_ext.OPS
    assert backend.get().constrained_negatives is UF.constrained_negatives
    assert "constrained_negatives" in UF.__all__ and "dense_constrained_negatives" in UF.__all__

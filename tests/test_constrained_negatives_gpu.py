"""MI355X: type-constrained strict negatives on the device -- ``ultra_constrained_negative`` against the plain numpy definition
(tests/negative_definition.py) on lists of one, two and three chunks, against ``functional.strict_negatives`` where the draw is
unconstrained or falls back, against ``functional.candidate_select`` on the counts, captured into a hipGraph, through both
bindings and between guard bands.  Entities and counts are integers: ``torch.equal`` everywhere."""
import numpy as np
import pytest
import torch

import negative_definition as ND

pytestmark = pytest.mark.gpu

OK, BAD_SHAPE, NULL_POINTER = 0, 2, 3


def _dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


_on_device = {}


def _inputs(name):
    """The tensors of a case on the device, moved once: ``(dict of tensors, CandidateSets)``."""
    from ultra_torchdrug_amd import data
    if name not in _on_device:
        c = ND.case(name)
        t = {key: torch.from_numpy(c[key]).to(_dev()) for key in ("set_of", "anchor", "rel", "rand", "keys")}
        _on_device[name] = t, data.candidate_sets(c["sets"], c["n_node"]).to(_dev())
    return _on_device[name]


def _call(name, **kw):
    from ultra_torchdrug_amd import functional as UF
    c = ND.case(name)
    t, sets = _inputs(name)
    args = dict(keys=t["keys"], anchor=t["anchor"], rel=t["rel"], n_rel=c["n_rel"], n_node=c["n_node"], rand=t["rand"], sets=sets,
                set_of=t["set_of"], min_free=1, return_free=True)
    args.update(kw)
    return UF.constrained_negatives(**args)


def _same(got, want):
    out, n_free = got
    assert out.dtype == torch.int64 and n_free.dtype == torch.int64
    assert torch.equal(out.cpu(), torch.from_numpy(want[0])) and torch.equal(n_free.cpu(), torch.from_numpy(want[1]))


# ------------------------------------------------------------------------------------------------------------- the operator
@pytest.mark.parametrize("name", list(ND.CASES))
def test_the_kernel_equals_the_definition(name):
    """Lists of 0 to 2000 entities with two ``-1`` rows at N = 3000; 32768 in one chunk; 32769 and 70001 with a ``-1`` row at
    N = 80000 (the edge rands 0, below one, 0.5 and 1.0 make samples land in every chunk); only the first and the last item free;
    a chunk without a free entity between, and before, chunks that have some."""
    c = ND.case(name)
    got = _call(name)
    _same(got, ND.expected(name))
    out, n_free = got[0].cpu().numpy(), got[1].cpu().numpy()
    if name == "chunks":                                                         # samples land in every chunk of both lists
        for q, n_chunks in ((0, 2), (1, 3)):
            at = np.searchsorted(c["sets"][q], out[q])
            assert set((at // ND.CHUNK).tolist()) == set(range(n_chunks))
    if name == "ends":
        assert n_free.tolist()[:2] == [2, 2]
        for q in (2, 3):
            at = np.searchsorted(c["sets"][q], out[q]) // ND.CHUNK
            assert set(at.tolist()) == ({0, 2} if q == 2 else {1, 2})


@pytest.mark.parametrize("n_sample", [1, 3, 300])
def test_sample_counts_below_and_past_one_workgroup(n_sample):
    c = ND.case("edges")
    rand = ND.wide_rand("edges", 300)[:, 1:1 + n_sample] if n_sample < 300 else ND.wide_rand("edges", 300)
    rand = np.ascontiguousarray(rand)
    assert n_sample == 1 or (rand == 1).any()
    got = _call("edges", rand=torch.from_numpy(rand).to(_dev()))
    _same(got, ND.draw(c["n_node"], c["sets"], c["set_of"], c["known_rows"], rand))
    assert got[0].shape == (len(c["set_of"]), n_sample)
    if n_sample == 300:                                                          # and past one workgroup on three chunks
        rand = ND.wide_rand("chunks", 300)
        c = ND.case("chunks")
        _same(_call("chunks", rand=torch.from_numpy(rand).to(_dev())),
              ND.draw(c["n_node"], c["sets"], c["set_of"], c["known_rows"], rand))


@pytest.mark.parametrize("n", [1000, 70001])
def test_every_entity_gives_the_words_of_strict_negatives(n):
    """``set_of`` all ``-1``, ``sets=None`` and a set that lists every entity explicitly: the exact words of
    ``functional.strict_negatives`` for the same ``rand``."""
    from ultra_torchdrug_amd import data, functional as UF
    dev = _dev()
    rng = np.random.default_rng(n)
    rows, n_rel = 6, 3
    anchor = torch.from_numpy(rng.choice(n, rows, replace=False)).to(dev)
    rel = torch.from_numpy(rng.integers(0, n_rel, rows)).to(dev)
    known = [np.unique(rng.integers(0, n, size)) for size in (0, 1, 50, n // 3, n // 2, 5)]
    keys = torch.from_numpy(np.unique(np.concatenate([(int(a) * n_rel + int(r)) * n + k for a, r, k in
                                                      zip(anchor.tolist(), rel.tolist(), known)]))).to(dev)
    rand = torch.from_numpy(ND.edge_rand(rng, rows, 128)).to(dev)
    want = UF.strict_negatives(keys, anchor, rel, n_rel, n, rand)
    sets = data.candidate_sets([np.arange(n), [3]], n, device=dev)
    minus = torch.full((rows,), -1, dtype=torch.int64, device=dev)
    free = n - torch.tensor([len(k) for k in known], device=dev)
    for kw in (dict(sets=None, set_of=None), dict(sets=sets, set_of=None), dict(sets=sets, set_of=minus),
               dict(sets=sets, set_of=torch.zeros_like(minus))):
        out, n_free = UF.constrained_negatives(keys, anchor, rel, n_rel, n, rand, return_free=True, **kw)
        assert torch.equal(out, want) and torch.equal(n_free, free), kw


def test_strictness_membership_and_the_counts_of_candidate_select():
    from ultra_torchdrug_amd import functional as UF
    for name in ("edges", "chunks"):
        c = ND.case(name)
        t, sets = _inputs(name)
        out, n_free = _call(name)
        pred = torch.zeros(len(c["set_of"]), c["n_node"], device=_dev())
        counts = UF.candidate_select(pred, sets, t["set_of"], 1, t["keys"], t["anchor"], t["rel"], c["n_rel"], outputs=("n_free",))
        assert torch.equal(n_free, counts.n_free)
        for q, row in enumerate(out.cpu().tolist()):
            if n_free[q] >= 1:
                listed = range(c["n_node"]) if c["set_of"][q] == -1 else set(c["sets"][c["set_of"][q]].tolist())
                assert all(e in listed for e in row), (name, q)
            assert not any(e in c["known_rows"][q] for e in row), (name, q)


def test_rows_that_fall_back_give_the_row_of_strict_negatives():
    """A set entirely known, an empty set, a set id of ``S`` and of ``-2``, ``min_free = 5`` against 4 free entities: the row of
    ``strict_negatives``, with the set-side count in ``n_free``; a row with every entity known gives 0."""
    from ultra_torchdrug_amd import data, functional as UF
    dev = _dev()
    n, n_rel = 500, 2
    rng = np.random.default_rng(31)
    lists = [np.arange(10, 60), [], np.arange(100, 110), np.arange(0, 500, 7), np.arange(200, 300)]
    sets = data.candidate_sets(lists, n, device=dev)
    set_of = torch.tensor([0, 1, 5, -2, 2, 3, 4], device=dev)
    anchor = torch.arange(7, device=dev) * 3
    rel = torch.tensor([0, 1, 0, 1, 0, 1, 0], device=dev)
    known = [np.arange(0, 80), np.arange(5), np.arange(5), np.arange(5), np.arange(100, 106), np.arange(0, 30), np.arange(n)]
    keys = torch.from_numpy(np.unique(np.concatenate([(int(a) * n_rel + int(r)) * n + k for a, r, k in
                                                      zip(anchor.tolist(), rel.tolist(), known)]))).to(dev)
    rand = torch.from_numpy(ND.edge_rand(rng, 7, 128)).to(dev)
    strict = UF.strict_negatives(keys, anchor, rel, n_rel, n, rand)
    out, n_free = UF.constrained_negatives(keys, anchor, rel, n_rel, n, rand, sets, set_of, min_free=5, return_free=True)
    own = len([e for e in range(0, 500, 7) if e >= 30])
    assert n_free.tolist() == [0, 0, 0, 0, 4, own, 0]
    for q in (0, 1, 2, 3, 4, 6):
        assert torch.equal(out[q], strict[q]), q
    assert (out[6] == 0).all()
    assert set(out[5].tolist()) <= set(range(0, 500, 7)) and not torch.equal(out[5], strict[5])
    again, _ = UF.constrained_negatives(keys, anchor, rel, n_rel, n, rand, sets, set_of, min_free=4, return_free=True)
    assert set(again[4].tolist()) == {106, 107, 108, 109}                        # four free entities are enough for min_free = 4
    want = ND.draw(n, [np.asarray(l, dtype=np.int64) for l in lists], set_of.tolist(), [set(k.tolist()) for k in known],
                   rand.cpu().numpy(), 5)
    assert np.array_equal(out.cpu().numpy(), want[0])


def test_items_out_of_range_are_skipped_and_ptr_values_clamped():
    from ultra_torchdrug_amd import data, functional as UF
    dev = _dev()
    n = 100
    items = torch.tensor([-5, 2, 4, 100, 7, 2 ** 31 - 1, 9, 11], dtype=torch.int32, device=dev)
    keys = torch.tensor([4], device=dev)                                         # (0, 0, 4) is known
    zero = torch.zeros(3, dtype=torch.int64, device=dev)
    rand = torch.from_numpy(ND.edge_rand(np.random.default_rng(1), 3, 64)).to(dev)
    strict = UF.strict_negatives(keys, zero, zero, 1, n, rand)
    # set 0: positions [-3, 5) clamped to [0, 5): -5 and 100 skipped, 4 known;  set 1: [5, 90) clamped to [5, 8): 2^31 - 1 skipped;
    # set 2: [90, 3) clamped to [8, 8), the empty list: the row falls back
    sets = data.CandidateSets(torch.tensor([-3, 5, 90, 3], device=dev), items, n, max_len=8, validate=False)
    out, n_free = UF.constrained_negatives(keys, zero, zero, 1, n, rand, sets, torch.tensor([0, 1, 2], device=dev), return_free=True)
    assert n_free.tolist() == [2, 2, 0]
    assert set(out[0].tolist()) == {2, 7} and set(out[1].tolist()) == {9, 11} and torch.equal(out[2], strict[2])
    # set 0: [9, 3) clamped to [8, 8): empty;  set 1: [3, 90) clamped to [3, 8): 100 and 2^31 - 1 skipped, 7, 9 and 11 free
    sets = data.CandidateSets(torch.tensor([9, 3, 90, 3], device=dev), items, n, max_len=8, validate=False)
    out, n_free = UF.constrained_negatives(keys, zero, zero, 1, n, rand, sets, torch.tensor([1, 1, 0], device=dev), return_free=True)
    assert n_free.tolist() == [3, 3, 0] and set(out[:2].flatten().tolist()) == {7, 9, 11} and torch.equal(out[2], strict[2])
    # NaN, a negative number, exactly 1.0 and a product that overflows: the first and the last free entity
    nan =torch.tensor([[float("nan"), -1.0, 1.0, 3.0e38]] * 3, device=dev)
    out = UF.constrained_negatives(keys, zero, zero, 1, n, nan, sets, torch.tensor([1, -1, 7], device=dev))
    assert out.tolist() == [[7, 7, 11, 11], [0, 0, 99, 99], [0, 0, 99, 99]]


def test_host_checks_return_their_status_before_any_launch():
    from ultra_torchdrug_amd import _lib
    lib = _lib.load()
    dev = _dev()
    n, rows, n_sample = 100, 2, 4
    ptr, items = torch.tensor([0, 3], device=dev), torch.tensor([1, 2, 3], dtype=torch.int32, device=dev)
    ids = torch.zeros(rows, dtype=torch.int64, device=dev)
    keys = torch.tensor([5], device=dev)
    rand = torch.zeros(rows, n_sample, device=dev)
    out = torch.full((rows, n_sample), 7, dtype=torch.int64, device=dev)
    n_free = torch.full((rows,), 7, dtype=torch.int64, device=dev)

    def run(**kw):
        a = dict(keys=keys, n_keys=1, anchor=ids, rel=ids, set_of=ids, index_stride=1, n_query=rows, n_rel=2, n_node=n, ptr=ptr,
                 items=items, n_sets=1, n_items=3, rand=rand, n_sample=n_sample, min_free=1, out=out, n_free=n_free)
        a.update(kw)
        return lib.ultra_constrained_negative(*[v.data_ptr() if isinstance(v, torch.Tensor) else v for v in a.values()], None)

    for status, kw in ((BAD_SHAPE, dict(n_node=0)), (BAD_SHAPE, dict(n_node=2 ** 31)), (BAD_SHAPE, dict(n_rel=0)),
                       (BAD_SHAPE, dict(n_node=2 ** 31 - 1, n_rel=3)), (BAD_SHAPE, dict(n_sample=0)), (BAD_SHAPE, dict(min_free=0)),
                       (BAD_SHAPE, dict(n_query=-1)), (BAD_SHAPE, dict(n_keys=-1)), (BAD_SHAPE, dict(n_sets=-1)),
                       (BAD_SHAPE, dict(n_items=-1)), (BAD_SHAPE, dict(index_stride=-1)), (NULL_POINTER, dict(ptr=None)),
                       (NULL_POINTER, dict(items=None)), (NULL_POINTER, dict(anchor=None)), (NULL_POINTER, dict(rel=None)),
                       (NULL_POINTER, dict(rand=None)), (NULL_POINTER, dict(out=None)), (NULL_POINTER, dict(keys=None)),
                       (OK, dict(n_query=0)), (OK, dict(n_query=0, out=None, rand=None))):
        assert run(**kw) == status, kw
    torch.cuda.synchronize()
    assert (out == 7).all() and (n_free == 7).all()                              # nothing ran
    assert run(n_free=None) == OK and run(set_of=None, ptr=None, items=None) == OK and run(keys=None, n_keys=0) == OK
    assert run(items=None, n_items=0, ptr=torch.tensor([0, 0], device=dev)) == OK
    torch.cuda.synchronize()
    assert (out != 7).all()


def test_strided_views_and_a_column_of_a_transposed_batch():
    from ultra_torchdrug_amd import functional as UF
    c = ND.case("edges")
    t, sets = _inputs("edges")
    want = _call("edges")
    rows = len(c["set_of"])
    batch = torch.stack([t["anchor"], t["set_of"], t["rel"]], dim=1).contiguous()                  # (B, 3): columns of stride 3
    a, s, r = batch.t()
    assert a.stride(0) == 3
    got = UF.constrained_negatives(t["keys"], a, r, c["n_rel"], c["n_node"], t["rand"], sets, s, return_free=True)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    wide = torch.zeros(rows, 5, dtype=torch.int64, device=_dev())
    wide[:, 0], wide[:, 2], wide[:, 4] = t["anchor"], t["rel"], t["set_of"]
    got = UF.constrained_negatives(t["keys"], wide[:, 0], wide[:, 2], c["n_rel"], c["n_node"], t["rand"], sets, wide[:, 4],
                                   return_free=True)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    # strides that differ are made contiguous, not refused
    got = UF.constrained_negatives(t["keys"], a, r, c["n_rel"], c["n_node"], t["rand"], sets, t["set_of"], return_free=True)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


def test_the_ctypes_binding_equals_the_torch_extension(monkeypatch):
    from ultra_torchdrug_amd import _torch_ext
    assert _torch_ext.binding() == "torch"
    first = {name: _call(name) for name in ("edges", "chunks")}
    alone = _call("edges", return_free=False)
    monkeypatch.setenv("ULTRA_BINDING", "ctypes")
    for name, want in first.items():
        got = _call(name)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    assert torch.equal(_call("edges", return_free=False), alone) and torch.equal(alone, first["edges"][0])


@pytest.mark.parametrize("name", ["edges", "chunks"])
def test_captured_into_a_hipgraph_and_replayed_twice(name):
    c = ND.case(name)
    t, _ = _inputs(name)
    rng = np.random.default_rng(5)
    rands = [ND.edge_rand(rng, *c["rand"].shape) for _ in range(2)]
    static = t["rand"].clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _call(name, rand=static)                                                 # warm-up: the outputs enter the cache
    torch.cuda.current_stream().wait_stream(side)
    captured = torch.cuda.CUDAGraph()
    with torch.cuda.graph(captured, stream=side):
        got = _call(name, rand=static)
    for rand in rands:                                                           # two replays, new numbers in the same buffer
        static.copy_(torch.from_numpy(rand))
        captured.replay()
        torch.cuda.synchronize()
        eager = _call(name, rand=torch.from_numpy(rand).to(_dev()))
        assert torch.equal(got[0], eager[0]) and torch.equal(got[1], eager[1])
        _same(got, ND.draw(c["n_node"], c["sets"], c["set_of"], c["known_rows"], rand))


# ------------------------------------------------------------------------------------------------------------ memory bounds
@pytest.mark.parametrize("n_sample", [1, 300])
@pytest.mark.parametrize("length", [65, 1025, ND.CHUNK + 1])
def test_the_launch_stays_inside_its_operands(length, n_sample, monkeypatch):
    """Inputs between zero / NaN bands, outputs poisoned between pattern bands (the ctypes binding allocates them in
    ``functional.py``, where the guard sees them): no guard word changes, and the outputs equal the definition, so every word of
    them was written.  The longest list ends at the last item of ``items`` and at the last entity."""
    from guarded_memory import guarded
    from ultra_torchdrug_amd import data, functional as UF
    monkeypatch.setenv("ULTRA_BINDING", "ctypes")
    dev = _dev()
    n = length + 40
    c = ND.make_case(n, [7, length], seed=length, n_all=1, n_sample=n_sample)
    c["sets"][1][-1] = n - 1
    c["known_rows"][1].discard(n - 1)
    keys = ND.completion_keys(np.array([(a, e, r) for a, r, known in zip(c["anchor"], c["rel"], c["known_rows"]) for e in known]),
                              0, c["n_rel"], n)
    sets = data.candidate_sets(c["sets"], n)
    with guarded("functional") as guard:
        rand, ptr, items, set_of, anchor, rel, keys_d = [
            guard.banded(torch.as_tensor(x).to(dev)) for x in (c["rand"], sets.ptr, sets.items, c["set_of"], c["anchor"], c["rel"],
                                                               keys)]
        banded = data.CandidateSets(ptr, items, n, sets.max_len, validate=False)
        out, n_free = UF.constrained_negatives(keys_d, anchor, rel, c["n_rel"], n, rand, banded, set_of, return_free=True)
        guard.check()
        fallen = UF.constrained_negatives(keys_d, anchor, rel, c["n_rel"], n, rand, banded, set_of, min_free=10 ** 6)
        guard.check()
    want = ND.draw(n, c["sets"], c["set_of"], c["known_rows"], c["rand"])
    assert (out >= 0).all() and (n_free >= 0).all()                              # no -1 poison left
    _same((out, n_free), want)
    assert np.array_equal(fallen.cpu().numpy(), ND.draw(n, c["sets"], None, c["known_rows"], c["rand"])[0])

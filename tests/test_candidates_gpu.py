"""MI355X: candidate sets on the device -- ``ultra_candidate_select_f32`` in its one-launch and its two-launch form against the
plain-Python definition (tests/candidate_definition.py: integers equal, values bit for bit), against ``ultra_topk_keys`` /
``ultra_filtered_rank_keys`` when every query takes all entities, captured into a hipGraph, through both bindings, between guard
bands and past 2^32 bytes of scores; ``task.answer(candidates=...)`` / ``task.rank_among`` / ``engine.evaluate_constrained``
against masks over the scores of ``predict`` and against the CPU twin of the task."""
import ctypes

import numpy as np
import pytest
import torch

import candidate_definition as CD
from sampled_graphs import small_task, wide_batch, wide_graph
from topk_definition import completions, same_bits

pytestmark = pytest.mark.gpu

OK, BAD_SHAPE, NULL_POINTER, WORKSPACE = 0, 2, 3, 4


def _dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _same(got, want, what=None):
    """A ``CandidateSelection`` of the device against the definition's dict: integers equal, floats bit for bit."""
    for name in ("top_index", "rank", "n_free", "member"):
        if getattr(got, name) is not None:
            assert getattr(got, name).dtype == (torch.uint8 if name == "member" else torch.int64), name
            assert np.array_equal(getattr(got, name).cpu().numpy(), want[name]), (name, what)
    if got.top_value is not None:
        assert got.top_value.dtype == torch.float32 and same_bits(got.top_value.cpu().numpy(), want["top_value"]), what


def _equal(a, b):
    for x, y in zip(a, b):
        assert (x is None) == (y is None)
        if x is not None:
            assert x.dtype == y.dtype and (same_bits(x.cpu().numpy(), y.cpu().numpy()) if x.is_floating_point() else torch.equal(x, y))


_on_device = {}


def _inputs(name):
    """The tensors of a case on the device, moved once: ``(dict of tensors, CandidateSets)``."""
    from ultra_torchdrug_amd import data
    if name not in _on_device:
        c = CD.case(name)
        t = {key: torch.from_numpy(c[key]).to(_dev()) for key in ("pred", "set_of", "anchor", "rel", "target", "keys")}
        _on_device[name] = t, data.candidate_sets(c["sets"], c["n_node"]).to(_dev())
    return _on_device[name]


def _call(name, k, **kw):
    from ultra_torchdrug_amd import functional as UF
    c = CD.case(name)
    t, sets = _inputs(name)
    args = dict(pred=t["pred"], sets=sets, set_of=t["set_of"], k=k, keys=t["keys"], anchor=t["anchor"], rel=t["rel"],
                n_rel=c["n_rel"], target=t["target"], max_len=c["max_len"])
    args.update(kw)
    return UF.candidate_select(**args)


# ------------------------------------------------------------------------------------------------------------- the operator
@pytest.mark.parametrize("k", [1, 10, 128])
@pytest.mark.parametrize("name", list(CD.CASES))
def test_the_kernel_equals_the_definition(name, k):
    c = CD.case(name)
    assert CD.tie_fraction(c) >= 0.2
    assert (c["max_len"] > CD.SLICE) == (name == "slices")
    want = CD.expected(name, k)
    got = _call(name, k)
    _same(got, want, (name, k))
    if name == "edges":
        assert want["n_free"][3] == 0 and want["rank"][3] == 1 and (want["top_index"][3] == -1).all() and want["n_free"][1] < 10
    if name == "slices":
        assert want["n_free"][1] == 0 and want["rank"][1] == 1 and want["n_free"][2] > 50000


@pytest.mark.parametrize("name", ["edges", "slices"])
def test_sets_filters_targets_and_strides_in_one_call(name):
    from ultra_torchdrug_amd import functional as UF
    c = CD.case(name)
    t, sets = _inputs(name)
    k = 10
    n, rows = c["n_node"], len(c["pred"])
    assert set(c["set_of"].tolist()) > {-1} and (c["target"] == -1).any()                         # -1 next to real sets and targets
    _same(_call(name, k, set_of=None, sets=None), CD.expected(name, k, with_sets=False), "set_of=None")
    _same(_call(name, k, keys=None, anchor=None, rel=None), CD.expected(name, k, filtered=False), "keys=None")
    _same(_call(name, k, target=None), CD.expected(name, k, with_target=False), "target=None")
    wide = torch.full((rows, n + 37), float("nan"), device=_dev())                                # row_stride > n_node
    wide[:, :n] = t["pred"]
    index = torch.stack([t["anchor"], t["rel"], t["set_of"]], dim=1)                              # index_stride 3
    assert index[:, 0].stride(0) == 3 and wide[:, :n].stride(0) == n + 37
    got = _call(name, k, pred=wide[:, :n], anchor=index[:, 0], rel=index[:, 1], set_of=index[:, 2], target=index.new_tensor(
        np.stack([c["target"]] * 2, axis=1))[:, 1])
    _same(got, CD.expected(name, k), "strided")
    # a set_of whose stride differs from the anchors' is copied, not misread
    _same(_call(name, k, anchor=index[:, 0], rel=index[:, 1]), CD.expected(name, k), "mixed strides")
    # max_len cuts a list to its first positions
    cut = 700 if name == "edges" else 40000
    want = CD.select(c["pred"], c["sets"], c["set_of"], c["known_rows"], c["target"], k, max_len=cut)
    _same(_call(name, k, max_len=cut), want, "max_len")
    assert isinstance(got, UF.CandidateSelection)


@pytest.mark.parametrize("n", [1000, 70001])
def test_all_entities_equals_topk_keys_and_filtered_rank_keys(n):
    from ultra_torchdrug_amd import functional as UF
    dev = _dev()
    rng = np.random.default_rng(n)
    rows, n_rel = 5, 4
    pred = torch.from_numpy(CD.grid_scores(rng, rows, n)).to(dev)
    anchor = torch.from_numpy(rng.choice(n, rows, replace=False)).to(dev)
    rel = torch.from_numpy(rng.integers(0, n_rel, rows)).to(dev)
    other = [np.union1d(rng.integers(0, n, 300), [0, n - 1]) for _ in range(rows)]
    triples = np.concatenate([np.stack([np.full(len(o), int(a)), o, np.full(len(o), int(r))], axis=1)
                              for o, a, r in zip(other, anchor.tolist(), rel.tolist())])
    keys = torch.from_numpy(CD.completion_keys(triples, 0, n_rel, n)).to(dev)
    target = torch.from_numpy(rng.integers(0, n, rows)).to(dev)
    for k in (1, 10, 128):
        value, index = UF.topk_keys(pred, k, keys, anchor, rel, n_rel, n)
        rank = UF.filtered_rank_keys(pred, target, keys, anchor, rel, n_rel, n)
        for set_of in (None, torch.full((rows,), -1, dtype=torch.int64, device=dev)):
            got = UF.candidate_select(pred, None if set_of is None else _empty_sets(n), set_of, k, keys, anchor, rel, n_rel, target)
            assert torch.equal(got.top_index, index) and same_bits(got.top_value.cpu().numpy(), value.cpu().numpy())
            assert torch.equal(got.rank, rank) and got.member.all()
            assert torch.equal(got.n_free, UF.filter_counts(keys, anchor, rel, n_rel, n))


def _empty_sets(n):
    from ultra_torchdrug_amd import data
    return data.candidate_sets([[]], n).to(_dev())


@pytest.mark.parametrize("name", ["edges", "slices"])
def test_each_subset_of_the_outputs_alone(name):
    full = _call(name, 10)
    subsets = CD.subsets() if name == "edges" else [(o,) for o in CD.OUTPUTS] + [("rank", "n_free", "member")]
    for outputs in subsets:
        got = _call(name, 10, outputs=outputs)
        _equal(got, [value if o in outputs else None for o, value in zip(CD.OUTPUTS, full)])
    _equal(_call(name, 0, outputs=("rank", "n_free")), [None, None, full.rank, full.n_free, None])


def test_host_checks_return_their_status_before_any_launch():
    from ultra_torchdrug_amd import _lib
    lib = _lib.load()
    dev = _dev()
    n, rows = 100, 2
    pred = torch.zeros(rows, n, device=dev)
    ptr, items = torch.tensor([0, 3], device=dev), torch.tensor([1, 2, 3], dtype=torch.int32, device=dev)
    ids = torch.zeros(rows, dtype=torch.int64, device=dev)
    keys = torch.tensor([5], device=dev)
    top_index = torch.full((rows, 128), 7, dtype=torch.int64, device=dev)
    top_value = torch.full((rows, 128), 7.0, device=dev)
    counts = torch.full((3, rows), 7, dtype=torch.int64, device=dev)
    member = torch.full((rows,), 7, dtype=torch.uint8, device=dev)
    ws = torch.zeros(64, dtype=torch.int64, device=dev)

    def run(**kw):
        a = dict(pred=pred, n_query=rows, n_node=n, row_stride=n, ptr=ptr, items=items, n_sets=1, n_items=3, set_of=ids, max_len=3,
                 keys=keys, n_keys=1, anchor=ids, rel=ids, index_stride=1, n_rel=2, target=ids, target_stride=1, k=10,
                 top_index=top_index, top_value=top_value, rank=counts[0], n_free=counts[1], member=member, workspace=None,
                 workspace_bytes=0)
        a.update(kw)
        return lib.ultra_candidate_select_f32(*[v.data_ptr() if isinstance(v, torch.Tensor) else v for v in a.values()], None)

    none = dict(top_index=None, top_value=None, rank=None, n_free=None, member=None)
    for status, kw in ((BAD_SHAPE, dict(k=0)), (BAD_SHAPE, dict(k=129)), (BAD_SHAPE, dict(n_node=0)), (BAD_SHAPE, dict(n_node=2 ** 31)),
                       (BAD_SHAPE, dict(row_stride=n - 1)), (BAD_SHAPE, dict(n_rel=0)), (BAD_SHAPE, dict(n_query=-1)),
                       (BAD_SHAPE, dict(max_len=-1)), (BAD_SHAPE, dict(max_len=2 ** 31)), (BAD_SHAPE, dict(index_stride=-1)),
                       (BAD_SHAPE, dict(n_query=65536, max_len=CD.SLICE + 1)), (BAD_SHAPE, dict(n_node=2 ** 31 - 1, row_stride=2 ** 31, n_rel=3)),
                       (NULL_POINTER, none), (NULL_POINTER, dict(pred=None)), (NULL_POINTER, dict(anchor=None)),
                       (NULL_POINTER, dict(ptr=None)), (WORKSPACE, dict(max_len=CD.SLICE + 1)),
                       (WORKSPACE, dict(max_len=CD.SLICE + 1, workspace=ws, workspace_bytes=2 * rows * (8 * 10 + 16) - 8)),
                       (OK, dict(n_query=0)), (OK, dict(n_query=0, **none))):
        assert run(**kw) == status, kw
    torch.cuda.synchronize()
    assert (top_index == 7).all() and (top_value == 7).all() and (counts == 7).all() and (member == 7).all()      # nothing ran
    assert run(k=0, top_index=None, top_value=None) == OK and run(n_rel=0, keys=None) == OK                       # k, n_rel unused
    assert run(max_len=CD.SLICE + 1, workspace=ws, workspace_bytes=2 * rows * (8 * 10 + 16)) == OK
    torch.cuda.synchronize()
    size = lambda *a: int(lib.ultra_candidate_select_workspace(*a))
    assert size(5, CD.SLICE, 10) == 0 and size(5, CD.SLICE + 1, 10) == 5 * 2 * (80 + 16) and size(5, 70001, 0) == 5 * 3 * 16
    assert size(0, 70001, 10) == 0 and size(3, 70001, 128) == 3 * 3 * (1024 + 16)


@pytest.mark.parametrize("name", ["edges", "slices"])
def test_captured_into_a_hipgraph_and_replayed_twice(name):
    c = CD.case(name)
    t, _ = _inputs(name)
    rng = np.random.default_rng(5)
    scores = [CD.grid_scores(rng, *c["pred"].shape) for _ in range(2)]
    static = t["pred"].clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _call(name, 10, pred=static)                                             # warm-up: outputs and workspace enter the cache
    torch.cuda.current_stream().wait_stream(side)
    captured = torch.cuda.CUDAGraph()
    with torch.cuda.graph(captured, stream=side):
        got = _call(name, 10, pred=static)
    for score in scores:                                                         # two replays, new scores in the same buffer
        static.copy_(torch.from_numpy(score))
        captured.replay()
        torch.cuda.synchronize()
        _same(got, CD.select(score, c["sets"], c["set_of"], c["known_rows"], c["target"], 10), "replay")
        _equal(got, _call(name, 10, pred=torch.from_numpy(score).to(_dev())))


@pytest.mark.parametrize("name", ["edges", "slices"])
def test_the_ctypes_binding_equals_the_torch_extension(name, monkeypatch):
    from ultra_torchdrug_amd import _torch_ext
    assert _torch_ext.binding() == "torch"
    first = _call(name, 10)
    part = _call(name, 10, outputs=("top_value", "member"))
    monkeypatch.setenv("ULTRA_BINDING", "ctypes")
    _equal(first, _call(name, 10))
    _equal(part, _call(name, 10, outputs=("top_value", "member")))
    _same(_call(name, 128), CD.expected(name, 128), "ctypes")


# ------------------------------------------------------------------------------------------------------------ memory bounds
@pytest.mark.parametrize("length", [65, 1025, CD.SLICE + 1])
def test_the_launch_stays_inside_its_operands(length, monkeypatch):
    """Inputs between NaN / zero bands, outputs and the workspace poisoned between pattern bands (the ctypes binding allocates
    them in ``functional.py``, where the guard sees them): no guard word changes and the results equal the definition, so every
    output word was written.  The longest list ends at the last item of ``items`` and the last entity of the row."""
    from guarded_memory import guarded, has_poison
    from ultra_torchdrug_amd import data, functional as UF
    monkeypatch.setenv("ULTRA_BINDING", "ctypes")
    dev = _dev()
    n = length + 40
    c = CD.make_case(n, [7, length], seed=length, n_all=1)
    c["sets"][1][-1] = n - 1
    c["known_rows"][1].discard(n - 1)
    keys = CD.completion_keys(np.array([(a, e, r) for a, r, known in zip(c["anchor"], c["rel"], c["known_rows"]) for e in known]),
                              0, c["n_rel"], n)
    sets = data.candidate_sets(c["sets"], n)
    with guarded("functional") as guard:
        pred, ptr, items, set_of, anchor, rel, target, keys_d = [
            guard.banded(torch.as_tensor(x).to(dev)) for x in (c["pred"], sets.ptr, sets.items, c["set_of"], c["anchor"], c["rel"],
                                                               c["target"], keys)]
        banded = data.CandidateSets(ptr, items, n, sets.max_len, validate=False)
        got = UF.candidate_select(pred, banded, set_of, 128, keys_d, anchor, rel, c["n_rel"], target, max_len=c["max_len"])
        guard.check()
        assert not has_poison(got.top_value)
        _same(got, CD.select(c["pred"], c["sets"], c["set_of"], c["known_rows"], c["target"], 128), length)
        short = UF.candidate_select(pred[:2], banded, set_of[:2], 128, keys_d, anchor[:2], rel[:2], c["n_rel"], target[:2],
                                    max_len=sets.max_len) if length <= CD.SLICE else None
        guard.check()
    if short is not None:
        _same(short, {key: value[:2] for key, value in CD.select(c["pred"], c["sets"], c["set_of"], c["known_rows"], c["target"],
                                                                 128).items()}, "short")


def test_a_row_that_starts_past_4_gib_of_scores():
    """64-bit row addressing: the last of three rows starts past 2^32 bytes of ``pred`` (a row stride just above 2^29 floats in
    an uninitialised 4.3 GB buffer, only the rows' own entities filled); the same rows from a small tensor are the reference."""
    from ultra_torchdrug_amd import functional as UF
    c = CD.case("edges")
    t, sets = _inputs("edges")
    pick = torch.tensor([11, 6, 13], device=_dev())                              # the 2000-item list, the NaN target, every entity
    n, stride = c["n_node"], 2 ** 29 + 1024
    assert 2 * stride * 4 > 2 ** 32
    big = torch.empty(2 * stride + n, device=_dev())
    view = big.as_strided((3, n), (stride, 1))
    view.copy_(t["pred"][pick])
    args = [sets, t["set_of"][pick], 128, t["keys"], t["anchor"][pick], t["rel"][pick], c["n_rel"], t["target"][pick]]
    got = UF.candidate_select(view, *args)
    small = UF.candidate_select(t["pred"][pick], *args)
    _equal(got, small)
    want = CD.expected("edges", 128)
    _same(got, {key: value[pick.cpu().numpy()] for key, value in want.items()}, "past 4 GiB")
    del big, view


# ------------------------------------------------------------------------------------------------------------- task, engine
@pytest.fixture(scope="module")
def small():
    from ultra_torchdrug_amd import data
    graph = wide_graph()
    cpu, task = small_task(graph), small_task(graph)                            # the same seed: the same weights
    with torch.no_grad():
        for t in (cpu, task):
            t.model.mlp.layers[-1].weight.neg_()                                 # known completions lead the unfiltered lists
    task = task.to(_dev())
    triples = graph.edge_list.numpy()
    part = triples[(triples[:, 0] + triples[:, 1]) % 3 != 0]                     # some targets fall outside their set
    sets = data.relation_candidates(torch.from_numpy(part), 300, 5)
    lists = [sets.set(s).tolist() for s in range(10)]
    stray = next(e for e in range(300) if e not in lists[2])
    batch = torch.cat([wide_batch(graph), torch.tensor([[4, stray, 2]])])
    return {"graph": graph, "task": task, "cpu": cpu, "batch": batch, "stray": len(batch) - 1, "triples": triples, "sets": sets,
            "lists": lists}


@pytest.mark.parametrize("head", [False, True])
def test_task_answer_among_candidates_equals_masked_predict(small, head):
    task, batch, sets = small["task"], small["batch"], small["sets"]
    side = 1 if head else 0
    dev = _dev()
    with torch.no_grad():
        pred = task.predict(batch.to(dev))[:, side].cpu().numpy()
    anchor, rel = batch[:, side], batch[:, 2]
    lists = [np.array(l, dtype=np.int64) for l in small["lists"]]
    known = [set(completions(small["triples"], side, int(a), int(r)).tolist()) for a, r in zip(anchor, rel)]
    chosen = torch.tensor([(-1, 0, 7, 3)[q % 4] for q in range(len(batch))])
    for k, set_of in ((10, None), (128, None), (10, chosen)):
        entities, scores = task.answer(anchor.to(dev), rel.to(dev), k=k, head=head, candidates=sets,
                                       candidate_set=None if set_of is None else set_of.to(dev))
        want = CD.select(pred, lists, (rel + 5 * side).tolist() if set_of is None else set_of.tolist(), known, None, k)
        assert entities.is_cuda and np.array_equal(entities.cpu().numpy(), want["top_index"])
        # the all-entity score head of answer and predict's score agree on the order; the value is answer's own score
        assert same_bits(scores.cpu().numpy(), np.where(want["top_index"] >= 0, np.take_along_axis(
            pred, np.maximum(want["top_index"], 0), axis=1), np.float32("-inf")))


def _want_ranks(small, batch, pred):
    mask, target = small["cpu"].target(batch)
    in_set = torch.zeros(len(batch), 2, 300, dtype=torch.bool)
    for b, (h, t, r) in enumerate(batch.tolist()):
        in_set[b, 0, small["lists"][r]] = True
        in_set[b, 1, small["lists"][r + 5]] = True
    pos = pred.gather(-1, target.unsqueeze(-1))
    return (torch.sum((pos <= pred) & mask & in_set, dim=-1) + 1, in_set.gather(-1, target.unsqueeze(-1))[..., 0],
            (mask & in_set).sum(dim=-1))


def _metrics_hold(got, ranks, n_free):
    """The metrics of ``evaluate_constrained`` against exact rational means of the ranks inside (``ranks`` / ``n_free``: the
    members' only).  A mean is a fp64 sum of ``n`` terms of at most the largest term, divided once: every partial sum is off by
    at most half an ulp of it, so the result is within ``(n + 1) * 2^-53`` of the exact mean times the largest term."""
    from fractions import Fraction
    ranks, n_free = ranks.tolist(), n_free.tolist()
    n = len(ranks)
    want = {"mrr": (sum(Fraction(1, r) for r in ranks), 1), "mr": (sum(ranks), max(ranks)),
            "mean_candidates": (sum(n_free), max(n_free))}
    for top in (1, 3, 10):
        want["hits@%d" % top] = (sum(1 for r in ranks if r <= top), 1)
    for name, (total, largest) in want.items():
        assert abs(Fraction(got[name]) - Fraction(total) / n) <= Fraction(n + 1, 2 ** 53) * largest, name


def test_rank_among_and_evaluate_constrained(small):
    from ultra_torchdrug_amd import engine
    task, batch, sets, stray = small["task"], small["batch"], small["sets"], small["stray"]
    dev = _dev()
    with torch.no_grad():
        pred = task.predict(batch.to(dev))
    ranks, member, n_free = task.rank_among(batch.to(dev), sets, pred=pred)
    want = _want_ranks(small, batch, pred.cpu())
    assert ranks.is_cuda and member.dtype == torch.bool
    assert torch.equal(ranks.cpu(), want[0]) and torch.equal(member.cpu(), want[1]) and torch.equal(n_free.cpu(), want[2])
    assert not member[stray, 0] and member.any()
    _equal(task.rank_among(batch.to(dev), sets), (ranks, member, n_free))
    results = [engine.evaluate_constrained(task, batch, sets, batch_size=b) for b in (16, 3)]
    for got in results:
        assert got["outside"] == int((~want[1]).sum()) and got["outside"] >= 1
        assert torch.equal(got["ranks"].cpu(), torch.where(want[1], want[0], torch.zeros_like(want[0])))
        _metrics_hold(got, want[0][want[1]], want[2][want[1]])


def test_the_cpu_twin_of_the_task_gives_the_same_results(small):
    """The same ids, membership and counts from the CPU task; its ranks and answers are held to ITS OWN scores in
    tests/test_candidates_cpu.py (host and device matrix products round differently, so scores differ in their last bits)."""
    from ultra_torchdrug_amd import engine
    task, cpu, batch, sets = small["task"], small["cpu"], small["batch"], small["sets"]
    dev = _dev()
    on_dev, on_cpu = task.rank_among(batch.to(dev), sets), cpu.rank_among(batch, sets)
    assert torch.equal(on_dev[1].cpu(), on_cpu[1]) and torch.equal(on_dev[2].cpu(), on_cpu[2])
    a, b = engine.evaluate_constrained(task, batch, sets), engine.evaluate_constrained(cpu, batch, sets)
    assert a["outside"] == b["outside"] and a["mean_candidates"] == b["mean_candidates"]
    # the device scores through the CPU twin of the operator: the same words as the kernel
    with torch.no_grad():
        pred = task.predict(batch.to(dev)).cpu()
    twin = cpu.rank_among(batch, sets, pred=pred)
    _equal(tuple(x.cpu() for x in on_dev), twin)
    got = engine.answer(task, batch[:, 0].to(dev), batch[:, 2].to(dev), k=10, batch_size=2, candidates=sets)
    want = task.answer(batch[:, 0].to(dev), batch[:, 2].to(dev), k=10, candidates=sets)
    assert torch.equal(got[0], want[0])


def test_engine_answer_among_candidates_replays_the_fused_score_head():
    """A 64-wide model has the fused all-entity score head: ``engine.answer`` scores its chunks through one captured
    ``GraphedScores``, enqueues the selection on each and equals ``task.answer`` chunk for chunk, eager and replayed."""
    from ultra_torchdrug_amd import data, engine
    from ultra_torchdrug_amd.task import build_ultra
    dev = _dev()
    graph = wide_graph()
    torch.manual_seed(5)
    task = build_ultra(graph.num_relation, hidden_dims=(64,) * 2, rel_layers=2, num_negative=8, full_batch_eval=True)
    task.preprocess(graph)
    task = task.eval().to(dev)
    sets = data.relation_candidates(graph.edge_list[::3], 300, 5).to(dev)
    g = torch.Generator().manual_seed(4)
    anchor, relation = torch.randint(0, 300, (21,), generator=g).to(dev), torch.randint(0, 5, (21,), generator=g).to(dev)
    chosen = torch.randint(-1, 10, (21,), generator=g).to(dev)
    for head in (False, True):
        for set_of in (None, chosen):
            want = []
            for i in range(0, 21, 4):                                            # chunks of 4, the last one repeating its end
                ids = torch.arange(i, i + 4, device=dev).clamp(max=20)
                want.append(task.answer(anchor[ids], relation[ids], k=10, head=head, candidates=sets,
                                        candidate_set=None if set_of is None else set_of[ids]))
            want = torch.cat([w[0] for w in want])[:21], torch.cat([w[1] for w in want])[:21]
            for graphed in (False, True):
                got = engine.answer(task, anchor, relation, k=10, head=head, batch_size=2, graphed=graphed, candidates=sets,
                                    candidate_set=set_of)
                assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), (head, graphed)
            lists = [sets.set(s).tolist() for s in range(10)]
            for q in range(21):
                s = int(relation[q]) + 5 * head if set_of is None else int(set_of[q])
                assert s == -1 or set(want[0][q][want[0][q] >= 0].tolist()) <= set(lists[s])

"""No GPU: candidate sets on the host -- the builders of ``data`` against brute-force loops, ``functional.dense_candidate_select``
against the plain-Python definition (tests/candidate_definition.py) on the cases the device kernel is held to, and
``task.answer(candidates=...)`` / ``task.rank_among`` / ``engine.evaluate_constrained`` on a CPU task against masks built from the
scores of ``task.predict``.  Integers are compared exactly and values bit for bit."""
import numpy as np
import pytest
import torch

import candidate_definition as CD
from sampled_graphs import small_task, wide_batch, wide_graph
from topk_definition import completions, same_bits, topk_rows


def _same(got, want, what=None):
    for name in ("top_index", "rank", "n_free", "member"):
        if getattr(got, name) is not None:
            assert getattr(got, name).dtype == (torch.uint8 if name == "member" else torch.int64), name
            assert np.array_equal(getattr(got, name).cpu().numpy(), want[name]), (name, what)
    if got.top_value is not None:
        assert got.top_value.dtype == torch.float32 and same_bits(got.top_value.cpu().numpy(), want["top_value"]), what


def _sets_of(case, device="cpu"):
    from ultra_torchdrug_amd import data
    return data.candidate_sets(case["sets"], case["n_node"]).to(device)


# ------------------------------------------------------------------------------------------------------------- the builders
def test_relation_candidates_equals_a_loop_over_the_triples():
    from ultra_torchdrug_amd import data
    rng = np.random.default_rng(3)
    triples = np.stack([rng.integers(0, 40, 300), rng.integers(0, 40, 300), rng.choice([0, 1, 3, 4, 6], 300)], axis=1)
    triples = np.concatenate([triples, triples[:50]])                            # duplicates
    sets = data.relation_candidates(torch.from_numpy(triples), 40, 7)            # relations 2 and 5 have no triple
    tails, heads = [set() for _ in range(7)], [set() for _ in range(7)]
    for h, t, r in triples.tolist():
        tails[r].add(t)
        heads[r].add(h)
    want = [sorted(s) for s in tails + heads]
    assert sets.num_sets == 14 and len(sets) == 14 and sets.num_node == 40
    assert sets.ptr.dtype == torch.int64 and sets.items.dtype == torch.int32
    assert [sets.set(s).tolist() for s in range(14)] == want
    assert want[2] == [] and want[5] == [] and want[9] == [] and want[12] == []
    assert sets.max_len == max(len(w) for w in want) and isinstance(sets.max_len, int)
    assert sets.ptr.tolist() == np.concatenate([[0], np.cumsum([len(w) for w in want])]).tolist()
    none = data.relation_candidates(torch.zeros(0, 3, dtype=torch.int64), 40, 2)
    assert none.ptr.tolist() == [0] * 5 and none.items.numel() == 0 and none.max_len == 0
    for bad in ([[40, 0, 0]], [[0, -1, 0]], [[0, 0, 7]]):
        with pytest.raises(ValueError):
            data.relation_candidates(torch.tensor(bad), 40, 7)


def test_candidate_sets_sorts_deduplicates_and_rejects():
    from ultra_torchdrug_amd import data
    sets = data.candidate_sets([[9, 3, 3, 0, 9], [], torch.tensor([5, 4]), np.array([7], dtype=np.int32)], 10)
    assert [sets.set(s).tolist() for s in range(4)] == [[0, 3, 9], [], [4, 5], [7]]
    assert sets.ptr.tolist() == [0, 3, 3, 5, 6] and sets.max_len == 3 and sets.num_node == 10
    assert data.candidate_sets([], 10).ptr.tolist() == [0]
    for bad in ([[10]], [[0], [-1]], [[0.5]]):
        with pytest.raises(ValueError):
            data.candidate_sets(bad, 10)
    moved = sets.to("cpu")
    assert torch.equal(moved.ptr, sets.ptr) and torch.equal(moved.items, sets.items) and moved.max_len == 3


def test_the_constructor_validates_once():
    from ultra_torchdrug_amd import data
    i32 = lambda *x: torch.tensor(x, dtype=torch.int32)
    ok = data.CandidateSets(torch.tensor([0, 0, 2, 2, 3]), i32(3, 4, 0), 5)      # a set may start below the end of the one before
    assert ok.max_len == 2 and ok.num_sets == 4
    for ptr, items in (([0, 2], i32(1, 1)), ([0, 2], i32(2, 1)), ([0, 1], i32(5)), ([0, 1], i32(-1)), ([1, 2], i32(0, 1)),
                       ([0, 3], i32(0, 1)), ([0, 2, 1, 2], i32(0, 1)), ([0, 1], torch.tensor([0]))):
        with pytest.raises(ValueError):
            data.CandidateSets(torch.tensor(ptr), items, 5)
    with pytest.raises(ValueError):
        data.CandidateSets(torch.tensor([0, 1]), i32(0), 2 ** 31)


# ------------------------------------------------------------------------------------------------------------ the dense twin
@pytest.mark.parametrize("k", [1, 10, 128])
@pytest.mark.parametrize("name", list(CD.CASES))
def test_the_dense_twin_equals_the_definition(name, k):
    from ultra_torchdrug_amd import functional as UF
    c = CD.case(name)
    assert CD.tie_fraction(c) >= 0.2                                             # at least a fifth of the compared pairs tie
    t = {key: torch.from_numpy(c[key]) for key in ("pred", "set_of", "anchor", "rel", "target", "keys")}
    sets = _sets_of(c)
    got = UF.candidate_select(t["pred"], sets, t["set_of"], k, t["keys"], t["anchor"], t["rel"], c["n_rel"], t["target"],
                              max_len=c["max_len"])
    want = CD.expected(name, k)
    _same(got, want, (name, k))
    twin = UF.dense_candidate_select(t["pred"], sets, t["set_of"], k, t["keys"], t["anchor"], t["rel"], c["n_rel"], t["target"])
    _same(twin, want, (name, k, "default max_len"))
    if name == "edges":
        assert want["n_free"][3] == 0 and want["rank"][3] == 1 and (want["top_index"][3] == -1).all()
        assert np.isinf(want["top_value"][3]).all() and want["n_free"][1] <= 1 and want["member"].any() and not want["member"].all()
        raw = UF.candidate_select(t["pred"], sets, t["set_of"], k, None, None, None, 1, t["target"])
        _same(raw, CD.expected(name, k, filtered=False), "keys=None")
        every = UF.candidate_select(t["pred"], None, None, k, t["keys"], t["anchor"], t["rel"], c["n_rel"], None)
        _same(every, CD.expected(name, k, with_sets=False, with_target=False), "set_of=None, target=None")
        assert not every.rank.any() and not every.member.any()
        for outputs in (("rank",), ("n_free", "member"), ("top_value",)):
            part = UF.candidate_select(t["pred"], sets, t["set_of"], k, t["keys"], t["anchor"], t["rel"], c["n_rel"], t["target"],
                                       outputs=outputs)
            for o in CD.OUTPUTS:
                assert (getattr(part, o) is None) == (o not in outputs)
            _same(part, want, outputs)


def test_candidate_select_refuses_bad_arguments():
    from ultra_torchdrug_amd import data, functional as UF
    c = CD.case("edges")
    t = {key: torch.from_numpy(c[key]) for key in ("pred", "set_of", "anchor", "rel", "target", "keys")}
    sets = _sets_of(c)
    args = lambda **kw: dict(dict(pred=t["pred"], sets=sets, set_of=t["set_of"], k=10, keys=t["keys"], anchor=t["anchor"],
                                  rel=t["rel"], n_rel=3, target=t["target"]), **kw)
    UF.candidate_select(**args())
    for bad in (dict(k=0), dict(k=129), dict(pred=t["pred"].double()), dict(pred=t["pred"][:, ::2]), dict(set_of=t["set_of"].int()),
                dict(set_of=t["set_of"][:3]), dict(sets=None), dict(sets=data.candidate_sets(c["sets"], 3001)),
                dict(anchor=None), dict(n_rel=0), dict(target=t["target"][:2]), dict(outputs=()), dict(outputs=("known",)),
                dict(keys=t["keys"].int()), dict(max_len=-1)):
        with pytest.raises(RuntimeError):
            UF.candidate_select(**args(**bad))
    UF.candidate_select(**args(k=0, outputs=("rank",)))                          # k only counts when a top output is asked for


def test_binding_lists_the_entries_and_keeps_the_abi():
    from ultra_torchdrug_amd import _lib, _torch_ext, backend, functional as UF
    assert {"ultra_candidate_select_f32", "ultra_candidate_select_workspace"} <= set(_lib.EXPORTS) and _lib.ABI_VERSION == 8
    assert "candidate_select" in _torch_ext.OPS and backend.get().candidate_select is UF.candidate_select
    assert UF.CANDIDATE_OUTPUTS == CD.OUTPUTS and UF.CANDIDATE_SLICE == CD.SLICE


# ------------------------------------------------------------------------------------------------------------- task, engine
@pytest.fixture(scope="module")
def small():
    from ultra_torchdrug_amd import data
    graph = wide_graph()
    task = small_task(graph)
    with torch.no_grad():
        task.model.mlp.layers[-1].weight.neg_()                                  # known completions lead the unfiltered lists
    triples = graph.edge_list.numpy()
    # the type constraints come from PART of the graph, so that some test triples have a target outside its set
    part = triples[(triples[:, 0] + triples[:, 1]) % 3 != 0]
    sets = data.relation_candidates(torch.from_numpy(part), 300, 5)
    return {"graph": graph, "task": task, "batch": wide_batch(graph), "triples": triples, "sets": sets,
            "lists": [sets.set(s).tolist() for s in range(10)]}


def _want_answers(small, pred, anchor, set_of, side, k, filtered=True):
    known = [set(completions(small["triples"], side, int(a), int(r)).tolist()) if filtered else set()
             for a, r in zip(anchor[0], anchor[1])]
    return CD.select(pred, [np.array(l, dtype=np.int64) for l in small["lists"]], set_of, known, None, k)


@pytest.mark.parametrize("head", [False, True])
def test_task_answer_among_candidates_equals_masked_predict(small, head):
    task, batch, sets = small["task"], small["batch"], small["sets"]
    side = 1 if head else 0
    with torch.no_grad():
        pred = task.predict(batch)[:, side].numpy()
    anchor, rel = batch[:, side], batch[:, 2]
    q_rel = (rel + 5 * side).tolist()
    for k in (10, 128):
        entities, scores = task.answer(anchor, rel, k=k, head=head, candidates=sets)
        want = _want_answers(small, pred, (anchor.tolist(), rel.tolist()), q_rel, side, k)
        assert entities.dtype == torch.int64 and scores.dtype == torch.float32
        assert np.array_equal(entities.numpy(), want["top_index"]) and same_bits(scores.numpy(), want["top_value"])
        for q in range(len(batch)):
            assert set(entities[q][entities[q] >= 0].tolist()) <= set(small["lists"][q_rel[q]])
    chosen = torch.tensor([(-1, 0, 7, 3)[q % 4] for q in range(len(batch))])
    entities, scores = task.answer(anchor, rel, k=10, head=head, filtered=False, candidates=sets, candidate_set=chosen)
    want = _want_answers(small, pred, (anchor.tolist(), rel.tolist()), chosen.tolist(), side, 10, filtered=False)
    assert np.array_equal(entities.numpy(), want["top_index"]) and same_bits(scores.numpy(), want["top_value"])
    with_hops = task.answer(anchor, rel, k=10, head=head, candidates=sets, with_hops=True)
    assert len(with_hops) == 3 and with_hops[2].shape == (len(batch), 10)


def test_task_answer_checks_its_candidate_arguments(small):
    from ultra_torchdrug_amd import data
    task, sets = small["task"], small["sets"]
    a, r = torch.tensor([3, 4]), torch.tensor([0, 1])
    user = data.candidate_sets([[1, 2, 3], [250]], 300)
    got = task.answer(a, r, k=4, candidates=user, candidate_set=torch.tensor([1, 0]), filtered=False)
    assert got[0][0].tolist() == [250, -1, -1, -1] and sorted(got[0][1][:3].tolist()) == [1, 2, 3] and got[0][1, 3] == -1
    for kw in (dict(candidates=user), dict(candidate_set=torch.tensor([0, 0])), dict(candidates=user, candidate_set=torch.tensor([2, 0])),
               dict(candidates=user, candidate_set=torch.tensor([-2, 0])), dict(candidates=user, candidate_set=torch.tensor([0])),
               dict(candidates=data.candidate_sets([[1]], 299), candidate_set=torch.tensor([0, 0])),
               dict(candidates=[[1, 2]], candidate_set=torch.tensor([0, 0])), dict(candidates=sets, k=129)):
        with pytest.raises(ValueError):
            task.answer(a, r, **kw)
    empty = task.answer(a[:0], r[:0], k=3, candidates=sets)
    assert empty[0].shape == (0, 3) and empty[1].shape == (0, 3)


def test_without_candidates_answer_is_the_unconstrained_path(small):
    from ultra_torchdrug_amd import functional as UF
    task, graph, batch = small["task"], small["graph"], small["batch"]
    for head in (False, True):
        side = 1 if head else 0
        torch.manual_seed(7)
        first = task.answer(batch[:, side], batch[:, 2], k=10, head=head)
        torch.manual_seed(7)
        again = task.answer(batch[:, side], batch[:, 2], k=10, head=head, candidates=None, candidate_set=None)
        with torch.no_grad():
            pred = task.predict(batch)[:, side]
        value, index = UF.topk_keys(pred, 10, graph.completion_keys(side), batch[:, side], batch[:, 2], 5, 300)
        known = [completions(small["triples"], side, int(b[side]), int(b[2])) for b in batch]
        for got in (first, again):
            assert torch.equal(got[0], index) and same_bits(got[1].numpy(), value.numpy())
            assert np.array_equal(got[0].numpy(), topk_rows(pred.numpy(), 10, known)[0])


def _want_ranks(small, batch, pred):
    """``sum((pos <= pred) & mask & in_set) + 1``, membership and the candidate counts from dense masks."""
    task = small["task"]
    mask, target = task.target(batch)                                            # (B, 2, N) bool: not a known completion
    in_set = torch.zeros(len(batch), 2, 300, dtype=torch.bool)
    for b, (h, t, r) in enumerate(batch.tolist()):
        in_set[b, 0, small["lists"][r]] = True
        in_set[b, 1, small["lists"][r + 5]] = True
    pos = pred.gather(-1, target.unsqueeze(-1))
    ranks = torch.sum((pos <= pred) & mask & in_set, dim=-1) + 1
    return ranks, in_set.gather(-1, target.unsqueeze(-1))[..., 0], (mask & in_set).sum(dim=-1)


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


def _test_triples(small):
    """The batch of the other feature tests and one triple whose tail is not in its relation's range."""
    lists = small["lists"]
    stray = next(t for t in range(300) if t not in lists[2])
    batch = torch.cat([small["batch"], torch.tensor([[4, stray, 2]])])
    return batch, len(batch) - 1


def test_rank_among_equals_the_masked_count(small):
    task = small["task"]
    batch, stray = _test_triples(small)
    with torch.no_grad():
        pred = task.predict(batch)
    ranks, member, n_free = task.rank_among(batch, small["sets"])
    want = _want_ranks(small, batch, pred)
    assert ranks.dtype == torch.int64 and member.dtype == torch.bool and n_free.dtype == torch.int64
    assert torch.equal(ranks, want[0]) and torch.equal(member, want[1]) and torch.equal(n_free, want[2])
    assert not member[stray, 0] and ranks[stray, 0] >= 1 and not member.all() and member.any()
    again = task.rank_among(batch, small["sets"], pred=pred)
    assert all(torch.equal(x, y) for x, y in zip(again, (ranks, member, n_free)))
    assert (ranks <= task.rank_batch(batch, pred=pred)).all()                    # fewer candidates never rank a target lower


def test_evaluate_constrained_reports_the_metrics_of_those_ranks(small):
    from ultra_torchdrug_amd import engine
    task = small["task"]
    batch, stray = _test_triples(small)
    with torch.no_grad():
        ranks, member, n_free = _want_ranks(small, batch, task.predict(batch))
    got = engine.evaluate_constrained(task, batch, small["sets"], batch_size=len(batch))
    assert got["outside"] == int((~member).sum()) and got["outside"] >= 1 and member.any()
    assert torch.equal(got["ranks"], torch.where(member, ranks, torch.zeros_like(ranks))) and got["ranks"][stray, 0] == 0
    _metrics_hold(got, ranks[member], n_free[member])
    # in chunks: the same sides are outside, and a rank moves only where the host matrix products, which block their sums by the
    # batch shape, reorder two scores -- every triple alone is held to its own predict
    for i in (0, stray):
        alone = engine.evaluate_constrained(task, batch[i:i + 1], small["sets"], batch_size=3)
        with torch.no_grad():
            want = _want_ranks(small, batch[i:i + 1], task.predict(batch[i:i + 1]))
        assert torch.equal(alone["ranks"], torch.where(want[1], want[0], torch.zeros_like(want[0])))
    chunks = engine.evaluate_constrained(task, batch, small["sets"], batch_size=3)
    assert chunks["outside"] == got["outside"] and torch.equal(chunks["ranks"] > 0, got["ranks"] > 0)
    none = engine.evaluate_constrained(task, batch[:0], small["sets"])
    assert none["outside"] == 0 and none["ranks"].shape == (0, 2) and none["mrr"] != none["mrr"]
    with pytest.raises(ValueError):
        engine.evaluate_constrained(task, torch.tensor([[0, 300, 0]]), small["sets"])


def test_engine_answer_passes_the_candidates_through_its_chunks(small):
    from ultra_torchdrug_amd import engine
    task, sets = small["task"], small["sets"]
    g = torch.Generator().manual_seed(3)
    anchor, relation = torch.randint(0, 300, (37,), generator=g), torch.randint(0, 5, (37,), generator=g)
    chosen = torch.randint(-1, 10, (37,), generator=g)
    for head in (False, True):
        for kw in (dict(candidates=sets), dict(candidates=sets, candidate_set=chosen)):
            got = engine.answer(task, anchor, relation, k=10, head=head, batch_size=8, **kw)
            chunks = [task.answer(anchor[i:i + 16], relation[i:i + 16], k=10, head=head, candidates=sets,
                                  candidate_set=None if "candidate_set" not in kw else chosen[i:i + 16]) for i in range(0, 37, 16)]
            assert got[0].shape == (37, 10) and torch.equal(got[0], torch.cat([c[0] for c in chunks]))
            assert same_bits(got[1].numpy(), torch.cat([c[1] for c in chunks]).numpy())
    with pytest.raises(ValueError):
        engine.answer(task, anchor, relation, candidate_set=chosen)
    with pytest.raises(ValueError):
        engine.answer(task, anchor, relation, candidates=sets, candidate_set=chosen + 10)

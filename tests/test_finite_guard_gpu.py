"""MI355X: the divergence guard -- ``ultra_nonfinite_scan_f32`` / ``ultra_nonfinite_commit`` on their own, and
``engine.FiniteGuard`` inside captured training steps (one graph, the after and the phased modes with a one-rank RCCL group, one
guard shared by the captured steps of two graphs, ``poll_every``).  S-tiny, 16 negatives, batches of 8."""
import copy

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

C = 4096                # fp32 elements per block of the scan kernel (ultra_nonfinite_scan_chunk)
T = 32                  # tensors per launch (ultra_nonfinite_scan_tensors)
WEIGHT = "model.layers.0.linear.weight"
INF, NAN = float("inf"), float("nan")


def _dev():
    return torch.device("cuda:0")


def _from_bits(words):
    return torch.from_numpy(np.asarray(words, dtype=np.uint32).view(np.float32))


def _pending(tensors, first_index=0):
    from ultra_torchdrug_amd import functional as UF
    record = UF.nonfinite_record(_dev())
    UF.nonfinite_scan(tensors, record, first_index=first_index)
    step, tripped, tensor, pending = record.tolist()
    assert (step, tripped, tensor) == (0, -1, -1)               # a scan writes `pending` and nothing else
    return pending


def test_scan_kernel_sizes_positions_views_and_bit_patterns():
    from ultra_torchdrug_amd import _lib, functional as UF
    lib = _lib.load()
    assert lib.ultra_nonfinite_scan_chunk() == C and lib.ultra_nonfinite_scan_tensors() == T
    dev, clean = _dev(), UF.GUARD_CLEAN
    bad_words = [0x7f800000, 0xff800000, 0x7fc00000, 0xffc00000, 0x7f800001, 0xffbfffff]       # +-inf, NaNs of both signs
    fine_words = [0x00000001, 0x807fffff, 0x7f7fffff, 0xff7fffff, 0x80000000]                  # denormals, +-FLT_MAX, -0.0
    for n in (0, 1, C - 1, C, C + 1, 2 * C + 5):
        base = np.full(n, 0x3f800000, dtype=np.uint32)
        assert _pending([_from_bits(base).to(dev)], 3) == clean, n
        for at in sorted({0, n - 1} if n else ()):
            for word in bad_words:
                words = base.copy()
                words[at] = word
                assert _pending([_from_bits(words).to(dev)], 3) == 3, (n, at, hex(word))
            words = base.copy()
            words[at] = fine_words[(n + at) % len(fine_words)]
            assert _pending([_from_bits(words).to(dev)], 3) == clean, (n, at)
    assert _pending([_from_bits(fine_words * 3).to(dev)]) == clean
    # views that start 1, 2 and 3 elements into an allocation: only the view's own elements count, all of them do
    for n in (C + 3, 9):
        for offset in (1, 2, 3):
            for at, want in ((offset - 1, clean), (offset, 0), (n - 1, 0), (n // 2, 0)):
                whole = torch.ones(n)
                whole[at] = NAN if at % 2 else -INF
                whole = whole.to(dev)
                view = whole[offset:]
                assert view.data_ptr() % 16 == 4 * offset and _pending([view]) == want, (n, offset, at)
    # against numpy on random bit patterns: 45 tensors of odd sizes (two launches), some empty, some views
    rng = np.random.default_rng(11)
    words = []
    for i in range(45):
        w = rng.integers(0, 2 ** 32, size=int(rng.integers(0, 3 * C)) if i % 5 else 0, dtype=np.uint64).astype(np.uint32)
        if i < 20 or i % 2:
            w &= np.uint32(0xbfffffff)                         # exponent bits not all ones: finite
        words.append(w)
    bad = [i for i, w in enumerate(words) if ((w & np.uint32(0x7f800000)) == np.uint32(0x7f800000)).any()]
    assert bad and bad[0] >= 20
    tensors = [_from_bits(np.concatenate([[0xffffffff], w]).astype(np.uint32)).to(dev)[1:] for w in words]     # (a NaN in front of each view)
    assert _pending(tensors, 7) == 7 + bad[0]


def test_scan_lists_longer_than_a_launch_two_bad_tensors_and_refusals():
    from ultra_torchdrug_amd import functional as UF
    dev, clean = _dev(), UF.GUARD_CLEAN
    good = [torch.full((5 + i,), float(i), device=dev) for i in range(T + 1)]
    assert _pending(good) == clean and _pending([]) == clean
    last = list(good)
    last[T] = torch.tensor([1.0, INF, 2.0], device=dev)                             # the one tensor of the second launch
    assert _pending(last, 2) == 2 + T
    two = list(last)
    two[9] = torch.tensor([NAN], device=dev)
    assert _pending(two, 2) == 2 + 9                                                # the lower index wins, across launches ...
    two[4], two[9] = None, torch.zeros(0, device=dev)                               # (None / empty: skipped, indices kept)
    two[11] = torch.tensor([-INF], device=dev)
    two[30] = torch.tensor([NAN], device=dev)
    assert _pending(two, 2) == 2 + 11                                               # ... and inside one
    record = UF.nonfinite_record(dev)
    for bad in (torch.zeros(3, dtype=torch.float64, device=dev), torch.zeros(3, dtype=torch.bfloat16, device=dev),
                torch.zeros(3, dtype=torch.int32, device=dev)):
        with pytest.raises(RuntimeError, match="fp32"):
            UF.nonfinite_scan([good[0], bad], record)
    with pytest.raises(RuntimeError, match="on cpu"):
        UF.nonfinite_scan([torch.zeros(3)], record)
    with pytest.raises(RuntimeError, match="contiguous"):
        UF.nonfinite_scan([torch.zeros(4, 4, device=dev).t()], record)
    assert record.tolist() == [0, -1, -1, clean]
    # the record on the device: commit latches, counts, stays sticky
    UF.nonfinite_scan(two, record, first_index=2)
    UF.nonfinite_commit(record, advance=False)
    assert record.tolist() == [0, 1, 13, clean]
    UF.nonfinite_scan([two[11]], record, first_index=0)
    UF.nonfinite_commit(record)
    assert record.tolist() == [1, 1, 13, clean]
    UF.nonfinite_commit(record)
    assert record.tolist() == [2, 1, 13, clean]


# ------------------------------------------------------------------------------------------------ captured steps
def _build(seed=1024):
    from ultra_torchdrug_amd.data import synthetic_triples
    from ultra_torchdrug_amd.graph import Graph
    from ultra_torchdrug_amd.task import build_ultra
    triples, n, r = synthetic_triples("S-tiny", seed)
    torch.manual_seed(seed)
    task = build_ultra(r)
    task.preprocess(Graph(torch.from_numpy(triples), num_node=n, num_relation=r))
    task.num_negative = 16
    return task.to(_dev()).train(), triples


def _batches(triples, n=5):
    return [torch.from_numpy(triples[8 * i:8 * i + 8]).to(_dev()) for i in range(n)]


def _bits_of(task):
    return {k: p.detach().view(torch.int32).clone() for k, p in task.named_parameters()}


def _same_optimizer_state(optimizer, state):
    now = optimizer.state_dict()
    assert set(now["state"]) == set(state["state"])
    for key, slot in state["state"].items():
        for name, value in slot.items():
            assert torch.equal(now["state"][key][name], value), (key, name)


def _poison(task, value=INF):
    with torch.no_grad():
        weight = dict(task.named_parameters())[WEIGHT]
        saved = weight[1, 5].clone()
        weight[1, 5] = value
    return saved


def _restore(task, saved):
    with torch.no_grad():
        dict(task.named_parameters())[WEIGHT][1, 5] = saved


def _trips_on_the_weight(task, optimizer, call, guard, batch, want_step):
    """Poison the weight, call: NonFiniteError(parameter, WEIGHT, want_step), twice; nothing was touched.  Restores the weight
    and resets the guard."""
    from ultra_torchdrug_amd import engine
    saved = _poison(task)
    before, state = _bits_of(task), copy.deepcopy(optimizer.state_dict())
    for _ in range(2):
        with pytest.raises(engine.NonFiniteError) as caught:
            call(batch)
        assert (caught.value.step, caught.value.kind, caught.value.name) == (want_step, "parameter", WEIGHT)
    torch.cuda.synchronize()
    after = _bits_of(task)
    assert all(torch.equal(before[k], after[k]) for k in before)
    _same_optimizer_state(optimizer, state)
    assert guard.tripped
    guard.reset()
    _restore(task, saved)
    assert not guard.tripped


def test_guarded_captured_steps_equal_unguarded_ones():
    from ultra_torchdrug_amd import engine, functional as UF
    task, triples = _build()
    twin = copy.deepcopy(task)
    batches = _batches(triples, 4)
    runs = []
    for model, guarded in ((task, False), (twin, True)):
        optimizer = torch.optim.AdamW(model.parameters(), lr=1e-3)
        guard = engine.FiniteGuard(model) if guarded else None
        step = engine.GraphedTrainStep(model, optimizer, batches[0], guard=guard)
        assert step.mode == "single"
        if guarded:
            assert guard.record.tolist() == [0, -1, -1, UF.GUARD_CLEAN]             # the captures left no step behind
        losses = []
        for b in batches[1:]:
            torch.manual_seed(int(b[0, 0]))
            losses.append(step(b)[0].item())
        runs.append(losses)
        if guarded:
            assert guard.record.tolist() == [3, -1, -1, UF.GUARD_CLEAN] and guard.calls == 3
    assert runs[0] == runs[1] and all(np.isfinite(runs[0]))
    for (k, a), (_, b) in zip(task.named_parameters(), twin.named_parameters()):
        assert torch.equal(a, b), k


def test_parameter_trip_in_a_captured_step_then_reset_and_continue_like_eager():
    from ultra_torchdrug_amd import engine
    twin, triples = _build()
    batches = _batches(triples, 5)
    optimizer = torch.optim.AdamW(twin.parameters(), lr=1e-3)
    guard = engine.FiniteGuard(twin)
    step = engine.GraphedTrainStep(twin, optimizer, batches[0], guard=guard)
    for b in batches[:2]:
        step(b)
    _trips_on_the_weight(twin, optimizer, step, guard, batches[2], want_step=3)
    # from here on: the captured guarded steps against eager unguarded ones from the same state
    task, _ = _build()
    task.load_state_dict(copy.deepcopy(twin.state_dict()))
    opt_e = torch.optim.AdamW(task.parameters(), lr=1e-3)
    opt_e.load_state_dict(copy.deepcopy(optimizer.state_dict()))
    for b in batches[2:]:
        loss_g = step(b)[0].item()
        task._static_negative = step.last_negatives.clone()
        loss_e = engine.train_step(task, opt_e, b)[0].item()
        task._static_negative = None
        assert loss_g == loss_e and np.isfinite(loss_g)
    for (k, a), (_, b) in zip(task.named_parameters(), twin.named_parameters()):
        assert torch.equal(a, b), k
    assert guard.record.tolist()[:2] == [6, -1]                                     # 2 good + 1 bad + 3 good steps


def test_loss_trip_with_finite_parameters():
    from ultra_torchdrug_amd import engine
    twin, triples = _build()
    batches = _batches(triples, 3)
    optimizer = torch.optim.AdamW(twin.parameters(), lr=1e-3)
    guard = engine.FiniteGuard(twin)
    step = engine.GraphedTrainStep(twin, optimizer, batches[0], guard=guard)
    step(batches[0])
    head = [k for k, _ in twin.named_parameters() if k.startswith("model.mlp.") and k.endswith(".weight")][-1]
    with torch.no_grad():
        dict(twin.named_parameters())[head].fill_(3e38)                             # finite, and the scores overflow
    # the precondition, on an unguarded eager step of a copy: a non-finite loss out of finite parameters
    probe, _ = _build()
    probe.load_state_dict(copy.deepcopy(twin.state_dict()))
    assert all(bool(torch.isfinite(p).all()) for p in probe.parameters())
    loss, _ = probe(batches[1])
    assert not bool(torch.isfinite(loss))
    before = _bits_of(twin)
    with pytest.raises(engine.NonFiniteError) as caught:
        step(batches[1])
    assert (caught.value.step, caught.value.kind, caught.value.name) == (2, "loss", "loss")
    after = _bits_of(twin)
    assert all(torch.equal(before[k], after[k]) for k in before)


def test_poll_every_third_call_names_the_first_bad_step():
    from ultra_torchdrug_amd import engine
    twin, triples = _build()
    batches = _batches(triples, 4)
    optimizer = torch.optim.AdamW(twin.parameters(), lr=1e-3)
    guard = engine.FiniteGuard(twin, poll_every=3)
    step = engine.GraphedTrainStep(twin, optimizer, batches[0], guard=guard)
    step(batches[0])                                                                # call 1
    _poison(twin)
    step(batches[1])                                                                # call 2: bad, not polled, applied
    with pytest.raises(engine.NonFiniteError) as caught:
        step(batches[2])                                                            # call 3: the poll
    assert (caught.value.step, caught.value.kind, caught.value.name) == (2, "parameter", WEIGHT)
    assert guard.calls == 3
    with pytest.raises(engine.NonFiniteError):
        step(batches[3])
    assert guard.calls == 3                                                         # a tripped guard runs nothing


@pytest.mark.parametrize("mode", ["phased", "after"])
def test_parameter_trip_in_a_captured_step_of_a_one_rank_group(mode):
    import os
    import torch.distributed as dist
    from ultra_torchdrug_amd import engine
    assert not dist.is_initialized()
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    port = 29537 + (mode == "after")
    dist.init_process_group("nccl", init_method="tcp://127.0.0.1:%d" % port, rank=0, world_size=1, device_id=_dev())
    try:
        twin, triples = _build()
        batches = _batches(triples, 4)
        optimizer = torch.optim.AdamW(twin.parameters(), lr=1e-3)
        reducer = engine.GradientReducer(twin, overlap=True, single_rank=True)
        guard = engine.FiniteGuard(twin)
        step = engine.GraphedTrainStep(twin, optimizer, batches[0], reducer=reducer, phased=(mode == "phased"), guard=guard)
        assert step.mode == mode                                                # (phased: _verify_phases passed with the guard)
        step(batches[0])
        rounds = reducer.rounds
        _trips_on_the_weight(twin, optimizer, step, guard, batches[1], want_step=2)
        assert reducer.rounds == rounds + 1                                     # the bad step's buckets went out and were retired
        # ... and the steps go on, equal to eager steps on the replays' negatives
        task, _ = _build()
        task.load_state_dict(copy.deepcopy(twin.state_dict()))
        opt_e = torch.optim.AdamW(task.parameters(), lr=1e-3)
        opt_e.load_state_dict(copy.deepcopy(optimizer.state_dict()))
        for b in batches[2:]:
            loss_g = step(b)[0].item()
            task._static_negative = step.last_negatives.clone()
            loss_e = engine.train_step(task, opt_e, b)[0].item()
            task._static_negative = None
            assert loss_g == loss_e
        for (k, a), (_, b) in zip(task.named_parameters(), twin.named_parameters()):
            assert torch.equal(a, b), (mode, k)
        reducer.remove_hooks()
        with pytest.raises(ValueError, match="reduce_in_graph"):
            engine.GraphedTrainStep(twin, optimizer, batches[0], reducer=reducer, reduce_in_graph=True, guard=guard)
    finally:
        dist.destroy_process_group()


def test_one_guard_shared_by_the_captured_steps_of_two_graphs():
    from ultra_torchdrug_amd import engine
    from ultra_torchdrug_amd.data import synthetic_triples
    from ultra_torchdrug_amd.graph import Graph
    twin, triples = _build()
    other, n2, r2 = synthetic_triples((200, 1500, 5), 11)
    twin.add_context("second", Graph(torch.from_numpy(other), num_node=n2, num_relation=r2))
    twin.to(_dev()).train()
    pools = {"default": torch.from_numpy(triples).to(_dev()), "second": torch.from_numpy(other).to(_dev())}
    optimizer = torch.optim.AdamW(twin.parameters(), lr=1e-3)
    guard = engine.FiniteGuard(twin)
    graphed = engine.GraphedMultiGraphTrainStep(twin, optimizer, 8, guard=guard)
    assert set(graphed.steps) == {"default", "second"} and all(s.guard is guard for s in graphed.steps.values())
    assert guard.record.tolist()[0] == 0
    graphed((pools["default"][:8], "default"))
    graphed((pools["second"][:8], "second"))
    graphed((pools["second"][8:13], "second"))                                      # ragged: the eager step, the same guard
    assert guard.record.tolist()[:2] == [3, -1]
    call = lambda batch: graphed((batch, "second"))
    _trips_on_the_weight(twin, optimizer, call, guard, pools["second"][16:24], want_step=4)
    saved = _poison(twin)
    with pytest.raises(engine.NonFiniteError) as caught:                            # the other graph's capture, the same record
        graphed((pools["default"][8:16], "default"))
    assert (caught.value.step, caught.value.kind, caught.value.name) == (5, "parameter", WEIGHT)
    guard.reset()
    _restore(twin, saved)
    loss, _ = graphed((pools["default"][8:16], "default"))
    assert bool(torch.isfinite(loss)) and guard.record.tolist()[:2] == [6, -1]

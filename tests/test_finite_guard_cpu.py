"""The divergence guard without a GPU: the dense path of ``functional.nonfinite_scan`` against the bit-pattern definition, the
record's semantics, ``engine.train_step(guard=)`` on CPU tensors (the rspmm operator is played by the CPU oracle, test
infrastructure), and two gloo ranks of which one is poisoned."""
import copy
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle_ops import oracle_rspmm

HERE = os.path.dirname(os.path.abspath(__file__))
WEIGHT = "model.layers.0.linear.weight"


def _bits(*words):
    return torch.from_numpy(np.array(words, dtype=np.uint32).view(np.float32))


# (bit pattern, non-finite?): exponent bits all ones <=> non-finite
PATTERNS = [
    (0x7f800000, True), (0xff800000, True),                         # +inf, -inf
    (0x7fc00000, True), (0xffc00000, True),                         # quiet NaN of both signs
    (0x7f800001, True), (0xff800001, True), (0x7fffffff, True), (0xffbfffff, True),    # signalling NaNs, other payloads
    (0x00000001, False), (0x807fffff, False), (0x00400000, False),  # denormals
    (0x7f7fffff, False), (0xff7fffff, False),                       # +-FLT_MAX
    (0x80000000, False), (0x00000000, False), (0x3f800000, False),  # -0.0, 0.0, 1.0
]


def _numpy_definition(array):
    return bool(((array.view(np.uint32) & np.uint32(0x7f800000)) == np.uint32(0x7f800000)).any())


def test_dense_scan_equals_the_bit_pattern_definition():
    from ultra_torchdrug_amd import functional as UF
    for word, bad in PATTERNS:
        assert _numpy_definition(np.array([word], dtype=np.uint32)) == bad
        for n, at in ((1, 0), (7, 0), (7, 6), (7, 3)):
            t = _bits(*[word if i == at else 0x3f800000 for i in range(n)])
            record = UF.nonfinite_record(torch.device("cpu"))
            UF.nonfinite_scan([torch.zeros(3), t, torch.zeros(0)], record, first_index=5)
            assert record.tolist() == [0, -1, -1, 6 if bad else UF.GUARD_CLEAN], (hex(word), n, at)
    # random bit patterns, tensor by tensor, against numpy
    rng = np.random.default_rng(5)
    tensors = []
    for i in range(40):
        words = rng.integers(0, 2 ** 32, size=int(rng.integers(0, 40)), dtype=np.uint64).astype(np.uint32)
        if i % 3:
            words &= np.uint32(0xbfffffff)                                          # exponent below 2^0: finite
        tensors.append(words)
    for i in (17, 30):                                                              # two that are bad for certain
        tensors[i] = np.concatenate([tensors[i], np.array([0xff800123], dtype=np.uint32)])
    want = [i for i, w in enumerate(tensors) if _numpy_definition(w)]
    assert len(want) >= 2
    record = UF.nonfinite_record(torch.device("cpu"))
    UF.nonfinite_scan([torch.from_numpy(w.view(np.float32)) for w in tensors], record, first_index=2)
    assert record[UF.GUARD_PENDING].item() == 2 + want[0]
    with pytest.raises(RuntimeError, match="fp32"):
        UF.nonfinite_scan([torch.zeros(3, dtype=torch.float64)], record)
    with pytest.raises(RuntimeError, match="fp32"):
        UF.nonfinite_scan([torch.zeros(3, dtype=torch.int32)], record)
    with pytest.raises(RuntimeError, match="record"):
        UF.nonfinite_scan([torch.zeros(3)], torch.zeros(4, dtype=torch.int64))


def test_record_semantics_lowest_index_sticky_trip_step_count_and_reset():
    from ultra_torchdrug_amd import engine, functional as UF
    inf, nan = float("inf"), float("nan")
    record = UF.nonfinite_record(torch.device("cpu"))
    good, bad_a, bad_b = torch.ones(5), torch.tensor([1.0, nan]), torch.tensor([-inf])
    UF.nonfinite_scan([good, good], record)
    UF.nonfinite_commit(record)
    assert record.tolist() == [1, -1, -1, UF.GUARD_CLEAN]                          # a clean step: only counted
    UF.nonfinite_scan([good, None, bad_b], record, first_index=10)                  # a None entry keeps its index
    UF.nonfinite_scan([good, bad_a, good, bad_b], record, first_index=3)            # two bad tensors, 4 and 6, after index 12
    assert record.tolist() == [1, -1, -1, 4]                                        # the lowest index, whatever the order
    UF.nonfinite_commit(record)
    assert record.tolist() == [2, 2, 4, UF.GUARD_CLEAN]                             # tripped in step 2, by tensor 4
    UF.nonfinite_scan([bad_a], record, first_index=0)
    UF.nonfinite_commit(record)
    assert record.tolist() == [3, 2, 4, UF.GUARD_CLEAN]                             # sticky: the first trip stays
    # a latch in the middle of a step: what was scanned before it is reported ahead of a lower index scanned after it
    record = UF.nonfinite_record(torch.device("cpu"), step=7)
    UF.nonfinite_scan([bad_a], record, first_index=9)
    UF.nonfinite_commit(record, advance=False)
    assert record.tolist() == [7, 8, 9, UF.GUARD_CLEAN]
    UF.nonfinite_scan([bad_a], record, first_index=0)
    UF.nonfinite_commit(record)
    assert record.tolist() == [8, 8, 9, UF.GUARD_CLEAN]

    # the guard's own record, names and reset()
    model = torch.nn.Linear(3, 2)
    guard = engine.FiniteGuard(model)
    assert guard.names == ["loss", "parameter weight", "parameter bias", "gradient weight", "gradient bias"]
    model.bias.grad = torch.tensor([0.0, nan])                                      # `weight` has no gradient: skipped, index kept
    guard.scan_parameters()
    guard.scan_loss(torch.tensor(1.0))
    guard.scan_gradients()
    guard.commit()
    assert not guard.tripped                                                        # nothing has been read yet
    with pytest.raises(engine.NonFiniteError) as caught:
        guard.check()
    assert (caught.value.step, caught.value.kind, caught.value.name) == (1, "gradient", "bias") and guard.tripped
    assert isinstance(caught.value, FloatingPointError)
    with pytest.raises(engine.NonFiniteError):
        guard.check()
    guard.reset()
    assert not guard.tripped and guard.record.tolist() == [1, -1, -1, UF.GUARD_CLEAN]
    guard.check()
    with pytest.raises(ValueError):
        engine.FiniteGuard(model, poll_every=0)


def _build():
    from ultra_torchdrug_amd.data import synthetic_triples
    from ultra_torchdrug_amd.graph import Graph
    from ultra_torchdrug_amd.task import build_ultra
    triples, n, r = synthetic_triples("S-tiny", 1024)
    torch.manual_seed(1024)
    task = build_ultra(r)
    task.preprocess(Graph(torch.from_numpy(triples), num_node=n, num_relation=r))
    task.num_negative = 16
    return task.train(), torch.from_numpy(triples)


def _bits_of(task):
    return {k: p.detach().view(torch.int32).clone() for k, p in task.named_parameters()}


def test_cpu_train_step_raises_at_the_step_that_finds_an_infinite_weight_and_touches_nothing():
    from ultra_torchdrug_amd import engine
    task, triples = _build()
    optimizer = torch.optim.AdamW(task.parameters(), lr=1e-3)
    guard = engine.FiniteGuard(task)
    names = [k for k, _ in task.named_parameters()]
    assert guard.names == ["loss"] + ["parameter " + k for k in names] + ["gradient " + k for k in names]
    with oracle_rspmm(0):
        for s in range(2):
            loss, _ = engine.train_step(task, optimizer, triples[8 * s:8 * s + 8], guard=guard)
            assert torch.isfinite(loss)
        assert guard.record.tolist()[:2] == [2, -1] and not guard.tripped
        with torch.no_grad():
            dict(task.named_parameters())[WEIGHT][1, 5] = float("inf")
        before, state = _bits_of(task), copy.deepcopy(optimizer.state_dict())
        for _ in range(2):                                                          # ... and every later call raises again
            with pytest.raises(engine.NonFiniteError) as caught:
                engine.train_step(task, optimizer, triples[16:24], guard=guard)
            assert (caught.value.step, caught.value.kind, caught.value.name) == (3, "parameter", WEIGHT)
    after = _bits_of(task)
    assert all(torch.equal(before[k], after[k]) for k in before)
    now = optimizer.state_dict()
    assert now["param_groups"] == state["param_groups"] and set(now["state"]) == set(state["state"])
    for key, slot in state["state"].items():
        for name, value in slot.items():
            assert torch.equal(now["state"][key][name], value), (key, name)


def test_two_gloo_ranks_raise_at_the_same_call_when_one_of_them_is_poisoned():
    child = os.path.join(HERE, "finite_guard_ranks_child.py")
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    procs = [subprocess.Popen([sys.executable, child, str(r), "2", str(port)], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                              text=True) for r in range(2)]
    reports = []
    try:
        for proc in procs:
            out, err = proc.communicate(timeout=300)
            lines = [line for line in out.splitlines() if line.startswith("{")]
            assert proc.returncode == 0 and lines, err[-2000:]
            reports.append(json.loads(lines[-1]))
    finally:
        for proc in procs:
            if proc.poll() is None:
                proc.kill()
    r0, r1 = sorted(reports, key=lambda r: r["rank"])
    assert r0["raised_at"] == r1["raised_at"] == 3 and r0["steps_done"] == r1["steps_done"] == 2
    assert (r1["kind"], r1["name"], r1["step"]) == ("parameter", WEIGHT, 3)         # the poisoned rank names its tensor
    assert (r0["kind"], r0["name"], r0["step"]) == (None, None, 3)                  # the other one learnt it from the flag
    assert r0["raises_again"] and r1["raises_again"]
    assert r0["local_only_passes"] and not r1["local_only_passes"]                  # communicate=False: each rank for itself
    assert r0["barrier"] and r1["barrier"]                                          # the collective sequences stayed equal

"""The HIP path, held to RECORDED RUNS OF THE REFERENCE'S OWN PYTHON (``tests/golden/reference_*.npz``; made by
``oracle/reference_record.py``; see ``tests/test_reference_fixtures_cpu.py`` for what the recordings are).  Reads ``tests/golden/``
only.

Bound of every comparison: ``max|X - truth| <= 4 * ref_dev + floor * scale``; ``truth`` is the reference's float64 run where it has
one, else its float32 run; ``ref_dev`` and ``scale`` are measured on the reference alone (``reference_fixtures.json``).  The factor
4: the kernels sum in yet another order and contract nothing, the reference's Linear runs through a BLAS.  ``FLOORS``: measured
once on an MI355X -- the largest observed ``max|X - truth| / scale`` of each group of quantities, doubled -- and never above what
the suite grants the same quantities against its own float64 path (``tests/test_reference_definition_gpu.py``): 2e-5 for
activations and scores, 5e-4 for gradients.  The measured values are in ``reference_fixtures.json`` under ``mi355x``.

Where the recorded branch of the reference (``message`` + ``aggregate``) and the rspmm branch the kernels mirror are different
functions, the comparison says so: max / min see a duplicate triple as two messages there and as one edge of summed weight here
(that output row is left out, and the gradients are those of the second recorded run, whose upstream is zero at that row); PNA
over TransE squares the operands in the rspmm branch (``ultra/layer.py:367``) and the message in the recorded one (``:283``): its
statistics are held, not its output."""
import numpy as np
import pytest
import torch

import reference_fixture as RF
import reference_runs as RR

pytestmark = pytest.mark.gpu

CAP_ACTIVATION, CAP_GRADIENT = 2e-5, 5e-4
FLOORS = {                           # observed on the MI355X -> doubled
    "layer_output": 7e-7,            # 3.27e-7
    "layer_gradient": 1.5e-6,        # 7.47e-7
    "entity_hidden": 8e-7,           # 3.51e-7
    "entity_score": 1.1e-6,          # 5.49e-7
    "task_relation": 1.4e-6,         # 6.69e-7
    "task_predict": 1.4e-6,          # 6.50e-7
    "task_loss": 5e-7,               # 2.16e-7
    "task_gradient": 2.4e-6,         # 1.17e-6
    # not against a recording: the HIP route against the materialised route on the device, both float32 sums of up to 81 terms in
    # two orders (n * 2^-24 of the sum of |terms|, a few times the largest entry): the activations' cap
    "pna_statistic": 2e-5,
}
WIDE = dict(wide_ids=True, piece_len=512)
NOT_DUPLICATE = [i for i in range(RF.LAYER_NODES) if i != RF.LAYER_DUPLICATE_ROW]


def _dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def _check(group, name, key, got, rows=None):
    assert FLOORS[group] <= (CAP_GRADIENT if group.endswith("gradient") else CAP_ACTIVATION)
    err, scale, ref_dev = RR.deviation(name, key, got, rows)
    print("%-14s %-60s %.3e of scale (reference's own %.3e)" % (group, key, err / scale, ref_dev / scale))
    assert err <= 4 * ref_dev + FLOORS[group] * scale, \
        "%s: %.3g from the reference's run (its own deviation %.3g, scale %.3g, floor %.1e)" % (key, err, ref_dev, scale, FLOORS[group])


class _knob:
    """``ultra_rspmm_force_general_path(bits)`` for the duration, reset on exit."""

    def __init__(self, bits):
        self.bits = bits

    def __enter__(self):
        from ultra_torchdrug_amd import _lib
        self.lib = _lib.load()
        self.lib.ultra_rspmm_force_general_path(self.bits)

    def __exit__(self, *exc):
        self.lib.ultra_rspmm_force_general_path(0)


class _fast_inference:
    def __init__(self, on):
        self.on = on

    def __enter__(self):
        from ultra_torchdrug_amd import functional as UF
        self.UF, self.saved = UF, UF.FAST_INFERENCE
        UF.FAST_INFERENCE = self.on

    def __exit__(self, *exc):
        self.UF.FAST_INFERENCE = self.saved


# ------------------------------------------------------------------------------------------------- (a) layers
@pytest.mark.parametrize("knob", [0, 1, 4])
@pytest.mark.parametrize("message", RF.MESSAGES)
@pytest.mark.parametrize("aggregate", ["sum", "max"])
def test_sum_and_max_layers_equal_the_recording(aggregate, message, knob):
    """One layer through the HIP rspmm (rotate: the native rotate operator) on 37 nodes with a hub row, isolated nodes, a
    self-loop, a duplicate triple, zero weights and B * D = 18 columns: inference (boundary fused into the kernel) and training
    (autograd route) forms, under the default dispatch, the general kernels (bit 0) and bit 2: output and every gradient.  Max:
    without the duplicate's output row, and the gradients of the second recorded run (upstream zero at that row)."""
    dev = _dev()
    masked = aggregate == "max"
    rows = NOT_DUPLICATE if masked else None
    with _knob(knob):
        inference = RR.layer_run(aggregate, message, dev, grad=False)
        training = RR.layer_run(aggregate, message, dev, grad=True, masked=masked)
    assert len(inference) == 1 and len(training) == 11
    for key, value in inference.items():
        _check("layer_output", "layers", key, value, rows)
    for key, value in training.items():
        if key.endswith("/output"):
            _check("layer_output", "layers", key, value, rows)
        else:
            _check("layer_gradient", "layers_masked" if masked else "layers", key, value)


@pytest.mark.parametrize("message", RF.MESSAGES)
def test_mean_layers_equal_the_recording(message):
    """Mean on its own route (sum kernel, then the division by the weighted degree + 1, which equals the recorded branch's number
    of messages on this graph): output and every gradient."""
    dev = _dev()
    for key, value in RR.layer_run("mean", message, dev, grad=False).items():
        _check("layer_output", "layers", key, value)
    for key, value in RR.layer_run("mean", message, dev, grad=True).items():
        _check("layer_output" if key.endswith("/output") else "layer_gradient", "layers", key, value)


@pytest.mark.parametrize("message", ["distmult", "rotate"])
def test_pna_layers_equal_the_recording(message):
    """PNA on its own route, output and every gradient: four rspmm walks for DistMult (without the duplicate's output row, whose
    max / min differ by construction; gradients of the second recorded run), the materialised route for rotate (every row, the
    first run)."""
    dev = _dev()
    masked = message == "distmult"
    rows = NOT_DUPLICATE if masked else None
    name = "pna_%s/output" % message
    _check("layer_output", "layers", name, RR.layer_run("pna", message, dev, grad=False)[name], rows)
    got = RR.layer_run("pna", message, dev, grad=True, masked=masked)
    assert len(got) == 11
    for key, value in got.items():
        if key.endswith("/output"):
            _check("layer_output", "layers", key, value, rows)
        else:
            _check("layer_gradient", "layers_masked" if masked else "layers", key, value)


def test_pna_over_transe_differs_from_the_recording_in_the_squares_only():
    """PNA over TransE on the HIP route is the reference's rspmm branch, which is another function than the recorded one (the mean
    of squares sums ``w (r^2 + x^2)``, ``ultra/layer.py:367``, against ``w (r + x)^2``, ``:283``): mean, max, min and the degree
    equal those of the materialised route of the same layer, and the mean of squares equals it once the cross term is added
    (``reference_runs.pna_transe_statistics``).  The layer OUTPUT is 1.9e-1 of its scale away from the recording and is not held."""
    import contextlib
    fast, slow, cross, out = RR.pna_transe_statistics(_dev(), contextlib.nullcontext())
    RR.check_pna_transe_statistics(fast, slow, cross, FLOORS["pna_statistic"])
    err, scale, _ = RR.deviation("layers", "pna_transe/output", out)
    print("pna / transe: rspmm route %.3e of scale from the recorded branch" % (err / scale))
    assert err > 1e-3 * scale               # if this ever fails the two branches have become one function: compare the output


# ------------------------------------------------------------------------------------------------- (b) entity model
@pytest.mark.parametrize("knob,plan", [(0, None), (1, None), (4, None), (256, None), (1024, None), (0, WIDE)],
                         ids=["default", "knob1", "knob4", "knob256", "knob1024", "wide_ids"])
def test_entity_model_equals_the_recording(knob, plan):
    """``TransferNBFNet`` 6 x 64 in the shipped configuration on 211 nodes / 1 500 triples (a node of degree above 128, isolated
    nodes), B = 4 rows x 9 candidates mixing corrupted tails and heads with a head == tail row: every layer's hidden state (whole
    rows at four nodes, the feature sum of every row) and the scores.  ``wide_ids``: the row-per-group rspmm kernels.  (``forward``
    on candidate lists never reads ``FAST_INFERENCE``; that switch and the fused-layer forms run in the ``predict`` tests.)"""
    dev = _dev()
    with _knob(knob):
        got = RR.entity_run("main", dev, plan=plan)
    assert len(got) == 13
    for key, value in got.items():
        _check("entity_score" if "/scores_" in key else "entity_hidden", "entity_model", key, value)


@pytest.mark.parametrize("name", sorted(RR.ENTITY_CONFIGS))
@pytest.mark.parametrize("mode", ["removed", "one_hop"])
def test_entity_model_with_removed_edges_equals_the_recording(name, mode):
    """The same scores with ``all_loss`` set: the batch's own edges (``removed``) or every edge between its heads and tails
    (``one_hop``) carry no messages -- zero weights on the cached plans for summed DistMult messages, a new graph otherwise."""
    got = RR.entity_run(name, _dev(), mode=mode)
    for key, value in got.items():
        _check("entity_score", "entity_model", key, value)


@pytest.mark.parametrize("name", ["small_pna_distmult", "small_rotate_sum"])
def test_small_entity_models_equal_the_recording(name):
    """Two layers, 16 wide: rotate / sum (native rotate operator) and PNA / DistMult (distinct triples, unit weights: both
    branches of the reference are one function here)."""
    for key, value in RR.entity_run(name, _dev()).items():
        _check("entity_score" if "/scores_" in key else "entity_hidden", "entity_model", key, value)


# ------------------------------------------------------------------------------------------------- (c) the task
@pytest.fixture(scope="module")
def gpu_task():
    task, batch, negatives, keys = RR.build_task(_dev())
    assert keys == ([], [])
    return task.eval(), batch, negatives


def _compare_ranks(ranking, context):
    """Issue "Ranks": exact where no unfiltered candidate's recorded score lies within twice the score tolerance of the target's,
    within the number of such candidates elsewhere; at most 10 % of the pairs in the second class."""
    a, stat = RR.arrays("pipeline"), RR.stats("pipeline")["predict"]
    _, _, _, positives, _ = RF.entity_batch(RF.entity_triples())
    tolerance = 4 * stat["ref_dev"] + FLOORS["task_predict"] * stat["scale"]
    near = RR.rank_classes(a["predict/R0"], positives, RR.recorded_mask(), tolerance)
    assert (near > 0).sum() <= 0.1 * near.size
    diff = np.abs(ranking.cpu().numpy() - a["ranking"])
    assert (diff <= near).all(), (context, ranking, a["ranking"], near)


def test_relation_graph_on_the_device_equals_the_recording(gpu_task):
    task = gpu_task[0]
    graph = task.rel_graphs[0]
    assert graph.edge_list.is_cuda and graph.num_node == 2 * RF.ENTITY_RELATIONS and graph.num_relation == 4
    assert np.array_equal(graph.edge_list.cpu().numpy(), RR.arrays("pipeline")["relation_graph/edge_list"].astype(np.int64))
    from ultra_torchdrug_amd.rel_model import construct_relation_graph
    again = construct_relation_graph(task.fact_graph)                     # built on the device (the native blocks)
    assert np.array_equal(again.edge_list.cpu().numpy(), graph.edge_list.cpu().numpy())


@pytest.mark.parametrize("fast", [True, False], ids=["fast", "layers"])
def test_relation_representations_equal_the_recording(gpu_task, fast):
    task, batch, _ = gpu_task
    with _fast_inference(fast), torch.no_grad():
        relation = task.relation_representations(batch[:, 2])[0]
    _check("task_relation", "pipeline", "relation_output", relation)


@pytest.mark.parametrize("fast,plan", [(True, None), (False, None), (True, WIDE)], ids=["fast", "layers", "wide_ids"])
def test_predict_and_ranks_equal_the_recording(gpu_task, fast, plan):
    """``predict`` over all entities, eager: the fused inference sequence, the layer-by-layer path, and the fused sequence on a
    row-per-group plan (``layer_forward`` / ``layer_score_forward``); ``rank_batch`` on its scores."""
    task, batch, _ = gpu_task
    und = task.model._undirected(task.fact_graph)
    saved = und._relcsr
    try:
        if plan is not None:
            from ultra_torchdrug_amd import RelCSR
            e = und.edge_list
            und._relcsr = RelCSR(e[:, 1].contiguous(), e[:, 0].contiguous(), e[:, 2].contiguous(), None, und.num_node,
                                 und.num_node, und.num_relation, **plan)
            # a row-per-group plan, which the fused layer forms take: the test must not quietly fall back to two launches
            assert und._relcsr.fwd.row_ptr is not None and und._relcsr.fwd.n_pieces == 0
            from ultra_torchdrug_amd import functional as UF
            calls = []
            real = (UF.layer_forward, UF.layer_score_forward)
            UF.layer_forward = lambda *a, **k: (lambda out: (calls.append(out is not None), out)[1])(real[0](*a, **k))
            UF.layer_score_forward = lambda *a, **k: (lambda out: (calls.append(out is not None), out)[1])(real[1](*a, **k))
        with _fast_inference(fast), torch.no_grad():
            pred = task.predict(batch)
            ranking = task.rank_batch(batch, pred=pred)
    finally:
        und._relcsr = saved
        if plan is not None:
            UF.layer_forward, UF.layer_score_forward = real
    if plan is not None:
        assert len(calls) == 5 and all(calls), calls          # layers 2 - 5 fused, the last one with the score head inside
    _check("task_predict", "pipeline", "predict", pred)
    _compare_ranks(ranking, "eager")


def test_replayed_predict_and_evaluate_equal_the_recording(gpu_task):
    """``predict`` as a replayed hipGraph with the ranks behind it, and ``engine.evaluate``: ranks and the metric set."""
    from ultra_torchdrug_amd import engine
    task, batch, _ = gpu_task
    replay = engine.GraphedPredict(task, batch, with_ranks=True)
    pred = replay(batch)
    _check("task_predict", "pipeline", "predict", pred)
    _compare_ranks(replay.ranks(batch), "replay")
    metric, ranking = engine.evaluate(task, batch, batch_size=4)
    _compare_ranks(ranking, "evaluate")
    a = RR.arrays("pipeline")
    assert list(metric) == RR.stats()["metrics"]
    if not np.array_equal(ranking.cpu().numpy(), a["ranking"]):          # (near ties allowed above) the metrics of the exact ranks
        metric = task.evaluate(torch.from_numpy(a["ranking"]).to(ranking.device))
    assert np.allclose([float(v) for v in metric.values()], a["metrics/R0"], rtol=1e-6, atol=0)


@pytest.mark.parametrize("temperature", [1.0, 0.0])
def test_eager_training_step_equals_the_recording(gpu_task, temperature):
    """The training branch of ``predict`` (first half of the batch corrupts tails, second half heads) and the loss on the
    recorded negatives: the loss and every parameter gradient (48 seeded entries, a seeded projection and the norm of each)."""
    task, batch, negatives = gpu_task
    try:
        got = RR.train_step_run(task, batch, negatives, temperature)
    finally:
        task.adversarial_temperature = 1.0
        task.zero_grad(set_to_none=True)
        task.eval()
    assert len(got) == 83
    for key, value in got.items():
        _check("task_loss" if key.endswith("/loss") else "task_gradient", "pipeline", key, value)


def test_captured_training_step_equals_the_recording():
    """The same step as a ``GraphedTrainStep`` replay (a learning rate of zero keeps the recorded weights)."""
    from ultra_torchdrug_amd import engine
    task, batch, negatives, _ = RR.build_task(_dev())
    task.train()
    task._static_negative = negatives
    try:
        optimizer = torch.optim.SGD(task.parameters(), lr=0.0)
        step = engine.GraphedTrainStep(task, optimizer, batch)
        loss, _ = step(batch)
        got = RR.compact_gradients(task, loss, 1.0)
    finally:
        task._static_negative = None
    assert len(got) == 83
    for key, value in got.items():
        _check("task_loss" if key.endswith("/loss") else "task_gradient", "pipeline", key, value)

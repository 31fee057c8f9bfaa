"""Model architectures OTHER than the shipped one, held to recorded runs of the reference's own ``ultra/model.py`` /
``rel_model.py`` (``tests/golden/reference_architectures.npz``, made by ``oracle/reference_record.py::record_architectures``): the
variants of ``reference_fixture.ARCHITECTURES`` at 64, 16 and (``base``, ``max_plain``) 6 columns, three layers, on the entity
record's graph, batch and relation tables; two ``RelNBFNet`` on its relation graph.  The weights are regenerated from the seeds and
checked against the recorded per-tensor sums (``reference_runs._drawn_state``).

Bounds, as in ``test_reference_fixtures_cpu.py``: the float64 materialised route ``1e-10 * scale``; the float32 rspmm route on the C
oracle ``4 * ref_dev + 2e-5 * scale``.  ``max_plain`` / ``defaults`` (min / max): the fact graph with inverse edges holds every
triple once (asserted here and by the recorder), so the rspmm branch and the recorded branch compute one function on every row and
no row is left out.  Their backward is another matter: see ``test_float32_rspmm_route_equals_the_recording``.
"""
import numpy as np
import pytest
import torch

import reference_fixture as RF
import reference_runs as RR
from aten_definition import AtenDefinition
from oracle_ops import oracle_rspmm
import rspmm_definition

CPU = torch.device("cpu")
F64, ORACLE = 1e-10, 2e-5
MODES = ("eval", "all_entities", "train")
CASES = pytest.mark.parametrize("name,width", RF.ARCH_CASES, ids=["%s-%d" % c for c in RF.ARCH_CASES])


@pytest.fixture(autouse=True)
def _one_thread():
    keep = torch.get_num_threads()
    torch.set_num_threads(1)
    yield
    torch.set_num_threads(keep)


def _recorded_keys(tag):
    return sorted(k for k in RR.stats("architectures") if k.startswith(tag + "/"))


def _run_all(name, width, dtype, materialised):
    got = {}
    for mode in MODES:
        got.update(RR.architecture_run(name, width, CPU, dtype, mode, materialised=materialised))
    return got


def _check_all(name, width, got, floor, factor, rspmm_branch=False):
    """``rspmm_branch``: the run took the rspmm branch, whose min / max backward is another function than the recorded branch's
    at a tie (``reference_fixture.gradient_passes_an_extreme``): the gradients that pass one are held to the float64 run of the
    rspmm branch over the plain definition of the operator (``tests/rspmm_definition.py``), by the same rule; every other tensor
    to the recording."""
    tag = "%s_%d" % (name, width)
    RR.check_gradient_keys(tag, got)
    keys = _recorded_keys(tag)
    n_layers = len(RF.arch_arguments(name, width)["hidden_dims"])
    assert len([k for k in keys if "/hidden" in k]) == 2 * n_layers and len([k for k in keys if "/train/d_" in k]) >= 6
    behind = rspmm_definition.check_extreme_gradients(name, width, got, floor) if rspmm_branch else []
    assert bool(behind) == (rspmm_branch and name in RF.EXTREME_ARCHITECTURES) and len(keys) - len(behind) >= 2 * n_layers + 3 + 4
    for key in keys:
        if key not in behind:
            RR.check("architectures", key, got[key], floor, ref_factor=factor)


def test_the_record_is_complete_and_small():
    """Every variant x width is recorded with scores, scores over all entities, every hidden state, training scores and
    gradients; the reference agrees with itself; the three configurations it cannot run are named with their reasons and recorded
    nowhere; no triple of the graph with inverse edges occurs twice; the file respects the limit for a committed file."""
    import os
    meta = RR.stats()["architectures"]
    assert [tuple(c) for c in meta["cases"]] == RF.ARCH_CASES and len(RF.ARCH_CASES) == 28
    assert set(RF.ARCHITECTURES) == {"base", "no_shortcut", "no_ln", "tanh", "concat", "mlp1", "mlp3", "no_project", "not_mod",
                                     "one_layer", "defaults", "max_plain", "mean_transe"}
    assert all(64 in w and 16 in w for w in RF.ARCH_WIDTHS.values())
    assert [n for n, w in RF.ARCH_WIDTHS.items() if 6 in w] == ["base", "max_plain"]
    assert meta["not_runnable"] == RF.ARCH_NOT_RUNNABLE and len(RF.ARCH_NOT_RUNNABLE) == 3
    for reason in RF.ARCH_NOT_RUNNABLE.values():
        assert "ultra/" in reason                                   # each names the line of the reference that fails
    recorded = {k.split("/")[0] for k in RR.stats("architectures")}
    assert recorded == {"%s_%d" % c for c in RF.ARCH_CASES} | set(RF.REL_ARCHITECTURES)
    for key, stat in RR.stats("architectures").items():
        assert stat["scale"] > 0 and 0 <= stat["ref_dev"] <= 1e-5 * stat["scale"], (key, stat)
        assert key + "/T" in RR.arrays("architectures") or key + "/R0" in RR.arrays("architectures"), key
    assert RF.undirected_is_distinct(RF.entity_triples())
    assert os.path.getsize(os.path.join(RR.GOLDEN, "reference_architectures.npz")) <= 1 << 20


@CASES
def test_float64_materialised_route_equals_the_recording(name, width):
    """``message`` + ``aggregate`` of this package in float64: scores (batch, all entities), hidden states, training scores and
    every gradient."""
    with RR.backend_use(AtenDefinition()):
        got = _run_all(name, width, torch.float64, True)
    _check_all(name, width, got, F64, 0.0)


@CASES
def test_float32_rspmm_route_equals_the_recording(name, width):
    """The rspmm branch on the C oracle (strictly sequential order) in float32: the same tensors.  (PNA over DistMult and max
    on distinct triples with unit weights: both branches of the reference are one function in the forward direction.  Their
    BACKWARD differs at ties of min / max, which a stack has by construction -- the recorded branch feeds one tied message, the
    rspmm branch every tied edge; 0.12 (``defaults``, 64) to 1.5 (``max_plain``, 16) of a gradient's scale apart.  For
    ``max_plain`` and ``defaults`` the gradients that pass such a backward are therefore held to the float64 run of the rspmm
    branch itself, ``(4 * own + 2e-5) * scale`` with ``own`` the float32 deviation of that definition from its float64 run, the worst
    over these gradients of the case.  Measured: the
    oracle lies 2e-7 of scale from it for ``max_plain`` and ``defaults`` at 16; 2.4e-2 for ``defaults`` at 64, where the
    definition's own float32 run lies 2.3e-2 away too: the PNA backward of that stack is ill-conditioned in float32 -- a
    precision effect, present with no kernel and no oracle involved; two summation orders differ by 2e-7 only.)"""
    with oracle_rspmm(piece=0):
        got = _run_all(name, width, torch.float32, False)
    _check_all(name, width, got, ORACLE, 4.0, rspmm_branch=True)


@pytest.mark.parametrize("tag", sorted(RF.REL_ARCHITECTURES))
def test_relation_models_equal_the_recording(tag):
    """``RelNBFNet`` 16 wide, and two layers at 64 (float32 only, ``ultra/rel_model.py:353``; ``ref_dev`` over the reference's
    runs on permuted edge lists): the materialised route and the rspmm route on the C oracle."""
    with RR.backend_use(AtenDefinition()):
        got = RR.relation_architecture_run(tag, CPU, materialised=True)
    RR.check("architectures", tag + "/relation_output", got[tag + "/relation_output"], 2e-6)
    with oracle_rspmm(piece=0):
        got = RR.relation_architecture_run(tag, CPU)
    RR.check("architectures", tag + "/relation_output", got[tag + "/relation_output"], ORACLE)


RECORDED = """base_64 base_16 base_6 no_shortcut_64 no_shortcut_16 no_ln_64 no_ln_16 tanh_64 tanh_16 concat_64 concat_16 mlp1_64 mlp1_16
mlp3_64 mlp3_16 no_project_64 no_project_16 not_mod_64 not_mod_16 one_layer_64 one_layer_16 defaults_64 defaults_16 max_plain_64
max_plain_16 max_plain_6 mean_transe_64 mean_transe_16 rel_hidden16 rel_two_layers""".split()


def test_no_recorded_variant_is_left_out():
    """Every recorded case -- the list is spelled out here, not derived -- is a parameter of BOTH comparison tests of this module
    and of the device module's value and route tests, and none of them carries any mark but ``parametrize`` (no skip, no
    expected failure).  What the reference cannot run carries its reason."""
    assert sorted({k.split("/")[0] for k in RR.arrays("architectures")}) == sorted(RECORDED)
    import test_reference_architectures_gpu as device
    for test, want in ((test_float64_materialised_route_equals_the_recording, RECORDED[:28]),
                       (test_float32_rspmm_route_equals_the_recording, RECORDED[:28]),
                       (test_relation_models_equal_the_recording, RECORDED[28:]),
                       (device.test_values_equal_the_recording, RECORDED[:28]), (device.test_routes, RECORDED[:28]),
                       (device.test_relation_models_equal_the_recording, RECORDED[28:])):
        marks = test.pytestmark
        assert [m.name for m in marks] == ["parametrize"], (test.__name__, marks)
        cases = marks[0].args[1]
        assert sorted(c if isinstance(c, str) else "%s_%d" % tuple(c) for c in cases) == sorted(want), test.__name__
    assert sorted(RF.ARCH_NOT_RUNNABLE) == ["not_mod_no_project", "symmetric", "unequal_hidden_dims"]


def test_definition_of_the_rspmm_branch_equals_the_recording_where_the_branches_agree():
    """``tests/rspmm_definition.py`` in float64, train mode, on the two min / max variants: every tensor that does not pass a
    min / max backward equals the recording (1e-10 of scale) -- the model wrapper over the definition IS the reference there --
    and the others lie apart from it (the tie rule)."""
    for name in RF.EXTREME_ARCHITECTURES:
        for width in RF.ARCH_WIDTHS[name]:
            tag = "%s_%d" % (name, width)
            truth, own_dev = rspmm_definition.rspmm_branch_training_run(name, width)
            agree = [k for k in _recorded_keys(tag) if "/train/" in k and not RF.gradient_passes_an_extreme(name, width, k)]
            assert len(agree) >= 5
            for key in agree:
                RR.check("architectures", key, truth[key], F64, ref_factor=0.0)


@pytest.mark.parametrize("width", [64, 16])
def test_symmetric_is_the_mean_of_the_two_directions(width):
    """``symmetric=True`` has no run of the reference (``ultra/model.py:187`` raises).  DECISION: the reading
    of ``ultra/model.py:185-191`` without the stray fourth argument -- the feature gathered at the tails from the Bellman-Ford
    started at the heads, averaged with the feature gathered at the heads from the one started at the tails, then the score
    head.  Pinned against two plain ``bellmanford`` calls composed here, float64, materialised route."""
    from ultra_torchdrug_amd.model import TransferNBFNet
    kwargs = RF.arch_arguments("base", width)
    triples = RF.entity_triples()
    _, _, _, positives, _ = RF.entity_batch(triples)
    # symmetric needs ONE tail per row too (model.py:186): the positives alone, all as tail queries
    h, t, r = (torch.from_numpy(positives[:, i:i + 1].copy()) for i in range(3))
    with RR.default_dtype(torch.float64), RR.backend_use(AtenDefinition()), torch.no_grad():
        model = TransferNBFNet(symmetric=True, **kwargs)
        state = RF.draw_state({k: v.shape for k, v in model.state_dict().items()}, RF.arch_seed("base", width))
        model.load_state_dict({k: torch.from_numpy(v) for k, v in state.items()})
        model = model.double().eval()
        graph = RR.fact_graph(CPU)
        und = model._undirected(graph)
        und.requires_grad = True
        und.edge_weight = und.edge_weight.double()
        tables = [torch.from_numpy(table) for table in RF.rel_query_list(RF.ARCH_LAYERS + 1, 4, width)]
        score = model(graph, tables, h, t, r)
        rows = torch.arange(4)
        forward = model.bellmanford(und, h[:, 0], r[:, 0])["node_feature"][t[:, 0], rows]
        backward = model.bellmanford(und, t[:, 0], r[:, 0])["node_feature"][h[:, 0], rows]
        want = model.mlp((forward + backward) / 2).squeeze(-1).view(4, 1)
        one_way = model.mlp(forward).squeeze(-1).view(4, 1)
    assert score.shape == (4, 1)
    assert float((score - want).abs().max()) <= F64 * float(want.abs().max())
    assert float((score - one_way).abs().max()) > 1e-3 * float(want.abs().max())       # the second direction does enter

"""The HIP path on model architectures OTHER than the shipped one, held to recorded runs of the reference's own code
(``tests/golden/reference_architectures.npz``; ``tests/test_reference_architectures_cpu.py`` says what the recordings are): every
variant of ``reference_fixture.ARCHITECTURES`` at 64, 16 and (two of them) 6 columns, and WHICH entry points each of them reaches.

(a) Values.  ``max|X - truth| <= 4 * ref_dev + floor * scale`` against the reference's float64 run.  The floor of a tensor is the
one the shipped ``main`` record's tensor of the same kind has (``test_reference_fixtures_gpu.py``: hidden states 8e-7, scores of a
batch 1.1e-6, scores over all entities 1.4e-6, gradients 2.4e-6, relation representations 1.4e-6); no variant needs or gets a
larger one.  ``reference_fixtures.json`` keeps, under ``mi355x.architectures``, the measured deviation of the HIP path and of the
float32 ATen definition of the same variant on the same device (``tests/aten_definition.py``, no kernel of this package).

Min / max stacks (``max_plain``, ``defaults``): every value is compared with the recording on every row.  Of the gradients, those
that pass the backward of a min / max are another function on the rspmm branch than on the recorded one at a tie (``reference_fixture.
gradient_passes_an_extreme``; ties are structural in a stack): they are held, by the same rule and the same floor, to the float64
run of the rspmm branch over the plain definition of the operator (``tests/rspmm_definition.py``), with that definition's own
float32 deviation (the worst over these gradients of the case) in the place of ``ref_dev``.  Measured: 2e-7 .. 1.5e-6 of scale for ``max_plain`` and ``defaults`` at 16; for
``defaults`` at 64 up to about 3e-2, where the definition's own float32 run lies 2.3e-2 from its float64 run -- the PNA backward
of that stack is ill-conditioned in float32, kernel or no kernel -- against 0.12 between the two branches.

(b) Routes.  A recording proxy around the backend counts the entry points the model code calls; ``ROUTES`` says, per variant and
width, which must appear and which must not -- written from the documented conditions of ``layer._fusable``, ``_pna_fusable``, the
frontier first layer, ``model._relation_tables``, ``_fast_stack``, ``_fused_head_ok`` and the ``score_candidates`` branch, not by
calling them.
"""
import collections

import pytest
import torch

import reference_fixture as RF
import reference_runs as RR
import rspmm_definition

pytestmark = pytest.mark.gpu

FLOORS = {"hidden": 8e-7, "scores": 1.1e-6, "scores_all": 1.4e-6, "gradient": 2.4e-6, "relation": 1.4e-6}
MODES = ("eval", "all_entities", "train")
CASES = pytest.mark.parametrize("name,width", RF.ARCH_CASES, ids=["%s-%d" % c for c in RF.ARCH_CASES])
FAM_QUAD, FAM_PACKED, FAM_GENERAL = 2, 3, 4          # csrc/plan_path.h


def _dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def group_of(key):
    if "/train/d_" in key:
        return "gradient"
    if key.endswith("/scores_all"):
        return "scores_all"
    if key.endswith("scores"):
        return "scores"
    return "relation" if key.endswith("/relation_output") else "hidden"


class RecordingBackend:
    """The backend in force behind an object that counts the calls of its entry points (predicates -- ``accepts``,
    ``*_supported`` -- and plain attributes pass uncounted) and notes the block width of every sparse boundary handed to
    ``rspmm_forward``."""

    def __init__(self, inner):
        self._inner = inner
        self.calls = collections.Counter()
        self.boundary_blocks = []

    def __getattr__(self, name):
        value = getattr(self._inner, name)
        if not callable(value) or name == "accepts" or name.endswith("_supported"):
            return value

        def counted(*args, **kwargs):
            self.calls[name] += 1
            if name == "rspmm_forward" and kwargs.get("boundary") is not None:
                self.boundary_blocks.append(int(kwargs["boundary"][1].shape[-1]))
            return value(*args, **kwargs)
        return counted


_RUNS = {}


def hip_runs(name, width):
    """The three runs of one case on the HIP backend, once per session: ``(tensors on the host, {mode: calls}, {mode: boundary
    blocks}, {mode: launch records})``."""
    if (name, width) not in _RUNS:
        from ultra_torchdrug_amd import _lib, backend
        got, calls, blocks, records = {}, {}, {}, {}
        for mode in MODES:
            proxy = RecordingBackend(backend.get())
            _lib.launch_records_clear()
            with backend.use(proxy):
                out = RR.architecture_run(name, width, _dev(), torch.float32, mode)
            torch.cuda.synchronize()
            records[mode] = _lib.launch_records()
            got.update({k: (v.detach().double().cpu() if torch.is_tensor(v) else v) for k, v in out.items()})
            calls[mode], blocks[mode] = proxy.calls, proxy.boundary_blocks
        _RUNS[(name, width)] = (got, calls, blocks, records)
    return _RUNS[(name, width)]


# ------------------------------------------------------------------------------------------------- (a) values
@CASES
def test_values_equal_the_recording(name, width):
    tag = "%s_%d" % (name, width)
    got = hip_runs(name, width)[0]
    keys = RR.check_gradient_keys(tag, got)
    assert len(keys) >= 6
    # (the gradients behind a min / max backward: against the rspmm branch's own float64 run, by the same rule and floor)
    behind = rspmm_definition.check_extreme_gradients(name, width, got, FLOORS["gradient"])
    assert bool(behind) == (name in RF.EXTREME_ARCHITECTURES)
    for key in sorted(k for k in RR.stats("architectures") if k.startswith(tag + "/") and k not in behind):
        err, scale, ref_dev = RR.deviation("architectures", key, got[key])
        floor = FLOORS[group_of(key)]
        print("%-10s %-56s %.3e of scale (reference's own %.3e)" % (group_of(key), key, err / scale, ref_dev / scale))
        assert err <= 4 * ref_dev + floor * scale, \
            "%s: %.3g from the reference's run (its own deviation %.3g, scale %.3g, floor %.1e)" % (key, err, ref_dev, scale, floor)


@pytest.mark.parametrize("tag", sorted(RF.REL_ARCHITECTURES))
def test_relation_models_equal_the_recording(tag):
    """``RelNBFNet`` 16 wide (no 64-only kernel applies) and two layers at 64 (the fast relation stack)."""
    got = RR.relation_architecture_run(tag, _dev())
    err, scale, ref_dev = RR.deviation("architectures", tag + "/relation_output", got[tag + "/relation_output"])
    print("%-10s %-56s %.3e of scale (reference's own %.3e)" % ("relation", tag, err / scale, ref_dev / scale))
    assert err <= 4 * ref_dev + FLOORS["relation"] * scale, (tag, err, ref_dev, scale)


# ------------------------------------------------------------------------------------------------- (b) routes
ONLY_64 = {"rspmm_frontier", "first_layer_forward", "layer_forward", "layer_score_forward", "combine", "combine_forward", "sum_layer",
           "score_all_entities", "score_candidates", "relation_project", "relation_project_train", "pna_combine_forward"}
EPILOGUES = {"combine", "combine_forward", "sum_layer", "pna_combine_forward"}
HEADS = {"score_all_entities", "score_candidates"}
PROJECTIONS = {"relation_project", "relation_project_train"}


def _route(must, must_not=()):
    return set(must), set(must_not)


def _shipped_like():
    """64 wide, DistMult / sum, relu, projected, the 128 -> 128 -> 1 head: frontier first layer, fused epilogue, fused heads."""
    return {
        "eval": _route({"rspmm_frontier", "rspmm_forward", "combine", "score_candidates"},
                       {"sum_layer", "generalized_rspmm", "rspmm_sum_plus", "score_all_entities"}),
        "all_entities": _route({"rspmm_frontier", "rspmm_forward", "combine", "score_all_entities"},
                               {"sum_layer", "generalized_rspmm", "score_candidates"}),
        "train": _route({"sum_layer", "score_candidates"},
                        {"combine", "rspmm_frontier", "generalized_rspmm", "score_all_entities"}),
    }


def _edit(routes, **changes):
    """``routes`` with, per mode, entry points moved: ``mode=(add to must, add to must_not)``; ``every=`` applies to all modes.
    What enters one set leaves the other."""
    out = {mode: (set(must), set(must_not)) for mode, (must, must_not) in routes.items()}
    for mode in out:
        for add, drop in (changes.get("every", ((), ())), changes.get(mode, ((), ()))):
            must, must_not = out[mode]
            out[mode] = ((must | set(add)) - set(drop), (must_not | set(drop)) - set(add))
    return out


ROUTES_64 = {
    "base": _shipped_like(),
    "no_ln": _shipped_like(),                   # the fused epilogue has a form without LayerNorm
    "no_shortcut": _shipped_like(),             # ... and without the shortcut
    # tanh: no fused epilogue in any mode (the kernels know relu or none); the frontier, the projection and the heads stay
    "tanh": _edit(_shipped_like(), every=((), EPILOGUES), train=({"rspmm_sum_plus"}, ())),
    # another head than 128 -> 128 -> 1: neither fused head
    "concat": _edit(_shipped_like(), every=((), HEADS)),
    "mlp1": _edit(_shipped_like(), every=((), HEADS)),
    "mlp3": _edit(_shipped_like(), every=((), HEADS)),
    # (the grouped relation projection: ``test_grouped_relation_projection``)
    "no_project": _shipped_like(),
    "not_mod": _shipped_like(),
    # one layer: the frontier layer is the only one
    "one_layer": _edit(_shipped_like(), eval=((), {"rspmm_forward"}), all_entities=((), {"rspmm_forward"})),
    # PNA: one-walk statistics + fused 13-wide epilogue in inference, four rspmm calls per layer under grad
    "defaults": {
        "eval": _route({"pna_statistics", "pna_combine_forward", "score_candidates"},
                       {"generalized_rspmm", "combine", "sum_layer", "rspmm_frontier", "score_all_entities"}),
        "all_entities": _route({"pna_statistics", "pna_combine_forward", "score_all_entities"},
                               {"generalized_rspmm", "combine", "sum_layer", "rspmm_frontier", "score_candidates"}),
        "train": _route({"generalized_rspmm", "score_candidates"},
                        {"pna_statistics", "pna_combine_forward", "combine", "sum_layer", "rspmm_frontier"}),
    },
    # max: no frontier (a zero message is not "no message"), no one-node layer; the 2-wide epilogue is the shipped one
    "max_plain": {
        "eval": _route({"rspmm_forward", "combine", "score_candidates"},
                       {"rspmm_frontier", "sum_layer", "generalized_rspmm", "pna_statistics", "score_all_entities"}),
        "all_entities": _route({"rspmm_forward", "combine", "score_all_entities"},
                               {"rspmm_frontier", "sum_layer", "generalized_rspmm", "score_candidates"}),
        "train": _route({"generalized_rspmm", "combine", "score_candidates"},
                        {"sum_layer", "rspmm_sum_plus", "rspmm_frontier", "rspmm_forward"}),
    },
    # mean of TransE messages: no frontier (r + 0 is not 0), no one-node layer; sum kernel, division, shipped epilogue
    "mean_transe": {
        "eval": _route({"rspmm_forward", "combine", "score_candidates"},
                       {"rspmm_frontier", "sum_layer", "generalized_rspmm", "score_all_entities"}),
        "all_entities": _route({"rspmm_forward", "combine", "score_all_entities"},
                               {"rspmm_frontier", "sum_layer", "generalized_rspmm", "score_candidates"}),
        "train": _route({"rspmm_sum_plus", "combine", "score_candidates"},
                        {"sum_layer", "rspmm_frontier", "rspmm_forward"}),
    },
}
# the fused inference sequence of ``score_both_sides`` (``_fast_stack``): DistMult / sum, relu or none, projected, Mod layers, no
# concatenation
FAST_STACK_64 = {"base", "no_ln", "no_shortcut", "one_layer", "mlp1", "mlp3"}
# how often: layers x calls per layer (three layers; ``one_layer`` one)
COUNTS_64 = {
    ("base", "eval"): {"rspmm_frontier": 1, "rspmm_forward": 2, "combine": 3, "score_candidates": 1},
    ("base", "train"): {"sum_layer": 3},
    ("tanh", "eval"): {"rspmm_frontier": 1, "rspmm_forward": 2},
    ("tanh", "train"): {"rspmm_sum_plus": 3},
    ("one_layer", "all_entities"): {"rspmm_frontier": 1, "combine": 1, "score_all_entities": 1},
    ("defaults", "eval"): {"pna_statistics": 3, "pna_combine_forward": 3},
    ("defaults", "train"): {"generalized_rspmm": 12},
    ("max_plain", "eval"): {"rspmm_forward": 3, "combine": 3},
    ("max_plain", "train"): {"generalized_rspmm": 3, "combine": 3},
    ("mean_transe", "train"): {"rspmm_sum_plus": 3, "combine": 3},
}


def narrow_route(name, mode):
    """16 and 6 wide: no 64-only entry point at all; the operators that take any width do the work."""
    aggregate = RF.arch_arguments(name, 16)["aggregate_func"]
    if mode == "train":
        must = {"sum": {"rspmm_sum_plus"}, "mean": {"rspmm_sum_plus"}, "max": {"generalized_rspmm"}, "pna": {"generalized_rspmm"}}[aggregate]
    else:
        must = {"pna_statistics"} if aggregate == "pna" else {"rspmm_forward"}
    return set(must), set(ONLY_64)


@CASES
def test_routes(name, width):
    _, calls, blocks, records = hip_runs(name, width)
    for mode in MODES:
        must, must_not = ROUTES_64[name][mode] if width == 64 else narrow_route(name, mode)
        # the recorded runs give every layer a relation table of its own; the grouped projection wants ONE table for all
        # layers (``model._relation_tables``: ``conv.relation is relation``) and is declined by every variant here -- but by the
        # one with ONE layer (``test_grouped_relation_projection`` runs the others with a shared table)
        if (name, width) == ("one_layer", 64):
            must = must | {"relation_project_train" if mode == "train" else "relation_project"}
            must_not = must_not | (PROJECTIONS - must)
        else:
            must_not = must_not | PROJECTIONS
        seen = set(calls[mode])
        print("%s_%d %-12s %s" % (name, width, mode, dict(calls[mode])))
        assert must <= seen, "%s_%d %s: %s did not run" % (name, width, mode, sorted(must - seen))
        assert not (must_not & seen), "%s_%d %s: %s ran" % (name, width, mode, sorted(must_not & seen))
        for entry, count in COUNTS_64.get((name, mode), {}).items() if width == 64 else ():
            assert calls[mode][entry] == count, (name, mode, entry, calls[mode][entry], count)
        if mode != "train" and blocks[mode]:
            assert set(blocks[mode]) == {width}, (name, width, mode, blocks[mode])       # the sparse boundary, one block per query
    if width != 64 and RF.arch_arguments(name, width)["aggregate_func"] != "pna":
        n_layers = len(RF.arch_arguments(name, width)["hidden_dims"])
        assert blocks["eval"] == [width] * n_layers, (name, width, blocks["eval"])
    if width == 6:
        # ``boundary_ok`` (csrc/plan_path.h) is false for a 6-column block: neither the quad nor the row-per-group kernel, whose
        # lanes hold four columns of ONE query block
        count, rows = records["eval"]
        assert count >= 3 and rows
        for row in rows:
            assert row["status"] == 0 and row["family"] in (FAM_PACKED, FAM_GENERAL), row


@pytest.mark.parametrize("name,grouped", [("base", True), ("tanh", True), ("defaults", True), ("no_project", False), ("not_mod", False)])
def test_grouped_relation_projection(name, grouped):
    """ONE relation table for all layers, as the task hands it over: at 64 columns the projected ``Mod`` layers get their
    ``(R, B * D)`` tables from one launch (``relation_project``; under grad ``relation_project_train``), ``project=False`` and
    ``mod=False`` models never do, and nobody does at 16.  The scores equal those of the float32 ATen definition of the same
    call on the device within the batch scores' floor."""
    from aten_definition import AtenDefinition
    from ultra_torchdrug_amd import backend
    dev = _dev()
    triples = RF.entity_triples()
    h, t, r = (torch.from_numpy(a).to(dev) for a in RF.entity_batch(triples)[:3])
    for width in (64, 16):
        model = RR.architecture_model(name, width, dev).eval()
        table = torch.from_numpy(RF.rel_query_list(1, 4, width)[0]).float().to(dev)
        graph = RR.fact_graph(dev)
        with torch.no_grad():
            proxy = RecordingBackend(backend.get())
            with backend.use(proxy):
                score = model(graph, [table], h, t, r)
            assert (proxy.calls["relation_project"] == 1) == (grouped and width == 64), (name, width, dict(proxy.calls))
            assert not proxy.calls["relation_project_train"]
            model._undirected(graph).requires_grad = True
            with backend.use(AtenDefinition()):
                want = model(graph, [table], h, t, r)
            model._undirected(graph).requires_grad = False
        scale = float(want.abs().max())
        print("%s_%d shared table: %.3e of scale from the ATen definition" % (name, width, float((score - want).abs().max()) / scale))
        # the HIP side gets the batch scores' floor, the float32 ATen side four times the reference's own float32 deviation
        own = RR.stats("architectures")["%s_%d/scores" % (name, width)]
        assert float((score - want).abs().max()) <= (FLOORS["scores"] + 4 * own["ref_dev"] / own["scale"]) * scale
        model.train()
        proxy = RecordingBackend(backend.get())
        with backend.use(proxy):
            model(graph, [table.clone().requires_grad_()], h, t, r)
        assert (proxy.calls["relation_project_train"] == 1) == (grouped and width == 64), (name, width, dict(proxy.calls))
        assert not proxy.calls["relation_project"]


@pytest.mark.parametrize("name", sorted(RF.ARCHITECTURES))
def test_fast_stack_covers_the_documented_variants_only(name):
    """``_fast_stack`` (the fused sequence of ``score_both_sides``) and ``_fused_head_ok`` at 64 columns; nothing at 16."""
    dev = _dev()
    index = torch.zeros(4, dtype=torch.long, device=dev)
    with torch.no_grad():
        model = RR.architecture_model(name, 64, dev).eval()
        assert (model._fast_stack() is not None) == (name in FAST_STACK_64), name
        assert model._fused_head_ok(index, None) == (name not in ("concat", "mlp1", "mlp3")), name
        narrow = RR.architecture_model(name, 16, dev).eval()
        assert narrow._fast_stack() is None and not narrow._fused_head_ok(index, None)


@pytest.mark.parametrize("name", sorted(FAST_STACK_64))
def test_fused_inference_sequence_equals_the_aten_definition(name):
    """``score_both_sides`` (what full-batch evaluation calls: ``prepare_queries``, the grouped projection for both sides, the
    sparse first layer or the frontier, fused layers where the plan has them, the fused head) on the variants ``_fast_stack``
    covers, with ONE relation table as the task hands it over: the ``(2 B, N)`` scores of both sides against the float32 ATen
    definition of the same queries on the device (no kernel of this package) -- the HIP side gets the floor of scores over all
    entities, the ATen side four times the reference's own float32 deviation of that kind of tensor.  ``mlp1`` / ``mlp3`` have
    the stack but not the head: the sequence declines them."""
    from aten_definition import AtenDefinition
    from ultra_torchdrug_amd import backend
    dev = _dev()
    positives = RF.entity_batch(RF.entity_triples())[3]
    batch = torch.from_numpy(positives).to(dev)
    model = RR.architecture_model(name, 64, dev).eval()
    table = torch.from_numpy(RF.rel_query_list(1, 4, 64)[0]).float().to(dev)
    graph = RR.fact_graph(dev)
    with torch.no_grad():
        proxy = RecordingBackend(backend.get())
        with backend.use(proxy):
            score = model.score_both_sides(graph, table, batch)
        print("%s_64 score_both_sides %s" % (name, dict(proxy.calls)))
        if name in ("mlp1", "mlp3"):
            assert score is None and not (set(proxy.calls) & ONLY_64)
            return
        assert score is not None and tuple(score.shape) == (8, RF.ENTITY_NODES)
        assert proxy.calls["prepare_queries"] == 1 and proxy.calls["relation_project"] == 1
        assert proxy.calls["first_layer_forward"] == 1 and (proxy.calls["score_all_entities"] + proxy.calls["layer_score_forward"]) >= 1
        every = torch.arange(RF.ENTITY_NODES, device=dev).expand(4, -1)
        h = torch.cat([batch[:, :1].expand(-1, RF.ENTITY_NODES), every])
        t = torch.cat([every, batch[:, 1:2].expand(-1, RF.ENTITY_NODES)])
        r = torch.cat([batch[:, 2:], batch[:, 2:]]).expand(-1, RF.ENTITY_NODES)
        tables = [torch.cat([table, table])]
        model._undirected(graph).requires_grad = True
        with backend.use(AtenDefinition()):
            want = model(graph, tables, h, t, r)
        model._undirected(graph).requires_grad = False
    scale = float(want.abs().max())
    own = RR.stats("architectures")["%s_64/scores_all" % name]
    err = float((score - want).abs().max())
    print("%s_64 score_both_sides: %.3e of scale from the ATen definition" % (name, err / scale))
    assert err <= (FLOORS["scores_all"] + 4 * own["ref_dev"] / own["scale"]) * scale

"""Test infrastructure: run THIS package's layers, models and task on the inputs of the recorded reference runs
(``tests/reference_fixture.py``, ``tests/golden/reference_*.npz``) -- on any device, in either precision, through whichever
backend is installed -- and compare with the recordings.  Shared by ``test_reference_fixtures_cpu.py`` and ``_gpu.py``.

Bound of every comparison (issue "Tolerances"): ``max|X - truth| <= 4 * ref_dev + floor * scale`` with ``ref_dev`` and ``scale``
from ``reference_fixtures.json`` -- measured on the reference alone -- and ``truth`` the float64 run where one exists."""
import json
import os

import numpy as np
import torch

import reference_fixture as RF

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ENTITY_CONFIGS = {"main": (64, 6, "distmult", "sum"), "small_rotate_sum": (RF.SMALL_DIM, 2, "rotate", "sum"),
                  "small_pna_distmult": (RF.SMALL_DIM, 2, "distmult", "pna")}
_CACHE = {}


def arrays(name):
    """``reference_<name>.npz`` as a dict, loaded once."""
    if name not in _CACHE:
        with np.load(os.path.join(GOLDEN, "reference_%s.npz" % name)) as f:
            _CACHE[name] = {k: f[k] for k in f.files}
        for key in [k for k in _CACHE[name] if k.endswith("/train/gradients/T")]:
            # the compact gradients of one architecture record, stacked in the sorted order of their names
            prefix = key[:-len("gradients/T")] + "d_"
            names = sorted(k for k in stats(name) if k.startswith(prefix))
            matrix = _CACHE[name].pop(key)
            assert len(names) == len(matrix), key
            _CACHE[name].update({n + "/T": row for n, row in zip(names, matrix)})
    return _CACHE[name]


def stats(name=None):
    if "json" not in _CACHE:
        with open(os.path.join(GOLDEN, "reference_fixtures.json")) as f:
            _CACHE["json"] = json.load(f)
    meta = _CACHE["json"]
    return meta if name is None else meta["tensors"]["reference_%s.npz" % name]


def state_dict(name, prefix, rename=""):
    """The float16 weights stored under ``prefix/`` as float32 tensors, keys prefixed with ``rename``."""
    out = {}
    for key, value in arrays(name).items():
        if key.startswith(prefix + "/") and value.dtype == np.float16:
            out[rename + key[len(prefix) + 1:]] = torch.from_numpy(value.astype(np.float32))
    return out


def truth(name, key):
    a = arrays(name)
    return a[key + "/T"] if key + "/T" in a else a[key + "/R0"].astype(np.float64)


def deviation(name, key, got, rows=None):
    """``(max|got - truth|, scale, ref_dev)``; ``rows``: compare these rows of the first axis only."""
    want = truth(name, key)
    got = np.asarray(got.detach().cpu().double().numpy() if torch.is_tensor(got) else got, dtype=np.float64)
    assert got.shape == want.shape, (key, got.shape, want.shape)
    assert np.isfinite(got).all(), key
    if rows is not None:
        got, want = got[rows], want[rows]
    s = stats(name)[key]
    return float(np.abs(got - want).max()), s["scale"], s["ref_dev"]


def check(name, key, got, floor, rows=None, ref_factor=4.0, report=None):
    err, scale, ref_dev = deviation(name, key, got, rows)
    if report is not None:
        report[key] = err / max(scale, 1e-300)
    assert err <= ref_factor * ref_dev + floor * scale, \
        "%s: %.3g from the reference's run (its own deviation %.3g, scale %.3g, floor %.1e)" % (key, err, ref_dev, scale, floor)
    return err / max(scale, 1e-300)


def backend_use(ops):
    from ultra_torchdrug_amd import backend
    return backend.use(ops)


class default_dtype:
    def __init__(self, dtype):
        self.dtype = dtype

    def __enter__(self):
        self.saved = torch.get_default_dtype()
        torch.set_default_dtype(self.dtype)

    def __exit__(self, *exc):
        torch.set_default_dtype(self.saved)


def _t(array, device, dtype=None):
    return torch.as_tensor(np.asarray(array), dtype=dtype).to(device)


# ------------------------------------------------------------------------------------------------- (a) one layer
def layer_graph(device, materialised, dtype=torch.float32):
    from ultra_torchdrug_amd.graph import Graph
    G = RF.layer_graph()
    graph = Graph(_t(G["edge_list"], device), _t(G["edge_weight"], device, torch.float32), G["num_node"], G["num_relation"])
    # (the container keeps float32 weights; a float64 run of the definition reads them -- and log(degree) of PNA -- in float64)
    graph.edge_weight = graph.edge_weight.to(dtype)
    graph.requires_grad = bool(materialised)            # the reference's switch to message + aggregate (layer.py:299)
    return graph


def layer_run(aggregate, message, device, dtype=torch.float32, materialised=False, grad=True, graph=None, masked=False,
              statistics=None):
    """One ``GeneralizedRelationalConvNBFMod`` of this package with the recorded weights on the recorded inputs: the output
    and (``grad``) the gradients of the seeded upstream, under the keys of ``reference_layers.npz``.  ``masked``: the upstream
    that is zero at the duplicate triple's row (the gradients of ``reference_layers_masked.npz``).  ``statistics``: a list that
    receives the arguments of the layer's ``_pna`` call (mean, mean of squares, max, min, degree)."""
    from ultra_torchdrug_amd.layer import GeneralizedRelationalConvNBFMod
    name = "%s_%s" % (aggregate, message)
    inputs = RF.layer_inputs(aggregate, message)
    d, n_rel = RF.LAYER_DIM, 2 * RF.LAYER_BASE_RELATIONS
    with default_dtype(dtype):
        conv = GeneralizedRelationalConvNBFMod(d, d, n_rel, d, message, aggregate, layer_norm=True, activation="relu", project=True)
        conv.load_state_dict(state_dict("layers", name))
        conv = conv.to(device=device, dtype=dtype)
        if statistics is not None:
            plain = conv._pna
            conv._pna = lambda *args: (statistics.extend(a.detach() for a in args), plain(*args))[1]
        graph = layer_graph(device, materialised, dtype) if graph is None else graph
        relation = _t(inputs["relation"], device, dtype).requires_grad_(grad)
        x = _t(inputs["input"], device, dtype).requires_grad_(grad)
        conv.relation = relation
        graph.query, graph.boundary = _t(inputs["query"], device, dtype), _t(inputs["boundary"], device, dtype)
        graph.boundary_sparse = graph.relation_tables = None
        with torch.set_grad_enabled(grad):
            out = conv(graph, x)
        got = {name + "/output": out.detach()}
        if grad:
            out.backward(_t(inputs["upstream_masked" if masked else "upstream"], device, dtype))
            got[name + "/d_input"], got[name + "/d_relation"] = x.grad, relation.grad
            for key, p in conv.named_parameters():
                got["%s/d_%s" % (name, key)] = p.grad
    return got


def pna_transe_statistics(device, route):
    """PNA over TransE, where the reference's two branches are different functions: the rspmm branch sums ``w (r^2 + x^2)`` for
    the mean of squares (``ultra/layer.py:367``), the recorded branch ``w (r + x)^2`` (``:283``).  Returns what can still be
    held: the five statistics of the rspmm route next to those of the materialised route of the same layer (which
    ``test_reference_fixtures_cpu.py::test_aten_definition_of_a_layer_equals_the_recording[pna-transe]`` holds to the recording), the cross term
    ``2 sum(w r x) / (degree + 1)`` that separates the two means of squares, and the layer outputs of both."""
    fast, slow = [], []
    with route:
        out = layer_run("pna", "transe", device, grad=False, statistics=fast)["pna_transe/output"]
    from aten_definition import AtenDefinition
    with backend_use(AtenDefinition()):
        layer_run("pna", "transe", device, grad=False, materialised=True, statistics=slow)
    inputs, G = RF.layer_inputs("pna", "transe"), RF.layer_graph()
    from ultra_torchdrug_amd.layer import GeneralizedRelationalConvNBFMod
    d, n, n_rel = RF.LAYER_DIM, RF.LAYER_NODES, 2 * RF.LAYER_BASE_RELATIONS
    conv = GeneralizedRelationalConvNBFMod(d, d, n_rel, d, "transe", "pna", layer_norm=True, activation="relu", project=True)
    conv.load_state_dict(state_dict("layers", "pna_transe"))
    with torch.no_grad():
        table = conv.double().relation_projection(torch.from_numpy(inputs["relation"])).transpose(0, 1)           # (R, B, D)
    e, w = torch.from_numpy(G["edge_list"]), torch.from_numpy(G["edge_weight"])
    cross = torch.zeros(n, len(RF.LAYER_QUERIES), d, dtype=torch.float64).index_add_(
        0, e[:, 1], 2 * w.view(-1, 1, 1) * table[e[:, 2]] * torch.from_numpy(inputs["input"])[e[:, 0]])
    cross = cross / (torch.from_numpy(np.bincount(G["edge_list"][:, 1], weights=G["edge_weight"], minlength=n)) + 1).view(-1, 1, 1)
    return [t.double().cpu().reshape(n, -1, d) if t.numel() > n else t.double().cpu() for t in fast], \
        [t.double().cpu().reshape(n, -1, d) if t.numel() > n else t.double().cpu() for t in slow], cross, out


def check_pna_transe_statistics(fast, slow, cross, floor):
    keep = [i for i in range(RF.LAYER_NODES) if i != RF.LAYER_DUPLICATE_ROW]
    for name, a, b, rows in (("mean", fast[0], slow[0], None), ("max", fast[2], slow[2], keep), ("min", fast[3], slow[3], keep),
                             ("mean of squares + cross term", fast[1] + cross, slow[1], None)):
        a, b = (a, b) if rows is None else (a[rows], b[rows])
        scale = float(b.abs().max())
        print("pna / transe %-30s %.3e of scale" % (name, float((a - b).abs().max()) / scale))
        assert float((a - b).abs().max()) <= floor * scale, (name, float((a - b).abs().max()), scale)
    assert torch.equal(fast[4].reshape(-1), slow[4].reshape(-1))                     # degree + 1


# ------------------------------------------------------------------------------------------------- (b) the entity model
def entity_model(name, device, dtype=torch.float32, remove_one_hop=False):
    from ultra_torchdrug_amd.model import TransferNBFNet
    dim, n_layers, message, aggregate = ENTITY_CONFIGS[name]
    model = TransferNBFNet(input_dim=dim, hidden_dims=[dim] * n_layers, num_relation=RF.ENTITY_RELATIONS, message_func=message,
                           aggregate_func=aggregate, short_cut=True, layer_norm=True, project=True, mod=True,
                           remove_one_hop=remove_one_hop)
    model.load_state_dict(state_dict("entity_model", name))
    return model.to(device=device, dtype=dtype).eval()


def fact_graph(device):
    from ultra_torchdrug_amd.graph import Graph
    triples = RF.entity_triples()
    return Graph(_t(triples[:RF.ENTITY_TRIPLES], device), num_node=RF.ENTITY_NODES, num_relation=RF.ENTITY_RELATIONS)


def entity_run(name, device, dtype=torch.float32, mode="plain", materialised=False, plan=None):
    """This package's ``TransferNBFNet`` with the recorded weights on the recorded batch: the scores of ``mode`` (plain / removed /
    one_hop, as recorded) and, for plain, every layer's hidden state in the recorded form.  ``plan``: keyword arguments of a
    ``RelCSR`` to walk instead of the graph's default plans (``wide_ids=True``: the row-per-group and fused-layer kernels)."""
    dim, n_layers, _, _ = ENTITY_CONFIGS[name]
    with default_dtype(dtype):
        model = entity_model(name, device, dtype, remove_one_hop=(mode == "one_hop"))
        graph = fact_graph(device)
        und = model._undirected(graph)
        und.requires_grad = bool(materialised)
        und.edge_weight = und.edge_weight.to(dtype)
        if plan is not None:
            from ultra_torchdrug_amd import RelCSR
            e = und.edge_list
            und._relcsr = RelCSR(e[:, 1].contiguous(), e[:, 0].contiguous(), e[:, 2].contiguous(), None, und.num_node, und.num_node,
                                 und.num_relation, **plan)
        h, t, r, _, _ = RF.entity_batch(RF.entity_triples())
        tables = [_t(table, device, dtype) for table in RF.rel_query_list(n_layers + 1, 4, dim)]
        hiddens = []
        handles = [conv.register_forward_hook(lambda mod, args, out: hiddens.append(out.detach())) for conv in model.layers]
        try:
            with torch.no_grad():
                all_loss = None if mode == "plain" else torch.zeros((), device=device)
                score = model(graph, tables, _t(h, device), _t(t, device), _t(r, device), all_loss=all_loss)
        finally:
            for handle in handles:
                handle.remove()
    got = {"%s/scores_%s" % (name, mode): score}
    if mode == "plain":
        assert len(hiddens) == n_layers
        for i, hidden in enumerate(hiddens):                # (the layers of this package add the shortcut themselves)
            got["%s/hidden%d_rows" % (name, i)] = hidden[list(RF.HIDDEN_ROWS)]
            got["%s/hidden%d_rowsum" % (name, i)] = hidden.double().sum(-1)
    return got


# ------------------------------------------------------------------------------------------------- (d) other architectures
def _drawn_state(tag, module, seed):
    """The weights ``RF.draw_state`` regenerates for ``module``, checked against the recorded per-tensor sums."""
    state = RF.draw_state({k: v.shape for k, v in module.state_dict().items()}, seed)
    want = stats()["architectures"]["weight_checksums"][tag]
    assert sorted(want) == sorted(state), (tag, sorted(set(want) ^ set(state)))
    for key, value in state.items():
        assert float(value.sum()) == want[key], (tag, key)
    return {k: torch.from_numpy(v) for k, v in state.items()}


def architecture_model(name, width, device, dtype=torch.float32):
    from ultra_torchdrug_amd.model import TransferNBFNet
    model = TransferNBFNet(**RF.arch_arguments(name, width))
    model.load_state_dict(_drawn_state("%s_%d" % (name, width), model, RF.arch_seed(name, width)))
    return model.to(device=device, dtype=dtype)


def architecture_run(name, width, device, dtype=torch.float32, mode="eval", materialised=False):
    """This package's ``TransferNBFNet`` in the variant ``name`` (``RF.ARCHITECTURES``) with the regenerated weights on the
    recorded inputs, under the keys of ``reference_architectures.npz``.  ``mode``: ``eval`` -- the scores of the 4 x 9 batch and
    every layer's hidden state; ``all_entities`` -- the scores of the four queries over every entity (the caller's promise
    ``all_entities=True``, as ``task.predict`` gives it); ``train`` -- train mode under grad: the scores and, for the seeded
    upstream, the compact gradient of every parameter and relation table that receives one."""
    tag = "%s_%d" % (name, width)
    triples = RF.entity_triples()
    with default_dtype(dtype):
        model = architecture_model(name, width, device, dtype)
        n_layers = len(model.layers)
        graph = fact_graph(device)
        und = model._undirected(graph)
        und.requires_grad = bool(materialised)
        und.edge_weight = und.edge_weight.to(dtype)
        tables = [_t(table, device, dtype) for table in RF.rel_query_list(n_layers + 1, 4, width)]
        if mode == "train":
            model.train()
            tables = [table.requires_grad_() for table in tables]
            h, t, r, _, _ = RF.entity_batch(triples)
            with torch.enable_grad():
                score = model(graph, tables, _t(h, device), _t(t, device), _t(r, device))
                score.backward(_t(RF.arch_upstream(name, width), device, dtype))
            got = {tag + "/train/scores": score.detach()}
            for key, p in list(model.named_parameters()) + [("rel_query_list.%d" % i, table) for i, table in enumerate(tables)]:
                if p.grad is not None:
                    got["%s/train/d_%s" % (tag, key)] = RF.compact(key, p.grad.detach().cpu().double().numpy())
            return got
        model.eval()
        if mode == "all_entities":
            h, t, r = RF.arch_all_entities(triples)
            with torch.no_grad():
                score = model(graph, tables, _t(h, device), _t(t, device), _t(r, device), all_entities=True)
            return {tag + "/scores_all": score}
        assert mode == "eval", mode
        h, t, r, _, _ = RF.entity_batch(triples)
        hiddens = []
        handles = [conv.register_forward_hook(lambda mod, args, out: hiddens.append(out.detach())) for conv in model.layers]
        try:
            with torch.no_grad():
                score = model(graph, tables, _t(h, device), _t(t, device), _t(r, device))
        finally:
            for handle in handles:
                handle.remove()
    got = {tag + "/scores": score}
    assert len(hiddens) == n_layers
    for i, hidden in enumerate(hiddens):                    # (the layers of this package add the shortcut themselves)
        got["%s/hidden%d_rows" % (tag, i)] = hidden[list(RF.HIDDEN_ROWS)]
        got["%s/hidden%d_rowsum" % (tag, i)] = hidden.double().sum(-1)
    return got


def check_gradient_keys(tag, got):
    """The gradients of a training run against the recorded set: every recorded one is there, and one the reference leaves
    ``None`` is, where this package produces it at all, exactly zero."""
    prefix = tag + "/train/d_"
    want = {k for k in stats("architectures") if k.startswith(prefix)}
    have = {k for k in got if k.startswith(prefix)}
    assert want <= have, sorted(want - have)
    for key in have - want:
        assert not np.asarray(got[key]).any(), key
    return sorted(want)


def relation_architecture_run(tag, device, materialised=False):
    """The relation-model twin: this package's ``RelNBFNet`` in the configuration ``RF.REL_ARCHITECTURES[tag]`` on the relation
    graph of the fact graph, for the batch's four relations (float32 only, as the reference's)."""
    from ultra_torchdrug_amd.rel_model import RelNBFNet, construct_relation_graph
    kwargs = RF.REL_ARCHITECTURES[tag]
    rel_model = RelNBFNet(input_type="ones", num_relation=2 * RF.ENTITY_RELATIONS, **kwargs)
    rel_model.load_state_dict(_drawn_state(tag, rel_model, 9100 + kwargs["hidden"] + kwargs["num_layers"]))
    rel_model = rel_model.float().to(device).eval()
    rel_graph = construct_relation_graph(fact_graph(device))
    rel_graph.requires_grad = bool(materialised)
    _, _, _, positives, _ = RF.entity_batch(RF.entity_triples())
    with torch.no_grad():
        out = rel_model(rel_graph, None, _t(positives[:, 2], device))["node_feature"]
    return {tag + "/relation_output": out}


# ------------------------------------------------------------------------------------------------- (c) the task
def build_task(device, **kwargs):
    """The shipped task with the recorded weights loaded through ``checkpoint.load_checkpoint``, the filter graph of all known
    triples and the fact graph of the first 1 500.  Returns ``(task, batch, negatives, (missing, unexpected))``."""
    from ultra_torchdrug_amd.checkpoint import load_checkpoint
    from ultra_torchdrug_amd.graph import Graph
    from ultra_torchdrug_amd.task import build_ultra
    triples = RF.entity_triples()
    _, _, _, positives, negatives = RF.entity_batch(triples)
    options = dict(num_negative=negatives.shape[1], metric=tuple(stats()["metrics"]))
    options.update(kwargs)
    task = build_ultra(RF.ENTITY_RELATIONS, **options)
    state = state_dict("entity_model", "main", "model.")
    state.update(state_dict("pipeline", "rel_models.0", "rel_models.0."))
    keys = load_checkpoint(task, {"model": state})
    mask = torch.zeros(len(triples), dtype=torch.bool)
    mask[:RF.ENTITY_TRIPLES] = True
    task.preprocess(Graph(torch.from_numpy(triples), num_node=RF.ENTITY_NODES, num_relation=RF.ENTITY_RELATIONS), mask)
    return task.to(device), _t(positives, device), _t(negatives, device), keys


def train_step_run(task, batch, negatives, temperature):
    """Loss and compact gradients (``reference_fixture.compact``) of one training step on the recorded negatives."""
    task.train()
    task.adversarial_temperature = temperature
    task.zero_grad(set_to_none=True)
    task._static_negative = negatives
    try:
        loss, _ = task(batch)
        loss.backward()
    finally:
        task._static_negative = None
    return compact_gradients(task, loss, temperature)


def compact_gradients(task, loss, temperature):
    tag = "train_t%d" % int(temperature)
    got = {tag + "/loss": loss.detach().reshape(1)}
    for key, p in task.named_parameters():
        if p.grad is not None:
            got["%s/d_%s" % (tag, key)] = RF.compact(key, p.grad.detach().cpu().double().numpy())
    return got


def rank_classes(pred, positives, mask, tolerance):
    """Issue "Ranks": per (triple, side) the number of unfiltered candidates whose recorded score lies within twice the score
    tolerance of the target's.  0: the rank is compared exactly; otherwise within that number."""
    pred = np.asarray(pred, dtype=np.float64)
    target = np.stack([positives[:, 1], positives[:, 0]], axis=1)
    near = np.zeros(target.shape, dtype=np.int64)
    for b in range(pred.shape[0]):
        for side in range(2):
            keep = mask[b, side].copy()
            keep[target[b, side]] = False
            near[b, side] = int((np.abs(pred[b, side] - pred[b, side, target[b, side]])[keep] <= 2 * tolerance).sum())
    return near


def recorded_mask():
    packed = arrays("pipeline")["filter_mask"]
    return np.unpackbits(packed, axis=-1)[..., :RF.ENTITY_NODES].astype(bool)

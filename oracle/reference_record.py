"""Test infrastructure: record runs of the REFERENCE'S OWN Python on small graphs as fixtures under ``tests/golden/``.

    python -m oracle.reference_record [--reference PATH] [--out DIR] [--check [--last-bits]]

The reference's ``ultra/layer.py``, ``model.py``, ``rel_model.py`` and ``task.py`` are loaded unmodified from ``PATH`` over the
stand-in modules of ``oracle/torchdrug_standin.py`` (its DECISIONS list what the stand-in decides) and run on the CPU with one
thread.  The inputs come from ``tests/reference_fixture.py``, which the tests share; weights are drawn on a grid of multiples of
2^-10 and stored as float16 under the reference's own state-dict names.  ``--check`` records into memory and compares with the
committed files instead of writing.

What the files pin is the reference's Python: ``message`` + ``aggregate`` of its layers, its two stacks, scoring, ``predict``,
ranking, metrics, the loss and its gradients.  They do NOT pin torchdrug's native ``generalized_rspmm`` (its summation order, its
identity for an empty min / max row), ``variadic_sample`` (the negatives are inputs here) or the checkpoints.

Files (every tensor ``x`` as ``x/T`` = the float64 run where one exists and ``x/R0`` = the float32 run):

* ``reference_layers.npz``: one ``GeneralizedRelationalConvNBFMod`` per (sum, mean, max, pna) x (distmult, transe, rotate): output
  and the gradients of a seeded upstream with respect to the input, the relation table and every parameter.
* ``reference_layers_masked.npz``: for max and pna a second gradient run of the same layers whose upstream is zero at the row the
  duplicate triple ends in.  No gradient passes through that row, where the reference's rspmm branch (one edge of summed weight)
  and the recorded branch (two messages) are different functions for min / max; everywhere else they agree, so these are the
  gradients the rspmm route of this package is held to.
* ``reference_entity_model.npz``: ``TransferNBFNet`` 6 x 64 in the shipped configuration on 211 nodes / 1 500 triples / 11
  relations, B = 4 x 9 candidates: scores (plain, with the batch's edges removed, with the one-hop rule), and every layer's hidden
  state as its whole rows at ``HIDDEN_ROWS`` plus the sum over the features of EVERY row (whole states would be 0.4 MB each;
  ``node_feature`` is the last of them next to the query rows, which the helper regenerates);
  two smaller 2-layer records (rotate / sum, pna / distmult, 16 wide) in the same form.
* ``reference_pipeline.npz``: relation graph (integers), ``RelNBFNet`` output, ``predict`` over all entities, ranks, metrics, and
  the training branch + loss for ``adversarial_temperature`` 1 and 0 with every parameter gradient in the compact form of
  ``reference_fixture.compact``.  The relation model is float32 only (``rel_model.py:353``): runs ``R0`` .. ``R4``, ``R1`` .. ``R4``
  with the edge lists of both graphs permuted (the same multiset of edges: equally valid runs).
* ``reference_architectures.npz``: ``TransferNBFNet`` with 3 layers in the variants of ``reference_fixture.ARCHITECTURES`` (one
  argument of the shipped set changed each; the reference's constructor defaults; max; mean of TransE) at 64 and 16 columns,
  ``base`` and ``max_plain`` also at 6, on the entity record's graph, batch and relation tables: eval scores of the batch and of
  its four queries over all entities, hidden states in the compact form, and a train-mode run under grad (scores, compact
  gradients of a seeded upstream, stacked into one matrix per case in the sorted order of their names).  The weights are NOT
  stored (``RF.draw_state`` regenerates them; the json holds a float64 sum per tensor), and only the batch's scores keep ``R0``.
  Two ``RelNBFNet`` (16 wide; 2 layers at 64) on the relation graph, float32, ``ref_dev`` over two runs on permuted edge lists.
  Not recorded, because the reference's code raises: ``symmetric=True``, unequal ``hidden_dims``, ``mod=False, project=False``.
* ``reference_fixtures.json``: shapes, seeds, torch version, and per tensor ``scale`` and ``ref_dev`` (``max|R0 - T|``, or
  ``max_k max|Rk - R0|``).  Its ``mi355x`` section (floors measured on the device) is kept as it is.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import reference_fixture as RF                      # noqa: E402
from oracle import torchdrug_standin as standin     # noqa: E402

SCORE_FLOOR_CAP = 2e-5          # the largest floor a score comparison may be granted (tests/test_reference_definition_gpu.py)
FILES = ("reference_layers.npz", "reference_layers_masked.npz", "reference_entity_model.npz", "reference_pipeline.npz",
         "reference_architectures.npz")
METRICS = ("mr", "mrr", "hits@1", "hits@3", "hits@10", "mrr-tail", "hits@1-tail", "hits@10-tail", "mrr-head")


class Record:
    """Arrays of one file plus the json entries of its float tensors."""

    def __init__(self):
        self.arrays, self.stats = {}, {}

    def integer(self, name, value):
        self.arrays[name] = np.asarray(value)

    def weights(self, prefix, state):
        for key, value in state.items():
            half = np.asarray(value, dtype=np.float16)
            assert (half.astype(np.float64) == np.asarray(value, dtype=np.float64)).all(), key
            self.arrays["%s/%s" % (prefix, key)] = half

    def tensor(self, name, truth=None, runs=()):
        runs = [np.asarray(r, dtype=np.float32) for r in runs]
        if truth is not None:
            truth = np.asarray(truth, dtype=np.float64)
            self.arrays[name + "/T"] = truth
            dev = float(np.abs(runs[0].astype(np.float64) - truth).max()) if runs else 0.0
            scale = float(np.abs(truth).max())
        else:
            dev = max([float(np.abs(r.astype(np.float64) - runs[0].astype(np.float64)).max()) for r in runs[1:]] or [0.0])
            scale = float(np.abs(runs[0]).max())
        for k, run in enumerate(runs):
            self.arrays["%s/R%d" % (name, k)] = run
        self.stats[name] = dict(scale=scale, ref_dev=dev, shape=list((truth if truth is not None else runs[0]).shape))


def _t(array, dtype=None):
    return torch.as_tensor(np.asarray(array), dtype=dtype)


def _load_state(module, state, dtype):
    module.load_state_dict({k: _t(v, dtype) for k, v in state.items()})
    return module.to(dtype)


def _np(tensor):
    return tensor.detach().cpu().numpy()


# --------------------------------------------------------------------------------------------------------- (a)
def record_layers(U):
    """-> (the twelve layers, the second gradient run of max / pna whose upstream is zero at the duplicate triple's row)."""
    rec, masked = Record(), Record()
    G = RF.layer_graph()
    d = RF.LAYER_DIM
    for aggregate in RF.AGGREGATES:
        for message in RF.MESSAGES:
            name = "%s_%s" % (aggregate, message)
            inputs = RF.layer_inputs(aggregate, message)
            results = {}
            for tag, dtype in (("T", torch.float64), ("R0", torch.float32)):
                torch.set_default_dtype(dtype)
                try:
                    graph = standin.Graph(G["edge_list"], G["edge_weight"], G["num_node"], G["num_relation"])
                    conv = U.layer.GeneralizedRelationalConvNBFMod(d, d, G["num_relation"], d, message, aggregate, layer_norm=True,
                                                                   activation="relu", project=True)
                    if tag == "T":
                        state = RF.draw_state({k: v.shape for k, v in conv.state_dict().items()}, 100 + len(rec.stats))
                        rec.weights(name, state)
                    _load_state(conv, state, dtype)
                    relation = _t(inputs["relation"], dtype).requires_grad_()
                    x = _t(inputs["input"], dtype).requires_grad_()
                    conv.relation = relation
                    graph.query, graph.boundary = _t(inputs["query"], dtype), _t(inputs["boundary"], dtype)
                    out = conv(graph, x)
                    out.backward(_t(inputs["upstream"], dtype), retain_graph=True)
                    got = {"output": _np(out), "d_input": _np(x.grad), "d_relation": _np(relation.grad)}
                    for key, p in conv.named_parameters():
                        got["d_" + key] = _np(p.grad)
                    results[tag] = got
                    if aggregate in RF.MASKED_AGGREGATES:
                        x.grad = relation.grad = None
                        conv.zero_grad(set_to_none=True)
                        out.backward(_t(inputs["upstream_masked"], dtype))
                        again = {"d_input": _np(x.grad), "d_relation": _np(relation.grad)}
                        for key, p in conv.named_parameters():
                            again["d_" + key] = _np(p.grad)
                        results[tag + "/masked"] = again
                finally:
                    torch.set_default_dtype(torch.float32)
            for key in results["T"]:
                rec.tensor("%s/%s" % (name, key), results["T"][key], [results["R0"][key]])
            for key in results.get("T/masked", ()):
                masked.tensor("%s/%s" % (name, key), results["T/masked"][key], [results["R0/masked"][key]])
    return rec, masked


# --------------------------------------------------------------------------------------------------------- (b)
def _spy_hiddens(model):
    """Every layer's hidden state AFTER the shortcut: the input of the next layer, and the node feature's first half."""
    seen = {"inputs": [], "feature": None}
    handles = [conv.register_forward_pre_hook(lambda mod, args: seen["inputs"].append(args[1].detach())) for conv in model.layers]
    plain = model.bellmanford

    def spy(*args, **kwargs):
        out = plain(*args, **kwargs)
        seen["feature"] = out["node_feature"].detach()
        return out
    model.bellmanford = spy

    def hiddens():
        # (the last hidden state stands right before the query columns, with and without ``concat_hidden``; equal widths)
        width = seen["inputs"][-1].shape[-1]
        return seen["inputs"][1:] + [seen["feature"][..., -2 * width:-width]]

    def release():
        for handle in handles:
            handle.remove()
        del model.bellmanford
    return seen, hiddens, release


def _entity_run(U, dtype, state, triples, dim, n_layers, message, aggregate, rel_list):
    torch.set_default_dtype(dtype)
    try:
        h, t, r, positives, negatives = RF.entity_batch(triples)
        h, t, r = _t(h), _t(t), _t(r)
        got = {}
        for mode in ("plain", "removed", "one_hop"):
            model = U.model.TransferNBFNet(input_dim=dim, hidden_dims=[dim] * n_layers, num_relation=RF.ENTITY_RELATIONS,
                                           message_func=message, aggregate_func=aggregate, short_cut=True, layer_norm=True,
                                           project=True, mod=True, remove_one_hop=(mode == "one_hop"))
            if state is None:
                state = RF.draw_state({k: v.shape for k, v in model.state_dict().items()}, 7000 + dim + n_layers)
            _load_state(model, state, dtype).eval()
            graph = standin.Graph(triples[:RF.ENTITY_TRIPLES], None, RF.ENTITY_NODES, RF.ENTITY_RELATIONS)
            tables = [_t(table, dtype) for table in rel_list]
            seen, hiddens, release = _spy_hiddens(model)
            with torch.no_grad():
                all_loss = None if mode == "plain" else torch.zeros(())
                score = model(graph, tables, h, t, r, all_loss=all_loss)
            release()
            got["scores_" + mode] = _np(score)
            if mode == "plain":
                for i, hidden in enumerate(hiddens()):
                    got["hidden%d_rows" % i] = _np(hidden[list(RF.HIDDEN_ROWS)])
                    got["hidden%d_rowsum" % i] = _np(hidden.sum(-1))
        return got, state
    finally:
        torch.set_default_dtype(torch.float32)


def record_entity(U):
    rec = Record()
    triples = RF.entity_triples()
    configs = [("main", 64, 6, "distmult", "sum"), ("small_rotate_sum", RF.SMALL_DIM, 2, "rotate", "sum"),
               ("small_pna_distmult", RF.SMALL_DIM, 2, "distmult", "pna")]
    for name, dim, n_layers, message, aggregate in configs:
        rel_list = RF.rel_query_list(n_layers + 1, 4, dim)
        truth, state = _entity_run(U, torch.float64, None, triples, dim, n_layers, message, aggregate, rel_list)
        single, _ = _entity_run(U, torch.float32, state, triples, dim, n_layers, message, aggregate, rel_list)
        rec.weights(name, state)
        for key in truth:
            rec.tensor("%s/%s" % (name, key), truth[key], [single[key]])
    return rec


# --------------------------------------------------------------------------------------------------------- (c)
def _harness(U, model, rel_model, fact_graph, graph, rel_graph, negatives, temperature):
    """The task's functions on a plain object that carries what they read (``task.py:228-277, 279-295, 307-351, 160-195``)."""
    task = U.task.KnowledgeGraphCompletionAdapted
    names = ("predict", "target", "get_ranking", "evaluate", "_calculate_t_mask", "_calculate_h_mask", "forward")
    members = {n: getattr(task, n) for n in names}
    members["_strict_negative"] = lambda self, *index: _t(negatives)
    holder = type("RecordedTask", (), members)()
    holder.__dict__.update(model=model, rel_models=[rel_model], rel_graphs=[rel_graph], fact_graph=fact_graph, graph=graph,
                           num_entity=RF.ENTITY_NODES, num_relation=RF.ENTITY_RELATIONS, num_negative=negatives.shape[1],
                           full_batch_eval=True, device=torch.device("cpu"), filtered_ranking=True, metric=METRICS,
                           criterion={"bce": 1}, adversarial_temperature=temperature, sample_weight=False, strict_negative=True,
                           metric_per_rel=False)
    return holder


def record_pipeline(U, entity_state):
    rec = Record()
    triples = RF.entity_triples()
    _, _, _, positives, negatives = RF.entity_batch(triples)
    batch = _t(positives)
    torch.manual_seed(0)
    model = U.model.TransferNBFNet(input_dim=64, hidden_dims=[64] * 6, num_relation=RF.ENTITY_RELATIONS, message_func="distmult",
                                   aggregate_func="sum", short_cut=True, layer_norm=True, project=True, mod=True)
    _load_state(model, entity_state, torch.float32)
    rel_model = U.rel_model.RelNBFNet(input_dim=64, hidden=64, num_layers=6, input_type="ones",
                                      num_relation=2 * RF.ENTITY_RELATIONS)
    rel_state = RF.draw_state({k: v.shape for k, v in rel_model.state_dict().items()}, 9001)
    _load_state(rel_model, rel_state, torch.float32)
    rec.weights("rel_models.0", rel_state)
    graph = standin.Graph(triples, None, RF.ENTITY_NODES, RF.ENTITY_RELATIONS)
    fact = standin.Graph(triples[:RF.ENTITY_TRIPLES], None, RF.ENTITY_NODES, RF.ENTITY_RELATIONS)
    rel_graph = rel_model.construct_relation_graph(fact)
    assert rel_graph.num_node == 2 * RF.ENTITY_RELATIONS and rel_graph.num_relation == 4
    rec.integer("relation_graph/edge_list", _np(rel_graph.edge_list).astype(np.int16))

    runs = []
    rng = np.random.RandomState(5)
    for k in range(5):
        fact_k, rel_k = fact, rel_graph
        if k:
            fact_k = fact.edge_mask(_t(rng.permutation(fact.num_edge)))
            rel_k = rel_graph.edge_mask(_t(rng.permutation(rel_graph.num_edge)))
        got = {}
        model.eval(), rel_model.eval()
        task = _harness(U, model, rel_model, fact_k, graph, rel_k, negatives, 1.0)
        with torch.no_grad():
            got["relation_output"] = _np(rel_model(rel_k, None, batch[:, 2])["node_feature"])
            pred = task.predict(batch)
            target = task.target(batch)
            got["predict"] = _np(pred)
            got["ranking"] = _np(task.get_ranking(pred, target))
            got["filter_mask"] = _np(target[0])
            got["metrics"] = np.array([float(v) for v in task.evaluate(pred, target).values()])
        model.train(), rel_model.train()
        for temperature in (1.0, 0.0):
            task = _harness(U, model, rel_model, fact_k, graph, rel_k, negatives, temperature)
            model.zero_grad(set_to_none=True), rel_model.zero_grad(set_to_none=True)
            loss, _ = task.forward(batch)
            loss.backward()
            tag = "train_t%d" % int(temperature)
            got[tag + "/loss"] = _np(loss).reshape(1)
            for prefix, module in (("model.", model), ("rel_models.0.", rel_model)):
                for key, p in module.named_parameters():
                    if p.grad is not None:
                        got["%s/d_%s%s" % (tag, prefix, key)] = RF.compact(prefix + key, _np(p.grad))
        runs.append(got)
    first = runs[0]
    rec.integer("ranking", first["ranking"])
    rec.integer("filter_mask", np.packbits(first["filter_mask"], axis=-1))
    assert all((run["ranking"] == first["ranking"]).all() for run in runs), "the reference's own runs rank differently"
    for key in first:
        if key in ("ranking", "filter_mask"):
            continue
        if key == "relation_output" or "/d_" in key:     # R1 .. R4 enter ref_dev; only R0 is stored
            rec.tensor(key, None, [run[key] for run in runs])
            for k in range(1, 5):
                del rec.arrays["%s/R%d" % (key, k)]
            continue
        rec.tensor(key, None, [run[key] for run in runs])
    _assert_tie_condition(first, rec.stats["predict"], positives)
    return rec


def _assert_tie_condition(run, stat, positives):
    """Issue, "Ranks": at most 10 % of the (triple, side) pairs may have an unfiltered candidate within twice the score tolerance
    of the target -- checked on the reference alone, with the largest floor a score comparison may be granted."""
    tolerance = 4 * stat["ref_dev"] + SCORE_FLOOR_CAP * stat["scale"]
    pred, mask = run["predict"].astype(np.float64), run["filter_mask"].copy()
    target = np.stack([positives[:, 1], positives[:, 0]], axis=1)
    near = 0
    for b in range(pred.shape[0]):
        for side in range(2):
            gap = np.abs(pred[b, side] - pred[b, side, target[b, side]])
            mask[b, side, target[b, side]] = False
            near += bool((gap[mask[b, side]] <= 2 * tolerance).any())
    stat["score_tolerance_cap"], stat["near_tie_pairs"] = tolerance, near
    assert near <= 0.1 * pred.shape[0] * 2, "%d of %d (triple, side) pairs are near ties: change the seed" % (near, 2 * len(pred))


# --------------------------------------------------------------------------------------------------------- (d)
def _compact_gradients(got, model, tables):
    for key, p in model.named_parameters():
        if p.grad is not None:
            got["train/d_" + key] = RF.compact(key, _np(p.grad))
    for i, table in enumerate(tables):
        if table.grad is not None:
            got["train/d_rel_query_list.%d" % i] = RF.compact("rel_query_list.%d" % i, _np(table.grad))


def _architecture_run(U, dtype, name, width, state, triples):
    """Eval (batch scores, scores over all entities, hidden states) and one training forward + backward of one variant."""
    torch.set_default_dtype(dtype)
    try:
        kwargs = RF.arch_arguments(name, width)
        model = U.model.TransferNBFNet(**kwargs)
        if state is None:
            state = RF.draw_state({k: v.shape for k, v in model.state_dict().items()}, RF.arch_seed(name, width))
        _load_state(model, state, dtype).eval()
        n_layers = len(kwargs["hidden_dims"])
        h, t, r, _, _ = RF.entity_batch(triples)
        got = {}
        with torch.no_grad():
            tables = [_t(table, dtype) for table in RF.rel_query_list(n_layers + 1, 4, width)]
            graph = standin.Graph(triples[:RF.ENTITY_TRIPLES], None, RF.ENTITY_NODES, RF.ENTITY_RELATIONS)
            seen, hiddens, release = _spy_hiddens(model)
            got["scores"] = _np(model(graph, tables, _t(h), _t(t), _t(r)))
            release()
            for i, hidden in enumerate(hiddens()):
                got["hidden%d_rows" % i] = _np(hidden[list(RF.HIDDEN_ROWS)])
                got["hidden%d_rowsum" % i] = _np(hidden.sum(-1))
            ha, ta, ra = RF.arch_all_entities(triples)
            got["scores_all"] = _np(model(graph, tables, _t(ha), _t(ta), _t(ra)))
        model.train()
        tables = [_t(table, dtype).requires_grad_() for table in RF.rel_query_list(n_layers + 1, 4, width)]
        graph = standin.Graph(triples[:RF.ENTITY_TRIPLES], None, RF.ENTITY_NODES, RF.ENTITY_RELATIONS)
        score = model(graph, tables, _t(h), _t(t), _t(r))
        score.backward(_t(RF.arch_upstream(name, width), dtype))
        got["train/scores"] = _np(score)
        _compact_gradients(got, model, tables)
        return got, state
    finally:
        torch.set_default_dtype(torch.float32)


def record_architectures(U):
    """``TransferNBFNet`` in the variants of ``reference_fixture.ARCHITECTURES`` (3 layers; 64, 16 and -- two of them -- 6 wide) on
    the entity record's graph, batch and relation tables, and two ``RelNBFNet`` on the pipeline record's relation graph.  The
    weights are not stored: ``RF.draw_state`` regenerates them, and the returned checksums (float64 sum per tensor) pin the draw.
    Min / max (``max_plain``, ``defaults``): the fact graph with inverse edges holds every triple once (asserted), so the recorded
    branch and the rspmm branch are one function on EVERY row, and no row is left out."""
    rec, checksums = Record(), {}
    triples = RF.entity_triples()
    assert RF.undirected_is_distinct(triples), "a duplicate triple: min / max of the two branches differ at its row"
    for name, width in RF.ARCH_CASES:
        truth, state = _architecture_run(U, torch.float64, name, width, None, triples)
        single, _ = _architecture_run(U, torch.float32, name, width, state, triples)
        assert sorted(truth) == sorted(single)
        tag = "%s_%d" % (name, width)
        checksums[tag] = {key: float(np.asarray(value, dtype=np.float64).sum()) for key, value in state.items()}
        into = rec
        for key in truth:
            into.tensor("%s/%s" % (tag, key), truth[key], [single[key]])
            if key not in ("scores", "train/scores"):     # ref_dev is kept; the float32 run itself for the batch's scores only
                del into.arrays["%s/%s/R0" % (tag, key)]
        # the compact gradients (50 numbers each) as ONE matrix, rows in the sorted order of their names: a zip member per
        # gradient would cost as much as its numbers (``reference_runs.arrays`` unpacks them under their own keys)
        names = sorted(key for key in truth if key.startswith("train/d_"))
        into.arrays["%s/train/gradients/T" % tag] = np.stack([into.arrays.pop("%s/%s/T" % (tag, key)) for key in names])
    # the relation model: float32 only (rel_model.py:353)
    fact = standin.Graph(triples[:RF.ENTITY_TRIPLES], None, RF.ENTITY_NODES, RF.ENTITY_RELATIONS)
    _, _, _, positives, _ = RF.entity_batch(triples)
    for tag, kwargs in RF.REL_ARCHITECTURES.items():
        rel_model = U.rel_model.RelNBFNet(input_type="ones", num_relation=2 * RF.ENTITY_RELATIONS, **kwargs)
        state = RF.draw_state({k: v.shape for k, v in rel_model.state_dict().items()}, 9100 + kwargs["hidden"] + kwargs["num_layers"])
        _load_state(rel_model, state, torch.float32).eval()
        checksums[tag] = {key: float(np.asarray(value, dtype=np.float64).sum()) for key, value in state.items()}
        rel_graph = rel_model.construct_relation_graph(fact)
        runs = []
        rng = np.random.RandomState(6)
        for k in range(3):                  # the edge list permuted: equally valid runs, whose spread is ref_dev
            rel_k = rel_graph if not k else rel_graph.edge_mask(_t(rng.permutation(rel_graph.num_edge)))
            with torch.no_grad():
                runs.append(_np(rel_model(rel_k, None, _t(positives[:, 2]))["node_feature"]))
        rec.tensor(tag + "/relation_output", None, runs)
        for k in (1, 2):
            del rec.arrays["%s/relation_output/R%d" % (tag, k)]
    return rec, checksums


# --------------------------------------------------------------------------------------------------------- driver
def record(reference):
    torch.set_num_threads(1)
    torch.manual_seed(0)
    U = standin.load_reference(reference)
    layers, masked = record_layers(U)
    entity = record_entity(U)
    state = {k[len("main/"):]: v.astype(np.float64) for k, v in entity.arrays.items() if k.startswith("main/") and v.dtype == np.float16}
    pipeline = record_pipeline(U, state)
    architectures, checksums = record_architectures(U)
    records = dict(zip(FILES, (layers, masked, entity, pipeline, architectures)))
    meta = dict(torch=torch.__version__.split("+")[0], numpy_stream="RandomState (MT19937)", threads=1, grid="2^-10",
                seeds=dict(torch_manual_seed=0, layer_graph=370, layer_inputs="1000 + 10 * aggregate + message", layer_weights="100 + 11 * pair",
                           entity_triples=211, entity_batch=49, rel_query_list="77 + dim", entity_weights="7000 + dim + layers",
                           relation_weights=9001, edge_permutations=5, compact="sum of the name's characters + size",
                           architecture_weights="8000 + 100 * variant + width", architecture_upstream="weights' seed + 50000",
                           architecture_relation_weights="9100 + hidden + layers", architecture_edge_permutations=6),
                architectures=dict(layers=RF.ARCH_LAYERS, cases=[list(c) for c in RF.ARCH_CASES], not_runnable=RF.ARCH_NOT_RUNNABLE,
                                   relation_models=RF.REL_ARCHITECTURES, weight_checksums=checksums),
                metrics=list(METRICS), hidden_rows=list(RF.HIDDEN_ROWS), layer_dim=RF.LAYER_DIM,
                layer_duplicate_row=RF.LAYER_DUPLICATE_ROW,
                shapes=dict(layer_graph=[RF.LAYER_NODES, int(len(RF.layer_graph()["edge_list"])), 2 * RF.LAYER_BASE_RELATIONS],
                            entity_graph=[RF.ENTITY_NODES, RF.ENTITY_TRIPLES, RF.ENTITY_RELATIONS], batch=[4, 9]),
                tensors={name: rec.stats for name, rec in records.items()})
    return records, meta


def main(argv=None):
    parser = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    parser.add_argument("--reference", default=os.environ.get("ULTRA_REFERENCE", "/root/reference"))
    parser.add_argument("--out", default=os.path.join(ROOT, "tests", "golden"))
    parser.add_argument("--check", action="store_true", help="compare with the committed files (equality), write nothing")
    parser.add_argument("--last-bits", action="store_true", help="with --check: list, do not count, floats that moved in their last bits")
    args = parser.parse_args(argv)
    records, meta = record(args.reference)
    json_path = os.path.join(args.out, "reference_fixtures.json")
    if args.check:
        # integers, weights and floats: EQUAL.  ``--last-bits`` (never used by the tests): on a CPU whose BLAS picks another kernel
        # behind nn.Linear, float arrays within 1e-6 (float32) / 1e-12 (float64) of their scale are listed but not counted
        worst = moved = 0
        for name, rec in records.items():
            with np.load(os.path.join(args.out, name)) as have:
                assert sorted(have.files) == sorted(rec.arrays), "%s: other tensors than recorded" % name
                for key, value in rec.arrays.items():
                    old = have[key]
                    if old.shape == value.shape and old.dtype == value.dtype and np.array_equal(old, value):
                        continue
                    close = False
                    if args.last_bits and old.shape == value.shape and old.dtype == value.dtype and value.dtype in (np.float32, np.float64):
                        eps = 1e-12 if value.dtype == np.float64 else 1e-6
                        close = bool(np.abs(old.astype(np.float64) - value).max() <= eps * max(np.abs(old).max(), 1e-30))
                    moved += close
                    worst += not close
                    print("%s %s %s" % ("last bits" if close else "DIFFERS", name, key))
        with open(json_path) as f:
            have = json.load(f)
        have.pop("mi355x", None)
        if not moved and have != json.loads(json.dumps(meta)):       # (ref_dev moves with the arrays)
            print("DIFFERS reference_fixtures.json")
            worst += 1
        print("check: %s" % ("%d differences" % worst if worst else "the committed fixtures are reproduced"
                             + (" (%d float arrays moved in their last bits)" % moved if moved else "")))
        return 1 if worst else 0
    kept = None
    if os.path.isfile(json_path):
        with open(json_path) as f:
            kept = json.load(f).get("mi355x")
    for name, rec in records.items():
        np.savez_compressed(os.path.join(args.out, name), **rec.arrays)
        print("%s: %d arrays, %d bytes" % (name, len(rec.arrays), os.path.getsize(os.path.join(args.out, name))))
    if kept is not None:
        meta["mi355x"] = kept
    with open(json_path, "w") as f:
        json.dump(meta, f, indent=1, sort_keys=True)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())

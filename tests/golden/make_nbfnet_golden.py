"""Regenerates tests/golden/reference_nbfnet.npz and reference_nbfnet.json: runs of the REFERENCE'S OWN
``NeuralBellmanFordNetwork`` (``ultra/model.py:198-392``, ``models.NBFNet``) that this package's class of the same name is held to.

The reference's ``model.py`` and ``layer.py`` are loaded unmodified over the stand-in modules of ``oracle/torchdrug_standin.py``
(``load_reference``) and run on the CPU with one thread, with the helpers of ``oracle/reference_record.py``.  Graph, triples and the
4 x 9 batch are those of ``tests/reference_fixture.py``; the cases, their seeds and their batches are in ``tests/nbfnet_cases.py``,
which the tests share.  Four cases of 3 layers each:

    shipped64       64-d, distmult / sum, short_cut, layer_norm, dependent=True: eval scores of the batch, scores of its four
                    queries over all entities, hidden states (whole rows at HIDDEN_ROWS + the row sums of every node), and a
                    train-mode run with ``all_loss`` (the batch's edges removed) with the compact gradients of every parameter
    paper32         32-d, distmult / pna, short_cut, layer_norm, dependent=True: the eval tensors
    independent16   16-d, transe / sum, dependent=False: eval and train tensors
    homogeneous16   num_relation=None, 16-d, distmult / sum on the graph without its relation column: eval scores of 1-D h, t and
                    the train tensors

Every tensor ``x`` is kept as ``x/T``, the float64 run; the float32 run ``x/R0`` is kept for the batch's scores only, the json has
``scale`` and ``ref_dev = max|R0 - T|`` of every tensor (``Record.tensor``).  The weights come from ``RF.draw_state`` and are not
stored: the json pins a float64 sum per tensor, and lists the state dict's keys and shapes.

    python tests/golden/make_nbfnet_golden.py [--reference PATH] [--check]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))

import nbfnet_cases as NC                           # noqa: E402
import reference_fixture as RF                      # noqa: E402
from oracle import reference_record as REC          # noqa: E402
from oracle import torchdrug_standin as standin     # noqa: E402

FILE, META = "reference_nbfnet.npz", "reference_nbfnet.json"


def _run(U, dtype, name, state, triples):
    torch.set_default_dtype(dtype)
    try:
        model = U.model.NeuralBellmanFordNetwork(**NC.CASES[name])
        if state is None:
            state = RF.draw_state({k: v.shape for k, v in model.state_dict().items()}, NC.seed(name))
        REC._load_state(model, state, dtype).eval()
        edge_list, n_rel = NC.edges(name, triples)
        to = lambda a: None if a is None else REC._t(a)
        h, t, r = (to(a) for a in NC.batch(name, triples))
        got = {}
        with torch.no_grad():
            graph = standin.Graph(edge_list, None, RF.ENTITY_NODES, n_rel)
            seen, hiddens, release = REC._spy_hiddens(model)
            got["scores"] = REC._np(model(graph, h, t, r))
            release()
            if name in NC.HIDDEN:
                for i, hidden in enumerate(hiddens()):
                    got["hidden%d_rows" % i] = REC._np(hidden[list(RF.HIDDEN_ROWS)])
                    got["hidden%d_rowsum" % i] = REC._np(hidden.sum(-1))
                ha, ta, ra = RF.arch_all_entities(triples)
                got["scores_all"] = REC._np(model(graph, REC._t(ha), REC._t(ta), REC._t(ra)))
        if name in NC.TRAINED:
            model.train()
            graph = standin.Graph(edge_list, None, RF.ENTITY_NODES, n_rel)
            score = model(graph, h, t, r, all_loss=torch.zeros(()))
            score.backward(REC._t(NC.upstream(name, triples), dtype))
            got["train/scores"] = REC._np(score)
            REC._compact_gradients(got, model, ())
        shapes = {k: list(v.shape) for k, v in model.state_dict().items()}
        return got, state, shapes
    finally:
        torch.set_default_dtype(torch.float32)


def record(reference):
    torch.set_num_threads(1)
    torch.manual_seed(0)
    U = standin.load_reference(reference)
    rec, checksums, state_shapes = REC.Record(), {}, {}
    triples = RF.entity_triples()
    for name in NC.CASES:
        truth, state, shapes = _run(U, torch.float64, name, None, triples)
        single, _, _ = _run(U, torch.float32, name, state, triples)
        assert sorted(truth) == sorted(single)
        checksums[name] = {key: float(np.asarray(value, dtype=np.float64).sum()) for key, value in state.items()}
        state_shapes[name] = shapes
        for key in truth:
            rec.tensor("%s/%s" % (name, key), truth[key], [single[key]])
            if key not in ("scores", "train/scores"):
                del rec.arrays["%s/%s/R0" % (name, key)]
        names = sorted(key for key in truth if key.startswith("train/d_"))
        if names:        # the compact gradients (50 numbers each) as one matrix, rows in the sorted order of their names
            rec.arrays["%s/train/gradients/T" % name] = np.stack([rec.arrays.pop("%s/%s/T" % (name, key)) for key in names])
    meta = dict(torch=torch.__version__.split("+")[0], threads=1, grid="2^-10", layers=NC.LAYERS,
                cases={name: dict(kwargs) for name, kwargs in NC.CASES.items()},
                seeds=dict(torch_manual_seed=0, weights="12000 + 100 * case + width", upstream="weights' seed + 50000",
                           entity_triples=211, entity_batch=49, compact="sum of the name's characters + size"),
                shapes=dict(entity_graph=[RF.ENTITY_NODES, RF.ENTITY_TRIPLES, RF.ENTITY_RELATIONS], batch=[4, 9], homogeneous_batch=[36]),
                hidden_rows=list(RF.HIDDEN_ROWS), trained=list(NC.TRAINED), state_dict=state_shapes, weight_checksums=checksums,
                tensors=rec.stats)
    return rec, meta


def main(argv=None):
    parser = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    parser.add_argument("--reference", default=os.environ.get("ULTRA_REFERENCE", "/root/reference"))
    parser.add_argument("--out", default=HERE)
    parser.add_argument("--check", action="store_true", help="compare with the committed files (equality), write nothing")
    args = parser.parse_args(argv)
    rec, meta = record(args.reference)
    meta = json.loads(json.dumps(meta))
    if args.check:
        worst = 0
        with np.load(os.path.join(args.out, FILE)) as have:
            if sorted(have.files) != sorted(rec.arrays):
                print("DIFFERS %s: other tensors than recorded" % FILE)
                worst += 1
            for key, value in rec.arrays.items():
                if key in have.files and not (have[key].shape == value.shape and have[key].dtype == value.dtype
                                              and np.array_equal(have[key], value)):
                    print("DIFFERS %s %s" % (FILE, key))
                    worst += 1
        with open(os.path.join(args.out, META)) as f:
            if json.load(f) != meta:
                print("DIFFERS %s" % META)
                worst += 1
        print("check: %s" % ("%d differences" % worst if worst else "the committed fixtures are reproduced"))
        return 1 if worst else 0
    np.savez_compressed(os.path.join(args.out, FILE), **rec.arrays)
    with open(os.path.join(args.out, META), "w") as f:
        json.dump(meta, f, indent=1, sort_keys=True)
        f.write("\n")
    print("%s: %d arrays, %d bytes" % (FILE, len(rec.arrays), os.path.getsize(os.path.join(args.out, FILE))))
    return 0


if __name__ == "__main__":
    sys.exit(main())

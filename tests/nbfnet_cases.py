"""The four recorded cases of ``NeuralBellmanFordNetwork`` (``tests/golden/reference_nbfnet.npz``), shared by the script that
records the reference's runs (``tests/golden/make_nbfnet_golden.py``) and by the tests that hold this package to them: constructor
arguments, seeds, the batch and the runs of THIS package's class in the recorded form.  Graph, triples and the 4 x 9 batch are
those of ``reference_fixture`` (211 nodes, 1 500 fact triples, 11 relations)."""
import json
import os

import numpy as np
import torch

import reference_fixture as RF

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
LAYERS = 3
CASES = {
    "shipped64": dict(input_dim=64, hidden_dims=[64] * LAYERS, num_relation=RF.ENTITY_RELATIONS, message_func="distmult",
                      aggregate_func="sum", short_cut=True, layer_norm=True, dependent=True),
    "paper32": dict(input_dim=32, hidden_dims=[32] * LAYERS, num_relation=RF.ENTITY_RELATIONS, message_func="distmult",
                    aggregate_func="pna", short_cut=True, layer_norm=True, dependent=True),
    "independent16": dict(input_dim=16, hidden_dims=[16] * LAYERS, num_relation=RF.ENTITY_RELATIONS, message_func="transe",
                          aggregate_func="sum", dependent=False),
    "homogeneous16": dict(input_dim=16, hidden_dims=[16] * LAYERS, num_relation=None, message_func="distmult",
                          aggregate_func="sum"),
}
TRAINED = ("shipped64", "independent16", "homogeneous16")        # the cases with a recorded training run
HIDDEN = ("shipped64", "paper32", "independent16")               # ... with recorded hidden states and all-entity scores


def seed(name):
    return 12000 + 100 * list(CASES).index(name) + CASES[name]["input_dim"]


def relational(name):
    return CASES[name]["num_relation"] is not None


def batch(name, triples):
    """``(h, t, r)``: the 4 x 9 batch of ``RF.entity_batch``; without relations its 36 pairs as 1-D ``h``, ``t`` and ``r = None``."""
    h, t, r, _, _ = RF.entity_batch(triples)
    if relational(name):
        return h, t, r
    return h.reshape(-1), t.reshape(-1), None


def edges(name, triples):
    """``(edge_list, num_relation)`` of the fact graph: the first 1 500 triples, without their relation column for a homogeneous case."""
    fact = triples[:RF.ENTITY_TRIPLES]
    return (fact, RF.ENTITY_RELATIONS) if relational(name) else (fact[:, :2], None)


def upstream(name, triples):
    """The seeded gradient of the training scores."""
    return RF.grid(np.random.RandomState(seed(name) + 50000), batch(name, triples)[0].shape, -1.0, 1.0)


_CACHE = {}


def stats():
    if "json" not in _CACHE:
        with open(os.path.join(GOLDEN, "reference_nbfnet.json")) as f:
            _CACHE["json"] = json.load(f)
    return _CACHE["json"]


def arrays():
    """The recorded arrays, the stacked gradients unpacked under their own names."""
    if "npz" not in _CACHE:
        with np.load(os.path.join(GOLDEN, "reference_nbfnet.npz")) as data:
            out = {key: data[key] for key in data.files}
        for name in TRAINED:
            names = sorted(k for k in stats()["tensors"] if k.startswith(name + "/train/d_"))
            for row, key in zip(out.pop(name + "/train/gradients/T"), names):
                out[key + "/T"] = row
        _CACHE["npz"] = out
    return _CACHE["npz"]


def deviation(key, got):
    """``(max|got - T|, scale, ref_dev)`` of one recorded tensor."""
    truth = arrays()[key + "/T"]
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == truth.shape, (key, got.shape, truth.shape)
    entry = stats()["tensors"][key]
    return float(np.abs(got - truth).max()), entry["scale"], entry["ref_dev"]


def model(name, device, dtype=torch.float32):
    """This package's class with the case's arguments and the drawn weights (their float64 sums are pinned by the json)."""
    from ultra_torchdrug_amd import NeuralBellmanFordNetwork
    net = NeuralBellmanFordNetwork(**CASES[name])
    state = RF.draw_state({k: v.shape for k, v in net.state_dict().items()}, seed(name))
    sums = stats()["weight_checksums"][name]
    assert {k: float(np.asarray(v, dtype=np.float64).sum()) for k, v in state.items()} == sums, name
    net.load_state_dict({k: torch.as_tensor(v, dtype=dtype) for k, v in state.items()}, strict=True)
    return net.to(device=device, dtype=dtype)


def run(name, device, dtype=torch.float32, mode="eval", materialised=False):
    """One run of this package's class in the recorded form: ``{key: tensor}`` under the recording's names."""
    from ultra_torchdrug_amd.graph import Graph
    triples = RF.entity_triples()
    net = model(name, device, dtype)
    edge_list, n_rel = edges(name, triples)
    graph = Graph(torch.from_numpy(edge_list).to(device), None, RF.ENTITY_NODES, n_rel)
    to = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(device)
    h, t, r = (to(a) for a in batch(name, triples))
    got = {}
    if relational(name):
        und = net._undirected(graph)
        und.requires_grad = bool(materialised)
        und.edge_weight = und.edge_weight.to(dtype)
    elif materialised:
        plain_graph = net.as_relational_graph

        def marked(g, self_loop=True):               # (a new graph per call: each has to take the materialised route)
            out = plain_graph(g, self_loop)
            out.requires_grad = True
            out.edge_weight = out.edge_weight.to(dtype)
            return out
        net.as_relational_graph = marked
    if mode == "eval":
        net.eval()
        hiddens = []
        handles = [conv.register_forward_hook(lambda mod, args, out: hiddens.append(out.detach())) for conv in net.layers]
        try:
            with torch.no_grad():
                got[name + "/scores"] = net(graph, h, t, r)
        finally:
            for handle in handles:
                handle.remove()
        if name in HIDDEN:
            assert len(hiddens) == LAYERS
            for i, hidden in enumerate(hiddens):                # (the layers of this package add the shortcut themselves)
                got["%s/hidden%d_rows" % (name, i)] = hidden[list(RF.HIDDEN_ROWS)]
                got["%s/hidden%d_rowsum" % (name, i)] = hidden.double().sum(-1)
            ha, ta, ra = (to(a) for a in RF.arch_all_entities(triples))
            with torch.no_grad():
                got[name + "/scores_all"] = net(graph, ha, ta, ra, all_entities=True)
        return got
    net.train()
    score = net(graph, h, t, r, all_loss=torch.zeros((), device=device))
    score.backward(to(upstream(name, triples)).to(dtype))
    got[name + "/train/scores"] = score.detach()
    for key, p in net.named_parameters():
        if p.grad is not None:
            got["%s/train/d_%s" % (name, key)] = torch.from_numpy(RF.compact(key, p.grad.detach().double().cpu().numpy()))
    return got

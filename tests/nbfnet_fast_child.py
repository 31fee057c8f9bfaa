"""Child process of ``test_nbfnet_gpu.py``: the layer-by-layer route of ``NeuralBellmanFordNetwork`` (``ULTRA_FAST_INFERENCE=0`` is
read at import, so it needs a process of its own).  Builds the seeded models of ``fast_cases()`` and writes the scores of
``forward(..., all_entities=True)`` for their queries to the ``.npz`` file named on the command line.

    ULTRA_FAST_INFERENCE=0 python tests/nbfnet_fast_child.py OUT.npz
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

FAST_CASES = {
    "shipped": dict(short_cut=True, layer_norm=True, activation="relu"),
    "plain": dict(short_cut=False, layer_norm=False, activation="relu"),
}


def fast_case(name, device):
    """``(model, graph, h (Q,), r (Q,))``: a seeded 6 x 64 model over ``sampled_graphs.wide_graph()`` and 2 x 13 queries in tail
    form (the batch's tails, then its heads under the inverse relations), as ``task.predict`` stacks them."""
    from sampled_graphs import wide_batch, wide_graph
    from ultra_torchdrug_amd import NeuralBellmanFordNetwork
    graph = wide_graph()
    torch.manual_seed(31 + list(FAST_CASES).index(name))
    model = NeuralBellmanFordNetwork(64, [64] * 6, graph.num_relation, message_func="distmult", aggregate_func="sum",
                                     dependent=True, **FAST_CASES[name]).eval().to(device)
    batch = wide_batch(graph)
    batch = batch[(batch[:, 0] < graph.num_node) & (batch[:, 1] < graph.num_node)].to(device)
    h = torch.cat([batch[:, 0], batch[:, 1]])
    r = torch.cat([batch[:, 2], batch[:, 2] + graph.num_relation])
    return model, graph.to(device), h, r


def general_scores(model, graph, h, r):
    """``forward(..., all_entities=True)`` on index grids that list every entity as the tail of every query."""
    n = graph.num_node
    every = torch.arange(n, device=h.device).unsqueeze(0).expand(len(h), -1)
    # (queries in tail form with r >= R: hand forward the head-corrupted rows it flips itself)
    tail_form = r < graph.num_relation
    base = torch.where(tail_form, r, r - graph.num_relation)
    anchor = h.unsqueeze(-1).expand(-1, n)
    h_index = torch.where(tail_form.unsqueeze(-1), anchor, every)
    t_index = torch.where(tail_form.unsqueeze(-1), every, anchor)
    with torch.no_grad():
        return model(graph, h_index, t_index, base.unsqueeze(-1).expand(-1, n), all_entities=True)


def main(path):
    from ultra_torchdrug_amd import functional as UF
    assert not UF.FAST_INFERENCE, "run with ULTRA_FAST_INFERENCE=0"
    device = torch.device("cuda:0")
    out = {}
    for name in FAST_CASES:
        model, graph, h, r = fast_case(name, device)
        out[name] = general_scores(model, graph, h, r).cpu().numpy()
    np.savez(path, **out)


if __name__ == "__main__":
    main(sys.argv[1])

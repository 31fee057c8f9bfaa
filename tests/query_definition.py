"""Shared by tests/test_query_{cpu,gpu}.py: the set boundary of ``include/ultra_rspmm.h`` restated in numpy, inputs with the
special values planted, and a hand evaluator that spells each of the 14 query structures as explicit ``task.project`` calls
plus torch ops (no parser, no tree walk).  Only ``task.project``, the task's single-source scores and torch are used here."""
import numpy as np
import torch

from topk_definition import topk_rows


def set_boundary_numpy(member, query, floor=None):
    """``(boundary fp32 (N, Q, D), count int32 (Q,))``: entity ``v`` is kept for query ``q`` iff ``m = member[q, v]`` is ``> 0``
    and ``>= floor[q]`` (comparisons with NaN are false); kept rows are ``m * query[q]`` in fp32, the others ``+0.0``."""
    member = np.asarray(member, dtype=np.float32)
    query = np.asarray(query, dtype=np.float32)
    n_query, n_node = member.shape
    out = np.zeros((n_node, n_query, query.shape[1]), dtype=np.float32)
    count = np.zeros(n_query, dtype=np.int32)
    with np.errstate(invalid="ignore", over="ignore"):
        for q in range(n_query):
            keep = member[q] > 0
            if floor is not None:
                keep &= member[q] >= np.float32(floor[q])
            rows = np.nonzero(keep)[0]
            out[rows, q, :] = member[q, rows, None] * query[q][None, :]
            count[q] = len(rows)
    return out, count


def special_members(n_query, n_node, seed, dim):
    """``(member (Q, N), query (Q, D), floor (Q,))`` fp32 torch tensors: uniform memberships with zeros of both signs, negatives,
    NaN and one ``inf`` planted, groups of equal values (ties) of which one is each row's floor, and a query vector with an
    ``inf`` and a NaN entry in row 0 (the zero rows must not see them)."""
    g = torch.Generator().manual_seed(seed)
    member = torch.rand(n_query, n_node, generator=g)
    member = (member * 16).floor() / 16                        # a grid of 16 values: many exact ties
    member[:, 0::7] = 0.0
    member[:, 3::11] = -0.0
    member[:, 5::13] = -member[:, 5::13]
    member[:, 6::17] = float("nan")
    if n_node > 9:
        member[0, 9] = float("inf")
    query = torch.randn(n_query, dim, generator=g)
    query[0, 0] = float("inf")
    query[0, dim - 1] = float("nan")
    floor = torch.full((n_query,), 0.5)                        # on the grid: the ties at 0.5 are all kept
    floor[1::3] = 0.40625                                      # off the grid
    if n_query > 2:
        floor[2] = 2.0                                         # above every membership: an empty set
    return member, query, floor


def first_hop(task, anchor, relation):
    """Memberships ``(Q, N)`` of the tails of ``(anchor, relation, ?)``, ``relation`` in ``[0, 2R)``: sigmoid of the task's
    single-source scores (``score_all_entities`` where the model has the fused head, else ``predict``)."""
    n_rel = task.num_relation
    base = relation % n_rel
    with torch.no_grad():
        pred = task.model.score_all_entities(task.fact_graph, task.relation_representations(base), anchor, relation)
        if pred is None:
            head = relation >= n_rel
            zero = torch.zeros_like(anchor)
            batch = torch.stack([torch.where(head, zero, anchor), torch.where(head, anchor, zero), base], dim=1)
            pred = task.predict(batch)[torch.arange(len(anchor), device=anchor.device), head.long()]
    return torch.sigmoid(pred)


def hand_memberships(task, name, anchors, relations, **cut):
    """The answer memberships ``(Q, N)`` of structure ``name``, written out by hand.  ``a(i)`` / ``r(i)``: column ``i`` of the
    anchors / relations (depth-first, left to right)."""
    a = lambda i: anchors[:, i]
    r = lambda i: relations[:, i]
    hop = lambda i, j: first_hop(task, a(i), r(j))
    proj = lambda p, j: task.project(p, r(j), **cut)
    if name == "1p":
        return hop(0, 0)
    if name == "2p":
        return proj(hop(0, 0), 1)
    if name == "3p":
        return proj(proj(hop(0, 0), 1), 2)
    if name == "2i":
        return hop(0, 0) * hop(1, 1)
    if name == "3i":
        return hop(0, 0) * hop(1, 1) * hop(2, 2)
    if name == "ip":
        return proj(hop(0, 0) * hop(1, 1), 2)
    if name == "pi":
        return proj(hop(0, 0), 1) * hop(1, 2)
    if name == "2u":
        return 1 - (1 - hop(0, 0)) * (1 - hop(1, 1))
    if name == "up":
        return proj(1 - (1 - hop(0, 0)) * (1 - hop(1, 1)), 2)
    if name == "2in":
        return hop(0, 0) * (1 - hop(1, 1))
    if name == "3in":
        return hop(0, 0) * hop(1, 1) * (1 - hop(2, 2))
    if name == "inp":
        return proj(hop(0, 0) * (1 - hop(1, 1)), 2)
    if name == "pin":
        return proj(hop(0, 0), 1) * (1 - hop(1, 2))
    if name == "pni":
        return (1 - proj(hop(0, 0), 1)) * hop(1, 2)
    raise KeyError(name)


# anchors and relations each structure consumes
SHAPES = {"1p": (1, 1), "2p": (1, 2), "3p": (1, 3), "2i": (2, 2), "3i": (3, 3), "ip": (2, 3), "pi": (2, 3), "2u": (2, 2),
          "up": (2, 3), "2in": (2, 2), "3in": (3, 3), "inp": (2, 3), "pin": (2, 3), "pni": (2, 3)}
# set projections per structure: every 'r' but the first after an anchor
SET_PROJECTIONS = {"1p": 0, "2p": 1, "3p": 2, "2i": 0, "3i": 0, "ip": 1, "pi": 1, "2u": 0, "up": 1, "2in": 0, "3in": 0, "inp": 1,
                   "pin": 1, "pni": 1}


def hand_answers(task, name, anchors, relations, k, **cut):
    """``(entities int64 (Q, k), membership fp32 (Q, k))`` from :func:`hand_memberships`: the numpy top-K of
    tests/topk_definition.py, with ``-1`` / ``0.0`` where the membership is not positive."""
    p = hand_memberships(task, name, anchors, relations, **cut).float()
    index, value = topk_rows(p.cpu().numpy(), k, None)
    listed = value > 0
    index = np.where(listed, index, -1)
    value = np.where(listed, value, np.float32(0)).astype(np.float32)
    return torch.from_numpy(index).to(p.device), torch.from_numpy(value).to(p.device)


def query_ids(name, n_query, n_node, n_rel2, seed):
    """Seeded ``(anchors (Q, A), relations (Q, P))`` for structure ``name``; relations over ``[0, n_rel2)``, inverses included."""
    g = torch.Generator().manual_seed(seed)
    n_anchor, n_relation = SHAPES[name]
    return torch.randint(0, n_node, (n_query, n_anchor), generator=g), torch.randint(0, n_rel2, (n_query, n_relation), generator=g)

"""Shared by tests/test_query_exact_{cpu,gpu}.py: the exact answer sets of the 14 query structures, the filtered rank of many
targets and the metrics over hard answers, restated in numpy / plain Python from their descriptions (include/ultra_rspmm.h,
DESIGN.md section 18).  Nothing here is imported from the package's operators: the projection is a boolean adjacency product,
each structure is spelled by hand (no parser, no tree walk), the rank is a double loop."""
import numpy as np
import torch

from query_definition import SHAPES

WORD = 64
SEGMENT = 1024              # edges of a row its lane group walks in ultra_sets_project; the tail launch takes the rest in pieces
RANK_TARGETS = 256          # targets per block of ultra_sets_rank
RANK_TILE = 1024            # entities per LDS tile of ultra_sets_rank


def adjacency(n_node, n_rel, node_in, node_out, rel, weight=None):
    """bool ``(n_rel, N, N)``: ``A[r, u, v]`` iff an edge ``u -> v`` of relation ``r`` has a non-zero (summed) weight."""
    total = np.zeros((n_rel, n_node, n_node), dtype=np.float64)
    weight = np.ones(len(node_in)) if weight is None else np.asarray(weight, dtype=np.float64)
    np.add.at(total, (np.asarray(rel), np.asarray(node_in), np.asarray(node_out)), weight)
    return total != 0


def graph_adjacency(graph):
    """:func:`adjacency` of a package Graph that already has its inverse edges."""
    e = graph.edge_list.cpu().numpy()
    return adjacency(graph.num_node, graph.num_relation, e[:, 0], e[:, 1], e[:, 2], graph.edge_weight.cpu().numpy())


def with_inverses(graph):
    """:func:`adjacency` over ``graph``'s triples and their inverses ``(t, h, r + R)``, built here from the triples."""
    e = graph.edge_list.cpu().numpy()
    w = graph.edge_weight.cpu().numpy()
    n_rel = graph.num_relation
    return adjacency(graph.num_node, 2 * n_rel, np.concatenate([e[:, 0], e[:, 1]]), np.concatenate([e[:, 1], e[:, 0]]),
                     np.concatenate([e[:, 2], e[:, 2] + n_rel]), np.concatenate([w, w]))


def project_numpy(adj, member, relation):
    """bool ``(Q, N)``: ``out[q, v]`` iff some ``u`` in ``member[q]`` has ``adj[relation[q], u, v]``."""
    member = np.asarray(member, dtype=bool)
    out = np.zeros_like(member)
    for q, r in enumerate(np.asarray(relation)):
        out[q] = adj[r][member[q]].any(axis=0)
    return out


def project_edges_numpy(n_node, node_in, node_out, rel, member, relation):
    """:func:`project_numpy` from the edge list itself (unit weights), for graphs too large for a dense adjacency."""
    member = np.asarray(member, dtype=bool)
    passes = member[:, np.asarray(node_in)] & (np.asarray(rel)[None, :] == np.asarray(relation)[:, None])      # (Q, E)
    count = np.zeros((n_node, member.shape[0]), dtype=np.int64)
    np.add.at(count, np.asarray(node_out), passes.T)
    return count.T > 0


def pack_numpy(member):
    """bool ``(Q, N)`` as uint64 ``(N, ceil(Q / 64))``: bit ``q % 64`` of word ``q // 64`` of row ``v``."""
    member = np.asarray(member, dtype=bool)
    n_query, n_node = member.shape
    out = np.zeros((n_node, (n_query + WORD - 1) // WORD), dtype=np.uint64)
    for q in range(n_query):
        out[member[q], q // WORD] |= np.uint64(1) << np.uint64(q % WORD)
    return out


def as_bits(member, device):
    """:func:`pack_numpy` as the int64 tensor the operators take."""
    return torch.from_numpy(pack_numpy(member).view(np.int64)).to(device)


def one_hot(nodes, n_node):
    out = np.zeros((len(nodes), n_node), dtype=bool)
    out[np.arange(len(nodes)), np.asarray(nodes)] = True
    return out


def hand_exact(adj, name, anchors, relations):
    """The exact answers bool ``(Q, N)`` of structure ``name`` over ``adj`` (inverse relations included), written out by hand;
    ``hop(i, j)``: the tails of anchor column ``i`` under relation column ``j``."""
    anchors, relations = np.asarray(anchors), np.asarray(relations)
    n_node = adj.shape[1]
    hop = lambda i, j: project_numpy(adj, one_hot(anchors[:, i], n_node), relations[:, j])
    proj = lambda s, j: project_numpy(adj, s, relations[:, j])
    if name == "1p":
        return hop(0, 0)
    if name == "2p":
        return proj(hop(0, 0), 1)
    if name == "3p":
        return proj(proj(hop(0, 0), 1), 2)
    if name == "2i":
        return hop(0, 0) & hop(1, 1)
    if name == "3i":
        return hop(0, 0) & hop(1, 1) & hop(2, 2)
    if name == "ip":
        return proj(hop(0, 0) & hop(1, 1), 2)
    if name == "pi":
        return proj(hop(0, 0), 1) & hop(1, 2)
    if name == "2u":
        return hop(0, 0) | hop(1, 1)
    if name == "up":
        return proj(hop(0, 0) | hop(1, 1), 2)
    if name == "2in":
        return hop(0, 0) & ~hop(1, 1)
    if name == "3in":
        return hop(0, 0) & hop(1, 1) & ~hop(2, 2)
    if name == "inp":
        return proj(hop(0, 0) & ~hop(1, 1), 2)
    if name == "pin":
        return proj(hop(0, 0), 1) & ~hop(1, 2)
    if name == "pni":
        return ~proj(hop(0, 0), 1) & hop(1, 2)
    raise KeyError(name)


NEGATION_FREE = ("1p", "2p", "3p", "2i", "3i", "ip", "pi", "2u", "up")
assert set(NEGATION_FREE) < set(SHAPES)


def ranks_double_loop(pred, excluded, target_ptr, target_entity):
    """int64 ``(T,)``: ``1 + #{v : not excluded[q, v] and pred[q, v] >= pred[q, target]}`` by a loop over targets and entities;
    ``excluded`` bool ``(Q, N)``.  Comparisons with NaN are false."""
    pred = np.asarray(pred, dtype=np.float32)
    n_query, n_node = pred.shape
    out = np.zeros(len(target_entity), dtype=np.int64)
    for q in range(n_query):
        scores, left_out = pred[q].tolist(), np.asarray(excluded[q]).tolist()      # (Python floats hold fp32 values exactly)
        for t in range(int(target_ptr[q]), int(target_ptr[q + 1])):
            threshold = scores[int(target_entity[t])]
            count = 0
            for v in range(n_node):
                if not left_out[v] and scores[v] >= threshold:
                    count += 1
            out[t] = 1 + count
    return out


def ranks_numpy(pred, excluded, target_ptr, target_entity):
    """:func:`ranks_double_loop` with the inner loop as one numpy comparison (the sizes where the double loop is slow; the CPU
    tests hold the two to each other)."""
    pred = np.asarray(pred, dtype=np.float32)
    out = np.zeros(len(target_entity), dtype=np.int64)
    with np.errstate(invalid="ignore"):
        for q in range(pred.shape[0]):
            for t in range(int(target_ptr[q]), int(target_ptr[q + 1])):
                out[t] = 1 + int(((pred[q] >= pred[q, int(target_entity[t])]) & ~excluded[q]).sum())
    return out


def hard_targets(easy, full):
    """``(hard bool (Q, N), excluded bool (Q, N), target_ptr (Q + 1,), query (T,), entity (T,))`` of the evaluation protocol."""
    hard = full & ~easy
    query, entity = np.nonzero(hard)
    ptr = np.concatenate([[0], np.cumsum(hard.sum(axis=1))]).astype(np.int64)
    return hard, easy | full, ptr, query.astype(np.int64), entity.astype(np.int64)


def metrics_numpy(query, rank, n_query):
    """The metrics over hard answers in float64: per query the mean over its answers, then the mean over the queries that have
    one."""
    query, rank = np.asarray(query), np.asarray(rank, dtype=np.int64)
    per = {"mrr": [], "mr": [], "hits@1": [], "hits@3": [], "hits@10": []}
    for q in range(n_query):
        mine = rank[query == q]
        if len(mine) == 0:
            continue
        per["mrr"].append(np.mean(1.0 / mine.astype(np.float64)))
        per["mr"].append(np.mean(mine.astype(np.float64)))
        for k in (1, 3, 10):
            per["hits@%d" % k].append(np.mean((mine <= k).astype(np.float64)))
    out = {name: float(np.mean(values)) if values else float("nan") for name, values in per.items()}
    out.update(num_queries=n_query, num_evaluated=len(per["mrr"]), num_hard_answers=int(len(rank)))
    return out


def held_out_task(seed=0, n_node=60, n_rel=4, n_triple=240):
    """A two-layer 16-wide model over ``n_triple`` distinct random triples of which the last quarter is held out: the filter
    graph has them, the fact graph does not."""
    from ultra_torchdrug_amd.graph import Graph
    from ultra_torchdrug_amd.task import build_ultra
    rng = np.random.default_rng(seed)
    key = rng.permutation(n_node * n_node * n_rel)[:n_triple]
    triples = np.stack([key // (n_node * n_rel), key // n_rel % n_node, key % n_rel], axis=1).astype(np.int64)
    fact_mask = torch.zeros(n_triple, dtype=torch.bool)
    fact_mask[:n_triple - n_triple // 4] = True
    torch.manual_seed(5)
    task = build_ultra(n_rel, hidden_dims=(16,) * 2, input_dim=16, rel_hidden=16, rel_layers=2, num_negative=8,
                       full_batch_eval=True)
    task.preprocess(Graph(torch.from_numpy(triples), num_node=n_node, num_relation=n_rel), fact_mask)
    return task.eval()


def sampled_ids(task, name, n_query=64, seed=3):
    """``data.sample_queries`` of structure ``name`` on the task's FILTER graph with inverse edges (so that answers that need a
    held-out edge occur), seeded per structure."""
    from ultra_torchdrug_amd import data
    g = torch.Generator().manual_seed(1000 * seed + list(SHAPES).index(name))
    return data.sample_queries(task.graph.cpu().undirected(add_inverse=True), name, n_query, g)


def projection_graph(group, weighted, seed=0):
    """The graph of the projection tests for the lane-group width ``group`` (16 / 32 / 64, chosen from the mean in-degree: below
    24, 24..47, 48 and more): ``(n_node, n_rel, node_in, node_out, rel, weight | None)`` with relations in ``[0, n_rel)``,
    ``n_rel = 6``.  Row 0 is longer than ``4 * group``; rows 1..3 are empty; node 4 has a self-loop; relation 3 is carried by no
    edge; relations 0 and ``n_rel - 1`` are; with ``weighted`` every seventh edge has weight 0 (it does not exist) and the rest
    weights other than 1."""
    rng = np.random.default_rng(seed + group)
    n_node, n_rel = 300, 6
    mean = {16: 8, 32: 30, 64: 52}[group]
    carried = np.array([0, 1, 2, 4, 5])
    others = np.delete(np.arange(n_node), 4)
    node_in = [rng.choice(n_node, size=4 * group + 7, replace=False), np.concatenate([[4], rng.choice(others, size=4, replace=False)])]
    node_out = [np.zeros(4 * group + 7, dtype=np.int64), np.full(5, 4)]
    for v in range(5, n_node):                      # sources are distinct within a row: no (u, v, r) twice, nothing to coalesce
        node_in.append(rng.choice(n_node, size=mean + 2, replace=False))
        node_out.append(np.full(mean + 2, v))
    node_in, node_out = np.concatenate(node_in).astype(np.int64), np.concatenate(node_out).astype(np.int64)
    rel = carried[rng.integers(0, len(carried), len(node_in))]
    rel[:2] = (0, n_rel - 1)
    loop = 4 * group + 7                            # the self-loop 4 -> 4: the first edge of row 4
    assert node_in[loop] == 4 and node_out[loop] == 4
    rel[loop] = n_rel - 1
    got = len(node_in) // n_node
    assert {16: got < 24, 32: 24 <= got < 48, 64: got >= 48}[group], (group, got)
    weight = None
    if weighted:
        weight = rng.integers(2, 5, len(node_in)).astype(np.float32) * 0.5
        weight[::7] = 0.0
        weight[loop] = 1.5
    return n_node, n_rel, node_in, node_out, rel, weight


def long_row_graph(weighted, seed=0):
    """Rows longer than the projection's lane groups walk: ``(n_node, n_rel, node_in, node_out, rel, weight | None)`` over 1 300
    nodes and 4 relations.  Row 0 has 2 600 edges (every node under two relations: its tail crosses two piece boundaries of the
    edge array), row 1 exactly ``SEGMENT``, row 2 one more (a tail of ONE edge, from its largest source), row 3 one fewer; every
    other row has two.  With ``weighted`` every fifth edge has weight 0."""
    rng = np.random.default_rng(seed)
    n_node, n_rel = 1300, 4
    everyone = np.arange(n_node)
    first = rng.integers(0, n_rel, n_node)
    node_in = [everyone, everyone, everyone[:SEGMENT], np.sort(rng.choice(n_node, SEGMENT + 1, replace=False)), everyone[-(SEGMENT - 1):]]
    node_out = [np.zeros(n_node), np.zeros(n_node), np.ones(SEGMENT), np.full(SEGMENT + 1, 2), np.full(SEGMENT - 1, 3)]
    rel = [first, (first + 1 + rng.integers(0, n_rel - 1, n_node)) % n_rel] + [rng.integers(0, n_rel, len(a)) for a in node_in[2:]]
    for v in range(4, n_node):
        node_in.append(rng.choice(n_node, 2, replace=False))
        node_out.append(np.full(2, v))
        rel.append(rng.integers(0, n_rel, 2))
    node_in, node_out, rel = (np.concatenate(x).astype(np.int64) for x in (node_in, node_out, rel))
    weight = None
    if weighted:
        weight = rng.integers(2, 5, len(node_in)).astype(np.float32) * 0.5
        weight[::5] = 0.0
        weight[2 * n_node + SEGMENT + SEGMENT] = 2.0                    # the one tail edge of row 2 exists
    return n_node, n_rel, node_in, node_out, rel, weight

"""Shared by tests/test_hop_distance_{cpu,gpu}.py: two independent definitions of the hop-distance operator, written from its
description (include/ultra_rspmm.h), and the graphs the tests walk.  Nothing here is imported from the
package's kernels.

The routine being restated is the reference's ``_get_shortest_distance`` (``/root/reference/ultra/model.py:302-314``, twin
``/root/reference/ultra/rel_model.py:77-89``): a table filled with ``num_node``, zeros at the sources, then ``num_iters`` rounds in
which every edge offers ``dist[node_in] + 1`` to ``node_out`` and the minimum is kept.

* :func:`iteration_form` -- that iteration in ATen (``scatter_reduce(amin)``): holds the cap and the sentinel by construction.
* :func:`queue_form` -- a plain queue BFS per source in numpy with the cap applied afterwards: holds the iteration form at sizes
  where that one is slow.

Both take the edge list ``(node_in, node_out)`` itself, not a CSR; an edge masked out (``keep``) is not in the list."""
import collections

import numpy as np
import torch


def iteration_form(n_node, node_in, node_out, sources, num_iters=100):
    """int32 ``(n_node, B)``; ``node_in`` / ``node_out`` / ``sources``: int64 sequences."""
    node_in = torch.as_tensor(np.asarray(node_in), dtype=torch.long)
    node_out = torch.as_tensor(np.asarray(node_out), dtype=torch.long)
    sources = torch.as_tensor(np.asarray(sources), dtype=torch.long)
    dist = torch.full((n_node, len(sources)), n_node, dtype=torch.int32)
    dist[sources, torch.arange(len(sources))] = 0
    if len(node_in) == 0:
        return dist
    index = node_out[:, None].expand(-1, len(sources))
    for _ in range(num_iters):
        offer = dist[node_in] + 1
        dist = dist.scatter_reduce(0, index, offer, "amin", include_self=True)
    return dist


def queue_form(n_node, node_in, node_out, sources, num_iters=100):
    """int32 numpy ``(n_node, B)``: breadth-first search from every source, then everything beyond the cap set to ``n_node``."""
    node_in, node_out = np.asarray(node_in, dtype=np.int64), np.asarray(node_out, dtype=np.int64)
    order = np.argsort(node_in, kind="stable")
    start = np.searchsorted(node_in[order], np.arange(n_node + 1))
    nbr = node_out[order]
    out = np.full((n_node, len(sources)), n_node, dtype=np.int32)
    for b, s in enumerate(np.asarray(sources, dtype=np.int64)):
        dist = np.full(n_node, -1, dtype=np.int64)
        dist[s] = 0
        queue = collections.deque([int(s)])
        while queue:
            u = queue.popleft()
            for v in nbr[start[u]:start[u + 1]]:
                if dist[v] < 0:
                    dist[v] = dist[u] + 1
                    queue.append(int(v))
        reached = (dist >= 0) & (dist <= num_iters)
        out[reached, b] = dist[reached]
    return out


def graph_of(n_node, node_in, node_out, weight=None, n_rel=1, rel=None):
    """A package Graph over the edge list (relation 0 unless given)."""
    from ultra_torchdrug_amd.graph import Graph
    node_in, node_out = np.asarray(node_in, dtype=np.int64), np.asarray(node_out, dtype=np.int64)
    rel = np.zeros_like(node_in) if rel is None else np.asarray(rel, dtype=np.int64)
    edges = torch.from_numpy(np.stack([node_in, node_out, rel], axis=1).reshape(-1, 3))
    weight = None if weight is None else torch.as_tensor(np.asarray(weight), dtype=torch.float32)
    return Graph(edges, weight, n_node, n_rel)


def small_graphs():
    """name -> (n_node, node_in, node_out, sources): the constructed cases of the issue, each a few nodes."""
    ring = list(range(5))
    return {
        "self_loop": (6, [0, 1, 1, 2, 4], [1, 1, 2, 3, 4], [0, 1, 4, 3]),
        "duplicate_edge": (5, [0, 0, 0, 1, 2, 2], [1, 1, 1, 2, 3, 3], [0, 2, 4]),
        "isolated_source": (6, [0, 1, 2, 0], [1, 2, 3, 3], [5, 0, 4]),
        "directed_5_cycle": (5, ring, [(i + 1) % 5 for i in ring], [0, 4, 2]),
        "two_components": (9, [0, 1, 2, 3, 5, 6, 7, 8], [1, 2, 3, 0, 6, 7, 8, 5], [0, 5, 4, 7]),
    }


def path_graph(n=130):
    return n, list(range(n - 1)), list(range(1, n))


def star_with_rows(group, n_hub=5000, seed=0):
    """A star whose centre (node 0) has ``n_hub`` in-edges, rows of in-degree 0, 1, group - 1, group and group + 1 (nodes 1..5)
    and filler rows of equal in-degree that bring the mean in-degree to the band in which the operator takes ``group`` lanes per
    row (16: below 24, 32: 24..47, 64: 48 and more).  Returns ``(n_node, node_in, node_out)``."""
    rng = np.random.default_rng(seed)
    leaves = np.arange(6, 6 + n_hub)
    n_fill = 400
    n_node = 6 + n_hub + n_fill
    node_in, node_out = [leaves], [np.zeros(n_hub, dtype=np.int64)]
    for row, deg in zip(range(1, 6), (0, 1, group - 1, group, group + 1)):
        node_in.append(rng.choice(n_node, size=deg, replace=False))
        node_out.append(np.full(deg, row, dtype=np.int64))
    # the centre feeds a few leaves back so that its column reaches beyond one hop
    node_in.append(np.zeros(40, dtype=np.int64))
    node_out.append(leaves[:40])
    mean = {16: 8, 32: 26, 64: 50}[group]
    have = sum(len(a) for a in node_in)
    per_row = -(-(mean * n_node - have) // n_fill)
    fill = np.arange(6 + n_hub, n_node)
    for row in fill:
        node_in.append(rng.choice(n_node, size=per_row, replace=False))
        node_out.append(np.full(per_row, row, dtype=np.int64))
    node_in, node_out = np.concatenate(node_in).astype(np.int64), np.concatenate(node_out).astype(np.int64)
    got = len(node_in) // n_node
    assert {16: got < 24, 32: 24 <= got < 48, 64: got >= 48}[group], (group, got)
    return n_node, node_in, node_out


def random_edges(n_node, n_edge, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, n_node, n_edge), rng.integers(0, n_node, n_edge)

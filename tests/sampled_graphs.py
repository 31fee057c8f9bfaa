"""Shared by tests/test_sampled_metrics_{cpu,gpu}.py: the constructed graphs, a small task over them, the fp64 binomial
sum of the sampled metric and a numpy restatement of the without-replacement draw (written here from the definition in
include/ultra_rspmm.h; nothing of it is imported from the package)."""
import math

import numpy as np
import torch

S = 50                                      # negatives per query and side of the sampled protocol


def ring_graph(extra=()):
    """64 nodes, 3 relations, edge (h, t, r) iff (t - h - r) mod 64 < 14: every (h, r, ?) has exactly 14 distinct tails and
    every (?, r, t) exactly 14 distinct heads, so every query has exactly 50 unfiltered candidates.  Some triples twice."""
    from ultra_torchdrug_amd.graph import Graph
    edges = [(h, (h + r + d) % 64, r) for r in range(3) for h in range(64) for d in range(14)]
    edges = np.array(edges + edges[:200] + list(extra), dtype=np.int64)
    return Graph(torch.from_numpy(edges), num_node=64, num_relation=3)


def wide_graph(full_row=False, seed=7):
    """300 nodes, 5 relations, 9000 random triples + the first 300 of them again (duplicates) + one query, (h=11, r=1, ?),
    with exactly 40 tails; no triple has head 9 under relation 3 (a query without completions).  ``full_row``: every
    node also completes (7, 2, ?) -- a query without a single unfiltered candidate -- and 270 nodes complete (13, 0, ?): a
    query with fewer candidates than the protocol draws."""
    from ultra_torchdrug_amd.graph import Graph
    rng = np.random.default_rng(seed)
    e = np.stack([rng.integers(0, 300, 9000), rng.integers(0, 300, 9000), rng.integers(0, 5, 9000)], axis=1)
    e = e[~((e[:, 0] == 9) & (e[:, 2] == 3))]
    e = e[~((e[:, 0] == 11) & (e[:, 2] == 1))]
    hub = np.stack([np.full(40, 11), rng.permutation(300)[:40], np.full(40, 1)], axis=1)
    parts = [e, e[:300], hub]
    if full_row:
        parts.append(np.stack([np.full(300, 7), np.arange(300), np.full(300, 2)], axis=1))
        parts.append(np.stack([np.full(270, 13), np.arange(270), np.full(270, 0)], axis=1))
    return Graph(torch.from_numpy(np.concatenate(parts).astype(np.int64)), num_node=300, num_relation=5)


def wide_batch(graph):
    """Triples to rank on :func:`wide_graph`: edges of the graph, the 40-tail hub, the query without completions, the
    query without candidates and the one with few (on the ``full_row`` graph), the last node; the targets of the
    constructed rows are arbitrary entities."""
    e = graph.edge_list
    rows = [e[i].tolist() for i in range(0, 8000, 1500)]
    rows += [e[(e[:, 0] == 11) & (e[:, 2] == 1)][0].tolist(), [9, 5, 3], [7, 0, 2], [13, 5, 0], [299, 298, 4]]
    return torch.tensor(rows, dtype=torch.long)


def small_task(graph, seed=5, **kwargs):
    """A two-layer 16-wide model over ``graph`` (transductive context: filter graph = fact graph)."""
    from ultra_torchdrug_amd.task import build_ultra
    torch.manual_seed(seed)
    task = build_ultra(graph.num_relation, hidden_dims=(16,) * 2, input_dim=16, rel_hidden=16, rel_layers=2, num_negative=8,
                       full_batch_eval=True, **kwargs)
    task.preprocess(graph)
    return task.eval()


def dense_samples(pred, target, mask, rand):
    """The entities the dense-mask path draws for a batch: int64 ``(B, 2, n_sample)``, ``-1`` in unused slots."""
    from ultra_torchdrug_amd.task import dense_sampled_ranks
    rows, n = mask.shape[0] * 2, mask.shape[-1]
    return dense_sampled_ranks(pred.reshape(rows, n), target.reshape(rows), mask.reshape(rows, n),
                               rand.reshape(rows, -1))[2].view(-1, 2, rand.shape[-1])


def tied_scores(rows, n, seed):
    """fp32 ``(rows, 2, n)`` scores on a grid of six values: many exact ties with the positive."""
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 6, (rows, 2, n), generator=g).float() * 0.5 - 1.0


def edge_rand(rows, seed, n_sample=S):
    """fp32 ``(rows, 2, n_sample)`` uniform numbers with the ends of [0, 1) planted: 0 and the largest float below 1."""
    g = torch.Generator().manual_seed(seed)
    rand = torch.rand(rows, 2, n_sample, generator=g)
    below_one = float(np.nextafter(np.float32(1), np.float32(0)))
    rand[0, 0, :] = below_one
    rand[0, 1, :] = 0.0
    rand[1:, :, 0::7] = below_one
    rand[1:, :, 3::7] = 0.0
    return rand


def binomial_fp64(rank, n_cand, k, n):
    """sum_{i<k} C(n, i) p^i (1 - p)^(n - i) with p = (rank - 1) / n_cand, in Python floats (fp64) and exact binomials."""
    p = (rank - 1) / n_cand
    return sum(math.comb(n, i) * p ** i * (1 - p) ** (n - i) for i in range(k))


def draw_numpy(free, rand_row):
    """The drawn entities of one query: ``free`` = its unfiltered entities ascending, ``rand_row`` fp32 ``(n_sample,)``."""
    n_free, n_sample = len(free), len(rand_row)
    chosen, out = [], []
    for j in range(min(n_sample, n_free)):
        m = n_free - j
        k = min(int(np.float32(rand_row[j]) * np.float32(m)), m - 1)      # fp32 product, truncated, clamped
        for c in sorted(chosen):
            if c <= k:
                k += 1
        chosen.append(k)
        out.append(int(free[k]))
    return out + [-1] * (n_sample - len(out))

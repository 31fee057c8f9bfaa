"""Shared by tests/test_grid_caps_gpu.py: the launchers whose grid is clamped by a CONSTANT ("Constant grid
caps"), restated here with the line each clamp stands on, the arithmetic of a case's trips, and the graphs the cases walk.

A kernel behind such a launcher covers what its grid does not with a loop (``x += gridDim.x * ...``).  ``CAPS[name]`` is the
work ONE pass of the clamped grid covers, in the unit the loop counts (rows, nodes, items, float4 pieces); a case has
``trips(work, CAPS[name]) >= 3``: two whole passes and a ragged third, so that doubling a clamp still leaves a second pass.
Nothing here is imported from the package."""
import numpy as np

CAPS = {
    # csrc/score_rows.inc:220 -- `if (blocks > 256) blocks = 256;`, 16 waves a workgroup, one candidate row a wave
    "score_rows_forward": 256 * 16,
    # csrc/hop_distance.hip:147 grid_for -- `blocks > 2048 ? 2048 : blocks`, 256 threads; the level kernel gives a row G lanes
    "hop_level_16": 2048 * 256 // 16,
    "hop_level_32": 2048 * 256 // 32,
    "hop_level_64": 2048 * 256 // 64,
    "hop_fill": 2048 * 256,                   # elements of the distance matrix / the pairs (hop_fill_kernel)
    "hop_clear": 2048 * 256,                  # nodes (hop_clear_kernel)
    # csrc/relcsr_build.hip:426 -- `want < 8192 ? ... : 8192`, 4 waves a workgroup, one node a wave
    "relation_marks": 8192 * 4,
    # csrc/query_set.hip:36,294 -- kMaxBlocks = 2048, one item (16 queries x 64 nodes) a workgroup
    "set_boundary": 2048,
    # csrc/first_layer_train.inc:271,280 -- `dim3(1024)`, 256 threads, 16 lanes a listed row
    "gather_rows": 1024 * 16,
    # csrc/sampler.inc:830 -- `if (blocks > 1024) blocks = 1024;`, 256 threads, one float4 a thread
    "relation_stack_inputs": 1024 * 256,
    # csrc/sampler.inc:934 -- `if (blocks > 1024) blocks = 1024;`, 256 threads, one float4 a thread and round
    "statistics": 1024 * 256 * 4,             # floats
    # csrc/frontier.inc:455 zero_fill_kernel behind `< 4096 ? ... : 4096` (score_rows.inc:236, first_layer_train.inc:265,
    # combine_fused_bwd.inc:476, epilogue.hip:827; const_fill_kernel epilogue.hip:920): 256 threads, one float4 a thread and
    # round.  The grid is sized for EIGHT rounds a thread, so the clamp binds from 8 * this many float4 on.
    "zero_fill": 4096 * 256,
    "zero_fill_clamp_binds": 4096 * 256 * 8,
    # csrc/rspmm_kernels.hip:453,480, csrc/rotate.inc:392,460 -- `if (blocks > 8192) blocks = 8192;`, one wave an edge
    "weight_grad": 8192 * 4,
}

# csrc/query_set.hip:33-34 (kTile, kChunk) and :268 (backward_shape: kMaxBlocks / n_chunks workgroups a chunk of queries)
SET_TILE, SET_CHUNK = 64, 16


def trips(work, per_trip):
    """Passes of a clamped grid over ``work`` units: the last one may be ragged."""
    return -(-int(work) // int(per_trip))


def set_boundary_items(n_query, n_node):
    """Work items of ``set_boundary_kernel`` (more than one chunk of queries: one 64-node tile an item)."""
    n_chunks = trips(n_query, SET_CHUNK)
    assert n_chunks > 1
    return n_chunks * trips(n_node, SET_TILE)


def set_boundary_backward_tiles(n_query, n_node):
    """``(tiles of a chunk, workgroups of a chunk)`` of ``set_boundary_backward_kernel`` for 16-query chunks (dim <= 16)."""
    n_chunks = trips(n_query, SET_CHUNK)
    assert n_chunks > 1
    return trips(n_node, SET_TILE), CAPS["set_boundary"] // n_chunks


# ---------------------------------------------------------------------------------------------------- hop distances
def degree_graph(n_node, degree, seed):
    """``(node_in, node_out)``: ``degree * n_node`` uniform edges; every node of the last pass's rows has in-edges."""
    rng = np.random.default_rng(seed)
    return rng.integers(0, n_node, degree * n_node), rng.integers(0, n_node, degree * n_node)


def alternating_path(n_node, per_trip, n_low=1000):
    """A path whose consecutive nodes alternate between ids below ``n_low`` (the first pass of the level kernel) and rows of the
    LAST pass, then of the second: ``(path, node_in, node_out)``.  At every odd level the only fresh node is found in a later
    pass, at every even level in the first and not in the last."""
    last = np.arange(trips(n_node, per_trip) * per_trip - per_trip, n_node)
    second = np.arange(per_trip + 5, per_trip + 5 + len(last))
    high = np.concatenate([last, second])
    assert len(high) <= n_low and (trips(n_node, per_trip) >= 3)
    low = np.arange(len(high)) * 3 % n_low                        # distinct below n_low (3 does not divide 1000)
    assert len(set(low.tolist())) == len(low)
    path = np.stack([low, high], axis=1).reshape(-1)
    return path, path[:-1].copy(), path[1:].copy()


# ---------------------------------------------------------------------------------------------------- relation graph
def planted_triples(n_node, per_trip, seed=0):
    """``(triples (T, 3) [head, tail, relation], n_rel = 6, planted)`` over ``n_node`` entities: relations 0..2 live among the
    nodes of the first pass; the head-head pairs (3, 4) and (2, 4) exist at ONE node of the second pass each and (0, 5) at one
    node of the third.  ``planted``: ``[(node, r1, r2)]``."""
    assert trips(n_node, per_trip) >= 3 and n_node - 3 >= 2 * per_trip
    rng = np.random.default_rng(seed)
    low = per_trip - 1000
    base = np.stack([rng.integers(0, low, 20000), rng.integers(0, low, 20000), rng.integers(0, 3, 20000)], axis=1)
    a, b, c = per_trip + 7233, per_trip + 27232, n_node - 3
    extra = np.array([[a, per_trip + 17232, 3], [a, per_trip + 17233, 4],           # (3, 4): heads at a
                      [b, per_trip + 17234, 4], [b, 11, 2],                         # (2, 4): heads at b
                      [c, n_node - 2, 5], [c, 12, 0]])                              # (0, 5): heads at c
    return np.concatenate([base, extra]).astype(np.int64), 6, [(a, 3, 4), (b, 2, 4), (c, 0, 5)]


def relation_planes_numpy(edges, n_node, n_rel):
    """bool ``(4, n_rel, n_rel)`` (hh, tt, ht, th) of an edge list WITH its inverse edges: the reference's four incidence products
    (rel_model.py:99-143) as dense integer matrix products."""
    heads, tails = np.zeros((n_node, n_rel), dtype=np.int64), np.zeros((n_node, n_rel), dtype=np.int64)
    heads[edges[:, 0], edges[:, 2]] = 1
    tails[edges[:, 1], edges[:, 2]] = 1
    return np.stack([heads.T @ heads, tails.T @ tails, heads.T @ tails, tails.T @ heads]) > 0

"""Seeded synthetic relational graphs shared by the tests (numpy only)."""
import numpy as np


def zipf_choice(rng, n, size, alpha=1.0):
    """Indices 0..n-1 with P(k) ~ 1/(k+1)^alpha, randomly relabelled so that hubs are not the low ids."""
    p = 1.0 / np.arange(1, n + 1, dtype=np.float64) ** alpha
    p /= p.sum()
    perm = rng.permutation(n)
    return perm[rng.choice(n, size=size, p=p)]


def random_graph(seed, n_node, n_edge, n_rel, skew=False, unique=False, weights=False, hub_row=None, hub_edges=0,
                 isolated=0, hub_src=None, hub_rel=None):
    """Returns dict(dst, src, rel, w) int64/float32 arrays.  `isolated` trailing nodes get no in-edges.  `hub_row` gets
    the first `hub_edges` edges as in-edges; `hub_src` the last `hub_edges` as out-edges; `hub_rel` is the relation of
    the middle `hub_edges` (three disjoint ranges when 3 * hub_edges <= n_edge, so the hubs do not merge into duplicates)."""
    rng = np.random.default_rng(seed)
    live = max(n_node - isolated, 1)
    if skew:
        dst = zipf_choice(rng, live, n_edge)
        src = zipf_choice(rng, n_node, n_edge)
        rel = zipf_choice(rng, n_rel, n_edge)
    else:
        dst = rng.integers(0, live, n_edge)
        src = rng.integers(0, n_node, n_edge)
        rel = rng.integers(0, n_rel, n_edge)
    if hub_row is not None and hub_edges:
        dst[:hub_edges] = hub_row
    if hub_src is not None and hub_edges:
        src[n_edge - hub_edges:] = hub_src
    if hub_rel is not None and hub_edges:
        rel[(n_edge - hub_edges) // 2:(n_edge + hub_edges) // 2] = hub_rel
    if unique and n_edge:
        key = (dst.astype(np.int64) * n_node + src) * n_rel + rel
        _, first = np.unique(key, return_index=True)
        first.sort()
        dst, src, rel = dst[first], src[first], rel[first]
    w = rng.uniform(0.25, 2.0, dst.shape[0]).astype(np.float32) if weights else None
    return dict(dst=dst.astype(np.int64), src=src.astype(np.int64), rel=rel.astype(np.int64), w=w)


# Rotate rspmm shapes (graph kwargs, nodes, relations, F, block), each the smallest that reaches one launch variant of
# csrc/rotate.inc (a pair tile = 64 complex pairs = 128 columns; the relation table sits in LDS up to 312 relations)
ROTATE_VARIANTS = {
    # 320 x 512 B > 156 KiB: the forward and d_input read the relation rows from memory, not LDS
    "beyond_lds": (dict(n_edge=4000, weights=True), 120, 320, 128, 64),
    # 12 pairs per query block: blocks straddle the 64-pair tiles; two tiles, the second partial (56 pairs)
    "straddle_hub": (dict(n_edge=4000, weights=True, skew=True, hub_row=3, hub_edges=300), 150, 5, 240, 24),
    "nine_tiles": (dict(n_edge=1500), 100, 7, 1152, 64),                    # 9 tiles, 8 slots per tile
    "eight_tiles": (dict(n_edge=1500, weights=True), 100, 7, 1024, 64),     # 8 tiles, 1 slot per tile
    "block2": (dict(n_edge=800, weights=True, isolated=10), 60, 3, 6, 2),   # one pair per block, 3 pairs in a wave, empty rows
    # distinct triples: the only case whose merged weights are all 1, so the only one on the kernels without a weight array
    # (duplicates of the cases above sum to 2); blocks straddle the two tiles as in straddle_hub
    "unit_weights": (dict(n_edge=1500, unique=True), 100, 7, 240, 24),
}


def kg_graph(seed, n_node, n_triple, n_base_rel, alpha=1.0):
    """SURVEY.md 8d generator: Zipf heads/tails/relations, inverse edges (t, h, r + n_base_rel) appended.
    Returns dst/src/rel as rspmm sees them (destination = tail), E = 2 * n_triple, R = 2 * n_base_rel."""
    rng = np.random.default_rng(seed)
    h = zipf_choice(rng, n_node, n_triple, alpha)
    t = zipf_choice(rng, n_node, n_triple, alpha)
    r = zipf_choice(rng, n_base_rel, n_triple, alpha)
    src = np.concatenate([h, t])
    dst = np.concatenate([t, h])
    rel = np.concatenate([r, r + n_base_rel])
    return dict(dst=dst.astype(np.int64), src=src.astype(np.int64), rel=rel.astype(np.int64), w=None)

"""Test infrastructure: the inputs of the recorded runs of the reference (``tests/golden/reference_*.npz``).

Everything here is regenerated from closed formulas and frozen generators (``numpy.random.RandomState``: the legacy MT19937
stream), so that the recorder (``oracle/reference_record.py``) and the tests build the SAME graphs, batches, inputs and upstream
gradients without storing them.  Values that enter floating-point arithmetic lie on a grid of multiples of 2^-10 (exact in
float16, float32 and float64).  Nothing in this module knows the reference or this package: plain numpy.

The layer graph is built so that the reference's two branches of one layer -- ``message`` + ``aggregate`` (what is recorded,
``ultra/layer.py:232-296``) and the rspmm branch (what the HIP path mirrors, ``:298-384``) -- define the same function on it
wherever that is possible:

* ``mean`` / ``pna``: the materialised branch divides by the NUMBER of messages of a node (``scatter_mean``), the rspmm branch
  by its weighted degree + 1.  The weights are not all one and some are zero, but the weights of the edges INTO one node add up to
  their number (pairs ``1 + d`` / ``1 - d``), so both divisors are equal.
* ``max`` / ``min``: the rspmm branch sees duplicate triples as ONE edge with the summed weight, the materialised branch as two
  messages.  The graph has one duplicate triple (weights 1.5 and 0.5); its destination is ``LAYER_DUPLICATE_ROW``.  The tests of
  the rspmm route of max / pna leave that output row out and compare the gradients of a second recorded run whose upstream is
  zero there (``upstream_masked``).  For sums both forms agree, and there the duplicate is held like every other edge.
"""
import numpy as np

GRID = 1024.0                       # values are k / GRID


def grid(rng, shape, lo, hi):
    """Multiples of 2^-10 in ``[lo, hi]`` (float64, exact in float16 for |x| <= 2)."""
    return rng.randint(int(round(lo * GRID)), int(round(hi * GRID)) + 1, size=shape).astype(np.float64) / GRID


# ----------------------------------------------------------------------------------------------- (a) one layer
LAYER_NODES = 37
LAYER_BASE_RELATIONS = 5            # 10 with inverses
LAYER_DIM = 6                       # B * D = 18 columns: no multiple of a 64-column tile or of a 16-byte row
LAYER_QUERIES = (5, 5, 20)          # two queries at the same node
LAYER_ISOLATED = (35, 36)
LAYER_HUB = 3
LAYER_DUPLICATE_ROW = 11
AGGREGATES = ("sum", "mean", "max", "pna")
MESSAGES = ("distmult", "transe", "rotate")
MASKED_AGGREGATES = ("max", "pna")  # a second gradient run with the upstream zeroed at LAYER_DUPLICATE_ROW is recorded for these


def layer_graph():
    """37 nodes, 5 relations made undirected (10), ~300 edges: a hub row of more than 64 edges, two isolated nodes, a
    self-loop, a duplicate triple, weights as the module docstring describes.  ``edge_list`` rows are (node_in, node_out, r)."""
    rng = np.random.RandomState(370)
    n_live = LAYER_NODES - len(LAYER_ISOLATED)
    triples = set()
    while len(triples) < 40:                                        # 40 triples into the hub and 40 out of it: with the inverses
        triples.add((int(rng.randint(0, n_live)), LAYER_HUB, int(rng.randint(0, LAYER_BASE_RELATIONS))))      # 80 edges end there
    while len(triples) < 80:
        triples.add((LAYER_HUB, int(rng.randint(0, n_live)), int(rng.randint(0, LAYER_BASE_RELATIONS))))
    while len(triples) < 148:
        h, t = int(rng.randint(0, n_live)), int(rng.randint(0, n_live))
        if h != t and LAYER_HUB not in (h, t):
            triples.add((h, t, int(rng.randint(0, LAYER_BASE_RELATIONS))))
    triples.add((9, 9, 2))                                          # the self-loop
    base = np.array(sorted(triples), dtype=np.int64)
    base = base[rng.permutation(len(base))]
    flipped = np.stack([base[:, 1], base[:, 0], base[:, 2] + LAYER_BASE_RELATIONS], axis=1)
    edges = np.concatenate([base, flipped])
    duplicate = np.array([[14, LAYER_DUPLICATE_ROW, 1]], dtype=np.int64)
    edges = edges[~((edges == duplicate[0]).all(axis=1))]
    edges = np.concatenate([edges, duplicate, duplicate])           # the duplicate triple, twice
    weight = np.ones(len(edges))
    steps = (0.25, 0.5, 0.75, 1.0)                                  # 1.0 gives a pair (2, 0): zero weights
    for node in range(LAYER_NODES):
        into = np.nonzero(edges[:, 1] == node)[0]
        if node == LAYER_DUPLICATE_ROW:
            into = into[:-2]                                        # the duplicate pair gets its own weights below
        for k in range(0, len(into) - 1, 2):
            d = steps[(node + k // 2) % 4]
            weight[into[k]], weight[into[k + 1]] = 1 + d, 1 - d
    weight[-2], weight[-1] = 1.5, 0.5
    count = np.bincount(edges[:, 1], minlength=LAYER_NODES)
    degree = np.bincount(edges[:, 1], weights=weight, minlength=LAYER_NODES)
    assert (count == degree).all() and count[LAYER_HUB] > 64 and (count[list(LAYER_ISOLATED)] == 0).all()
    assert (weight == 0).any() and (weight != 1).sum() > 100
    return dict(edge_list=edges, edge_weight=weight, num_node=LAYER_NODES, num_relation=2 * LAYER_BASE_RELATIONS)


def layer_inputs(aggregate, message):
    """Input ``(N, B, D)``, per-query relation table ``(B, 2R, D)``, boundary ``(N, B, D)`` (row ``LAYER_QUERIES[b]`` of block ``b``
    holds the query vector ``(B, D)``) and the upstream gradient of the layer's output; the same for every pair but for the seed."""
    rng = np.random.RandomState(1000 + 10 * AGGREGATES.index(aggregate) + MESSAGES.index(message))
    n, b, d = LAYER_NODES, len(LAYER_QUERIES), LAYER_DIM
    query = grid(rng, (b, d), -1.0, 1.0)
    boundary = np.zeros((n, b, d))
    for i, node in enumerate(LAYER_QUERIES):
        boundary[node, i] = query[i]
    out = dict(input=grid(rng, (n, b, d), -1.0, 1.0), relation=grid(rng, (b, 2 * LAYER_BASE_RELATIONS, d), -1.0, 1.0),
               query=query, boundary=boundary, upstream=grid(rng, (n, b, d), -1.0, 1.0))
    out["upstream_masked"] = out["upstream"].copy()
    out["upstream_masked"][LAYER_DUPLICATE_ROW] = 0.0                # no gradient passes through the duplicate triple's row
    return out


# ----------------------------------------------------------------------------------------------- (b), (c) the models
ENTITY_NODES = 211
ENTITY_TRIPLES = 1500
ENTITY_RELATIONS = 11
ENTITY_HUB = 0
ENTITY_ISOLATED = (209, 210)
ENTITY_TEST_TRIPLES = 24            # known completions that carry no messages (the filter graph has them, the fact graph not)
HIDDEN_ROWS = (0, 17, 101, 209)     # the nodes whose whole hidden rows are recorded: the hub, the self-loop, any node, an isolated one
SMALL_DIM = 16                      # width of the two smaller 2-layer records


def entity_triples():
    """``(1500 + 24, 3)`` DISTINCT (h, t, r) rows: node 0 is the tail of 140 triples, nodes 209 / 210 occur nowhere, (17, 17, 4) is
    a self-loop.  The first 1 500 rows are the fact graph, all rows the filter graph."""
    rng = np.random.RandomState(211)
    live = ENTITY_NODES - len(ENTITY_ISOLATED)
    triples = {(17, 17, 4)}
    while len(triples) < 141:
        triples.add((int(rng.randint(1, live)), ENTITY_HUB, int(rng.randint(0, ENTITY_RELATIONS))))
    while len(triples) < ENTITY_TRIPLES + ENTITY_TEST_TRIPLES:
        h, t = int(rng.randint(1, live)), int(rng.randint(1, live))
        triples.add((h, t, int(rng.randint(0, ENTITY_RELATIONS))))
    rows = np.array(sorted(triples), dtype=np.int64)
    return rows[rng.permutation(len(rows))]


def entity_batch(triples):
    """B = 4 rows x 9 candidates as ``(h_index, t_index, r_index)``, column 0 the positive (a fact triple): rows 0 - 1 corrupt the
    tail, rows 2 - 3 the head (the layout of a training batch, ``ultra/task.py:270-274``); row 1 is the self-loop (head == tail)."""
    rng = np.random.RandomState(49)
    fact = triples[:ENTITY_TRIPLES]
    loop = int(np.nonzero((fact == np.array([17, 17, 4])).all(axis=1))[0][0])
    to_hub = int(np.nonzero(fact[:, 1] == ENTITY_HUB)[0][0])
    others = [i for i in rng.permutation(ENTITY_TRIPLES) if i not in (loop, to_hub) and fact[i, 1] != ENTITY_HUB][:2]
    positives = fact[[others[0], loop, to_hub, others[1]]]
    negatives = rng.randint(0, ENTITY_NODES, size=(4, 8))
    negatives[0, 3], negatives[3, 5] = ENTITY_ISOLATED                  # isolated nodes are candidates too
    h = np.repeat(positives[:, :1], 9, axis=1)
    t = np.repeat(positives[:, 1:2], 9, axis=1)
    r = np.repeat(positives[:, 2:3], 9, axis=1)
    t[:2, 1:] = negatives[:2]
    h[2:, 1:] = negatives[2:]
    return h, t, r, positives, negatives


def rel_query_list(count, batch, dim):
    """``count`` seeded per-query relation tables ``(B, 2R, dim)``: the query table and one per layer (``ultra/model.py:149-153``)."""
    rng = np.random.RandomState(77 + dim)
    return [grid(rng, (batch, 2 * ENTITY_RELATIONS, dim), -1.0, 1.0) for _ in range(count)]


def draw_state(shapes, seed):
    """A state dict on the grid for ``{name: shape}``: LayerNorm gains in [0.5, 1.5], non-zero biases in +-[1/16, 1/2], matrices
    uniform with the spread of a fan-in initialisation times 2 -- times 6 in the score head, so that the scores of a query spread
    over several units and few candidates come near the target's score -- and embeddings in [-1, 1]."""
    rng = np.random.RandomState(seed)
    state = {}
    for name in sorted(shapes):
        shape = tuple(shapes[name])
        if "layer_norm" in name and name.endswith("weight"):
            value = grid(rng, shape, 0.5, 1.5)
        elif name.endswith("bias"):
            value = grid(rng, shape, 1 / 16, 1 / 2) * rng.choice([-1.0, 1.0], size=shape)
        elif len(shape) == 2 and ("relation.weight" in name or "dist_embed" in name):
            value = grid(rng, shape, -1.0, 1.0)
        else:
            bound = min((6.0 if name.startswith("mlp.") else 2.0) / np.sqrt(shape[-1]), 1.0)
            value = np.round(grid(rng, shape, -bound, bound) * 128) / 128          # 2^-7 steps: the stored file compresses
        state[name] = value
    return state


def compact(name, array):
    """A gradient in the form the pipeline record keeps it (whole gradients of every run would be megabytes): 48 seeded entries,
    the dot product with a seeded grid vector and the Euclidean norm, as one float64 vector of 50 numbers."""
    flat = np.asarray(array, dtype=np.float64).reshape(-1)
    rng = np.random.RandomState(sum(ord(c) for c in name) + flat.size)
    pick = rng.randint(0, flat.size, size=48)
    probe = grid(rng, flat.shape, -1.0, 1.0)
    return np.concatenate([flat[pick], [float(flat @ probe), float(np.sqrt(flat @ flat))]])


# ----------------------------------------------------------------------------------------------- (d) other architectures
ARCH_LAYERS = 3                     # a first, a middle and a last layer
ARCH_SHIPPED = dict(message_func="distmult", aggregate_func="sum", short_cut=True, layer_norm=True, activation="relu",
                    concat_hidden=False, num_mlp_layer=2, project=True, mod=True)
# every variant changes ONE argument of the shipped set (the last three: the sets the names say)
ARCHITECTURES = {
    "base": {},
    "no_shortcut": dict(short_cut=False),
    "no_ln": dict(layer_norm=False),
    "tanh": dict(activation="tanh"),
    "concat": dict(concat_hidden=True),
    "mlp1": dict(num_mlp_layer=1),
    "mlp3": dict(num_mlp_layer=3),
    "no_project": dict(project=False),
    "not_mod": dict(mod=False),                                     # GeneralizedRelationalConvNBF, dependent=True
    "one_layer": dict(layers=1),
    "defaults": dict(aggregate_func="pna", short_cut=False, layer_norm=False),      # the reference's constructor defaults
    "max_plain": dict(aggregate_func="max", layer_norm=False, short_cut=False),
    "mean_transe": dict(aggregate_func="mean", message_func="transe"),
}
ARCH_WIDTHS = {name: ((64, 16, 6) if name in ("base", "max_plain") else (64, 16)) for name in ARCHITECTURES}
ARCH_CASES = [(name, width) for name in ARCHITECTURES for width in ARCH_WIDTHS[name]]
# configurations the reference's own code cannot run: recorded nowhere, and why
ARCH_NOT_RUNNABLE = {
    "symmetric": "symmetric=True: ultra/model.py:187 passes a fourth argument to bellmanford",
    "unequal_hidden_dims": "unequal hidden_dims: ultra/layer.py:264 concatenates a boundary of another width",
    "not_mod_no_project": "mod=False, project=False: ultra/model.py:153 assigns a tensor over an nn.Embedding",
}
REL_ARCHITECTURES = {"rel_hidden16": dict(input_dim=16, hidden=16, num_layers=6), "rel_two_layers": dict(input_dim=64, hidden=64, num_layers=2)}


def arch_arguments(name, width):
    """Constructor arguments of ``TransferNBFNet`` for one variant at one width."""
    kwargs = dict(ARCH_SHIPPED)
    kwargs.update(ARCHITECTURES[name])
    layers = kwargs.pop("layers", ARCH_LAYERS)
    kwargs.update(input_dim=width, hidden_dims=[width] * layers, num_relation=ENTITY_RELATIONS)
    return kwargs


def arch_seed(name, width):
    return 8000 + 100 * list(ARCHITECTURES).index(name) + width


def arch_all_entities(triples):
    """The batch's four queries with EVERY entity on the corrupted side (``ultra/task.py:249-259``): rows 0 - 1 list all tails,
    rows 2 - 3 all heads."""
    _, _, _, positives, _ = entity_batch(triples)
    every = np.tile(np.arange(ENTITY_NODES), (4, 1))
    h = np.repeat(positives[:, :1], ENTITY_NODES, axis=1)
    t = np.repeat(positives[:, 1:2], ENTITY_NODES, axis=1)
    r = np.repeat(positives[:, 2:3], ENTITY_NODES, axis=1)
    t[:2], h[2:] = every[:2], every[2:]
    return h, t, r


def arch_upstream(name, width):
    """The seeded gradient of the 4 x 9 training scores."""
    return grid(np.random.RandomState(arch_seed(name, width) + 50000), (4, 9), -1.0, 1.0)


def undirected_is_distinct(triples):
    """Whether the fact graph with its inverse edges holds no triple twice: then min / max see the same messages on the
    materialised branch and on the rspmm branch (one coalesced edge per message) and every row can be held."""
    fact = triples[:ENTITY_TRIPLES]
    both = np.concatenate([fact, np.stack([fact[:, 1], fact[:, 0], fact[:, 2] + ENTITY_RELATIONS], axis=1)])
    return len(np.unique(both, axis=0)) == len(both)


EXTREME_ARCHITECTURES = ("defaults", "max_plain")       # the variants that aggregate with min / max


def gradient_passes_an_extreme(name, width, key):
    """Whether the gradient ``key`` of a training run of variant ``name`` passes through the backward of a min / max
    aggregation.  Every node a query has not reached holds the same row, so the min / max of a stack tie structurally, and at a
    tie the reference's two branches are different functions: the recorded branch (``scatter_max``) hands the gradient to ONE of
    the tied messages, the rspmm branch (torchdrug's native backward, which this package's operators mirror) to EVERY tied
    edge in full.  The score head and the last layer's ``linear`` lie behind every aggregation; everything else lies before one."""
    if name not in EXTREME_ARCHITECTURES or "/train/d_" not in key:
        return False
    last = len(arch_arguments(name, width)["hidden_dims"]) - 1
    behind = key.split("/train/d_")[1]
    return not (behind.startswith("mlp.") or behind.startswith("layers.%d.linear." % last))

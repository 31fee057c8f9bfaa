"""quad_kernel's tile order on a graph with split rows: the order is scheduling only.

A label's column tiles walked one after the other (knob bit 5 = 32) and side by side (knob 0, csrc/plan_path.h) must give
the oracle's bits in the plans' piece order, and each other's.  The graph is the smallest with pieces next to short chunks:
300 nodes, 24 relations, three rows of 300 - 700 in-edges built with piece_len = 128 and chunk_edges = 32, so those rows
split into 3 - 6 pieces while the other groups of a workgroup hold chunks of 32 edges.  F = 1 024 / 2 048 give 2 / 4 tiles
per XCD label; F = 1 088 gives 17 tiles, 8 slots per tile, the last label pass partly empty; F = 1 064 ends inside a tile (40
of its 64 columns: the relation tile's 16-byte staging writes zeros beyond F).  The 300 gathered rows fit LDS; knob bit 1
(2) keeps them out of it, which is the gather form of the kernel the large graphs run.
"""
import numpy as np
import pytest
import torch

from graphs import random_graph

pytestmark = pytest.mark.gpu

N, R = 300, 24
HUBS = ((7, 700), (150, 450), (299, 300))          # (row, in-edges)
PIECE, CHUNK = 128, 32
_memo = {}


def _t(a):
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.from_numpy(np.asarray(a)).to(torch.device("cuda:0"))


def _graph():
    """3 000 random distinct triples plus the hub rows' distinct (source, relation) pairs; unit weights."""
    if "graph" not in _memo:
        g = random_graph(21, N, 3000, R, unique=True)
        keep = ~np.isin(g["dst"], [h for h, _ in HUBS])
        dst, src, rel = [g["dst"][keep]], [g["src"][keep]], [g["rel"][keep]]
        rng = np.random.default_rng(22)
        for row, deg in HUBS:
            pick = rng.choice(N * R, size=deg, replace=False)
            dst.append(np.full(deg, row, dtype=np.int64)); src.append(pick // R); rel.append(pick % R)
        perm = rng.permutation(sum(len(d) for d in dst))
        _memo["graph"] = tuple(np.concatenate(a).astype(np.int64)[perm] for a in (dst, src, rel))
    return _memo["graph"]


def _case(oracle, F):
    """Plans, operands and the oracle's results for one width, computed once."""
    if F not in _memo:
        from ultra_torchdrug_amd import RelCSR
        dst, src, rel = _graph()
        csr = RelCSR(_t(dst), _t(src), _t(rel), None, N, N, R, piece_len=PIECE, chunk_edges=CHUNK)
        assert csr.piece_len == PIECE and csr.unit_weight and csr.fwd.n_pieces >= 3 + 4 + 6
        assert csr.kernel_order("add", "mul", F) == (PIECE, False)
        rng = np.random.default_rng(F)
        relation = rng.standard_normal((R, F)).astype(np.float32)
        x = rng.standard_normal((N, F)).astype(np.float32)
        csr_o = oracle.coalesce_csr(dst, src, rel, None, N, N, R)
        want = oracle.rspmm_forward(csr_o, relation, x, "add", "mul", piece=PIECE)
        want_b = node = value = None
        if F % 64 == 0:
            q = F // 64
            node = rng.integers(0, N, q).astype(np.int32)
            node[0] = HUBS[0][0]                  # a boundary row that is a split row: added by the fix-up pass
            value = rng.standard_normal((q, 64)).astype(np.float32)
            dense_b = np.zeros((N, q, 64), dtype=np.float32)
            dense_b[node, np.arange(q)] = value
            want_b = want + dense_b.reshape(N, F)
        _memo[F] = dict(csr=csr, relation=_t(relation), x=_t(x), want=want, want_b=want_b, node=node, value=value)
    return _memo[F]


def _run(case, knob, boundary):
    import ultra_torchdrug_amd as U
    from ultra_torchdrug_amd import functional as UF
    lib = U.require_library()
    lib.ultra_rspmm_force_general_path(knob)
    try:
        kw = dict(boundary=(_t(case["node"]), _t(case["value"]))) if boundary else {}
        out = UF.rspmm_forward(case["csr"], case["relation"], case["x"], "add", "mul", **kw)
        torch.cuda.synchronize()
        return out
    finally:
        lib.ultra_rspmm_force_general_path(0)


# (the sparse boundary is one 64-column block per query: F = 1 064 has none)
SHAPES = [(F, b) for F in (1024, 2048, 1088, 1064) for b in (False, True) if not (b and F % 64)]


@pytest.mark.parametrize("x_lds", [True, False], ids=["x_in_lds", "gathers"])
@pytest.mark.parametrize("F,boundary", SHAPES, ids=["F%d_%s" % (F, "sparse_boundary" if b else "plain") for F, b in SHAPES])
def test_tile_order_does_not_enter_the_result(oracle, F, boundary, x_lds):
    case = _case(oracle, F)
    base = 0 if x_lds else 2
    one_after_the_other = _run(case, base | 32, boundary)
    side_by_side = _run(case, base, boundary)
    want = case["want_b"] if boundary else case["want"]
    assert np.array_equal(one_after_the_other.cpu().numpy(), want)
    assert np.array_equal(side_by_side.cpu().numpy(), want)
    assert torch.equal(one_after_the_other, side_by_side)

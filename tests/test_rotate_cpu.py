"""Rotate messages without a GPU: the CPU twin of the HIP kernels (``torch.ops.ultra_mi.rspmm_rotate_fwd / _bwd``, reached
through ``functional.rotate_rspmm`` with CPU tensors) against the fp64 restatement of the definition
(``tests/rotate_restatement.py``), a hand-worked case, the argument errors of the Python and C interfaces, and the CPU rotate
layer against the layers' own ``aggregate(message())`` in fp64."""
import copy
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import rotate_restatement as RR
from graphs import ROTATE_VARIANTS, random_graph

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rotate_handcomputed.json")
CASES = {
    "d64_unit": (dict(n_edge=3000), 200, 7, 128, 64),
    "d32_weights_dups": (dict(n_edge=4000, weights=True, skew=True), 150, 5, 96, 32),
    "d6_hub_isolated": (dict(n_edge=3000, weights=True, hub_row=3, hub_edges=1200, isolated=30), 120, 9, 12, 6),
    **ROTATE_VARIANTS,
}


def _csr(g, n, r):
    from ultra_torchdrug_amd import RelCSR
    t = torch.from_numpy
    return RelCSR(t(g["dst"]), t(g["src"]), t(g["rel"]), None if g["w"] is None else t(g["w"]), n, n, r)


@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("sum", ["add", "min", "max"])
def test_cpu_forward_and_backward_match_the_fp64_restatement(case, sum):
    """Forward and both gradients of the CPU twin against fp64, entry by entry: |error| <= 1e-6 x the sum of the |terms| of
    that entry (forward under min / max: the largest |terms| of one message of the row).  1e-6 is the forward yardstick
    of this suite = 4 x the worst ratio of the fp32 ATen definition on these cases (2.4e-7).  Under min / max the output
    gradient is zeroed in both runs where the fp64 runner-up is within 4e-6 of the winner (``RR.ambiguous_cells``: fp32 may
    pick the other edge there); at most 0.1 % of the cells may be such, none an exact tie.

    Measured max |error| / yardstick of the twin (forward, d_input, d_relation), add / min / max,
    in units of 1e-7 (worst 3.22e-7):
        d64_unit           1.38 1.51 2.23  /  1.15 1.42 1.39  /  1.07 1.72 1.28
        d32_weights_dups   1.91 1.62 1.61  /  2.11 3.22 1.89  /  2.02 2.01 1.66
        d6_hub_isolated    1.10 2.25 0.96  /  1.46 1.30 1.09  /  1.25 1.18 1.39
        beyond_lds         1.82 2.53 1.80  /  1.42 1.47 1.44  /  1.42 1.60 1.44
        straddle_hub       2.86 2.23 1.92  /  2.37 2.39 1.84  /  2.44 1.97 1.88
        nine_tiles         1.89 1.69 1.56  /  1.12 1.61 1.71  /  1.12 1.67 1.77
        eight_tiles        1.84 1.85 1.57  /  1.72 2.07 1.92  /  1.56 1.78 2.07
        block2             0.91 0.92 1.18  /  1.10 1.09 1.09  /  1.11 0.98 0.94
        unit_weights       1.48 1.86 1.14  /  1.11 1.35 1.83  /  1.01 1.51 1.70
    At most 4 cells of a case are ambiguous (nine_tiles, min: 4 of 115 200)."""
    from ultra_torchdrug_amd import rotate_rspmm
    kw, n, r, F, block = CASES[case]
    g = random_graph(seed=len(case) + 3, n_node=n, n_rel=r, **kw)
    gen = torch.Generator().manual_seed(4)
    relation, x, grad = torch.randn(r, F, generator=gen), torch.randn(n, F, generator=gen), torch.randn(n, F, generator=gen)
    dst, src, rel, w = RR.coalesce(g["dst"], g["src"], g["rel"], g["w"], n, r)
    empty = torch.from_numpy(np.bincount(dst, minlength=n) == 0)
    assert empty.any() == (kw.get("isolated", 0) > 0)
    selected = None
    if sum != "add":
        selected = RR.selected_edges(dst, src, rel, w, relation, x, n, block, sum)
        ambiguous = RR.ambiguous_cells(dst, src, rel, w, relation, x, n, block, sum)
        cells = int((~empty).sum()) * F
        print("%s %s: %d ambiguous cells of %d" % (case, sum, int(ambiguous.sum()), cells))
        assert not RR.exact_ties(dst, selected, n).any()
        assert int(ambiguous.sum()) <= 1e-3 * cells
        grad = grad * ~ambiguous

    rel_t, x_t = relation.clone().requires_grad_(), x.clone().requires_grad_()
    out = rotate_rspmm(_csr(g, n, r), rel_t, x_t, sum=sum, block=block)
    out.backward(grad)
    rel64, x64 = relation.double().requires_grad_(), x.double().requires_grad_()
    want = RR.rotate_rspmm(dst, src, rel, w, rel64, x64, n, block, sum)
    want.backward(grad.double() * (~empty).unsqueeze(-1))

    scale = (RR.abs_scale if sum == "add" else RR.abs_max_scale)(dst, src, rel, w, relation, x, n, block)
    bound_x, bound_rel = RR.grad_abs_scale(dst, src, rel, w, relation, x, grad, block, selected)
    ident = {"add": 0.0, "min": RR.FLT_MAX, "max": -RR.FLT_MAX}[sum]
    assert (out.detach()[empty] == ident).all()
    for what, got, truth, bound in (("forward", out.detach(), want.detach(), scale), ("d_input", x_t.grad, x64.grad, bound_x),
                                    ("d_relation", rel_t.grad, rel64.grad, bound_rel)):
        err = (got.double() - truth).abs()
        ratio = (err / (bound + 1e-24)).max().item()
        print("%s %s %s: max err / yardstick %.3g" % (case, sum, what, ratio))
        assert bound.max() > 0
        assert (err <= 1e-6 * bound + 1e-30).all(), "%s: max err / yardstick %.3g" % (what, ratio)


def test_duplicate_triples_are_merged_by_weight_sum():
    from ultra_torchdrug_amd import rotate_rspmm
    gen = torch.Generator().manual_seed(2)
    relation, x = torch.randn(2, 8, generator=gen), torch.randn(3, 8, generator=gen)
    dup = dict(dst=np.array([1, 1, 0]), src=np.array([2, 2, 1]), rel=np.array([1, 1, 0]), w=np.array([0.5, 1.5, 1.0], np.float32))
    merged = dict(dst=np.array([1, 0]), src=np.array([2, 1]), rel=np.array([1, 0]), w=np.array([2.0, 1.0], np.float32))
    for sum in ("add", "max"):
        a = rotate_rspmm(_csr(dup, 3, 2), relation, x, sum, 4)
        b = rotate_rspmm(_csr(merged, 3, 2), relation, x, sum, 4)
        assert torch.equal(a, b)


def test_hand_worked_three_node_case():
    from ultra_torchdrug_amd import RelCSR, rotate_rspmm
    case = json.load(open(GOLDEN))
    e = np.array(case["edges"])
    csr = RelCSR(torch.from_numpy(e[:, 1].astype(np.int64)), torch.from_numpy(e[:, 0].astype(np.int64)),
                 torch.from_numpy(e[:, 2].astype(np.int64)), torch.tensor(e[:, 3], dtype=torch.float32),
                 case["n_node"], case["n_node"], case["n_rel"])
    x, relation = torch.tensor(case["input"]), torch.tensor(case["relation"])
    for sum, want in case["out"].items():
        assert torch.equal(rotate_rspmm(csr, relation, x, sum, case["block"]), torch.tensor(want, dtype=torch.float32)), sum


def test_argument_errors():
    from ultra_torchdrug_amd import rotate_rspmm, generalized_rspmm
    g = random_graph(seed=1, n_node=20, n_edge=60, n_rel=3)
    csr = _csr(g, 20, 3)
    relation, x = torch.randn(3, 12), torch.randn(20, 12)
    with pytest.raises(RuntimeError, match="even block"):
        rotate_rspmm(csr, relation, x, "add", block=3)
    with pytest.raises(RuntimeError, match="even block"):
        rotate_rspmm(csr, relation, x, "add", block=8)          # 12 % 8 != 0
    with pytest.raises(ValueError):
        rotate_rspmm(csr, relation, x, "mean", block=6)
    with pytest.raises(RuntimeError):                          # the raw operator checks it too
        row_ptr, src, rel, w = csr.csr_arrays
        torch.ops.ultra_mi.rspmm_rotate_fwd(row_ptr, src, rel, w, relation, x, 5, 0)
    sparse = torch.sparse_coo_tensor(torch.from_numpy(np.stack([g["dst"], g["src"], g["rel"]])), torch.ones(60), (20, 20, 3))
    with pytest.raises(RuntimeError, match="sparse values"):
        rotate_rspmm(sparse.requires_grad_(), relation, x, "add", block=6)
    with pytest.raises(ValueError):                            # generalized_rspmm keeps torchdrug's operator set
        generalized_rspmm(csr, relation, x, mul="rotate")


def test_c_abi_rejects_bad_block_op_and_foreign_plan():
    """The checks of ultra_rspmm_rotate_forward_f32 / _backward_f32 come before any device work."""
    from ultra_torchdrug_amd import _lib
    lib = _lib.load()
    seg = _lib.UltraSegments()
    p = ctypes.byref(seg)
    fwd = lambda F, block, sum_op, s=p: lib.ultra_rspmm_rotate_forward_f32(s, None, None, None, None, None, None, None, 0, 0, 0,
                                                                          F, block, sum_op, None)
    assert fwd(64, 64, 0) == 0                                  # empty plan: nothing to do
    assert fwd(64, 7, 0) == 2 and fwd(64, 0, 0) == 2 and fwd(96, 64, 0) == 2 and fwd(64, -2, 0) == 2    # ULTRA_ERR_BAD_SHAPE
    assert fwd(64, 64, 3) == 1                                  # ULTRA_ERR_BAD_OP
    foreign = _lib.UltraSegments()
    foreign.abi_version = 7
    assert fwd(64, 64, 0, ctypes.byref(foreign)) == 7           # ULTRA_ERR_ABI
    bwd = lambda block, sum_op: lib.ultra_rspmm_rotate_backward_f32(p, p, None, None, None, None, None, None, None, 0, 0, 0, 0,
                                                                    64, block, sum_op, None)
    assert bwd(5, 0) == 2 and bwd(64, 9) == 1


def _layer_case(aggregate_func, n=60, r=4, B=2, D=64):
    from ultra_torchdrug_amd.graph import Graph
    from ultra_torchdrug_amd.layer import GeneralizedRelationalConvNBFMod
    # mean: unit weights -- the reference's rspmm branch divides by the WEIGHTED degree, its message branch by the count
    weights = aggregate_func != "mean"
    # distinct triples: for max the rspmm convention (duplicates merged by weight sum) differs from the message branch
    g = random_graph(seed=7, n_node=n, n_edge=500, n_rel=r, weights=weights, unique=True)
    edges = torch.from_numpy(np.stack([g["src"], g["dst"], g["rel"]], axis=1))
    graph = Graph(edges, torch.from_numpy(g["w"]) if weights else None, num_node=n, num_relation=r)
    conv = GeneralizedRelationalConvNBFMod(D, D, r, D, message_func="rotate", aggregate_func=aggregate_func, layer_norm=True)
    gen = torch.Generator().manual_seed(9)
    conv.relation = torch.randn(B, r, D, generator=gen)
    graph.query = torch.randn(B, D, generator=gen)
    graph.boundary = torch.zeros(n, B, D)
    graph.boundary[torch.tensor([3, 11]), torch.arange(B)] = graph.query
    return conv, graph, torch.randn(n, B, D, generator=gen)


@pytest.mark.parametrize("aggregate_func", ["sum", "mean", "max"])
def test_cpu_rotate_layer_matches_aggregate_of_message_in_fp64(aggregate_func):
    conv, graph, x = _layer_case(aggregate_func)
    with torch.no_grad():
        got = conv.message_and_aggregate(graph, x)
        conv64, graph64 = copy.deepcopy(conv).double(), copy.copy(graph)
        conv64.relation = conv.relation.double()
        graph64.query, graph64.boundary = graph.query.double(), graph.boundary.double()
        graph64.edge_weight = graph.edge_weight.double()
        graph64.requires_grad = True
        want = conv64.aggregate(graph64, conv64.message(graph64, x.double()))
    assert got.shape == want.shape and got.dtype == torch.float32
    assert ((got.double() - want).abs() <= 1e-5 * want.abs().max() + 1e-6).all()


def test_cpu_rotate_layer_trains_through_the_native_operator():
    """Gradients of a CPU rotate layer (sum) reach the relation table and the input through rspmm_rotate_bwd."""
    conv, graph, x = _layer_case("sum")
    x = x.requires_grad_()
    conv.relation.requires_grad_()
    conv(graph, x).square().sum().backward()
    ref_conv, ref_x = copy.deepcopy(conv), x.detach().clone().requires_grad_()
    ref_conv.relation = conv.relation.detach().clone().requires_grad_()
    graph.requires_grad = True
    ref_conv(graph, ref_x).square().sum().backward()
    assert torch.allclose(x.grad, ref_x.grad, rtol=1e-4, atol=1e-4)
    assert torch.allclose(conv.relation.grad, ref_conv.relation.grad, rtol=1e-4, atol=1e-3)

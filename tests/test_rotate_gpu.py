"""Rotate messages on the MI355X (csrc/rotate.inc): the HIP plan kernels against their CPU twin
(``torch.ops.ultra_mi.rspmm_rotate_fwd / _bwd``), the fp64 restatement, both boundary forms, both bindings, the
``message_func="rotate"`` layers inside a whole task against the ATen definition, and the memory they no longer need.

Launch variants (``tests/graphs.py``, ``ROTATE_VARIANTS``): the relation table in LDS and beyond it, one / two / eight / nine pair
tiles, query blocks that straddle a tile, one pair per block, weighted and unit-weight plans, unsplit rows and rows of all
three plans summed in pieces.

Measured on an MI355X, split rows (``test_split_row_backward_matches_the_fp64_restatement``), max |error| / yardstick of
forward, d_input, d_relation for add / min / max in units of 1e-7 (the assertion holds them to 10; the fp32 ATen definition
measures 2.4, the CPU twin 3.2):
    beyond_lds     1.71 1.74 1.72  /  1.50 1.40 1.56  /  1.54 1.53 1.34
    straddle_hub   1.97 2.51 0.60  /  2.13 1.76 1.25  /  1.95 1.74 0.93
    nine_tiles     1.96 2.30 0.90  /  1.21 2.00 1.37  /  1.31 1.59 1.43
Unsplit rows equal the CPU twin bit for bit, so ``tests/test_rotate_cpu.py``'s table is theirs."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import rotate_restatement as RR
from graphs import ROTATE_VARIANTS, random_graph

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (graph kwargs, nodes, relations, F, block): unsplit rows everywhere (piece_len above every row length)
CASES = {
    "uniform_d64": (dict(n_edge=4000), 300, 7, 128, 64),
    "weights_dups_d32": (dict(n_edge=5000, weights=True, skew=True), 250, 5, 96, 32),
    "ragged_d6": (dict(n_edge=3000, weights=True, isolated=40), 200, 9, 12, 6),
    **ROTATE_VARIANTS,
}


def _dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def _csr(g, n, r, dev, **opts):
    from ultra_torchdrug_amd import RelCSR
    t = lambda a: torch.from_numpy(a).to(dev)
    return RelCSR(t(g["dst"]), t(g["src"]), t(g["rel"]), None if g["w"] is None else t(g["w"]), n, n, r, **opts)


def _operands(n, r, F, seed=5):
    gen = torch.Generator().manual_seed(seed)
    return (torch.randn(r, F, generator=gen), torch.randn(n, F, generator=gen), torch.randn(n, F, generator=gen))


def _run(csr, relation, x, grad, sum, block):
    from ultra_torchdrug_amd import rotate_rspmm
    rel_t, x_t = relation.clone().requires_grad_(), x.clone().requires_grad_()
    out = rotate_rspmm(csr, rel_t, x_t, sum=sum, block=block)
    out.backward(grad)
    return out.detach(), x_t.grad, rel_t.grad


@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("sum", ["add", "min", "max"])
def test_hip_equals_cpu_twin_on_unsplit_rows(case, sum):
    dev = _dev()
    kw, n, r, F, block = CASES[case]
    g = random_graph(seed=len(case), n_node=n, n_rel=r, **kw)
    relation, x, grad = _operands(n, r, F)
    csr_d = _csr(g, n, r, dev, piece_len=1 << 16)
    assert csr_d.fwd.n_pieces == 0 and csr_d.by_src.n_pieces == 0 and csr_d.by_rel.n_pieces == 0
    assert csr_d.unit_weight or case != "unit_weights"
    got = _run(csr_d, relation.to(dev), x.to(dev), grad.to(dev), sum, block)
    want = _run(_csr(g, n, r, torch.device("cpu")), relation, x, grad, sum, block)
    for a, b, what in zip(got, want, ("forward", "d_input", "d_relation")):
        assert torch.equal(a.cpu(), b), "%s differs from the CPU twin" % what
    again = _run(csr_d, relation.to(dev), x.to(dev), grad.to(dev), sum, block)
    for a, b in zip(got, again):
        assert torch.equal(a, b), "two runs differ"


def test_split_rows_sum_within_bound_and_min_max_equal_cpu_twin():
    """A hub row of 20 000 edges is summed in pieces: sums within 1e-6 of the sum of |terms| of the fp64 restatement,
    min / max (order-free) equal to the CPU twin; two runs bit-identical."""
    from ultra_torchdrug_amd import rotate_rspmm
    dev = _dev()
    n, r, F, block = 400, 6, 128, 64
    g = random_graph(seed=3, n_node=n, n_edge=30000, n_rel=r, weights=True, hub_row=7, hub_edges=20000)
    relation, x, _ = _operands(n, r, F)
    csr_d = _csr(g, n, r, dev)
    assert csr_d.fwd.n_pieces > 0
    dst, src, rel, w = RR.coalesce(g["dst"], g["src"], g["rel"], g["w"], n, r)
    want = RR.rotate_rspmm(dst, src, rel, w, relation, x, n, block, "add")
    scale = RR.abs_scale(dst, src, rel, w, relation, x, n, block)
    with torch.no_grad():
        out = rotate_rspmm(csr_d, relation.to(dev), x.to(dev), "add", block)
        assert torch.equal(out, rotate_rspmm(csr_d, relation.to(dev), x.to(dev), "add", block))
        assert ((out.cpu().double() - want).abs() <= 1e-6 * scale + 1e-30).all()
        csr_h = _csr(g, n, r, torch.device("cpu"))
        for sum in ("min", "max"):
            got = rotate_rspmm(csr_d, relation.to(dev), x.to(dev), sum, block)
            assert torch.equal(got.cpu(), rotate_rspmm(csr_h, relation, x, sum, block))


@pytest.mark.parametrize("case", ["beyond_lds", "straddle_hub", "nine_tiles"])
@pytest.mark.parametrize("sum", ["add", "min", "max"])
def test_split_row_backward_matches_the_fp64_restatement(case, sum):
    """Rows of all three plans summed in pieces of 64 (a hub destination, a hub source and a hub relation of 300 edges each):
    forward, d_input and d_relation of the HIP kernels against fp64, entry by entry, |error| <= 1e-6 x the sum of the |terms|
    of that entry (forward under min / max: the largest |terms| of one message, and equal to the CPU twin); under min / max
    the output gradient is zeroed where fp64 cannot tell the two best edges apart (at most 0.1 % of the cells, no exact tie).
    Two runs bit-identical."""
    from ultra_torchdrug_amd import rotate_rspmm
    dev = _dev()
    kw, n, r, F, block = ROTATE_VARIANTS[case]
    kw = dict(dict(hub_row=3, hub_edges=300), hub_src=5, hub_rel=1, **kw)
    g = random_graph(seed=len(case), n_node=n, n_rel=r, **kw)
    relation, x, grad = _operands(n, r, F)
    csr_d = _csr(g, n, r, dev, piece_len=64)
    assert csr_d.fwd.n_pieces > 0 and csr_d.by_src.n_pieces > 0 and csr_d.by_rel.n_pieces > 0
    dst, src, rel, w = RR.coalesce(g["dst"], g["src"], g["rel"], g["w"], n, r)
    cells = int((np.bincount(dst, minlength=n) > 0).sum()) * F
    selected = None
    if sum != "add":
        selected = RR.selected_edges(dst, src, rel, w, relation, x, n, block, sum)
        ambiguous = RR.ambiguous_cells(dst, src, rel, w, relation, x, n, block, sum)
        print("%s %s: %d ambiguous cells of %d" % (case, sum, int(ambiguous.sum()), cells))
        assert not RR.exact_ties(dst, selected, n).any()
        assert int(ambiguous.sum()) <= 1e-3 * cells
        grad = grad * ~ambiguous
    got = _run(csr_d, relation.to(dev), x.to(dev), grad.to(dev), sum, block)
    again = _run(csr_d, relation.to(dev), x.to(dev), grad.to(dev), sum, block)
    for a, b in zip(got, again):
        assert torch.equal(a, b), "two runs differ"
    if sum != "add":
        with torch.no_grad():
            assert torch.equal(got[0].cpu(), rotate_rspmm(_csr(g, n, r, torch.device("cpu")), relation, x, sum, block))

    rel64, x64 = relation.double().requires_grad_(), x.double().requires_grad_()
    want = RR.rotate_rspmm(dst, src, rel, w, rel64, x64, n, block, sum)
    want.backward(grad.double())
    scale = (RR.abs_scale if sum == "add" else RR.abs_max_scale)(dst, src, rel, w, relation, x, n, block)
    bound_x, bound_rel = RR.grad_abs_scale(dst, src, rel, w, relation, x, grad, block, selected)
    for what, a, truth, bound in zip(("forward", "d_input", "d_relation"), got, (want.detach(), x64.grad, rel64.grad),
                                     (scale, bound_x, bound_rel)):
        err = (a.cpu().double() - truth).abs()
        ratio = (err / (bound + 1e-24)).max().item()
        print("%s %s %s: max err / yardstick %.3g" % (case, sum, what, ratio))
        assert bound.max() > 0
        assert (err <= 1e-6 * bound + 1e-30).all(), "%s: max err / yardstick %.3g" % (what, ratio)


# (nodes, edges, hub edges, relations, B, D): the relation table in LDS, and beyond it (320 x 512 B > 156 KiB)
BOUNDARY_SHAPES = {"lds": (500, 20000, 9000, 8, 3, 64), "beyond_lds": (200, 8000, 3000, 320, 3, 64)}


@pytest.mark.parametrize("shape", list(BOUNDARY_SHAPES))
@pytest.mark.parametrize("sum", ["add", "min", "max"])
def test_both_boundary_forms_equal_operator_plus_epilogue(sum, shape):
    from ultra_torchdrug_amd import functional as UF
    dev = _dev()
    n, n_edge, hub_edges, r, B, D = BOUNDARY_SHAPES[shape]
    g = random_graph(seed=11, n_node=n, n_edge=n_edge, n_rel=r, weights=True, hub_row=2, hub_edges=hub_edges)
    csr = _csr(g, n, r, dev)
    assert csr.fwd.n_pieces > 0          # the hub row takes its epilogue in the fix-up pass
    relation, x, _ = (t.to(dev) for t in _operands(n, r, B * D))
    node = torch.tensor([2, 17, 2], dtype=torch.int32, device=dev)
    value = torch.randn(B, D, device=dev)
    dense = torch.zeros(n, B, D, device=dev)
    dense[node.long(), torch.arange(B, device=dev)] = value
    dense = dense.view(n, B * D)
    plain = UF.rotate_rspmm_forward(csr, relation, x, sum, D)
    want = plain + dense if sum == "add" else {"min": torch.min, "max": torch.max}[sum](plain, dense)
    assert torch.equal(UF.rotate_rspmm_forward(csr, relation, x, sum, D, add_rows=dense), want)
    assert torch.equal(UF.rotate_rspmm_forward(csr, relation, x, sum, D, boundary=(node, value)), want)


_CHILD = r"""
import sys, torch
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
from graphs import ROTATE_VARIANTS, random_graph
from ultra_torchdrug_amd import RelCSR, rotate_rspmm
dev = torch.device("cuda:0")
t = lambda a: torch.from_numpy(a).to(dev)
res = []
for shape in sys.argv[3:]:
    if shape == "hub":
        n, r, F, block = 300, 5, 128, 64
        g = random_graph(seed=21, n_node=n, n_edge=12000, n_rel=r, weights=True, hub_row=4, hub_edges=5000)
    else:
        kw, n, r, F, block = ROTATE_VARIANTS[shape]
        g = random_graph(seed=21, n_node=n, n_rel=r, **kw)
    csr = RelCSR(t(g["dst"]), t(g["src"]), t(g["rel"]), t(g["w"]), n, n, r)
    gen = torch.Generator().manual_seed(8)
    rel, x, grad = (torch.randn(*s, generator=gen).to(dev).requires_grad_() for s in ((r, F), (n, F), (n, F)))
    for s in ("add", "max"):
        out = rotate_rspmm(csr, rel, x, s, block)
        d_rel, d_x = torch.autograd.grad(out, (rel, x), grad)
        res += [out.detach().cpu(), d_rel.cpu(), d_x.cpu()]
torch.save(res, sys.argv[2])
"""


def test_ctypes_binding_gives_the_same_bits(tmp_path):
    """Both bindings, a fresh process each, on a hub graph (split rows) and on ``beyond_lds`` (no LDS relation table)."""
    outs = {}
    for binding in ("torch", "ctypes"):
        env = dict(os.environ, ULTRA_BINDING=binding)
        path = str(tmp_path / ("%s.pt" % binding))
        proc = subprocess.run([sys.executable, "-c", _CHILD, ROOT, path, "hub", "beyond_lds"], env=env, timeout=300,
                              capture_output=True, text=True)
        assert proc.returncode == 0, proc.stderr[-3000:]
        outs[binding] = torch.load(path)
    assert len(outs["torch"]) == len(outs["ctypes"]) == 12
    for a, b in zip(outs["torch"], outs["ctypes"]):
        assert torch.equal(a, b)


def _rotate_task(aggregate_func, dev):
    from ultra_torchdrug_amd.data import SHAPES as DATA_SHAPES, synthetic_triples
    from ultra_torchdrug_amd.graph import Graph
    from ultra_torchdrug_amd.model import TransferNBFNet
    from ultra_torchdrug_amd.rel_model import RelationModelList
    from ultra_torchdrug_amd.task import KnowledgeGraphCompletion
    n, n_fact, r = DATA_SHAPES["S-codexs"]
    triples, _, _ = synthetic_triples((n, n_fact + 32, r), 1024)
    mask = np.zeros(len(triples), dtype=bool)
    mask[:n_fact] = True
    torch.manual_seed(1024)
    # task.build_ultra's architecture with rotate messages in the entity stack; the reference's relation stack is always
    # DistMult (rel_model.py:392-400)
    model = TransferNBFNet(input_dim=64, hidden_dims=[64] * 6, num_relation=r, message_func="rotate",
                           aggregate_func=aggregate_func, short_cut=True, layer_norm=True, project=True, mod=True,
                           remove_one_hop=False)
    rel_models = RelationModelList(num_rel_models=1, num_relation=2 * r,
                                   rel_model=dict(class_str="RelNBFNet", input_dim=64, input_type="ones", num_layers=6,
                                                  hidden=64))
    task = KnowledgeGraphCompletion(model, rel_models, criterion="bce", num_negative=32, strict_negative=True,
                                    adversarial_temperature=1.0, sample_weight=False, full_batch_eval=True)
    task.preprocess(Graph(torch.from_numpy(triples), num_node=n, num_relation=r), torch.from_numpy(mask))
    return task.to(dev), torch.from_numpy(triples).to(dev), n_fact


@pytest.mark.parametrize("aggregate_func", ["sum", "max"])
def test_rotate_task_predict_and_training_step_match_the_fp64_definition(aggregate_func):
    """6-layer TransferNBFNet(message_func="rotate") under the shipped RelNBFNet on S-codexs: ``predict`` scores and integer
    ranks, and one training step's loss and gradients, against the whole task in the ATen definition (fp32 and fp64),
    with the yardsticks of tests/test_reference_definition_gpu.py (max: forward and loss only, as its DistMult max case)."""
    from aten_definition import aten_definition
    dev = _dev()
    task, triples, n_fact = _rotate_task(aggregate_func, dev)
    task.eval()
    batch = triples[n_fact:n_fact + 16]
    with torch.no_grad():
        pred_hip = task.predict(batch)
        rank_hip = task.rank_batch(batch, pred=pred_hip)
        with aten_definition(task):
            pred_aten = task.predict(batch)
        with aten_definition(task, double=True):
            pred_true = task.predict(batch)
            mask, target = task.target(batch)
            rank_true = task.get_ranking(pred_true, (mask, target))
    scale = pred_true.abs().max().item()
    e_hip = (pred_hip.double() - pred_true).abs().max().item()
    e_aten = (pred_aten.double() - pred_true).abs().max().item()
    assert e_hip <= 4 * e_aten + 1e-5 * scale, "scores: HIP %.3g vs ATen-fp32 %.3g (scale %.3g)" % (e_hip, e_aten, scale)
    pos = pred_true.gather(-1, target.unsqueeze(-1))
    gap = torch.where(mask, (pred_true - pos).abs(), torch.full_like(pred_true, float("inf")))
    gap.scatter_(-1, target.unsqueeze(-1), float("inf"))
    near = (gap <= 2 * e_hip + 1e-9).sum(dim=-1)
    assert ((rank_hip - rank_true).abs() <= near).all(), (rank_hip, rank_true, near)

    task.train()
    train_batch = triples[torch.randperm(n_fact, generator=torch.Generator().manual_seed(5))[:8].to(dev)]
    torch.manual_seed(5)
    negatives = task._strict_negative(*train_batch.t())

    def step():
        task.zero_grad(set_to_none=True)
        task._static_negative = negatives
        try:
            loss, _ = task(train_batch)
            loss.backward()
        finally:
            task._static_negative = None
        return float(loss), {k: p.grad.detach().double().clone() for k, p in task.named_parameters() if p.grad is not None}

    loss_hip, g_hip = step()
    with aten_definition(task):
        loss_aten, g_aten = step()
    with aten_definition(task, double=True):
        loss_true, g_true = step()
    task.zero_grad(set_to_none=True)
    assert abs(loss_hip - loss_true) <= 4 * abs(loss_aten - loss_true) + 1e-5 * abs(loss_true)
    if aggregate_func == "max":
        return          # ties of a maximum: a convention on which the reference's branches differ (see that file)
    assert g_hip.keys() == g_true.keys()
    for k in g_true:
        s = g_true[k].abs().max().item() + 1e-12
        e_hip, e_aten = (g_hip[k] - g_true[k]).abs().max().item(), (g_aten[k] - g_true[k]).abs().max().item()
        assert e_hip <= 4 * e_aten + 5e-4 * s, "%s: HIP %.3g vs ATen-fp32 %.3g (scale %.3g)" % (k, e_hip, e_aten, s)


def test_rotate_layer_forward_needs_no_edge_sized_tensor():
    """A rotate layer whose (E, B, 64) message tensor would be 2.3 GB: the forward's peak allocation rises by a few
    (N, B * 64) fp32 tensors only."""
    from ultra_torchdrug_amd.graph import Graph
    from ultra_torchdrug_amd.layer import GeneralizedRelationalConvNBFMod
    dev = _dev()
    n, E, r, B = 60000, 1_100_000, 20, 8
    gen = torch.Generator(device=dev).manual_seed(2)
    edges = torch.stack([torch.randint(0, n, (E,), device=dev, generator=gen), torch.randint(0, n, (E,), device=dev, generator=gen),
                         torch.randint(0, r, (E,), device=dev, generator=gen)], dim=1)
    assert E * B * 64 * 4 >= 2 ** 31
    graph = Graph(edges, num_node=n, num_relation=r)
    conv = GeneralizedRelationalConvNBFMod(64, 64, r, 64, message_func="rotate", aggregate_func="sum", layer_norm=True).to(dev)
    conv.relation = torch.randn(B, r, 64, device=dev, generator=gen)
    graph.query = torch.randn(B, 64, device=dev, generator=gen)
    h = torch.randint(0, n, (B,), device=dev, generator=gen)
    graph.boundary = torch.zeros(n, B, 64, device=dev)
    graph.boundary[h, torch.arange(B, device=dev)] = graph.query
    x = torch.randn(n, B, 64, device=dev, generator=gen)
    with torch.no_grad():
        first = conv(graph, x)           # builds and caches the plans
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        out = conv(graph, x)
        torch.cuda.synchronize()
        rise = torch.cuda.max_memory_allocated() - base
    assert torch.equal(first, out)
    row_bytes = n * B * 64 * 4
    assert rise <= 6 * row_bytes, "peak rose by %.1f MB, %.1f (N, B*64) tensors" % (rise / 2 ** 20, rise / row_bytes)

"""Test infrastructure: the model stack over a plain float64 DEFINITION of the rspmm operator -- the truth for what the
reference's rspmm branch computes where it is another function than the recorded ``message`` + ``aggregate`` branch.

That is the case for the gradients of a min / max aggregation at a tie: the recorded branch (``scatter_max``) hands the gradient to
one tied message, torchdrug's native backward -- which this package's operators mirror -- to EVERY tied edge in full
(``tests/exact_grid.py::definition``, numpy float64, to which ``test_exact_grid_cpu.py`` / ``_gpu.py`` hold the C oracle and every
kernel entry for entry).  :class:`DefinitionRSPMM` is the CPU backend of ``tests/oracle_ops.py`` with that definition behind
``generalized_rspmm``, forward and backward; everything else a training step touches runs as ATen ops.  In float64 it reproduces
the recordings of ``reference_architectures.npz`` to 1e-15 in every tensor that does NOT pass a min / max backward (asserted by
``test_reference_architectures_cpu.py``), which is what makes it a truth for the tensors that do."""
import numpy as np
import torch

import exact_grid as XG
import reference_fixture as RF
import reference_runs as RR
from oracle_ops import OracleFunctional


def _edges(csr):
    weight = None if csr.unit_weight else csr.weight.cpu().numpy().astype(np.float64)
    return [t.cpu().numpy() for t in (csr.dst, csr.src, csr.rel_id)] + [weight]


class _Definition(torch.autograd.Function):
    @staticmethod
    def forward(ctx, relation, input, csr, sum, mul):
        ctx.call = (csr, sum, mul)
        ctx.save_for_backward(relation, input)
        n_rows = csr.shape[0]
        out = XG.definition(*_edges(csr), relation.detach().numpy(), input.detach().numpy(), np.zeros((n_rows, input.shape[1])),
                            n_rows, sum, mul)[0]
        return torch.from_numpy(out).to(input.dtype)

    @staticmethod
    def backward(ctx, grad):
        csr, sum, mul = ctx.call
        relation, input = ctx.saved_tensors
        _, d_input, d_relation, _, _ = XG.definition(*_edges(csr), relation.detach().numpy(), input.detach().numpy(), grad.numpy(),
                                                     csr.shape[0], sum, mul)
        return torch.from_numpy(d_relation).to(relation.dtype), torch.from_numpy(d_input).to(input.dtype), None, None, None


class DefinitionRSPMM(OracleFunctional):
    def __init__(self):
        super().__init__(0)

    def generalized_rspmm(self, sparse, relation, input, sum="add", mul="mul"):
        return _Definition.apply(relation.contiguous(), input.contiguous(), sparse, sum, mul)


_TRUTH = {}


def rspmm_branch_training_run(name, width):
    """``(truth, own_dev)`` of the train-mode run of one architecture case on the rspmm branch: ``truth`` the float64 run over the
    definition, under the recorded keys; ``own_dev[key]`` = ``max|float32 run - float64 run|`` of the SAME definition: what
    ``ref_dev`` is for the recorded branch -- the float32 deviation of an evaluation that involves no kernel and no C oracle."""
    if (name, width) not in _TRUTH:
        from ultra_torchdrug_amd import backend
        cpu = torch.device("cpu")
        with backend.use(DefinitionRSPMM()):
            truth = RR.architecture_run(name, width, cpu, torch.float64, "train")
            single = RR.architecture_run(name, width, cpu, torch.float32, "train")
        as_array = lambda v: np.asarray(v.detach().double().numpy() if torch.is_tensor(v) else v, dtype=np.float64)
        truth = {k: as_array(v) for k, v in truth.items()}
        _TRUTH[(name, width)] = (truth, {k: float(np.abs(as_array(single[k]) - truth[k]).max()) for k in truth})
    return _TRUTH[(name, width)]


def check_extreme_gradients(name, width, got, floor):
    """The gradients of ``got`` that pass a min / max backward (``RF.gradient_passes_an_extreme``) against the float64 run of the
    rspmm branch: ``max|got - truth| <= (4 * own + floor) * scale`` -- the rule of every other comparison, with the rspmm
    branch's own truth and float32 deviation in the place of the recorded branch's.  ``own`` is the WORST ``own_dev / scale``
    over these gradients of the case, not each tensor's own figure: where a float32 evaluation is ill-conditioned (``defaults``
    at 64: 2.3e-2) its deviation is no property of a tensor but of where that evaluation's roundings happen to fall -- another
    float32 evaluation, or the same one run again on a device whose reductions are not ordered, puts its large deviations into
    other tensors (a bound per tensor was tried first and failed on ``layers.0.linear.weight``: 2.9e-5 against the definition's
    own 2.3e-6 there, while other tensors of the same run deviate by 1e-2).  Where it is well-conditioned ``own`` is below 1e-6
    and the bound is the floor rule's.  The bound must stay below the distance between the two branches, and the truth must
    DIFFER from the recording (else the two branches are one function here and the recording is the truth).  Returns the keys."""
    tag = "%s_%d" % (name, width)
    stats = RR.stats("architectures")
    behind = sorted(k for k in stats if k.startswith(tag + "/") and RF.gradient_passes_an_extreme(name, width, k))
    if not behind:
        return behind
    truth, own_dev = rspmm_branch_training_run(name, width)
    own = max(own_dev[key] / stats[key]["scale"] for key in behind)
    apart = max(float(np.abs(truth[key] - RR.truth("architectures", key)).max()) / stats[key]["scale"] for key in behind)
    print("%s: the rspmm branch's float32 run lies %.3e of scale from its float64 run, the recorded branch %.3e" % (tag, own, apart))
    assert apart > 1e-3 and 4 * own + floor < apart, (tag, own, apart)
    failed = []
    for key in behind:
        scale = stats[key]["scale"]
        value = np.asarray(got[key].detach().double().cpu().numpy() if torch.is_tensor(got[key]) else got[key], dtype=np.float64)
        assert np.isfinite(value).all(), key
        err = float(np.abs(value - truth[key]).max())
        print("%-10s %-60s %.3e of scale from the rspmm branch's float64 run (its own float32 run %.3e)"
              % ("extreme", key, err / scale, own_dev[key] / scale))
        if err > (4 * own + floor) * scale:
            failed.append("%s: %.3g of scale from the rspmm branch's float64 run (bound %.3g)" % (key, err / scale, 4 * own + floor))
    assert not failed, failed
    return behind

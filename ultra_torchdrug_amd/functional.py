"""Host-side mirror of ``torchdrug.layers.functional.generalized_rspmm`` for the MI355X HIP library.

Reference call sites: ``/root/reference/ultra/layer.py:134-167`` and ``:336-369``, always
``functional.generalized_rspmm(adjacency, relation_input, input, sum=<"add"|"max"|"min">, mul=<"mul"|"add">)``.
Same name, argument order, keyword names and error behaviour (unknown operator names raise ``ValueError``;
shape/device problems raise ``RuntimeError``).  Extension: ``sparse`` may be a cached :class:`RelCSR` instead of
a 3-D sparse COO tensor, so the sort torchdrug repeats on every call happens once per graph.

Everything numerical happens in native code; this module only validates, allocates outputs with torch and passes raw
pointers plus the current HIP stream across the C ABI of ``libultra_rspmm.so``.  CPU tensors (the reference's
``--gpus null`` runs, ``/root/reference/README.md:79,90``) go to the CPU kernels of the same dispatcher operators
(``torch.ops.ultra_mi.rspmm_fwd / rspmm_bwd``, ``csrc/torch_ext.cpp``): the operator itself, in the reference's
sequential order; the fused / plan-based extras of this module (boundary epilogue, frontier, fused layers, device-side
ranking and sampling) are MI355X-only and raise on CPU tensors.  Without the native libraries every operator raises: there
is no Python or PyTorch fallback, and the CPU oracle under ``oracle/`` is test infrastructure that is never imported here.
"""
import collections
import ctypes
import os

import torch

from . import _lib, _torch_ext
from .relcsr import RelCSR

__all__ = ["generalized_rspmm", "rspmm_forward", "rotate_rspmm", "rotate_rspmm_forward", "rotate_rspmm_backward_weight", "rspmm_backward_weight_blocks", "rotate_rspmm_backward_weight_blocks", "beam_search_step_batch", "first_layer_forward", "dense_layer_forward", "combine_forward", "combine", "linear_forward", "linear_supported", "score_all_entities", "relation_stack_inputs", "statistics", "bce_adversarial_loss", "candidate_tiles", "candidate_rows", "score_candidates", "hop_distance", "pack_sets", "unpack_sets", "seed_sets", "column_mask", "project_sets_exact", "set_ranks", "relation_select", "dense_relation_select", "candidate_select", "dense_candidate_select", "constrained_negatives", "dense_constrained_negatives", "query_tables", "dense_query_tables", "RelCSR"]

# Plans built from raw sparse tensors, most recent last.  Every entry holds strong references to the index and
# value tensors it was built from, so a (data_ptr, version) key cannot be reused by another live tensor.
_sparse_cache = collections.OrderedDict()
_SPARSE_CACHE_ENTRIES = 4


def accepts(tensor):
    """Backend interface (``backend.py``): the HIP library computes on device tensors only."""
    return bool(tensor.is_cuda)


def _ops(sum, mul):
    if sum not in _lib.SUM_OPS:
        raise ValueError("Can't find a rspmm operator for sum=`%s` (expected add, min or max)" % sum)
    if mul not in _lib.MUL_OPS:
        raise ValueError("Can't find a rspmm operator for mul=`%s` (expected mul or add)" % mul)
    return _lib.SUM_OPS[sum], _lib.MUL_OPS[mul]


def _as_relcsr(sparse):
    if isinstance(sparse, RelCSR):
        return sparse, None
    if not isinstance(sparse, torch.Tensor) or not sparse.is_sparse:
        raise TypeError("sparse must be a 3-D torch sparse COO tensor or a RelCSR, got %s" % type(sparse).__name__)
    idx, val = sparse._indices(), sparse._values()
    key = (idx.data_ptr(), val.data_ptr(), idx._version, val._version, tuple(sparse.shape))
    hit = _sparse_cache.get(key)
    if hit is None:
        hit = (RelCSR.from_sparse(sparse), idx, val)
        _sparse_cache[key] = hit
        while len(_sparse_cache) > _SPARSE_CACHE_ENTRIES:
            _sparse_cache.popitem(last=False)
    else:
        _sparse_cache.move_to_end(key)
    return hit[0], (sparse if sparse.requires_grad else None)


def _check_dense(csr, relation, input, require_hip=True):
    n_dst, n_src, n_rel = csr.shape
    if input.dim() != 2 or relation.dim() != 2:
        raise RuntimeError("relation and input must be 2-D, got %s and %s" % (tuple(relation.shape), tuple(input.shape)))
    if input.shape[0] != n_src:
        raise RuntimeError("Expect input to have %d rows, but found %d" % (n_src, input.shape[0]))
    if relation.shape[0] != n_rel:
        raise RuntimeError("Expect relation to have %d rows, but found %d" % (n_rel, relation.shape[0]))
    if relation.shape[1] != input.shape[1]:
        raise RuntimeError("Expect relation and input to have the same width, but found %d and %d"
                           % (relation.shape[1], input.shape[1]))
    if input.dtype != torch.float32 or relation.dtype != torch.float32:
        raise RuntimeError("rspmm is fp32 only (TF32 is disabled in the reference, script/run_full.py:19-20)")
    if require_hip and (not input.is_cuda or not relation.is_cuda):
        raise RuntimeError("this operator of ultra_torchdrug_amd runs on an MI355X (HIP) device only; "
                           "got input on %s, relation on %s (only generalized_rspmm has CPU kernels)"
                           % (input.device, relation.device))
    if input.device != relation.device or input.device != csr.device:
        raise RuntimeError("sparse, relation and input must be on one device (%s, %s, %s)"
                           % (csr.device, relation.device, input.device))


# The one way across the C boundary (``_lib.launch``): tensors -> pointers, None -> NULL, current stream, status check.
_launch, _ptr = _lib.launch, _lib.ptr


def _env_bool(name, default):
    """An ``ULTRA_*`` switch: on unless set to ``0`` where ``default`` is True, off unless set to ``1`` where it is False."""
    return os.environ.get(name, "1") != "0" if default else os.environ.get(name, "0") == "1"


def _env_float(name, default):
    return float(os.environ.get(name, default))


def _env_int(name, default):
    return int(os.environ.get(name, default))


def _not_fp32_on(device, tensors):
    """True unless every tensor is fp32 on the HIP device ``device``."""
    return any(t.dtype != torch.float32 or not t.is_cuda or t.device != device for t in tensors)


def _epilogue(weight, bias, ln_weight, ln_bias, ln_eps, relu, shortcut=None):
    """The argument run ``weight, bias, ln_weight, ln_bias, ln_eps, relu[, shortcut]`` of the epilogue kernels: the parameters
    contiguous, both LayerNorm vectors NULL without ``ln_weight``.  ``shortcut=None``: the entry has no such argument (the split
    three-kernel backward)."""
    has_ln = ln_weight is not None
    run = (weight.contiguous(), bias.contiguous(), ln_weight.contiguous() if has_ln else None,
           ln_bias.contiguous() if has_ln else None, float(ln_eps), int(bool(relu)))
    return run if shortcut is None else run + (int(bool(shortcut)),)


def _pointer_array(tensors):
    """``void *[len(tensors)]`` of the tensors' addresses (NULL for ``None``); the caller keeps the tensors alive."""
    return (ctypes.c_void_p * len(tensors))(*[_ptr(t) for t in tensors])


def _plan(seg):
    return None if seg is None else seg.pointer


def _workspace(seg, F, device):
    n = seg.workspace_rows * F
    if n == 0:
        return None, 0
    ws = torch.empty(n, dtype=torch.float32, device=device)
    return ws, n * 4


def _backward_workspace(by_src, by_rel, F, device):
    """``(workspace, bytes)`` of a backward over the plans in use (``None`` = that gradient is not wanted)."""
    n_ws = max(by_src.workspace_rows if by_src is not None else 0, by_rel.workspace_rows if by_rel is not None else 0) * F
    return (torch.empty(n_ws, dtype=torch.float32, device=device) if n_ws else None), n_ws * 4


def _check_boundary_epilogue(out, add_rows, boundary, block=None):
    """The boundary epilogue of ``rspmm_forward`` / ``rotate_rspmm_forward`` validated against the output ``out``:
    ``(add_rows, b_node, b_value)``, the dense form and the sparse form's values contiguous.  ``block`` (rotate): the value
    rows are exactly that wide."""
    F = out.shape[1]
    both = "give the boundary either dense (add_rows) or sparse (boundary), not both"
    if block is not None and add_rows is not None and boundary is not None:     # (rotate reports this before a bad add_rows)
        raise RuntimeError(both)
    if add_rows is not None:
        add_rows = add_rows.contiguous()
        if add_rows.shape != out.shape or add_rows.dtype != torch.float32 or add_rows.device != out.device:
            raise RuntimeError("add_rows must be fp32 %s on %s" % (tuple(out.shape), out.device))
    b_node = b_value = None
    if boundary is not None:
        if add_rows is not None:
            raise RuntimeError(both)
        b_node, b_value = boundary
        b_value = b_value.contiguous()
        if (b_node.dtype != torch.int32 or b_value.dtype != torch.float32 or b_node.dim() != 1 or b_value.dim() != 2
                or (b_value.shape[0] != b_node.shape[0] if block is None else b_value.shape != (b_node.shape[0], block))
                or b_value.numel() != F or b_node.device != out.device
                or b_value.device != out.device or not b_node.is_contiguous()):
            width = "D" if block is None else "%d" % block
            raise RuntimeError("boundary must be (int32 (B,), fp32 (B, %s)) with B * %s == %d on %s" % (width, width, F, out.device))
    return add_rows, b_node, b_value


def _check_d_input_add(d_input_add, input, sum, need_input):
    if d_input_add is not None and (not need_input or sum != "add" or not d_input_add.is_contiguous()
                                    or d_input_add.shape != input.shape or d_input_add.dtype != torch.float32):
        raise RuntimeError("d_input_add: contiguous fp32 tensor of input's shape, sum aggregation, with need_input")


def _boundary_value_grad(output_grad, b_node):
    """Gradient of a sparse boundary's values: row ``b_node[q]`` of query block ``q`` of ``output_grad``."""
    n_query = b_node.shape[0]
    blocks = output_grad.view(output_grad.shape[0], n_query, -1)
    return blocks[b_node.long(), torch.arange(n_query, device=output_grad.device)]


def rspmm_forward(csr, relation, input, sum="add", mul="mul", add_rows=None, boundary=None):
    """Forward only, no autograd.  ``add_rows`` fuses the boundary epilogue of ``layer.py:156,162,358,364``;
    ``boundary = (node, value)`` is the same epilogue with the boundary in its sparse form: ``node`` int32 ``(B,)``,
    ``value`` fp32 ``(B, D)`` with ``B * D == F`` -- row ``node[b]`` of query block ``b`` holds ``value[b]``, all else 0
    (what ``scatter_add_`` builds in ``model.py:106-107``)."""
    sum_op, mul_op = _ops(sum, mul)
    _check_dense(csr, relation, input)
    relation, input = relation.contiguous(), input.contiguous()
    F = input.shape[1]
    out = torch.empty(csr.shape[0], F, dtype=torch.float32, device=input.device)
    add_rows, b_node, b_value = _check_boundary_epilogue(out, add_rows, boundary)
    if out.numel() == 0:
        return out
    seg = csr.fwd
    if _torch_ext.binding() == "torch":         # through the dispatcher: torch.ops.ultra_mi (csrc/torch_ext.cpp)
        return _torch_ext.load().rspmm_plan_fwd(seg.plan_tensor, relation, input, add_rows, b_node, b_value,
                                                csr.shape[1], sum_op, mul_op)
    ws, ws_bytes = _workspace(seg, F, input.device)
    if boundary is not None:
        _launch(input.device, "ultra_rspmm_forward_boundary_f32", seg.pointer, relation, input, b_node, b_value,
                b_value.shape[1], out, ws, ws_bytes, csr.shape[1], csr.shape[2], F, sum_op, mul_op)
        return out
    _launch(input.device, "ultra_rspmm_forward_f32", seg.pointer, relation, input, add_rows, out, ws, ws_bytes, csr.shape[1],
            csr.shape[2], F, sum_op, mul_op)
    return out


def rspmm_forward_csr(row_ptr, src, rel, weight, relation, input, sum="add", mul="mul"):
    """The operator straight from a coalesced CSR (``ultra_rspmm_fwd_f32``, SURVEY.md 8b's raw entry): ``row_ptr`` int32
    ``(N + 1,)``, ``src`` / ``rel`` int32 ``(E,)`` sorted by (row, src, rel), ``weight`` fp32 ``(E,)`` or ``None``.
    No plan and no workspace; every row is reduced strictly sequentially (the reference order).  Forward only."""
    sum_op, mul_op = _ops(sum, mul)
    if input.dim() != 2 or relation.dim() != 2 or relation.shape[1] != input.shape[1]:
        raise RuntimeError("relation (R, F) and input (N_src, F) expected, got %s and %s"
                           % (tuple(relation.shape), tuple(input.shape)))
    tensors = [row_ptr, src, rel, relation, input] + ([weight] if weight is not None else [])
    if any(not t.is_cuda or t.device != input.device for t in tensors):
        raise RuntimeError("rspmm_forward_csr runs on an MI355X (HIP) device only. There is no CPU fallback.")
    if row_ptr.dtype != torch.int32 or src.dtype != torch.int32 or rel.dtype != torch.int32:
        raise RuntimeError("rspmm_forward_csr: row_ptr / src / rel must be int32")
    if input.dtype != torch.float32 or relation.dtype != torch.float32 or (weight is not None and weight.dtype != torch.float32):
        raise RuntimeError("rspmm is fp32 only (TF32 is disabled in the reference, script/run_full.py:19-20)")
    F = input.shape[1]
    if F % 4:
        raise RuntimeError("rspmm_forward_csr needs 16-byte rows (F % 4 == 0); use a RelCSR plan for other widths")
    n_rows, n_edges = row_ptr.numel() - 1, src.numel()
    relation, input = relation.contiguous(), input.contiguous()
    out = torch.empty(n_rows, F, dtype=torch.float32, device=input.device)
    if out.numel() == 0:
        return out
    _launch(input.device, "ultra_rspmm_fwd_f32", row_ptr.contiguous(), src.contiguous(), rel.contiguous(),
            weight.contiguous() if weight is not None else None, relation, input, out, n_rows, n_edges, relation.shape[0], F,
            sum_op, mul_op)
    return out


def pna_supported(csr):
    """Whether :func:`pna_statistics` takes this adjacency: every plan but those that carry a dense form (the relation graphs,
    whose sums run on the matrix cores in another documented order -- the four :func:`rspmm_forward` calls serve them)."""
    return csr.fwd.dense is None


def pna_statistics(csr, relation, input, mul="mul", add_rows=None, boundary=None):
    """The four statistics of ``aggregate_func="pna"`` from one walk of the forward plan (``ultra_rspmm_pna_forward_f32``):
    ``(4, n_rows, F)`` = sum, sum over the squared operands, max, min, each plane bit-identical to the :func:`rspmm_forward`
    call it replaces (``ultra/layer.py:160-167,362-369``); ``add_rows`` / ``boundary = (node, value)`` fuse the boundary as
    there: ``+ b``, ``+ b * b``, ``max(., b)``, ``min(., b)``.  Forward only, no autograd; HIP tensors only."""
    if mul not in _lib.MUL_OPS:
        raise ValueError("Can't find a rspmm operator for mul=`%s` (expected mul or add)" % mul)
    _check_dense(csr, relation, input)
    relation, input = relation.contiguous(), input.contiguous()
    F = input.shape[1]
    out = torch.empty(4, csr.shape[0], F, dtype=torch.float32, device=input.device)
    add_rows, b_node, b_value = _check_boundary_epilogue(out[0], add_rows, boundary)
    if not pna_supported(csr):
        raise RuntimeError("pna_statistics: this adjacency carries a dense form (a relation graph); use four rspmm_forward calls")
    if out.numel() == 0:
        return out
    seg = csr.fwd
    n_ws = 4 * seg.workspace_rows * F
    ws = torch.empty(n_ws, dtype=torch.float32, device=input.device) if n_ws else None
    _launch(input.device, "ultra_rspmm_pna_forward_f32", seg.pointer, relation, input, add_rows, b_node, b_value,
            b_value.shape[1] if b_value is not None else 0, out[0], out[1], out[2], out[3], ws, n_ws * 4, csr.shape[1],
            csr.shape[2], F, _lib.MUL_OPS[mul])
    return out


def pna_node_table(degree_out):
    """``(N, 3)`` fp32: degree, scale, inverse scale of every node, exactly as ``layer._pna`` computes them from
    ``degree_out = graph.degree_out + 1`` (``ultra/layer.py:150-152``): ``log``, ``/ mean()``, ``1 / clamp(min=1e-2)``."""
    degree = degree_out.reshape(-1, 1)
    scale = degree.log()
    scale = scale / scale.mean()
    return torch.cat([degree, scale, 1 / scale.clamp(min=1e-2)], dim=-1).contiguous()


def pna_combine_forward(input, statistics, node_table, weight, bias, ln_weight=None, ln_bias=None, ln_eps=1e-5, pna_eps=1e-6,
                        relu=True, shortcut=False, out=None, n_query=None):
    """Fused epilogue of a PNA layer, forward only (``ultra_pna_combine_forward_f32``): ``[input +] relu(LN(Linear(cat[input,
    _pna(statistics)])))`` without the ``(N, B, 768)`` update tensor.  ``input`` ``(N, B, 64)``; ``statistics`` ``(4, N, B * 64)``
    from :func:`pna_statistics` (or four ``(N, B * 64)`` tensors: sum, sq_sum, max, min, boundary included); ``node_table``
    ``(N, 3)`` from :func:`pna_node_table`; ``weight`` ``(64, 832)``.  ``input`` may also be ``(rows, 64)`` with ``n_query`` given: row ``i``
    is then (node ``i // n_query``, query ``i % n_query``) and ``node_table`` has ``ceil(rows / n_query)`` rows.  ``out``: an optional contiguous fp32 tensor of the input's shape to
    write into; it must not share memory with ``input`` or a statistic (the kernel reads a row's tensors after other rows
    have been written) -- that raises."""
    planes = [t.contiguous() for t in statistics]
    if n_query is None and input.dim() == 3:
        n_query = input.shape[1]
    rows = input.numel() // 64 if input.dim() >= 2 and input.shape[-1] == 64 else -1
    if (rows < 0 or input.dim() not in (2, 3) or not n_query or n_query < 1 or (input.dim() == 3 and n_query != input.shape[1])
            or tuple(weight.shape) != (64, 832) or len(planes) != 4 or any(t.numel() != input.numel() for t in planes)
            or tuple(node_table.shape) != (-(-rows // n_query), 3) or tuple(bias.shape) != (64,)):
        raise RuntimeError("pna_combine_forward handles 64 -> 64 layers with a (64, 832) weight: input (N, B, 64), four statistics of "
                           "N * B * 64 elements, node_table (N, 3); got input %s, weight %s, node_table %s"
                           % (tuple(input.shape), tuple(weight.shape), tuple(node_table.shape)))
    tensors = [input, node_table, weight, bias] + planes + ([ln_weight, ln_bias] if ln_weight is not None else [])
    if _not_fp32_on(input.device, tensors):
        raise RuntimeError("pna_combine_forward needs fp32 tensors on one HIP device (no CPU fallback)")
    input, node_table = input.contiguous(), node_table.contiguous()
    if out is None:
        out = torch.empty_like(input)
    else:
        if out.shape != input.shape or out.dtype != torch.float32 or out.device != input.device or not out.is_contiguous():
            raise RuntimeError("pna_combine_forward: out must be a contiguous fp32 tensor of the input's shape on its device")
        lo, hi = out.data_ptr(), out.data_ptr() + out.numel() * 4
        if any(t.data_ptr() < hi and lo < t.data_ptr() + t.numel() * 4 for t in [input] + planes):
            raise RuntimeError("pna_combine_forward: out must not alias input or a statistic")
    if out.numel() == 0:
        return out
    _launch(input.device, "ultra_pna_combine_forward_f32", input, *planes, node_table, int(n_query),
            *_epilogue(weight, bias, ln_weight, ln_bias, ln_eps, relu)[:5], float(pna_eps), int(bool(relu)), int(bool(shortcut)),
            out, input.numel() // 64, 64)
    return out


def frontier_supported(sum, mul, F):
    """The first-layer shortcut holds where a zero source row contributes exactly +-0: summed DistMult messages with a
    FINITE relation table (``inf * 0 = NaN`` in the full kernels; the caller tests the table, ``layer._frontier_tables_finite``)."""
    return sum == "add" and mul == "mul" and F % 64 == 0


def rspmm_frontier(csr, relation, boundary):
    """``rspmm_forward(csr, relation, <dense boundary>, "add", "mul", boundary=boundary)`` for the FIRST Bellman-Ford
    layer, whose input is the boundary itself (``ultra/model.py:116-120``): zero outside row ``node[b]`` of query block
    ``b``.  Visits only the out-edges of the boundary nodes; same bits as the full kernels (see ``csrc/frontier.inc``).
    ``boundary = (node int32 (B,), value fp32 (B, 64))``; forward only.  Precondition: ``relation`` is finite -- an
    ``inf`` / ``NaN`` entry reaches only the destinations of the boundary nodes' out-edges here, every destination of an
    edge of that relation in the full kernel (``tests/test_frontier_sampler_gpu.py::test_frontier_non_finite_*``)."""
    b_node, b_value = boundary
    b_value = b_value.contiguous()
    n_dst, n_src, n_rel = csr.shape
    F = b_value.numel()
    if relation.dim() != 2 or relation.shape != (n_rel, F) or relation.dtype != torch.float32 or not relation.is_cuda:
        raise RuntimeError("rspmm_frontier: relation must be fp32 (%d, %d) on the HIP device" % (n_rel, F))
    if (b_node.dtype != torch.int32 or b_node.dim() != 1 or b_value.dtype != torch.float32 or b_value.dim() != 2
            or b_value.shape != (b_node.shape[0], 64) or not b_node.is_contiguous()
            or b_node.device != relation.device or b_value.device != relation.device or csr.device != relation.device):
        raise RuntimeError("rspmm_frontier: boundary must be (int32 (B,), fp32 (B, 64)) on %s" % relation.device)
    if n_dst != n_src:
        raise RuntimeError("rspmm_frontier: the boundary rows index the source nodes of a square adjacency")
    relation = relation.contiguous()
    out = torch.empty(n_dst, F, dtype=torch.float32, device=relation.device)
    if out.numel() == 0:
        return out
    src_ptr, fwd_rank = csr.frontier_index
    _launch(relation.device, "ultra_rspmm_frontier_f32", csr.by_src.pointer, src_ptr, fwd_rank, relation, b_node, b_value, 64,
            out, n_dst, n_rel, F)
    return out


# Sparse first layer in inference (ultra_first_layer_sparse_f32).  ULTRA_SPARSE_FIRST_LAYER=0: frontier kernel + dense epilogue.
SPARSE_FIRST_LAYER = _env_bool("ULTRA_SPARSE_FIRST_LAYER", True)
# ... from this many output rows (nodes x queries) on: on a small dense graph a hub's out-edges reach most nodes, the list is
# most of the rows and its indexed epilogue loses to the dense one (S-codexs, 65 k rows: 17 us against 13; S-fb15k237, 465 k rows:
# 24 us against 108 on the hub-heaviest batch)
SPARSE_FIRST_LAYER_MIN_ROWS = 1 << 17


# The row list (and, in training, the compacted backward workspace: 5 x 64 floats per slot) is sized for the WORST head:
# n_query * (max_runs + 1) slots.  The density gates look at the degree-weighted mean; one hub that reaches most of the nodes in an
# otherwise sparse graph would pass them and allocate several (N, B, 64)-sized scratch tensors per step: the sparse
# forms are taken only where the longest list is at most this fraction of the nodes (ULTRA_SPARSE_FIRST_LAYER_MAX_LIST).
SPARSE_FIRST_LAYER_MAX_LIST = _env_float("ULTRA_SPARSE_FIRST_LAYER_MAX_LIST", 1.0)
# ... and, in training, where the backward's compacted workspace (5 rows of 64 floats per slot) stays within this many bytes
SPARSE_FIRST_LAYER_TRAIN_MAX_BYTES = _env_int("ULTRA_SPARSE_FIRST_LAYER_TRAIN_MAX_BYTES", 2 << 30)


def _first_layer_arguments(csr, relation, b_node, b_value):
    """What both sparse first-layer entries pass around their epilogue run: ``(device, head, tail, out, row_list, list_offset)``
    -- ``head`` the frontier index and the operands, ``tail`` the freshly allocated output, row list and list offsets with
    their sizes (``ultra_first_layer_sparse_f32`` / ``..._train_f32``)."""
    n_dst, _, n_rel = csr.shape
    n_query = b_node.shape[0]
    relation = relation.contiguous()
    dev = relation.device
    src_ptr, fwd_rank = csr.frontier_index
    run_prefix, max_runs = csr.frontier_runs
    out = torch.empty(n_dst, n_query, 64, dtype=torch.float32, device=dev)
    row_list = torch.empty(n_query * (max_runs + 1), dtype=torch.int32, device=dev)
    list_offset = torch.empty(n_query + 1, dtype=torch.int32, device=dev)
    head = (csr.by_src.pointer, src_ptr, fwd_rank, run_prefix, relation, b_node, b_value, n_query)
    tail = (out, row_list, row_list.numel(), int(max_runs), list_offset, n_dst, n_rel)
    return dev, head, tail, out, row_list, list_offset


def first_layer_forward(csr, relation, boundary, weight, bias, ln_weight=None, ln_bias=None, ln_eps=1e-5, relu=True,
                        shortcut=False, want_list=False):
    """The whole FIRST Bellman-Ford layer in inference -- ``rspmm_frontier`` followed by ``combine_forward(None, update, ...,
    input_boundary=boundary)``, bit for bit -- with the epilogue on the rows the frontier reaches only: every other row of the
    layer's output is one constant vector (``relu(LN(bias))``; ``ultra/model.py:116-127``), computed once and broadcast.
    ``boundary = (node int32 (Q,), value fp32 (Q, 64))``; returns ``(N, Q, 64)``, or ``None`` where the fused entry does not
    apply (vocabulary beyond LDS, more than 128 queries, outputs beyond 4 GiB: the caller runs the two calls)."""
    if not SPARSE_FIRST_LAYER:
        return None
    b_node, b_value = boundary
    n_dst, n_src, n_rel = csr.shape
    n_query = b_node.shape[0]
    lib = _lib.load()
    if (n_dst != n_src or n_dst * n_query < SPARSE_FIRST_LAYER_MIN_ROWS
            or not lib.ultra_first_layer_sparse_supported(n_dst, n_rel, n_query)
            or csr.frontier_runs[1] + 1 > SPARSE_FIRST_LAYER_MAX_LIST * n_dst):
        return None
    F = n_query * 64
    b_value = b_value.contiguous()
    tensors = [relation, b_value, weight, bias] + ([ln_weight, ln_bias] if ln_weight is not None else [])
    if (relation.dim() != 2 or tuple(relation.shape) != (n_rel, F) or tuple(b_value.shape) != (n_query, 64) or b_node.dtype != torch.int32
            or not b_node.is_contiguous() or tuple(weight.shape) != (64, 128)
            or _not_fp32_on(relation.device, tensors)
            or b_node.device != relation.device or csr.device != relation.device):
        raise RuntimeError("first_layer_forward: relation fp32 (%d, %d), boundary (int32 (Q,), fp32 (Q, 64)), a (64, 128) weight, "
                           "all on one HIP device" % (n_rel, F))
    dev, head, tail, out, row_list, list_offset = _first_layer_arguments(csr, relation, b_node, b_value)
    _launch(dev, "ultra_first_layer_sparse_f32", *head, *_epilogue(weight, bias, ln_weight, ln_bias, ln_eps, relu, shortcut), *tail)
    if want_list:           # (out, the rows that differ from the layer's constant row, their count on the device): second_layer_sources
        return out, row_list, list_offset[n_query:]
    return out


# First layer in TRAINING sparse end to end (csrc/first_layer_train.inc).  ULTRA_SPARSE_FIRST_LAYER_TRAIN=0: the dense epilogue forward
# and backward over all N x B rows (same gradients up to the association of three 64-float sums).
SPARSE_FIRST_LAYER_TRAIN = _env_bool("ULTRA_SPARSE_FIRST_LAYER_TRAIN", True)
# ... on graphs where a training batch's boundary nodes (heads of sampled edges: hubs are likely) reach at most this fraction of the
# nodes each (RelCSR.frontier_fraction): the sparse form's cost grows with the listed rows, the dense form's does not.
SPARSE_FIRST_LAYER_TRAIN_MAX_FRACTION = _env_float("ULTRA_SPARSE_FIRST_LAYER_TRAIN_MAX_FRACTION", 0.2)


def first_layer_train_forward(csr, relation, boundary, weight, bias, ln_weight=None, ln_bias=None, ln_eps=1e-5, relu=True,
                              shortcut=False):
    """The first layer of an entity Bellman-Ford in training: ``(update, out, row_list, list_count)`` -- ``update`` ``(N, Q, 64)`` holds
    the frontier's raw sums + boundary at the LISTED rows (every other row is unwritten and never read), ``out`` = the layer's output
    (the epilogue on the listed rows, one constant row elsewhere; the bits of ``rspmm_frontier`` + ``combine_forward(input_boundary=
    ...)``), ``row_list`` int32 the listed rows (``node * Q + q``, -1 = empty slot) and ``list_count`` a one-element device tensor with
    the number of slots in use -- what the epilogue's backward (``ultra_first_layer_epilogue_backward_f32``) works from.  ``None``
    where the entry does not apply."""
    if not SPARSE_FIRST_LAYER_TRAIN:
        return None
    b_node, b_value = boundary
    n_dst, n_src, n_rel = csr.shape
    n_query = b_node.shape[0]
    lib = _lib.load()
    if (n_dst != n_src or n_dst * n_query < SPARSE_FIRST_LAYER_MIN_ROWS or n_dst * n_query > (1 << 24) - 64
            or not lib.ultra_first_layer_sparse_supported(n_dst, n_rel, n_query)
            or csr.frontier_fraction > SPARSE_FIRST_LAYER_TRAIN_MAX_FRACTION
            or csr.frontier_runs[1] + 1 > SPARSE_FIRST_LAYER_MAX_LIST * n_dst
            or n_query * (csr.frontier_runs[1] + 1) * 5 * 256 > SPARSE_FIRST_LAYER_TRAIN_MAX_BYTES):
        return None
    F = n_query * 64
    b_value = b_value.contiguous()
    if (tuple(relation.shape) != (n_rel, F) or tuple(b_value.shape) != (n_query, 64) or b_node.dtype != torch.int32
            or not b_node.is_contiguous() or tuple(weight.shape) != (64, 128)):
        return None
    update = torch.empty(n_dst, n_query, 64, dtype=torch.float32, device=relation.device)
    dev, head, tail, out, row_list, list_offset = _first_layer_arguments(csr, relation, b_node, b_value)
    _launch(dev, "ultra_first_layer_sparse_train_f32", *head, *_epilogue(weight, bias, ln_weight, ln_bias, ln_eps, relu, shortcut),
            update, *tail)
    return update, out, row_list, list_offset[n_query:]


# Entity layers in inference as ONE launch (rspmm + epilogue, csrc/layer_fused.hip) on plans that run one row per lane group
# (big graphs: row pointers, no split rows).  ULTRA_FUSED_LAYER=0: the two launches (same bits).
FUSED_LAYER = _env_bool("ULTRA_FUSED_LAYER", True)
# ... and the last layer with the score head inside the same launch (ULTRA_FUSED_SCORE=0: layer launch + score launch)
FUSED_SCORE = _env_bool("ULTRA_FUSED_SCORE", True)


# The SECOND layer's gathers when the first layer was sparse: all but the listed rows of its input hold one constant vector, so
# every edge whose source is not listed gathers ONE fixed unlisted row instead (cache hits; same bits).  ULTRA_SECOND_LAYER_SOURCES=0:
# the plan's own sources.  Taken where the list is at most 1 / 64 of the nodes (beyond that the remapped gathers are DRAM
# gathers again and the pass over the edges that builds them is pure cost).
SECOND_LAYER_SOURCES = _env_bool("ULTRA_SECOND_LAYER_SOURCES", True)


def second_layer_sources(csr, row_list, list_count, n_query):
    """int32 ``(E + slack,)``: for every edge of the forward plan the row the SECOND layer gathers -- the edge's own source when
    the sparse first layer listed it (``row_list`` / ``list_count`` of ``first_layer_forward(want_list=True)``), one fixed
    unlisted row otherwise (``ultra_second_layer_sources``).  ``None`` where it does not apply (plans the fused layer does not
    take, lists that are not small against the node count)."""
    if not SECOND_LAYER_SOURCES or not FUSED_LAYER:
        return None
    n_dst, n_src, n_rel = csr.shape
    plan = csr.fwd
    lib = _lib.load()
    if (n_dst != n_src or not lib.ultra_layer_forward_supported(plan.pointer, n_query, n_rel)
            or row_list.numel() * 64 > n_src or row_list.numel() + 1 >= n_src):
        return None
    dev = row_list.device
    E = plan.n_edges
    slack = plan.node_a.numel() - E
    sources = torch.empty(E + slack, dtype=torch.int32, device=dev)
    bitmap = torch.empty((n_src + 31) // 32, dtype=torch.int32, device=dev)
    c_node = torch.empty(1, dtype=torch.int32, device=dev)
    _launch(dev, "ultra_second_layer_sources", plan.node_a, E, slack, row_list, list_count, row_list.numel(), n_query, n_src,
            bitmap, c_node, sources)
    return sources


def layer_forward(csr, relation, input, boundary, weight, bias, ln_weight=None, ln_bias=None, ln_eps=1e-5, relu=True,
                  shortcut=False, sources=None):
    """``[input +] relu(LN(Linear(cat[input, rspmm(csr, relation, input, "add", "mul") + boundary])))`` -- one entity layer of a
    Bellman-Ford in inference (/root/reference/ultra/layer.py:298-392, ultra/model.py:126-127) -- in ONE launch where the forward
    plan runs one row per lane group: ``rspmm_forward(..., boundary=)`` + ``combine_forward`` bit for bit, without the ``update``
    tensor ever reaching memory.  ``input``: ``(N, Q, 64)``; ``boundary = (node int32 (Q,), value fp32 (Q, 64))`` or ``None``.
    Returns ``(N, Q, 64)`` (a new tensor), or ``None`` where the fused entry does not apply (the caller runs the two calls)."""
    if not FUSED_LAYER or input.dim() != 3 or input.shape[-1] != 64:
        return None
    n_dst, n_src, n_rel = csr.shape
    n_query = input.shape[1]
    lib = _lib.load()
    plan = csr.fwd
    if n_dst != n_src or input.shape[0] != n_src or not lib.ultra_layer_forward_supported(plan.pointer, n_query, n_rel):
        return None
    F = n_query * 64
    b_node, b_value = (None, None) if boundary is None else boundary
    tensors = [relation, input, weight, bias] + ([ln_weight, ln_bias] if ln_weight is not None else []) + ([b_value] if b_value is not None else [])
    if (ln_weight is not None and ln_bias is None) or any(t.numel() != 64 for t in tensors[3:4 + (2 if ln_weight is not None else 0)]):
        return None                                  # (bias, LayerNorm vectors: 64 entries each -- the kernel reads 64)
    if (tuple(relation.shape) != (n_rel, F) or tuple(weight.shape) != (64, 128)
            or _not_fp32_on(input.device, tensors)
            or (b_node is not None and (b_node.dtype != torch.int32 or tuple(b_node.shape) != (n_query,) or tuple(b_value.shape) != (n_query, 64)))):
        return None
    relation, input = relation.contiguous(), input.contiguous()
    out = torch.empty_like(input)
    if sources is not None:
        if sources.dtype != torch.int32 or sources.numel() != plan.node_a.numel() or sources.device != input.device:
            raise RuntimeError("layer_forward: sources must be second_layer_sources() of this plan")
        entry, lead = "ultra_layer_forward_sources_f32", (plan.pointer, sources)
    else:
        entry, lead = "ultra_layer_forward_f32", (plan.pointer,)
    _launch(input.device, entry, *lead, relation, input, b_node.contiguous() if b_node is not None else None,
            b_value.contiguous() if b_value is not None else None, n_query,
            *_epilogue(weight, bias, ln_weight, ln_bias, ln_eps, relu, shortcut), out, n_rel)
    return out


def layer_score_forward(csr, relation, input, boundary, weight, bias, ln_weight, ln_bias, ln_eps, relu, shortcut, query, w1, b1, w2,
                        b2):
    """The LAST entity layer of full-batch evaluation AND the score head in one launch: ``score_all_entities(layer_forward(...),
    query, w1, b1, w2, b2)`` bit for bit -- scores ``(Q, N)`` -- with the layer's ``(N, Q, 64)`` output never reaching memory
    (/root/reference/ultra/model.py:120-138,177-193).  ``None`` where the entry does not apply (the caller runs the two calls)."""
    if not FUSED_LAYER or not FUSED_SCORE or input.dim() != 3 or input.shape[-1] != 64:
        return None
    n_dst, n_src, n_rel = csr.shape
    n_query = input.shape[1]
    lib = _lib.load()
    plan = csr.fwd
    if n_dst != n_src or input.shape[0] != n_src or not lib.ultra_layer_score_supported(plan.pointer, n_query, n_rel):
        return None
    F = n_query * 64
    b_node, b_value = (None, None) if boundary is None else boundary
    tensors = [relation, input, weight, bias, query, w1, b1, w2, b2] + ([ln_weight, ln_bias] if ln_weight is not None else []) \
        + ([b_value] if b_value is not None else [])
    if (ln_weight is not None and ln_bias is None) or bias.numel() != 64 or b1.numel() != 128 \
            or (ln_weight is not None and (ln_weight.numel() != 64 or ln_bias.numel() != 64)):
        return None
    if (tuple(relation.shape) != (n_rel, F) or tuple(weight.shape) != (64, 128) or tuple(w1.shape) != (128, 128) or w2.numel() != 128
            or b2.numel() != 1 or tuple(query.shape) != (n_query, 64)
            or _not_fp32_on(input.device, tensors)
            or (b_node is not None and (b_node.dtype != torch.int32 or tuple(b_node.shape) != (n_query,) or tuple(b_value.shape) != (n_query, 64)))):
        return None
    relation, input = relation.contiguous(), input.contiguous()
    score = torch.empty(n_query, n_src, dtype=torch.float32, device=input.device)
    qbias = torch.empty(n_query, 128, dtype=torch.float32, device=input.device)
    _launch(input.device, "ultra_layer_score_forward_f32", plan.pointer, relation, input,
            b_node.contiguous() if b_node is not None else None, b_value.contiguous() if b_value is not None else None, n_query,
            *_epilogue(weight, bias, ln_weight, ln_bias, ln_eps, relu, shortcut), query.contiguous(), w1.contiguous(),
            b1.contiguous(), w2.contiguous(), b2.contiguous(), qbias, score, n_rel)
    return score


# Relation-graph layers in inference as ONE launch where the plan carries its dense form (ultra_dense_layer_forward_f32).
# ULTRA_DENSE_LAYER=0: the dense rspmm and the epilogue as two launches (same bits).
DENSE_LAYER = _env_bool("ULTRA_DENSE_LAYER", True)


def dense_layer_forward(csr, relation, input, boundary, weight, bias, ln_weight=None, ln_bias=None, ln_eps=1e-5, relu=True,
                        shortcut=False):
    """One whole layer of a relation-graph Bellman-Ford in inference -- ``rspmm_forward(csr, relation, input.flatten(1), "add",
    "mul", boundary=boundary)`` followed by ``combine_forward(input, update, ...)``, bit for bit -- in one launch, on a graph whose
    plans carry their dense form (``/root/reference/ultra/layer.py:111-190``, ``ultra/rel_model.py:371-372``).  ``input``
    ``(N, Q, 64)``; returns a new ``(N, Q, 64)`` tensor, or ``None`` where the entry does not apply (the caller runs the two calls)."""
    if not DENSE_LAYER or not getattr(csr, "dense_form", False) or input.dim() != 3 or input.shape[-1] != 64:
        return None
    n, n_query = input.shape[0], input.shape[1]
    F = n_query * 64
    seg = csr.fwd
    lib = _lib.load()
    if seg.dense is None or csr.shape[0] != n or csr.shape[1] != n or csr.shape[2] != 4 or \
            not lib.ultra_dense_layer_supported(seg.pointer, n_query):
        return None
    b_node, b_value = boundary
    b_value = b_value.contiguous()
    tensors = [relation, input, b_value, weight, bias] + ([ln_weight, ln_bias] if ln_weight is not None else [])
    if (tuple(relation.shape) != (4, F) or tuple(b_value.shape) != (n_query, 64) or b_node.dtype != torch.int32
            or not b_node.is_contiguous() or tuple(weight.shape) != (64, 128)
            or _not_fp32_on(input.device, tensors)
            or b_node.device != input.device or csr.device != input.device):
        raise RuntimeError("dense_layer_forward: input fp32 (N, Q, 64), relation fp32 (4, Q * 64), boundary (int32 (Q,), fp32 "
                           "(Q, 64)), a (64, 128) weight, all on one HIP device")
    relation, input = relation.contiguous(), input.contiguous()
    out = torch.empty_like(input)
    _launch(input.device, "ultra_dense_layer_forward_f32", seg.pointer, relation, input, b_node, b_value, n_query,
            *_epilogue(weight, bias, ln_weight, ln_bias, ln_eps, relu, shortcut), out)
    return out


# Training: the backward's gathers skipped where the caller knows the gradient (last layer) or the input (first layer) rows are
# zero -- see rspmm_backward(active_dst=, active_src=).  ULTRA_ACTIVE_ROW_BACKWARD=0: every edge gathers.
ACTIVE_ROW_BACKWARD = _env_bool("ULTRA_ACTIVE_ROW_BACKWARD", True)


# d_relation of the first layer from the boundary nodes' out-edges alone (ultra_rspmm_drelation_boundary_f32) instead of the masked
# walk over every edge of the graph; ULTRA_BOUNDARY_DRELATION=0: the masked walk.
BOUNDARY_DRELATION = _env_bool("ULTRA_BOUNDARY_DRELATION", True)


def rspmm_drelation_boundary(csr, input, output_grad, b_node):
    """``d_relation`` of ``rspmm(sum="add", mul="mul")`` for an ``input`` that is zero outside row ``b_node[q]`` of 64-column block
    ``q`` (the first Bellman-Ford layer: ``ultra/model.py:106-107,116-120``): only those nodes' out-edges are visited.  Same bits as
    ``rspmm_backward(..., active_src=b_node)[1]``.  ``input`` ``(N_src, F)``, ``output_grad`` ``(N_dst, F)``, ``b_node`` int32
    ``(F / 64,)``; returns ``(R, F)``."""
    input, output_grad = input.contiguous(), output_grad.contiguous()
    dev, F = input.device, input.shape[1]
    n_dst, n_src, n_rel = csr.shape
    if (input.dtype != torch.float32 or output_grad.dtype != torch.float32 or not input.is_cuda or output_grad.device != dev
            or tuple(input.shape) != (n_src, F) or tuple(output_grad.shape) != (n_dst, F) or F % 64 != 0 or F == 0):
        raise RuntimeError("rspmm_drelation_boundary: fp32 device tensors (N_src, F) and (N_dst, F) with F a multiple of 64")
    if b_node.dtype != torch.int32 or not b_node.is_contiguous() or b_node.device != dev or tuple(b_node.shape) != (F // 64,):
        raise RuntimeError("rspmm_drelation_boundary: b_node must be contiguous int32 (%d,) on %s" % (F // 64, dev))
    items, src_ptr, src_relpos = csr.boundary_relation_index
    plan = csr.by_rel
    d_relation = torch.empty(n_rel, F, dtype=torch.float32, device=dev)
    n_ws = int(plan.n_pieces) * F
    ws = torch.empty(n_ws, dtype=torch.float32, device=dev) if n_ws else None
    _launch(dev, "ultra_rspmm_drelation_boundary_f32", plan.pointer, items, items.shape[0], src_ptr, src_relpos, b_node, input,
            output_grad, d_relation, ws, n_ws * 4, n_src, n_rel, F)
    return d_relation


def candidate_rows(t_index, n_node):
    """Per query ``b`` the set ``{t_index[b, j]}`` as a bitmap over the nodes, int32 ``(B, ceil(N / 32))`` -- the rows of the LAST
    layer's output the score head reads (``ultra/model.py:177-183``), i.e. the only rows where that output's gradient is
    non-zero.  One launch, static shapes (capturable).  ``None`` beyond 512 Ki nodes or when the masked backward is switched off."""
    if not ACTIVE_ROW_BACKWARD or not t_index.is_cuda or t_index.dtype != torch.int64 or t_index.dim() != 2:
        return None
    n_words = (int(n_node) + 31) // 32
    if n_words > 16384 or n_words == 0:
        return None
    t_index = t_index.contiguous()
    bits = torch.empty(t_index.shape[0], n_words, dtype=torch.int32, device=t_index.device)
    _launch(t_index.device, "ultra_node_bitmap", t_index, t_index.shape[0], t_index.shape[1], int(n_node), bits)
    return bits


def rspmm_backward(csr, relation, input, output, output_grad, sum="add", mul="mul", need_input=True,
                   need_relation=True, d_input_add=None, active_dst=None, active_src=None):
    """``(d_input, d_relation)``.  ``d_input_add`` (sum aggregation only): a contiguous ``(N_src, F)`` gradient the
    same rows already hold (from the layer's dense epilogue); the edge gradient is accumulated INTO it inside the
    kernel's row epilogue and the same tensor is returned -- no separate add pass.
    ``active_dst`` (sum aggregation): int32 ``(F / 64, ceil(N_dst / 32))`` bitmaps (:func:`candidate_rows`) -- the caller's
    promise that ``output_grad[v, block b]`` is zero wherever bit ``v`` of row ``b`` is clear; ``active_src`` (sum, mul = mul):
    int32 ``(F / 64,)`` -- the promise that ``input[u, block b]`` is zero unless ``u == active_src[b]``.  Same results bit for bit;
    the kernels skip the gathers of edges that can only add zero (``ultra_rspmm_backward_active_f32``)."""
    sum_op, mul_op = _ops(sum, mul)
    relation, input, output_grad = relation.contiguous(), input.contiguous(), output_grad.contiguous()
    F = input.shape[1]
    dev = input.device
    if (ACTIVE_ROW_BACKWARD and sum == "add" and F % 64 == 0 and F > 0 and (need_input or need_relation)
            and (active_dst is not None or (active_src is not None and mul == "mul"))):
        n_tiles = F // 64
        if active_dst is not None and (active_dst.dtype != torch.int32 or not active_dst.is_contiguous() or active_dst.device != dev
                                       or tuple(active_dst.shape) != (n_tiles, (csr.shape[0] + 31) // 32)):
            raise RuntimeError("rspmm_backward: active_dst must be contiguous int32 (%d, %d) on %s"
                               % (n_tiles, (csr.shape[0] + 31) // 32, dev))
        if active_src is not None and (active_src.dtype != torch.int32 or not active_src.is_contiguous() or active_src.device != dev
                                       or tuple(active_src.shape) != (n_tiles,)):
            raise RuntimeError("rspmm_backward: active_src must be contiguous int32 (%d,) on %s" % (n_tiles, dev))
        _check_d_input_add(d_input_add, input, sum, need_input)
        d_input = (d_input_add if d_input_add is not None else torch.empty_like(input)) if need_input else None
        d_relation = torch.empty_like(relation) if need_relation else None
        by_src = csr.by_src if need_input else None
        by_rel = csr.by_rel if need_relation else None
        ws, ws_bytes = _backward_workspace(by_src, by_rel, F, dev)
        _launch(dev, "ultra_rspmm_backward_active_f32", _plan(by_src), _plan(by_rel), relation, input, output_grad, d_input_add,
                d_input, d_relation, ws, ws_bytes, csr.shape[1], csr.shape[0], csr.shape[2], F, mul_op, active_dst,
                active_dst.shape[1] if active_dst is not None else 0, active_src if mul == "mul" else None)
        return d_input, d_relation
    _check_d_input_add(d_input_add, input, sum, need_input)
    d_input = (d_input_add if d_input_add is not None else torch.empty_like(input)) if need_input else None
    d_relation = torch.empty_like(relation) if need_relation else None
    if F == 0 or (not need_input and not need_relation):
        return d_input, d_relation
    by_src = csr.by_src if need_input else None
    by_rel = csr.by_rel if need_relation else None
    if _torch_ext.binding() == "torch":
        d_rel = _torch_ext.load().rspmm_plan_bwd(
            by_src.plan_tensor if by_src is not None else None, by_rel.plan_tensor if by_rel is not None else None,
            relation, input, output, output_grad, d_input, d_input_add is not None, csr.shape[1], csr.shape[0], sum_op, mul_op)
        return d_input, (d_rel if need_relation else None)
    ws, ws_bytes = _backward_workspace(by_src, by_rel, F, dev)
    _launch(dev, "ultra_rspmm_backward_accumulate_f32", _plan(by_src), _plan(by_rel), relation, input, output, output_grad,
            d_input_add, d_input, d_relation, ws, ws_bytes, csr.shape[1], csr.shape[0], csr.shape[2], F, sum_op, mul_op)
    return d_input, d_relation


def rspmm_backward_boundary_rows(csr, relation, output_grad, boundary_node, d_input, mul="mul"):
    """First layer of a Bellman-Ford in training: the rspmm's edge gradient of ``input`` at the rows autograd consumes -- row
    ``boundary_node[q]`` of query block ``q`` (the layer's input is the boundary, ``ultra/model.py:106-107,116-120``) -- added
    IN PLACE into ``d_input`` ``(N_src, Q * 64)`` (``ultra_rspmm_backward_boundary_rows_f32``: the out-edges of one node per
    query instead of the ``d_input`` pass over every edge).  Sum aggregation only."""
    _, mul_op = _ops("add", mul)
    n_query = boundary_node.shape[0]
    F = n_query * 64
    if (boundary_node.dtype != torch.int32 or not boundary_node.is_contiguous() or d_input.dtype != torch.float32
            or not d_input.is_contiguous() or tuple(d_input.shape) != (csr.shape[1], F) or not output_grad.is_contiguous()
            or tuple(output_grad.shape) != (csr.shape[0], F) or output_grad.dtype != torch.float32
            or tuple(relation.shape) != (csr.shape[2], F) or not relation.is_contiguous() or csr.shape[0] != csr.shape[1]):
        raise RuntimeError("rspmm_backward_boundary_rows: contiguous fp32 (N, Q * 64) gradients, int32 (Q,) nodes, a square adjacency")
    src_ptr, _ = csr.frontier_index
    lib = _lib.load()
    ws = torch.empty(max(int(lib.ultra_rspmm_backward_boundary_rows_workspace(n_query)) // 4, 1), dtype=torch.float32,
                     device=d_input.device)
    _launch(d_input.device, "ultra_rspmm_backward_boundary_rows_f32", csr.by_src.pointer, src_ptr, relation, output_grad,
            boundary_node, d_input, ws, ws.numel() * 4, csr.shape[1], n_query, F, mul_op)
    return d_input


def rspmm_backward_weight(csr, relation, input, output, output_grad, sum="add", mul="mul"):
    """d(values) of the coalesced edges (forward-plan order)."""
    sum_op, mul_op = _ops(sum, mul)
    relation, input, output_grad = relation.contiguous(), input.contiguous(), output_grad.contiguous()
    d_w = torch.zeros(csr.n_edges, dtype=torch.float32, device=input.device)
    if csr.n_edges == 0 or input.shape[1] == 0:
        return d_w
    _launch(input.device, "ultra_rspmm_backward_weight_f32", csr.fwd.pointer, relation, input, output, output_grad, d_w,
            csr.shape[2], input.shape[1], sum_op, mul_op)
    return d_w


def rspmm_backward_weight_blocks(csr, relation, input, output, output_grad, sum="add", mul="mul", block=64):
    """:func:`rspmm_backward_weight` per query block of ``block`` columns: fp32 ``(F / block, n_edges)``, row ``b`` the gradient
    summed over columns ``b * block .. (b + 1) * block - 1`` alone -- bit for bit :func:`rspmm_backward_weight` on a contiguous
    copy of those columns (``ultra_rspmm_backward_weight_blocks_f32``: one wave per edge walks the blocks)."""
    sum_op, mul_op = _ops(sum, mul)
    block, F = int(block), input.shape[1]
    if block <= 0 or F <= 0 or F % block:
        raise RuntimeError("rspmm_backward_weight_blocks: a positive block width that divides F = %d expected, got %d" % (F, block))
    relation, input, output_grad = relation.contiguous(), input.contiguous(), output_grad.contiguous()
    output = output.contiguous() if output is not None else None
    d_w = torch.empty(F // block, csr.n_edges, dtype=torch.float32, device=input.device)       # written completely
    if csr.n_edges == 0:
        return d_w
    _launch(input.device, "ultra_rspmm_backward_weight_blocks_f32", csr.fwd.pointer, relation, input, output, output_grad, d_w,
            csr.shape[2], F, block, sum_op, mul_op)
    return d_w


def combine_forward(input, update, weight, bias, ln_weight=None, ln_bias=None, ln_eps=1e-5, relu=True, shortcut=False,
                    reuse_update=False, input_boundary=None, z_out=None):
    """Fused ``combine`` (+ shortcut) of one layer, forward only: ``[input +] relu(LN(Linear(cat[input, update])))``
    (``ultra/layer.py:386-392``, ``ultra/model.py:126-127``).  ``input`` / ``update``: ``(..., 64)`` fp32 on the GPU.
    ``reuse_update``: the caller owns ``update`` and does not need it afterwards -- the result is written over it
    (every 32-row tile is read completely before it is written), which keeps a layer's working set at two
    ``(N, B, 64)`` tensors instead of three.  ``z_out`` (training): an ``input``-shaped fp32 tensor that receives the Linear's
    output before LayerNorm, for the fused backward (``ultra_combine_backward_fused_f32``) to load instead of recompute."""
    if input_boundary is not None:
        # first layer: `input` is the boundary (model.py:116-120), given as (node int32 (B,), value fp32 (B, 64)); the kernel
        # synthesises its rows -- row (v, q) = value[q] where v == node[q], +0 elsewhere -- instead of reading (N, B, 64) zeros
        if input is not None:
            raise RuntimeError("combine_forward: give the layer input either dense or as input_boundary, not both")
        b_node, b_value = input_boundary
        b_value = b_value.contiguous()
        n_query = b_node.shape[0]
        if (update.dim() != 3 or update.shape[1] != n_query or update.shape[-1] != 64 or tuple(weight.shape) != (64, 128)
                or b_node.dtype != torch.int32 or not b_node.is_contiguous() or b_value.shape != (n_query, 64)):
            raise RuntimeError("combine_forward(input_boundary=...): update (N, B, 64), node int32 (B,), value (B, 64)")
        tensors = [update, weight, bias, b_value] + ([ln_weight, ln_bias] if ln_weight is not None else [])
        if _not_fp32_on(update.device, tensors) or b_node.device != update.device:
            raise RuntimeError("combine_forward needs fp32 tensors on one HIP device (no CPU fallback)")
        update = update.contiguous()
        out = update if reuse_update else torch.empty_like(update)
        _launch(update.device, "ultra_combine_forward_boundary_f32", b_node, b_value, n_query, update,
                *_epilogue(weight, bias, ln_weight, ln_bias, ln_eps, relu, shortcut), out, update.numel() // 64, 64)
        return out
    if input.shape != update.shape or input.shape[-1] != 64 or tuple(weight.shape) != (64, 128):
        raise RuntimeError("combine_forward handles 64 -> 64 layers with a (64, 128) weight; got input %s, update %s, "
                           "weight %s" % (tuple(input.shape), tuple(update.shape), tuple(weight.shape)))
    tensors = [input, update, weight, bias] + ([ln_weight, ln_bias] if ln_weight is not None else [])
    if _not_fp32_on(input.device, tensors):
        raise RuntimeError("combine_forward needs fp32 tensors on one HIP device (no CPU fallback)")
    input, update = input.contiguous(), update.contiguous()
    out = update if reuse_update else torch.empty_like(input)
    rows = input.numel() // 64
    if z_out is not None and (z_out.shape != input.shape or z_out.dtype != torch.float32 or not z_out.is_contiguous()
                              or z_out.device != input.device):
        raise RuntimeError("combine_forward: z_out must be a contiguous fp32 tensor of the input's shape on its device")
    _launch(input.device, "ultra_combine_forward_f32", input, update,
            *_epilogue(weight, bias, ln_weight, ln_bias, ln_eps, relu, shortcut), out, z_out, rows, 64)
    return out


def linear_supported(in_dim, out_dim):
    """Shapes ``libultra_rspmm`` computes in its documented order: the relation projection and the score head."""
    return (in_dim, out_dim) in ((64, 64), (128, 128)) or (out_dim == 1 and in_dim % 4 == 0)


def linear_forward(input, weight, bias, relu=False):
    """``relu?(F.linear(input, weight, bias))`` (forward only) in the library's documented summation order: the
    small dense layers of ``ultra/layer.py:228,318-319`` and ``ultra/model.py:53,193``."""
    out_dim, in_dim = weight.shape
    if not linear_supported(in_dim, out_dim) or input.shape[-1] != in_dim or bias is None:
        raise RuntimeError("linear_forward: unsupported shape %s x %s" % (tuple(input.shape), tuple(weight.shape)))
    if _not_fp32_on(input.device, (input, weight, bias)):
        raise RuntimeError("linear_forward needs fp32 tensors on one HIP device (no CPU fallback)")
    x = input.contiguous()
    rows = x.numel() // in_dim
    out = torch.empty(tuple(input.shape[:-1]) + (out_dim,), dtype=torch.float32, device=input.device)
    _launch(input.device, "ultra_linear_forward_f32", x, weight.contiguous(), bias.contiguous(), out, rows, in_dim, out_dim,
            int(bool(relu)))
    return out


def _score_all_launch(hidden, query, w1, b1, w2, b2):
    """The one launch of :func:`score_all_entities` on contiguous fp32 device tensors."""
    n_node, batch, _ = hidden.shape
    out = torch.empty(batch, n_node, dtype=torch.float32, device=hidden.device)
    query_bias = torch.empty(batch, 128, dtype=torch.float32, device=hidden.device)     # the queries' share of layer 1
    _launch(hidden.device, "ultra_score_forward_f32", hidden, query, w1, b1, w2, b2, query_bias, out, n_node, batch)
    return out


def score_all_backward(hidden, query, w1, b1, w2, grad, want=(True,) * 6):
    """``ultra_score_backward_f32``: the gradients ``(d_hidden, d_query, d_w1, d_b1, d_w2, d_b2)`` of
    :func:`score_all_entities` for ``grad`` fp32 ``(B, N)`` (its rows may be strided), recomputing the pre-activations from
    ``hidden`` and ``query``; ``want[i]`` false: output ``i`` is skipped and returned as ``None``.  Deterministic."""
    n_node, batch, dim = hidden.shape
    if dim != 64 or tuple(query.shape) != (batch, 64) or tuple(w1.shape) != (128, 128) or w2.numel() != 128 or b1.numel() != 128:
        raise RuntimeError("score_all_backward handles the 64-d model with a 128 -> 128 -> 1 head")
    if tuple(grad.shape) != (batch, n_node) or n_node < 1 or batch < 1:
        raise RuntimeError("score_all_backward: grad must be (%d, %d) with both >= 1, got %s" % (batch, n_node, tuple(grad.shape)))
    if _not_fp32_on(hidden.device, (hidden, query, w1, b1, w2, grad)):
        raise RuntimeError("score_all_backward needs fp32 tensors on one HIP device (no CPU fallback)")
    dev = hidden.device
    hidden, query, w1, b1, w2 = hidden.contiguous(), query.contiguous(), w1.contiguous(), b1.contiguous(), w2.contiguous()
    if (n_node > 1 and grad.stride(1) != 1) or (batch > 1 and grad.stride(0) < n_node):
        grad = grad.contiguous()
    stride = grad.stride(0) if batch > 1 else n_node
    shapes = ((n_node, batch, 64), (batch, 64), (128, 128), (128,), (128,), (1,))
    outs = [torch.empty(shape, dtype=torch.float32, device=dev) if wanted else None for shape, wanted in zip(shapes, want)]
    with torch.cuda.device(dev):
        ws_bytes = int(_lib.load().ultra_score_backward_workspace(n_node, batch))
    if ws_bytes == 0:
        raise RuntimeError("score_all_backward: unsupported shape (N, B) = (%d, %d)" % (n_node, batch))
    workspace = torch.empty(ws_bytes // 4, dtype=torch.float32, device=dev)
    _launch(dev, "ultra_score_backward_f32", hidden, query, w1, b1, w2, grad, stride, *outs, workspace, ws_bytes, n_node, batch)
    return tuple(outs)


class _ScoreAllFunction(torch.autograd.Function):
    """:func:`score_all_entities` under autograd: the forward is inference's launch and keeps nothing but its inputs; the
    backward is ``ultra_score_backward_f32`` (no ``(N * B, 128)`` activation is ever stored)."""

    @staticmethod
    def forward(ctx, hidden, query, w1, b1, w2, b2):
        ctx.w2_shape, ctx.b2_shape = tuple(w2.shape), tuple(b2.shape)
        hidden, query, w1, b1, w2, b2 = (t.contiguous() for t in (hidden, query, w1, b1, w2, b2))
        ctx.save_for_backward(hidden, query, w1, b1, w2)
        return _score_all_launch(hidden, query, w1, b1, w2, b2)

    @staticmethod
    def backward(ctx, grad):
        hidden, query, w1, b1, w2 = ctx.saved_tensors
        outs = score_all_backward(hidden, query, w1, b1, w2, grad, ctx.needs_input_grad)
        d_w2 = None if outs[4] is None else outs[4].view(ctx.w2_shape)
        d_b2 = None if outs[5] is None else outs[5].view(ctx.b2_shape)
        return outs[0], outs[1], outs[2], outs[3], d_w2, d_b2


def score_all_entities(hidden, query, w1, b1, w2, b2):
    """Score head over ALL entities: ``hidden`` ``(N, B, 64)``, ``query`` ``(B, 64)`` ->  ``(B, N)``
    scores ``mlp(cat[hidden, query])`` (``ultra/model.py:134-138,177-193`` with every entity as candidate tail).  With grad
    enabled and an input that requires it the same launch runs as one autograd node (:class:`_ScoreAllFunction`) whose
    backward is ``ultra_score_backward_f32``; without, nothing is recorded."""
    n_node, batch, dim = hidden.shape
    if dim != 64 or tuple(query.shape) != (batch, 64) or tuple(w1.shape) != (128, 128) or w2.numel() != 128:
        raise RuntimeError("score_all_entities handles the 64-d model with a 128 -> 128 -> 1 head")
    tensors = (hidden, query, w1, b1, w2, b2)
    if _not_fp32_on(hidden.device, tensors):
        raise RuntimeError("score_all_entities needs fp32 tensors on one HIP device (no CPU fallback)")
    if torch.is_grad_enabled() and any(t.requires_grad for t in tensors):
        return _ScoreAllFunction.apply(*tensors)
    return _score_all_launch(hidden.contiguous(), query.contiguous(), w1.contiguous(), b1.contiguous(), w2.contiguous(),
                             b2.contiguous())


def _rows_in_place(t):
    """``t`` ``(B, R, 64)`` as the kernels can read it without a copy: rows of 64 contiguous floats at 16-byte-aligned
    strides (the relation stack returns its ``(R, B, 64)`` output transposed, ``ultra/rel_model.py:378``) -- else a
    contiguous copy."""
    if t.stride(2) == 1 and t.stride(0) % 4 == 0 and t.stride(1) % 4 == 0 and t.data_ptr() % 16 == 0:
        return t
    return t.contiguous()


def statistics(values, repeated=None, repeat=0):
    """``(norm, mean, std)`` (``Tensor.norm() / .mean() / .std()``, unbiased) of all elements of ``values`` together with the
    elements of ``repeated`` taken ``repeat`` times, as one fp32 ``(3,)`` tensor -- two launches, double accumulation
    (``ultra_statistics_f32``).  The reference's training metrics ``query_*`` / ``output_*`` (``ultra/model.py:158-160,
    178-181``); ``cat[hidden, query]`` is never built: ``statistics(hidden, query, n_node)``."""
    a = values.detach().contiguous()
    b = None if repeated is None else repeated.detach().contiguous()
    if a.dtype != torch.float32 or not a.is_cuda or (b is not None and (b.dtype != torch.float32 or b.device != a.device)):
        raise RuntimeError("statistics needs fp32 tensors on one HIP device (no CPU fallback)")
    lib = _lib.load()
    out = torch.empty(3, dtype=torch.float32, device=a.device)
    partials = torch.empty(2 * lib.ultra_statistics_blocks(a.numel()), dtype=torch.float64, device=a.device)
    _launch(a.device, "ultra_statistics_f32", a, a.numel(), b, b.numel() if b is not None else 0,
            int(repeat) if b is not None else 0, partials, out)
    return out


class _BCEAdversarial(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, temperature):
        pred = pred.contiguous()
        rows, cols = pred.shape
        loss = torch.empty(rows, dtype=torch.float32, device=pred.device)
        dpred = torch.empty_like(pred)
        _launch(pred.device, "ultra_bce_adversarial_f32", pred, rows, cols, float(temperature), loss, dpred)
        ctx.save_for_backward(dpred)
        return loss

    @staticmethod
    def backward(ctx, grad):
        (dpred,) = ctx.saved_tensors
        return grad.unsqueeze(-1) * dpred, None


def bce_adversarial_loss(pred, temperature):
    """Per-row training loss of ``ultra/task.py:169-180`` for logits ``pred`` ``(B, 1 + K)`` (positive in column 0): binary
    cross entropy with logits, negatives weighted by ``softmax(pred[:, 1:] / temperature)`` (no gradient through the
    weights; ``temperature <= 0``: ``1 / K`` each), weighted mean per row -- forward and gradient in one launch
    (``ultra_bce_adversarial_f32``).  Returns ``(B,)``."""
    if pred.dim() != 2 or pred.dtype != torch.float32 or not pred.is_cuda:
        raise RuntimeError("bce_adversarial_loss needs fp32 (B, 1 + K) logits on a HIP device (no CPU fallback)")
    return _BCEAdversarial.apply(pred, float(temperature))


SCORE_ROWS_MAX_CANDIDATES = 160        # ultra_score_rows_backward_f32 keeps a query's rows in LDS


class _ScoreRows(torch.autograd.Function):
    @staticmethod
    def forward(ctx, hidden, query, t_index, w1, b1, w2, b2):
        hidden, query, t_index = hidden.contiguous(), query.contiguous(), t_index.contiguous()
        w1, b1, w2, b2 = w1.contiguous(), b1.contiguous(), w2.contiguous(), b2.contiguous()
        n_batch, per_row = t_index.shape
        dev = hidden.device
        h = torch.empty(n_batch * per_row, 128, dtype=torch.float32, device=dev)
        in_rows = torch.empty(n_batch * per_row, 128, dtype=torch.float32, device=dev)
        score = torch.empty(n_batch, per_row, dtype=torch.float32, device=dev)
        _launch(dev, "ultra_score_rows_forward_f32", hidden, query, t_index, w1, b1, w2, b2, h, in_rows, score, n_batch, per_row)
        # the backward never reads `hidden` (its rows are in `in_rows`): only the shape is kept, so the step's largest
        # activation is not held alive until the score head's backward
        ctx.hidden_shape = tuple(hidden.shape)
        ctx.save_for_backward(query, t_index, w1, w2, h, in_rows)
        return score

    @staticmethod
    def backward(ctx, grad):
        query, t_index, w1, w2, h, in_rows = ctx.saved_tensors
        n_batch, per_row = t_index.shape
        dev = query.device
        grad = grad.contiguous()
        d_pre = torch.empty_like(h)
        partial = torch.empty(16 * 129 * 129, dtype=torch.float32, device=dev)
        d_hidden = torch.empty(ctx.hidden_shape, dtype=torch.float32, device=dev)
        d_query = torch.empty_like(query)
        d_w1 = torch.empty(128, 128, dtype=torch.float32, device=dev)
        d_b1 = torch.empty(128, dtype=torch.float32, device=dev)
        d_w2 = torch.empty(128, dtype=torch.float32, device=dev)
        d_b2 = torch.empty(1, dtype=torch.float32, device=dev)
        _launch(dev, "ultra_score_rows_backward_f32", None, query, t_index, w1, w2, h, in_rows, grad, d_pre, partial, d_hidden,
                d_query, d_w1, d_b1, d_w2, d_b2, ctx.hidden_shape[0], n_batch, per_row)
        return d_hidden, d_query, None, d_w1, d_b1, d_w2.view(1, 128), d_b2


def score_candidates_supported(hidden, query, t_index, w1, w2):
    """Shapes :func:`score_candidates` covers: the 64-d model with the 128 -> 128 -> 1 head, at most 160 candidates per query."""
    return (hidden.is_cuda and hidden.dtype == torch.float32 and hidden.dim() == 3 and hidden.shape[-1] == 64
            and tuple(query.shape) == (hidden.shape[1], 64) and query.dtype == torch.float32 and t_index.dtype == torch.int64
            and t_index.dim() == 2 and t_index.shape[0] == hidden.shape[1] and 0 < t_index.shape[1] <= SCORE_ROWS_MAX_CANDIDATES
            and tuple(w1.shape) == (128, 128) and w2.numel() == 128)


def score_candidates(hidden, query, t_index, w1, b1, w2, b2):
    """Scores ``(B, K)`` of the candidate tails of a training step: ``mlp(cat[hidden[t_index, arange(B)], query])`` with the
    shipped 128 -> 128 (relu) -> 1 head (``ultra/model.py:177-183,193``), differentiable in ``hidden``, ``query`` and the four
    parameters -- one forward launch, three backward launches (``ultra_score_rows_*``) instead of an index, a cat, two BLAS
    products and the ~50 launches of their backward.  ``hidden`` ``(N, B, 64)``, ``query`` ``(B, 64)``, ``t_index`` int64 ``(B, K)``."""
    if not score_candidates_supported(hidden, query, t_index, w1, w2):
        raise RuntimeError("score_candidates: (N, B, 64) / (B, 64) fp32 on a HIP device, int64 (B, K <= 160) candidates, "
                           "a 128 -> 128 -> 1 head")
    return _ScoreRows.apply(hidden, query, t_index, w1, b1, w2, b2)


def relation_graph_blocks(edge_list, n_node, n_rel):
    """The four blocks of ``construct_relation_graph`` (/root/reference/ultra/rel_model.py:99-143) for a graph WITH inverse
    edges on the device: bool ``(4, n_rel, n_rel)``, ``[type, r1, r2]`` True iff some entity is the head / tail of an ``r1``
    edge and the head / tail of an ``r2`` edge (type 0 hh, 1 tt, 2 ht, 3 th) -- the index pattern of the reference's four sparse
    incidence products, from ``ultra_relation_graph_marks`` (one wave per entity) instead of four spgemm calls over 2R rows of
    ~E / 2R entries each (117 s on S-stress; this: two key sorts + one launch).  One-off preprocessing: allocates and reads
    the host once (the list lengths)."""
    if not edge_list.is_cuda or edge_list.dtype != torch.int64 or edge_list.dim() != 2 or edge_list.shape[1] != 3:
        raise RuntimeError("relation_graph_blocks: edge_list must be int64 (E, 3) on the HIP device")
    n_node, n_rel = int(n_node), int(n_rel)
    dev = edge_list.device
    lists = []
    nodes = torch.arange(n_node + 1, device=dev) * n_rel
    for col in (0, 1):
        key = torch.unique(edge_list[:, col] * n_rel + edge_list[:, 2])          # sorted DISTINCT (entity, relation) pairs
        if key.numel() >= 2 ** 31:
            raise RuntimeError("relation_graph_blocks: more than 2^31 (entity, relation) pairs")
        ptr = torch.searchsorted(key, nodes).to(torch.int32)
        rel = (key % n_rel).to(torch.int32)
        lists += [ptr, rel]
    marks = torch.empty(4, n_rel, n_rel, dtype=torch.uint8, device=dev)
    _launch(dev, "ultra_relation_graph_marks", *lists, n_node, n_rel, marks)
    return marks.bool()


def relation_stack_inputs(weights, h_index):
    """Inputs of the relation stack's first layer in one launch (``ultra_relation_stack_inputs``): ``weights``: the layers'
    relation embeddings, each fp32 ``(R4, 64)``; ``h_index`` int64 ``(Q,)``.  Returns ``(tables (L, R4, Q * 64), ones (Q, 64),
    node32 int32 (Q,))`` -- ``stack(weights).unsqueeze(2).expand(-1, -1, Q, -1).reshape(L, R4, Q * 64)``, ``torch.ones(Q, 64)``
    and ``h_index.to(int32)`` (``ultra/rel_model.py:351-378``, ``ultra/layer.py:143-151``)."""
    n = len(weights)
    keep = [w.detach().contiguous() for w in weights]
    if (n == 0 or n > 8 or h_index.dtype != torch.int64 or h_index.dim() != 1 or not h_index.is_cuda
            or any(w.dtype != torch.float32 or w.dim() != 2 or w.shape != keep[0].shape or w.shape[1] != 64 or w.device != h_index.device
                   for w in keep)):
        raise RuntimeError("relation_stack_inputs: 1..8 fp32 (R, 64) tables and int64 (Q,) indices on one HIP device")
    n_rel, n_query, dev = keep[0].shape[0], h_index.shape[0], h_index.device
    tables = torch.empty(n, n_rel, n_query * 64, dtype=torch.float32, device=dev)
    ones = torch.empty(n_query, 64, dtype=torch.float32, device=dev)
    node32 = torch.empty(n_query, dtype=torch.int32, device=dev)
    if n_query:
        _launch(dev, "ultra_relation_stack_inputs", _pointer_array(keep), n, n_rel, n_query, h_index, h_index.stride(0), tables,
                ones, node32)
    return tables, ones, node32


def relation_project(relation, weights, repeat=1):
    """All layers' relation projections in one launch.  ``relation``: fp32 ``(B, R, 64)``; ``weights``: one
    ``(w1, b1, w2, b2)`` per layer (``nn.Linear`` weights ``(64, 64)`` / biases ``(64,)`` of the 2-layer
    ``relation_projection`` MLP, ``ultra/layer.py:228,318-319``).  Returns one ``(R, B * 64)`` table per layer
    -- ``relation_projection(relation).transpose(0, 1).flatten(1)`` (``layer.py:325-326``), bit for bit.
    ``repeat``: the tables of ``torch.cat([relation] * repeat)`` -- ``(R, repeat * B * 64)``, query block ``b + j B`` a copy of
    block ``b`` -- computed once (full-batch evaluation: tail and head queries share the relation representations)."""
    if relation.dim() != 3 or relation.shape[-1] != 64 or relation.dtype != torch.float32 or not relation.is_cuda:
        raise RuntimeError("relation_project: fp32 (B, R, 64) on a HIP device, got %s" % (tuple(relation.shape),))
    relation = _rows_in_place(relation)
    batch, n_rel, _ = relation.shape
    n = len(weights)
    cols = [[], [], [], []]
    for layer_weights in weights:
        for k, t in enumerate(layer_weights):
            t = t.detach().contiguous()
            if t.dtype != torch.float32 or t.device != relation.device or t.shape != ((64, 64) if k % 2 == 0 else (64,)):
                raise RuntimeError("relation_project: 64 -> 64 -> 64 fp32 projections only")
            cols[k].append(t)
    repeat = int(repeat)
    outs = [torch.empty(n_rel, repeat * batch * 64, dtype=torch.float32, device=relation.device) for _ in range(n)]
    if n == 0 or relation.numel() == 0:
        return outs
    _launch(relation.device, "ultra_relation_project_f32", relation, relation.stride(0), relation.stride(1),
            *[_pointer_array(col) for col in cols], _pointer_array(outs), n, batch, repeat, n_rel, 64)
    return outs


class _ProjectFunction(torch.autograd.Function):
    """All layers' relation projections as ONE autograd node: forward = :func:`relation_project` (one launch, the
    documented order, the tables inference uses), backward = ``ultra_relation_project_backward_f32`` (one launch + a
    small reduction) instead of autograd through 2 L ``nn.Linear`` + relu + transposes (~100 launches of a few
    microseconds per fine-tuning step)."""

    @staticmethod
    def forward(ctx, relation, *flat_weights):
        weights = [tuple(flat_weights[4 * l:4 * l + 4]) for l in range(len(flat_weights) // 4)]
        ctx.save_for_backward(relation, *flat_weights)
        tables = relation_project(relation, weights)
        return tuple(tables)

    @staticmethod
    def backward(ctx, *grads):
        relation, *flat_weights = ctx.saved_tensors
        relation = relation.contiguous()
        n = len(flat_weights) // 4
        batch, n_rel, _ = relation.shape
        dev = relation.device
        keep = [None if g is None else g.contiguous() for g in grads]
        w = [t.detach().contiguous() for t in flat_weights]
        d_w = [torch.empty_like(t) for t in w]
        d_layers = torch.empty(n, batch * n_rel, 64, dtype=torch.float32, device=dev)
        lib = _lib.load()
        blocks = ctypes.c_int64(0)
        _lib.check(lib.ultra_relation_project_backward_blocks(dev.index or 0, batch, n_rel, n, ctypes.byref(blocks)))
        ws = torch.empty(n * blocks.value * (2 * 64 * 64 + 128), dtype=torch.float32, device=dev)
        _launch(dev, "ultra_relation_project_backward_f32", relation, _pointer_array(w[0::4]), _pointer_array(w[1::4]),
                _pointer_array(w[2::4]), _pointer_array(keep), d_layers, _pointer_array(d_w[0::4]), _pointer_array(d_w[1::4]),
                _pointer_array(d_w[2::4]), _pointer_array(d_w[3::4]), ws, ws.numel() * 4, n, batch, n_rel, 64)
        d_relation = d_layers.sum(0).view(batch, n_rel, 64) if ctx.needs_input_grad[0] else None
        return (d_relation, *[g if need else None for g, need in zip(d_w, ctx.needs_input_grad[1:])])


def relation_project_train(relation, weights):
    """:func:`relation_project` with gradients (``relation`` and the four parameters of every layer): the training form
    of the grouped projections.  At most 8 layers per call (the kernels' parameter block)."""
    if len(weights) > 8:
        raise RuntimeError("relation_project_train: at most 8 layers per call")
    flat = [t for layer_weights in weights for t in layer_weights]
    return list(_ProjectFunction.apply(relation, *flat))


# Per-query relation tables of a NeuralBellmanFordNetwork (csrc/query_tables.hip): ULTRA_QUERY_TABLES=0
# sends every layer through its own nn.Linear + transposing copy again (A/B timing; the same definition, ATen's rounding).
QUERY_TABLES = _env_bool("ULTRA_QUERY_TABLES", True)
QUERY_TABLES_MAX_LAYERS = 8


def dense_query_tables(query, weights, biases, n_rel):
    """:func:`query_tables` in torch ops, in the dtype of ``query`` (the host twin and the fp64 definition): per layer
    ``F.linear(query, w, b).view(B, n_rel, D).transpose(0, 1)`` (``ultra/layer.py:58-61``) as an ``(n_rel, B * D)`` table."""
    batch = query.shape[0]
    return [torch.nn.functional.linear(query, w, b).view(batch, n_rel, -1).transpose(0, 1).reshape(n_rel, -1)
            for w, b in zip(weights, biases)]


def _query_table_arguments(what, query, weights, biases, n_rel):
    """Checks of :func:`query_tables_forward` / :func:`query_tables_backward`; returns ``(query, weights, biases, dims)`` with
    the query's rows dense (a column view keeps its row stride) and the parameters contiguous."""
    n_rel = int(n_rel)
    if query.dim() != 2 or query.shape[1] < 1 or query.dtype != torch.float32 or not query.is_cuda or n_rel < 0:
        raise RuntimeError("%s: query must be fp32 (B, K >= 1) on a HIP device, got %s" % (what, tuple(query.shape)))
    if not 1 <= len(weights) <= QUERY_TABLES_MAX_LAYERS or (biases is not None and len(biases) != len(weights)):
        raise RuntimeError("%s: 1 to %d layers with one bias each, got %d" % (what, QUERY_TABLES_MAX_LAYERS, len(weights)))
    if query.stride(1) != 1 or (query.shape[0] > 1 and query.stride(0) < query.shape[1]):
        query = query.contiguous()
    K = query.shape[1]
    dims, keep_w, keep_b = [], [], []
    for l, w in enumerate(weights):
        if w.dim() != 2 or w.shape[1] != K or w.dtype != torch.float32 or w.device != query.device \
                or (n_rel and (w.shape[0] % n_rel or not w.shape[0])) or (not n_rel and w.shape[0] < 1):
            raise RuntimeError("%s: weight %d must be fp32 (n_rel * D, %d) on %s, got %s" % (what, l, K, query.device, tuple(w.shape)))
        dims.append(w.shape[0] // n_rel if n_rel else w.shape[0])
        keep_w.append(w.detach().contiguous())
        if biases is not None:
            b = biases[l]
            if b.dtype != torch.float32 or b.device != query.device or tuple(b.shape) != (w.shape[0],):
                raise RuntimeError("%s: bias %d must be fp32 (%d,) on %s" % (what, l, w.shape[0], query.device))
            keep_b.append(b.detach().contiguous())
    return query, keep_w, keep_b, dims


def _row_stride(query):
    return query.stride(0) if query.shape[0] > 1 else query.shape[1]


def query_tables_forward(query, weights, biases, n_rel):
    """The tables of :func:`query_tables` without autograd: one launch of ``ultra_query_tables_f32`` for all layers."""
    query, w, b, dims = _query_table_arguments("query_tables", query.detach(), weights, biases, n_rel)
    n_rel, batch, K = int(n_rel), query.shape[0], query.shape[1]
    if _torch_ext.binding() == "torch":
        return list(_torch_ext.load().query_tables(query, w, b, n_rel))
    outs = [torch.empty(n_rel, batch * d, dtype=torch.float32, device=query.device) for d in dims]
    if batch and n_rel:
        _launch(query.device, "ultra_query_tables_f32", query, _row_stride(query), _pointer_array(w), _pointer_array(b),
                _pointer_array(outs), (ctypes.c_int64 * len(dims))(*dims), len(dims), batch, n_rel, K)
    return outs


def query_tables_backward(query, weights, grads, n_rel):
    """``(d_weights, d_biases, d_query)`` of :func:`query_tables` for the table gradients ``grads`` (``(n_rel, B * D_l)`` each,
    ``None`` = zeros): ONE call of ``ultra_query_tables_backward_f32``, deterministic (no atomics; the partial sums of
    ``d_query`` are added in ascending block order)."""
    query, w, _, dims = _query_table_arguments("query_tables_backward", query.detach(), weights, None, n_rel)
    n_rel, batch, K = int(n_rel), query.shape[0], query.shape[1]
    if len(grads) != len(w):
        raise RuntimeError("query_tables_backward: %d gradients for %d layers" % (len(grads), len(w)))
    keep = []
    for l, g in enumerate(grads):
        if g is not None:
            if g.dtype != torch.float32 or g.device != query.device or g.numel() != n_rel * batch * dims[l]:
                raise RuntimeError("query_tables_backward: gradient %d must be fp32 with %d x %d x %d entries on %s"
                                   % (l, n_rel, batch, dims[l], query.device))
            g = g.detach().contiguous()
        keep.append(g)
    if _torch_ext.binding() == "torch":
        out = list(_torch_ext.load().query_tables_backward(query, w, keep, n_rel))
        return out[:len(w)], out[len(w):2 * len(w)], out[-1]
    dev = query.device
    d_w = [torch.empty_like(t) for t in w]
    d_b = [torch.empty(t.shape[0], dtype=torch.float32, device=dev) for t in w]
    d_query = torch.empty(batch, K, dtype=torch.float32, device=dev)
    if not (batch and n_rel):
        for t in d_w + d_b:
            t.zero_()
        return d_w, d_b, d_query
    c_dims = (ctypes.c_int64 * len(dims))(*dims)
    need = int(_lib.load().ultra_query_tables_backward_workspace(len(dims), batch, n_rel, c_dims, K))
    ws = torch.empty(max(need, 4) // 4, dtype=torch.float32, device=dev)
    _launch(dev, "ultra_query_tables_backward_f32", query, _row_stride(query), _pointer_array(w), _pointer_array(keep),
            _pointer_array(d_w), _pointer_array(d_b), d_query, ws, need, c_dims, len(dims), batch, n_rel, K)
    return d_w, d_b, d_query


class _QueryTablesFunction(torch.autograd.Function):
    """All layers' per-query relation tables as ONE autograd node: forward = ``ultra_query_tables_f32``, backward =
    ``ultra_query_tables_backward_f32`` (one call for the gradients of every weight, every bias and the query)."""

    @staticmethod
    def forward(ctx, n_rel, query, *flat):
        n = len(flat) // 2
        ctx.n_rel = n_rel
        # a table nothing reads arrives in backward as None, not as a tensor of zeros: the C entry takes NULL for it and skips
        # that layer's d_query blocks
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(query, *flat[:n])
        return tuple(query_tables_forward(query, flat[:n], flat[n:], n_rel))

    @staticmethod
    def backward(ctx, *grads):
        query, *weights = ctx.saved_tensors
        d_w, d_b, d_query = query_tables_backward(query, weights, list(grads), ctx.n_rel)
        n = len(weights)
        need = ctx.needs_input_grad
        return (None, d_query if need[1] else None,
                *[g if need[2 + i] else None for i, g in enumerate(d_w)],
                *[g if need[2 + n + i] else None for i, g in enumerate(d_b)])


def query_tables(query, weights, biases, n_rel):
    """The relation tables of every ``dependent`` layer of a :class:`NeuralBellmanFordNetwork` from ONE launch: ``query`` fp32
    ``(B, K)`` (the query relations' embeddings), ``weights[l]`` ``(n_rel * D_l, K)`` and ``biases[l]`` ``(n_rel * D_l,)`` (the
    layers' ``relation_linear``).  Returns one ``(n_rel, B * D_l)`` table per layer -- ``relation_linear(query).view(B, n_rel,
    D_l).transpose(0, 1).flatten(1)`` (``ultra/layer.py:58-61``) in the summation order ``include/ultra_rspmm.h`` documents -- as
    one autograd node whose backward is one call too.  At most 8 layers.  CPU tensors and tensors that are not fp32 take
    :func:`dense_query_tables`, the same definition in torch ops."""
    tensors = [query] + list(weights) + list(biases)
    if not query.is_cuda or any(t.dtype != torch.float32 or t.device != query.device for t in tensors):
        return dense_query_tables(query, weights, biases, n_rel)
    if torch.is_grad_enabled() and any(t.requires_grad for t in tensors):
        return list(_QueryTablesFunction.apply(int(n_rel), query, *weights, *biases))
    return query_tables_forward(query, weights, biases, n_rel)


def prepare_queries(batch, rel_rep, n_base_rel):
    """The 2B tail-form queries of one full-batch evaluation step in ONE launch (``ultra_prepare_queries``): ``batch`` int64
    ``(B, 3)`` rows of (h, t, r); ``rel_rep`` fp32 ``(B, 2 R, 64)`` (the relation stack's output for the batch's relations).
    Returns ``(anchor int64 (2B,), anchor32 int32 (2B,), relation int64 (2B,), query fp32 (2B, 64))`` -- what
    ``cat([h, t])``, ``cat([r, r + R])`` and ``cat([rel_rep, rel_rep])[arange(2B), relation]`` give (task.py:249-259,
    model.py:76-83,101-105), nine index kernels of a few microseconds each otherwise."""
    batch = batch.contiguous()
    n_batch = batch.shape[0]
    if (batch.dtype != torch.int64 or batch.dim() != 2 or batch.shape[1] != 3 or not batch.is_cuda or rel_rep.dtype != torch.float32
            or rel_rep.dim() != 3 or rel_rep.shape[0] != n_batch or rel_rep.shape[2] != 64 or rel_rep.device != batch.device
            or 2 * int(n_base_rel) != rel_rep.shape[1]):
        raise RuntimeError("prepare_queries: batch int64 (B, 3) and rel_rep fp32 (B, 2 * n_base_rel, 64) on one HIP device")
    rel_rep = _rows_in_place(rel_rep)
    dev = batch.device
    anchor = torch.empty(2 * n_batch, dtype=torch.int64, device=dev)
    anchor32 = torch.empty(2 * n_batch, dtype=torch.int32, device=dev)
    relation = torch.empty(2 * n_batch, dtype=torch.int64, device=dev)
    query = torch.empty(2 * n_batch, 64, dtype=torch.float32, device=dev)
    if n_batch:
        _launch(dev, "ultra_prepare_queries", batch, rel_rep, rel_rep.stride(0), rel_rep.stride(1), n_batch, rel_rep.shape[1],
                int(n_base_rel), anchor, anchor32, relation, query)
    return anchor, anchor32, relation, query


def filtered_rank(pred, target, filt_ptr=None, filt_node=None):
    """``sum((pos_pred <= pred) & mask, -1) + 1`` (``ultra/task.py:307-315``) with the mask given as per-row lists of
    DISTINCT filtered candidates (``filt_ptr`` int32 ``(rows + 1,)``, ``filt_node`` int32) -- no dense ``(B, N)``
    boolean.  ``pred``: fp32 ``(rows, N)``; ``target``: int64 ``(rows,)``; returns int64 ``(rows,)``."""
    pred = pred.contiguous()
    rows, n_cand = pred.shape
    target = target.contiguous()
    if target.dtype != torch.int64 or target.shape != (rows,) or pred.dtype != torch.float32:
        raise RuntimeError("filtered_rank: pred fp32 (rows, N), target int64 (rows,)")
    if filt_ptr is not None and (filt_ptr.dtype != torch.int32 or filt_node.dtype != torch.int32
                                 or filt_ptr.shape != (rows + 1,) or not filt_ptr.is_contiguous()
                                 or not filt_node.is_contiguous()):
        raise RuntimeError("filtered_rank: filter lists must be int32 (rows + 1,) / int32 (n,)")
    rank = torch.empty(rows, dtype=torch.int64, device=pred.device)
    if rows == 0:
        return rank
    _launch(pred.device, "ultra_filtered_rank", pred, rows, n_cand, n_cand, target, filt_ptr,
            filt_node if filt_ptr is not None else None, rank)
    return rank


def remove_triples(graph, h, t, r, n_base_rel):
    """``graph`` (with inverse edges) minus the edges ``(h, t, r)`` / ``(t, h, r + n_base_rel)``, as zero weights on its
    cached plans: ``remove_easy_edges`` (``ultra/model.py:57-74``) for summed messages, natively and capturable."""
    if not graph.edge_list.is_cuda:
        # host graphs: the same zero weights from sorted triple keys (no device plans to patch)
        n, rels = graph.num_node, graph.num_relation
        h, t, r = h.reshape(-1), t.reshape(-1), r.reshape(-1)
        gone = torch.cat([(h * n + t) * rels + r, (t * n + h) * rels + r + n_base_rel])
        e = graph.edge_list
        keep = ~torch.isin((e[:, 0] * n + e[:, 1]) * rels + e[:, 2], gone)
        return graph.reweighted(graph.edge_weight * keep)
    return graph.without_triples(h, t, r, n_base_rel)


def remove_pairs(graph, h, t):
    """``graph`` (with inverse edges) minus EVERY edge between ``h[i]`` and ``t[i]`` -- either direction, any relation --, as zero
    weights on its cached plans: ``remove_easy_edges`` with ``remove_one_hop=True`` (``ultra/model.py:57-74``) for summed
    messages, natively and capturable (``ultra_pair_removal``).  Ids outside ``[0, num_node)`` match nothing."""
    if not graph.edge_list.is_cuda:
        # host graphs: the same zero weights from sorted pair keys (no device plans to patch)
        n = graph.num_node
        h, t = h.reshape(-1), t.reshape(-1)
        ok = (h >= 0) & (h < n) & (t >= 0) & (t < n)
        h, t = h[ok], t[ok]
        gone = torch.cat([h * n + t, t * n + h])
        e = graph.edge_list
        keep = ~torch.isin(e[:, 0] * n + e[:, 1], gone)
        return graph.reweighted(graph.edge_weight * keep)
    return graph.without_pairs(h, t)


def filtered_rank_keys(pred, target, keys, anchor, rel, n_rel, n_node=None):
    """Filtered ranks of one prediction side without filter lists or masks: ``pred`` fp32 ``(B, N)`` (a strided view of
    the ``(B, 2, N)`` scores is fine), ``target`` / ``anchor`` / ``rel`` int64 ``(B,)``; ``keys``: the graph's sorted
    distinct completion keys of that side (``Graph.completion_keys``) or ``None`` for the unfiltered rank.  Returns
    int64 ``(B,)``.  No host synchronisation (capturable).  ``n_node``: the node count the keys were built with; a
    mismatch with ``pred.shape[1]`` raises (the kernel decodes keys with the candidate count as stride)."""
    rows, n_cand = pred.shape
    if pred.dtype != torch.float32 or pred.stride(1) != 1 or not pred.is_cuda:
        raise RuntimeError("filtered_rank_keys: pred must be fp32 (B, N) with contiguous rows on the HIP device")
    if n_node is not None and int(n_node) != n_cand:
        # the keys were built as (anchor * n_rel + rel) * n_node + other: decoded with another stride the filter reads
        # other candidates' scores (or past the row) without any error
        raise RuntimeError("filtered_rank_keys: the scores list %d candidates but the completion keys were built over "
                           "%d nodes (filter graph and fact graph must share the entity set)" % (n_cand, int(n_node)))
    for name, t in (("target", target), ("anchor", anchor), ("rel", rel)):
        if t.dtype != torch.int64 or t.shape != (rows,) or t.device != pred.device:
            raise RuntimeError("filtered_rank_keys: %s must be int64 (%d,) on %s" % (name, rows, pred.device))
    if keys is not None and (keys.dtype != torch.int64 or keys.dim() != 1 or not keys.is_contiguous()
                             or keys.device != pred.device):
        raise RuntimeError("filtered_rank_keys: keys must be a contiguous int64 vector on %s" % pred.device)
    rank = torch.empty(rows, dtype=torch.int64, device=pred.device)
    if rows == 0:
        return rank
    anchor, rel = anchor.contiguous(), rel.contiguous()
    _launch(pred.device, "ultra_filtered_rank_keys", pred, rows, n_cand, pred.stride(0), target, target.stride(0), keys,
            keys.numel() if keys is not None else 0, anchor, rel, 1, int(n_rel), rank, 1)
    return rank


def strict_negatives(keys, anchor, rel, n_rel, n_node, rand):
    """Strict negative sampling (``ultra/task.py:102-118``) from the graph's sorted completion keys: for every row
    ``q`` and uniform number ``rand[q, s]`` the ``floor(rand * n_free)``-th entity that does NOT complete
    ``(anchor[q], rel[q], ?)`` -- the entity ``variadic_sample(mask.nonzero()[:, 1], mask.sum(-1), S)`` returns for the
    same numbers, with no ``(B, N)`` mask and no host synchronisation.  Returns int64 ``(B, S)``."""
    rows, n_sample = rand.shape
    if rand.dtype != torch.float32 or not rand.is_cuda or not rand.is_contiguous():
        raise RuntimeError("strict_negatives: rand must be contiguous fp32 (B, S) on the HIP device")
    anchor, rel = anchor.contiguous(), rel.contiguous()
    for name, t in (("anchor", anchor), ("rel", rel)):
        if t.dtype != torch.int64 or t.shape != (rows,) or t.device != rand.device:
            raise RuntimeError("strict_negatives: %s must be int64 (%d,) on %s" % (name, rows, rand.device))
    if keys.dtype != torch.int64 or keys.dim() != 1 or not keys.is_contiguous() or keys.device != rand.device:
        raise RuntimeError("strict_negatives: keys must be a contiguous int64 vector on %s" % rand.device)
    out = torch.empty(rows, n_sample, dtype=torch.int64, device=rand.device)
    if out.numel() == 0:
        return out
    _launch(rand.device, "ultra_strict_negative", keys, keys.numel(), anchor, rel, rows, int(n_rel), int(n_node), rand, n_sample,
            out)
    return out


def _index_pair(name, anchor, rel, rows, device):
    """``anchor`` / ``rel`` int64 ``(rows,)`` on ``device`` and the element stride both are read with: views that share a
    stride (the columns of a ``(B, 3)`` batch) go to the kernel as they are, anything else as contiguous copies."""
    for what, t in (("anchor", anchor), ("rel", rel)):
        if t.dtype != torch.int64 or t.shape != (rows,) or t.device != device:
            raise RuntimeError("%s: %s must be int64 (%d,) on %s" % (name, what, rows, device))
    if rows > 1 and (anchor.stride(0) != rel.stride(0) or anchor.stride(0) < 1):
        anchor, rel = anchor.contiguous(), rel.contiguous()
    return anchor, rel, (anchor.stride(0) if rows > 1 else 1)


def filter_counts(keys, anchor, rel, n_rel, n_node):
    """``mask.sum(-1)`` of the filter mask (``ultra/task.py:65-100``) without the mask: per query the number of entities
    that do NOT complete ``(anchor[q], rel[q], ?)`` in the graph whose sorted distinct completion keys ``keys`` are
    (``None``: unfiltered ranking, every count is ``n_node``) -- the denominator of the sampled metrics ``hits@K_N``
    (``ultra/task.py:498``).  ``anchor`` / ``rel``: int64 ``(B,)``, strided views are fine.  Returns int64 ``(B,)``.  No host
    synchronisation."""
    if not anchor.is_cuda:
        raise RuntimeError("filter_counts: anchor must be int64 (B,) on the HIP device")
    rows = anchor.shape[0] if anchor.dim() == 1 else -1
    anchor, rel, stride = _index_pair("filter_counts", anchor, rel, rows, anchor.device)
    if keys is not None and (keys.dtype != torch.int64 or keys.dim() != 1 or not keys.is_contiguous()
                             or keys.device != anchor.device):
        raise RuntimeError("filter_counts: keys must be a contiguous int64 vector on %s" % anchor.device)
    if int(n_node) <= 0 or int(n_rel) <= 0:
        raise RuntimeError("filter_counts: n_rel and n_node must be positive, got %d and %d" % (int(n_rel), int(n_node)))
    out = torch.empty(rows, dtype=torch.int64, device=anchor.device)
    if rows == 0:
        return out
    _launch(anchor.device, "ultra_filter_counts", keys, keys.numel() if keys is not None else 0, anchor, rel, stride, rows,
            int(n_rel), int(n_node), out)
    return out


SAMPLED_RANK_MAX = 64           # draws per query of ultra_sampled_rank_keys (one lane each)


def sampled_rank_keys(pred, target, keys, anchor, rel, n_rel, rand, n_node=None, return_samples=False):
    """The sampled ranking protocol ``toy_eval`` of the reference (``ultra/task.py:474-484``) on one prediction side, from
    the graph's sorted completion keys: per row ``min(S, n_free)`` distinct entities outside the completions of
    ``(anchor[q], rel[q], ?)`` are drawn without replacement -- the draw is DEFINED by the uniform numbers ``rand`` fp32
    ``(B, S)``, ``S <= 64`` (``include/ultra_rspmm.h``; ``task.sampled_free_ranks`` restates it) -- and the positive is ranked
    among their scores.  ``pred`` / ``target`` / ``keys`` / ``anchor`` / ``rel`` / ``n_node`` as in
    :func:`filtered_rank_keys`.  Returns ``(optimistic, pessimistic)`` int64 ``(B,)`` = ``#{pos < neg}``, ``#{pos <= neg}``,
    and with ``return_samples`` also the drawn entities int64 ``(B, S)`` in draw order (``-1`` in unused slots)."""
    if pred.dim() != 2 or pred.dtype != torch.float32 or pred.stride(1) != 1 or not pred.is_cuda:
        raise RuntimeError("sampled_rank_keys: pred must be fp32 (B, N) with contiguous rows on the HIP device")
    rows, n_cand = pred.shape
    if n_node is not None and int(n_node) != n_cand:
        raise RuntimeError("sampled_rank_keys: the scores list %d candidates but the completion keys were built over "
                           "%d nodes (filter graph and fact graph must share the entity set)" % (n_cand, int(n_node)))
    if target.dtype != torch.int64 or target.shape != (rows,) or target.device != pred.device:
        raise RuntimeError("sampled_rank_keys: target must be int64 (%d,) on %s" % (rows, pred.device))
    anchor, rel, stride = _index_pair("sampled_rank_keys", anchor, rel, rows, pred.device)
    if keys is not None and (keys.dtype != torch.int64 or keys.dim() != 1 or not keys.is_contiguous()
                             or keys.device != pred.device):
        raise RuntimeError("sampled_rank_keys: keys must be a contiguous int64 vector on %s" % pred.device)
    if rand.dim() != 2 or rand.shape[0] != rows or rand.dtype != torch.float32 or rand.device != pred.device:
        raise RuntimeError("sampled_rank_keys: rand must be fp32 (%d, S) on %s" % (rows, pred.device))
    n_sample = rand.shape[1]
    if not 1 <= n_sample <= SAMPLED_RANK_MAX:
        raise RuntimeError("sampled_rank_keys: 1 to %d samples per query, got %d" % (SAMPLED_RANK_MAX, n_sample))
    if rows and pred.stride(0) < n_cand:
        raise RuntimeError("sampled_rank_keys: the rows of pred overlap")
    rand = rand.contiguous()
    optimistic = torch.empty(rows, dtype=torch.int64, device=pred.device)
    pessimistic = torch.empty(rows, dtype=torch.int64, device=pred.device)
    samples = torch.empty(rows, n_sample, dtype=torch.int64, device=pred.device) if return_samples else None
    if rows:
        _launch(pred.device, "ultra_sampled_rank_keys", pred, rows, n_cand, pred.stride(0), target, target.stride(0), keys,
                keys.numel() if keys is not None else 0, anchor, rel, stride, int(n_rel), rand, n_sample, optimistic,
                pessimistic, samples)
    return (optimistic, pessimistic, samples) if return_samples else (optimistic, pessimistic)


TOPK_MAX = 128                  # answers per query of ultra_topk_keys


def dense_topk(pred, k, keys, anchor, rel, n_rel):
    """:func:`topk_keys` on host tensors, from a dense mask: the definition of ``include/ultra_rspmm.h`` as a stable descending
    sort (ties and ``-0.0 == +0.0`` keep their ascending index order) with NaN scores moved behind every number and the
    completions behind those."""
    rows, n = pred.shape
    group = torch.isnan(pred).long()                                    # 0 number, 1 NaN, 2 known completion
    if keys is not None and rows:
        base = (anchor * int(n_rel) + rel) * n
        first, last = torch.searchsorted(keys, base), torch.searchsorted(keys, base + n)
        count = last - first
        row = torch.repeat_interleave(torch.arange(rows), count)
        at = torch.arange(int(count.sum())) - torch.repeat_interleave(count.cumsum(0) - count, count) + first[row]
        group[row, keys[at] - base[row]] = 2
    by_score = torch.sort(torch.nan_to_num(pred, nan=0.0, posinf=float("inf"), neginf=-float("inf")), dim=1, descending=True,
                          stable=True).indices
    order = by_score.gather(1, torch.sort(group.gather(1, by_score), dim=1, stable=True).indices)
    if n < k:
        order = torch.cat([order, order.new_zeros(rows, k - n)], dim=1)
    order = order[:, :k]
    listed = torch.arange(k)[None, :] < (group != 2).sum(dim=1, keepdim=True)
    index = torch.where(listed, order, torch.full_like(order, -1))
    value = torch.where(listed, pred.gather(1, order), torch.full((), -float("inf"), dtype=pred.dtype))
    return value, index


def _dense_topk_groups(pred, group, k):
    """The ordering of :func:`dense_topk` on the device of ``pred`` ``(rows, n >= 1)``, from ``group`` int64 ``(rows, n)``: 0 a
    number, 1 a NaN, 2 left out.  Returns ``(value, index)`` of the ``k`` first positions of every row."""
    rows, n = pred.shape
    by_score = torch.sort(torch.nan_to_num(pred, nan=0.0, posinf=float("inf"), neginf=-float("inf")), dim=1, descending=True,
                          stable=True).indices
    order = by_score.gather(1, torch.sort(group.gather(1, by_score), dim=1, stable=True).indices)
    if n < k:
        order = torch.cat([order, torch.zeros(rows, k - n, dtype=order.dtype, device=order.device)], dim=1)
    order = order[:, :k]
    listed = torch.arange(k, device=pred.device)[None, :] < (group != 2).sum(dim=1, keepdim=True)
    index = torch.where(listed, order, torch.full_like(order, -1))
    value = torch.where(listed, pred.gather(1, order), torch.full((), -float("inf"), dtype=pred.dtype, device=pred.device))
    return value, index


def topk_keys(pred, k, keys, anchor, rel, n_rel, n_node=None):
    """The ``k`` best entities of every row of ``pred`` that do not complete ``(anchor[q], rel[q], ?)``, best first
    (``ultra_topk_keys``, the contract is in ``include/ultra_rspmm.h``): scores descending as floats, ``-0.0 == +0.0``, equal
    scores by ascending entity, NaN scores after every number.  ``pred`` / ``keys`` / ``anchor`` / ``rel`` / ``n_node`` as in
    :func:`sampled_rank_keys` (``keys=None``: nothing is filtered); ``1 <= k <= 128``.  Returns ``(value fp32 (B, k), index int64
    (B, k))``; a row with fewer than ``k`` candidates ends in ``index = -1`` / ``value = -inf``.  The filter is looked up in the
    sorted keys inside the kernel -- no ``(B, N)`` mask or masked copy of the scores -- with no host synchronisation; the
    workspace of rows longer than 32768 comes from the caching allocator before the launch.  CPU tensors take a dense path of
    the same definition."""
    if pred.dim() != 2 or pred.dtype != torch.float32 or (pred.shape[1] and pred.stride(1) != 1):
        raise RuntimeError("topk_keys: pred must be fp32 (B, N) with contiguous rows")
    rows, n_cand = pred.shape
    if n_cand < 1:
        raise RuntimeError("topk_keys: pred lists no candidate")
    if n_node is not None and int(n_node) != n_cand:
        raise RuntimeError("topk_keys: the scores list %d candidates but the completion keys were built over "
                           "%d nodes (filter graph and fact graph must share the entity set)" % (n_cand, int(n_node)))
    k = int(k)
    if not 1 <= k <= TOPK_MAX:
        raise RuntimeError("topk_keys: 1 to %d answers per query, got %d" % (TOPK_MAX, k))
    anchor, rel, stride = _index_pair("topk_keys", anchor, rel, rows, pred.device)
    if keys is not None and (keys.dtype != torch.int64 or keys.dim() != 1 or not keys.is_contiguous()
                             or keys.device != pred.device):
        raise RuntimeError("topk_keys: keys must be a contiguous int64 vector on %s" % pred.device)
    if keys is not None and int(n_rel) <= 0:
        raise RuntimeError("topk_keys: n_rel must be positive, got %d" % int(n_rel))
    if rows > 1 and pred.stride(0) < n_cand:
        raise RuntimeError("topk_keys: the rows of pred overlap")
    if not pred.is_cuda:
        return dense_topk(pred, k, keys, anchor, rel, n_rel)
    value = torch.empty(rows, k, dtype=torch.float32, device=pred.device)
    index = torch.empty(rows, k, dtype=torch.int64, device=pred.device)
    if rows:
        ws_bytes = int(_lib.load().ultra_topk_keys_workspace(rows, n_cand, k))
        ws = torch.empty(ws_bytes // 8, dtype=torch.int64, device=pred.device) if ws_bytes else None
        _launch(pred.device, "ultra_topk_keys", pred, rows, n_cand, pred.stride(0) if rows > 1 else n_cand, k, keys,
                keys.numel() if keys is not None else 0, anchor, rel, stride, int(n_rel), value, index, ws, ws_bytes)
    return value, index


# ---------------------------------------------------------------------------------------------------- relation prediction
RELATION_OUTPUTS = ("top_index", "top_value", "rank", "n_free", "known")      # bit i of the operator's `outputs` argument
RelationSelection = collections.namedtuple("RelationSelection", RELATION_OUTPUTS)


def relation_select_limit():
    """``L``: the longest candidate list ``ultra_relation_select_f32`` selects in one pass over LDS (longer lists take its
    multi-pass form)."""
    return int(_lib.load().ultra_relation_select_limit())


def dense_relation_known(cand, keys_head, keys_tail, h, t, n_rel, n_node):
    """bool ``(P, C)``: candidate relation ``cand[j]`` in ``[0, 2 * n_rel)`` is known for the pair ``(h[p], t[p])`` (the
    definition of ``ultra_relation_select_f32`` in torch ops, as a dense mask; ids out of range are never known)."""
    n_rel, n_node = int(n_rel), int(n_node)
    known = torch.zeros(len(h), len(cand), dtype=torch.bool, device=cand.device)
    pair_ok = (h >= 0) & (h < n_node) & (t >= 0) & (t < n_node)
    for keys, first in ((keys_head, 0), (keys_tail, n_rel)):
        if keys is None or keys.numel() == 0:
            continue
        rel = cand - first
        rel_ok = (rel >= 0) & (rel < n_rel)
        want = (h[:, None] * n_rel + rel.clamp(0, n_rel - 1)[None, :]) * n_node + t[:, None]
        at = torch.searchsorted(keys, want).clamp(max=keys.numel() - 1)
        known |= (keys[at] == want) & rel_ok[None, :] & pair_ok[:, None]
    return known


def dense_relation_select(score, cand, keys_head, keys_tail, h, t, target, n_rel, n_node, k):
    """:func:`relation_select` in torch ops from a dense ``(P, C)`` mask -- the twin CPU tensors take, and the definition the
    device kernel is timed against (it runs on any device)."""
    rows, n = score.shape
    dev = score.device
    ids = torch.arange(n, device=dev) if cand is None else cand
    if keys_head is None and keys_tail is None:
        known = torch.zeros(rows, n, dtype=torch.bool, device=dev)
    else:
        known = dense_relation_known(ids, keys_head, keys_tail, h, t, n_rel, n_node)
    n_free = (~known).sum(dim=1)
    rank = torch.zeros(rows, dtype=torch.int64, device=dev)
    if n == 0:
        return RelationSelection(torch.full((rows, k), -1, dtype=torch.int64, device=dev),
                                 torch.full((rows, k), -float("inf"), dtype=score.dtype, device=dev), rank, n_free,
                                 known.to(torch.uint8))
    if target is not None:
        hit = (ids[None, :] == target[:, None]) & (target >= 0)[:, None]
        at = hit.long().argmax(dim=1)                                    # the FIRST position that lists the target
        count = ((score.gather(1, at[:, None]) <= score) & ~known).sum(dim=1)
        rank = torch.where(hit.any(dim=1), 1 + count, rank)
    group = torch.where(known, torch.full_like(known, 2, dtype=torch.int64), torch.isnan(score).long())
    value, index = _dense_topk_groups(score, group, k)
    top_index = torch.where(index < 0, index, ids[index.clamp(min=0)])
    return RelationSelection(top_index, value, rank, n_free, known.to(torch.uint8))


def relation_select(score, cand, keys_head, keys_tail, h, t, target, n_rel, n_node, k, outputs=RELATION_OUTPUTS):
    """Relation prediction over a block of scores (``ultra_relation_select_f32``; the contract is in ``include/ultra_rspmm.h``,
    DESIGN.md section 20).  ``score`` fp32 ``(P, C)``: row ``p`` holds the scores of the candidate relations ``cand`` int64 ``(C,)``
    (ids in ``[0, 2 * n_rel)``, ``c >= n_rel`` the inverse of ``c - n_rel``; ``None``: the identity) for the pair ``(h[p], t[p])``.
    ``keys_head`` / ``keys_tail``: the filter graph's ``completion_keys(0)`` / ``completion_keys(1)`` (both ``None``: unfiltered,
    nothing is known); ``target`` int64 ``(P,)`` relation ids or ``None``.  Returns a :class:`RelationSelection`:
    ``top_index`` int64 / ``top_value`` fp32 ``(P, k)`` the best relations that are not known in the order of :func:`topk_keys`
    (equal scores by ascending position in ``cand``), ending in ``-1`` / ``-inf``; ``rank`` int64 ``(P,)`` the filtered rank of
    ``target`` (0: not a candidate); ``n_free`` int64 ``(P,)``; ``known`` uint8 ``(P, C)``.  ``outputs`` names the results to
    compute, the others are ``None``.  Strided views of ``score`` (unit stride along a row), ``h`` / ``t`` (one common stride) and
    ``target`` go to the kernel as they are; one launch, no workspace, no host synchronisation.  CPU tensors take
    :func:`dense_relation_select`."""
    if score.dim() != 2 or score.dtype != torch.float32 or (score.shape[1] and score.stride(1) != 1):
        raise RuntimeError("relation_select: score must be fp32 (P, C) with contiguous rows")
    rows, n_cand = score.shape
    dev = score.device
    k, n_rel, n_node = int(k), int(n_rel), int(n_node)
    if not 1 <= k <= TOPK_MAX:
        raise RuntimeError("relation_select: 1 to %d relations per pair, got %d" % (TOPK_MAX, k))
    if n_rel <= 0 or n_node <= 0 or float(n_node) ** 2 * n_rel >= 2.0 ** 63:
        raise RuntimeError("relation_select: n_rel and n_node must be positive with 64-bit keys, got %d and %d" % (n_rel, n_node))
    if rows > 1 and score.stride(0) < n_cand:
        raise RuntimeError("relation_select: the rows of score overlap")
    outputs = tuple(outputs)
    if not outputs or any(name not in RELATION_OUTPUTS for name in outputs):
        raise RuntimeError("relation_select: outputs must name some of %s, got %s" % (RELATION_OUTPUTS, outputs))
    if cand is not None and (cand.dtype != torch.int64 or cand.shape != (n_cand,) or cand.device != dev or not cand.is_contiguous()):
        raise RuntimeError("relation_select: cand must be a contiguous int64 (%d,) on %s" % (n_cand, dev))
    for name, keys in (("keys_head", keys_head), ("keys_tail", keys_tail)):
        if keys is not None and (keys.dtype != torch.int64 or keys.dim() != 1 or not keys.is_contiguous() or keys.device != dev):
            raise RuntimeError("relation_select: %s must be a contiguous int64 vector on %s" % (name, dev))
    filtered = keys_head is not None or keys_tail is not None
    if filtered and (h is None or t is None):
        raise RuntimeError("relation_select: a filtered selection needs h and t")
    stride = 1
    if h is not None or t is not None:
        if h is None or t is None:
            raise RuntimeError("relation_select: h and t come together")
        h, t, stride = _index_pair("relation_select", h, t, rows, dev)
    if target is not None and (target.dtype != torch.int64 or target.shape != (rows,) or target.device != dev):
        raise RuntimeError("relation_select: target must be int64 (%d,) on %s" % (rows, dev))
    if target is not None and rows > 1 and target.stride(0) < 0:
        target = target.contiguous()
    if not score.is_cuda:
        full = dense_relation_select(score, cand, keys_head, keys_tail, h, t, target, n_rel, n_node, k)
        return RelationSelection(*[value if name in outputs else None for name, value in zip(RELATION_OUTPUTS, full)])
    if _torch_ext.binding() == "torch":
        bits = sum(1 << RELATION_OUTPUTS.index(name) for name in set(outputs))
        full = _torch_ext.load().relation_select(score, cand, keys_head, keys_tail, h, t, target, n_rel, n_node, k, bits)
        return RelationSelection(*[value if name in outputs else None for name, value in zip(RELATION_OUTPUTS, full)])
    shapes = {"top_index": ((rows, k), torch.int64), "top_value": ((rows, k), torch.float32), "rank": ((rows,), torch.int64),
              "n_free": ((rows,), torch.int64), "known": ((rows, n_cand), torch.uint8)}
    out = {name: torch.empty(shape, dtype=dtype, device=dev) if name in outputs else None
           for name, (shape, dtype) in shapes.items()}
    if rows:
        _launch(dev, "ultra_relation_select_f32", score if n_cand else None, rows, n_cand, score.stride(0) if rows > 1 else n_cand,
                cand, keys_head, keys_head.numel() if keys_head is not None else 0, keys_tail,
                keys_tail.numel() if keys_tail is not None else 0, h, t, stride, target,
                target.stride(0) if (target is not None and rows > 1) else 1, n_rel, n_node, k,
                *[out[name] for name in RELATION_OUTPUTS])
    return RelationSelection(**out)


# ---------------------------------------------------------------------------------------------------------- candidate sets
CANDIDATE_OUTPUTS = ("top_index", "top_value", "rank", "n_free", "member")    # bit i of the operator's `outputs` argument
CandidateSelection = collections.namedtuple("CandidateSelection", CANDIDATE_OUTPUTS)
CANDIDATE_SLICE = 32768         # list positions per workgroup of ultra_candidate_select_f32; longer lists take two launches


def _candidate_arguments(name, pred, sets, set_of, k, keys, anchor, rel, n_rel, target, outputs, max_len):
    """The checked arguments of :func:`candidate_select` / :func:`dense_candidate_select`:
    ``(set_of, anchor, rel, index stride, target, outputs, max_len)``."""
    if pred.dim() != 2 or pred.dtype != torch.float32 or pred.shape[1] < 1 or pred.stride(1) != 1:
        raise RuntimeError("%s: pred must be fp32 (Q, N >= 1) with contiguous rows" % name)
    rows, n_node = pred.shape
    dev = pred.device
    if rows > 1 and pred.stride(0) < n_node:
        raise RuntimeError("%s: the rows of pred overlap" % name)
    if n_node >= 2 ** 31:
        raise RuntimeError("%s: entity ids are 31-bit, got %d entities" % (name, n_node))
    outputs = tuple(outputs)
    if not outputs or any(o not in CANDIDATE_OUTPUTS for o in outputs):
        raise RuntimeError("%s: outputs must name some of %s, got %s" % (name, CANDIDATE_OUTPUTS, outputs))
    if ("top_index" in outputs or "top_value" in outputs) and not 1 <= int(k) <= TOPK_MAX:
        raise RuntimeError("%s: 1 to %d entities per query, got %d" % (name, TOPK_MAX, int(k)))
    if sets is None and set_of is not None:
        raise RuntimeError("%s: set_of needs the sets" % name)
    if sets is not None:
        if int(sets.num_node) != n_node:
            raise RuntimeError("%s: the scores list %d entities but the sets were built over %d" % (name, n_node, int(sets.num_node)))
        if (sets.ptr.dtype != torch.int64 or sets.items.dtype != torch.int32 or sets.ptr.dim() != 1 or sets.items.dim() != 1
                or sets.ptr.numel() < 1 or sets.ptr.device != dev or sets.items.device != dev
                or not sets.ptr.is_contiguous() or not sets.items.is_contiguous()):
            raise RuntimeError("%s: the sets must hold contiguous ptr int64 (S + 1,) and items int32 on %s" % (name, dev))
    if set_of is not None and (set_of.dtype != torch.int64 or set_of.shape != (rows,) or set_of.device != dev):
        raise RuntimeError("%s: set_of must be int64 (%d,) on %s" % (name, rows, dev))
    if keys is not None and (keys.dtype != torch.int64 or keys.dim() != 1 or not keys.is_contiguous() or keys.device != dev):
        raise RuntimeError("%s: keys must be a contiguous int64 vector on %s" % (name, dev))
    if keys is not None and (anchor is None or rel is None):
        raise RuntimeError("%s: a filtered selection needs anchor and rel" % name)
    if keys is not None and (int(n_rel) <= 0 or float(n_node) ** 2 * int(n_rel) >= 2.0 ** 63):
        raise RuntimeError("%s: n_rel must be positive with 64-bit keys, got %d over %d entities" % (name, int(n_rel), n_node))
    stride = 1
    if anchor is not None or rel is not None:
        if anchor is None or rel is None:
            raise RuntimeError("%s: anchor and rel come together" % name)
        anchor, rel, stride = _index_pair(name, anchor, rel, rows, dev)
    if set_of is not None and rows > 1 and (set_of.stride(0) < 1 or (anchor is not None and set_of.stride(0) != stride)):
        if anchor is not None and stride != 1:
            anchor, rel, stride = anchor.contiguous(), rel.contiguous(), 1
        set_of = set_of.contiguous()
    if set_of is not None and anchor is None and rows > 1:
        stride = set_of.stride(0)
    if target is not None and (target.dtype != torch.int64 or target.shape != (rows,) or target.device != dev):
        raise RuntimeError("%s: target must be int64 (%d,) on %s" % (name, rows, dev))
    if target is not None and rows > 1 and target.stride(0) < 0:
        target = target.contiguous()
    if max_len is None:
        max_len = n_node                                  # (right for every set_of: a -1 takes all entities)
    max_len = int(max_len)
    if not 0 <= max_len < 2 ** 31:
        raise RuntimeError("%s: max_len must be in [0, 2^31), got %d" % (name, max_len))
    return set_of, anchor, rel, stride, target, outputs, max_len


def dense_candidate_select(pred, sets, set_of, k, keys, anchor, rel, n_rel, target=None, outputs=CANDIDATE_OUTPUTS, max_len=None):
    """:func:`candidate_select` in torch ops from dense ``(Q, N)`` masks -- the twin CPU tensors take, and the route the device
    kernel is timed against (it runs on any device; building the masks reads the host once)."""
    set_of, anchor, rel, _, target, outputs, max_len = _candidate_arguments(
        "dense_candidate_select", pred, sets, set_of, k, keys, anchor, rel, n_rel, target, outputs, max_len)
    rows, n = pred.shape
    dev = pred.device
    listed, known = _dense_listed_known(rows, n, dev, sets, set_of, max_len, keys, anchor, rel, n_rel)
    cand = listed & ~known
    n_free = cand.sum(dim=1)
    rank = torch.zeros(rows, dtype=torch.int64, device=dev)
    member = torch.zeros(rows, dtype=torch.uint8, device=dev)
    if target is not None:
        valid = (target >= 0) & (target < n)
        at = target.clamp(0, n - 1)[:, None]
        rank = torch.where(valid, 1 + ((pred.gather(1, at) <= pred) & cand).sum(dim=1), rank)
        member = (valid & listed.gather(1, at)[:, 0]).to(torch.uint8)
    top_value = top_index = None
    if "top_index" in outputs or "top_value" in outputs:
        group = torch.where(cand, torch.isnan(pred).long(), torch.full((), 2, dtype=torch.int64, device=dev))
        top_value, top_index = _dense_topk_groups(pred, group, int(k))
    full = dict(top_index=top_index, top_value=top_value, rank=rank, n_free=n_free, member=member)
    return CandidateSelection(*[full[name] if name in outputs else None for name in CANDIDATE_OUTPUTS])


def _dense_listed_known(rows, n, dev, sets, set_of, max_len, keys, anchor, rel, n_rel):
    """The dense ``(rows, n)`` bool masks of the candidate-set operators' torch twins: ``listed[q, e]`` -- entity ``e`` is in the
    list of row ``q`` (its first ``max_len`` positions) -- and ``known[q, e]`` -- ``e`` completes ``(anchor[q], rel[q], ?)``."""
    every = torch.arange(n, device=dev)[None, :] < max_len                       # the list of s == -1
    if set_of is None:
        listed = every.expand(rows, n)
    else:
        n_sets = sets.ptr.numel() - 1
        real = (set_of >= 0) & (set_of < n_sets)
        s = set_of.clamp(0, max(n_sets - 1, 0))
        n_items = sets.items.numel()
        first = sets.ptr[s].clamp(0, n_items) if n_sets else torch.zeros_like(s)
        last = torch.maximum(sets.ptr[s + 1].clamp(0, n_items), first) if n_sets else first
        count = torch.where(real, (last - first).clamp(max=max_len), torch.zeros_like(first))
        row = torch.repeat_interleave(torch.arange(rows, device=dev), count)
        at = torch.arange(int(count.sum()), device=dev) - torch.repeat_interleave(count.cumsum(0) - count, count) + first[row]
        item = sets.items[at].long()
        inside = (item >= 0) & (item < n)
        listed = torch.zeros(rows, n, dtype=torch.bool, device=dev)
        listed[row[inside], item[inside]] = True
        listed = torch.where((set_of == -1)[:, None], every, listed)
    known = torch.zeros(rows, n, dtype=torch.bool, device=dev)
    if keys is not None and rows and keys.numel():
        base = (anchor * int(n_rel) + rel) * n
        first, last = torch.searchsorted(keys, base), torch.searchsorted(keys, base + n)
        count = last - first
        row = torch.repeat_interleave(torch.arange(rows, device=dev), count)
        at = torch.arange(int(count.sum()), device=dev) - torch.repeat_interleave(count.cumsum(0) - count, count) + first[row]
        known[row, keys[at] - base[row]] = True
    return listed, known


def candidate_select(pred, sets, set_of, k, keys, anchor, rel, n_rel, target=None, outputs=CANDIDATE_OUTPUTS, max_len=None):
    """Rank, counts and the ``k`` best entities of every query AMONG A SET of admissible entities (``ultra_candidate_select_f32``;
    the contract is in ``include/ultra_rspmm.h``).  ``pred`` fp32 ``(Q, N)`` (a strided view with unit
    stride along a row is fine); ``sets``: a ``data.CandidateSets`` over ``N`` entities (``ptr`` int64 ``(S + 1,)``, ``items``
    int32, ascending and distinct inside a set) or ``None``; ``set_of`` int64 ``(Q,)``: the set of every query, ``-1`` = every
    entity (``None``: ``-1`` for all).  ``keys`` / ``anchor`` / ``rel`` / ``n_rel``: the filter of :func:`topk_keys` (``keys=None``:
    nothing is filtered); ``target`` int64 ``(Q,)`` entities (``-1``: none) or ``None``.  Returns a :class:`CandidateSelection`:
    ``top_index`` int64 / ``top_value`` fp32 ``(Q, k)`` the candidates -- listed and not known -- in the order of
    :func:`topk_keys` (equal scores by ascending ENTITY), ending in ``-1`` / ``-inf``; ``rank`` int64 ``(Q,)`` = ``1 + #{candidates
    e : pred[q, target] <= pred[q, e]}`` whether or not the target is listed (0 without a target); ``n_free`` int64 ``(Q,)`` the
    number of candidates; ``member`` uint8 ``(Q,)``: the target is listed.  ``outputs`` names the results to compute, the others
    are ``None``.  ``max_len``: an upper bound of every list's length, ``N`` when a ``-1`` may occur (the default; a caller that
    knows its ``set_of`` holds none passes ``sets.max_len``) -- lists of at most 32768 take one launch, longer ones two and a
    workspace from the caching allocator.  No host synchronisation.  CPU tensors take :func:`dense_candidate_select`."""
    if not pred.is_cuda:
        return dense_candidate_select(pred, sets, set_of, k, keys, anchor, rel, n_rel, target, outputs, max_len)
    set_of, anchor, rel, stride, target, outputs, max_len = _candidate_arguments(
        "candidate_select", pred, sets, set_of, k, keys, anchor, rel, n_rel, target, outputs, max_len)
    rows, n_node = pred.shape
    dev = pred.device
    want_top = "top_index" in outputs or "top_value" in outputs
    k = int(k) if want_top else 1
    ptr, items = (sets.ptr, sets.items) if sets is not None else (None, None)
    if _torch_ext.binding() == "torch":
        bits = sum(1 << CANDIDATE_OUTPUTS.index(name) for name in set(outputs))
        full = _torch_ext.load().candidate_select(pred, ptr, items, set_of, max_len, keys, anchor, rel, int(n_rel), target, k, bits)
        return CandidateSelection(*[value if name in outputs else None for name, value in zip(CANDIDATE_OUTPUTS, full)])
    shapes = {"top_index": ((rows, k), torch.int64), "top_value": ((rows, k), torch.float32), "rank": ((rows,), torch.int64),
              "n_free": ((rows,), torch.int64), "member": ((rows,), torch.uint8)}
    out = {name: torch.empty(shape, dtype=dtype, device=dev) if name in outputs else None
           for name, (shape, dtype) in shapes.items()}
    if rows:
        ws_bytes = int(_lib.load().ultra_candidate_select_workspace(rows, max_len, k if want_top else 0))
        ws = torch.empty(ws_bytes // 8, dtype=torch.int64, device=dev) if ws_bytes else None
        _launch(dev, "ultra_candidate_select_f32", pred, rows, n_node, pred.stride(0) if rows > 1 else n_node, ptr, items,
                ptr.numel() - 1 if ptr is not None else 0, items.numel() if items is not None else 0, set_of, max_len, keys,
                keys.numel() if keys is not None else 0, anchor, rel, stride, int(n_rel), target,
                target.stride(0) if (target is not None and rows > 1) else 1, k, *[out[name] for name in CANDIDATE_OUTPUTS],
                ws, ws_bytes)
    return CandidateSelection(**out)


# ------------------------------------------------------------------------------------------ type-constrained strict negatives
def _negative_arguments(name, keys, anchor, rel, n_rel, n_node, rand, sets, set_of, min_free, device_only):
    """The checked arguments of :func:`constrained_negatives` / :func:`dense_constrained_negatives`:
    ``(anchor, rel, set_of, index stride)``."""
    if rand.dim() != 2 or rand.dtype != torch.float32 or rand.shape[1] < 1 or not rand.is_contiguous() \
            or (device_only and not rand.is_cuda):
        raise RuntimeError("%s: rand must be contiguous fp32 (B, S >= 1)%s" % (name, " on the HIP device" if device_only else ""))
    rows, dev = rand.shape[0], rand.device
    n_rel, n_node, min_free = int(n_rel), int(n_node), int(min_free)
    if not 1 <= n_node < 2 ** 31 or n_rel <= 0 or float(n_node) ** 2 * n_rel >= 2.0 ** 63:
        raise RuntimeError("%s: %d entities (1 to 2^31 - 1) and %d relations (positive, 64-bit keys)" % (name, n_node, n_rel))
    if min_free < 1:
        raise RuntimeError("%s: min_free must be at least 1, got %d" % (name, min_free))
    if keys.dtype != torch.int64 or keys.dim() != 1 or not keys.is_contiguous() or keys.device != dev:
        raise RuntimeError("%s: keys must be a contiguous int64 vector on %s" % (name, dev))
    if sets is None and set_of is not None:
        raise RuntimeError("%s: set_of needs the sets" % name)
    if sets is not None:
        if int(sets.num_node) != n_node:
            raise RuntimeError("%s: %d entities but the sets were built over %d" % (name, n_node, int(sets.num_node)))
        if (sets.ptr.dtype != torch.int64 or sets.items.dtype != torch.int32 or sets.ptr.dim() != 1 or sets.items.dim() != 1
                or sets.ptr.numel() < 1 or sets.ptr.device != dev or sets.items.device != dev
                or not sets.ptr.is_contiguous() or not sets.items.is_contiguous()):
            raise RuntimeError("%s: the sets must hold contiguous ptr int64 (S + 1,) and items int32 on %s" % (name, dev))
    if set_of is not None and (set_of.dtype != torch.int64 or set_of.shape != (rows,) or set_of.device != dev):
        raise RuntimeError("%s: set_of must be int64 (%d,) on %s" % (name, rows, dev))
    anchor, rel, stride = _index_pair(name, anchor, rel, rows, dev)
    if set_of is not None and rows > 1 and set_of.stride(0) != stride:
        anchor, rel, set_of, stride = anchor.contiguous(), rel.contiguous(), set_of.contiguous(), 1
    return anchor, rel, set_of, stride


def dense_constrained_negatives(keys, anchor, rel, n_rel, n_node, rand, sets=None, set_of=None, min_free=1, return_free=False):
    """:func:`constrained_negatives` in torch ops over dense ``(B, N)`` masks -- the twin CPU tensors take, and the side the
    kernel is compared with (it runs on any device; building the masks reads the host once).  With ``free = listed & ~known``
    and ``n_free = free.sum(-1)``, a row with ``n_free >= min_free`` returns ``free.nonzero()``'s entities at
    ``(rand * n_free).long()`` -- the indexing of ``task.variadic_sample`` with ``rand`` given -- and any other row the same over
    ``~known``; an index is clamped into its row, and a row without any entity to draw gives 0."""
    anchor, rel, set_of, _ = _negative_arguments("dense_constrained_negatives", keys, anchor, rel, n_rel, n_node, rand, sets,
                                                 set_of, min_free, False)
    rows, n = rand.shape[0], int(n_node)
    listed, known = _dense_listed_known(rows, n, rand.device, sets, set_of, n, keys, anchor, rel, n_rel)
    free = listed & ~known
    n_free = free.sum(dim=1)
    constrained = n_free >= int(min_free)
    mask = torch.where(constrained[:, None], free, ~known)
    size = mask.sum(dim=1)
    index = (rand * size.unsqueeze(-1)).long()                                   # fp32 product, truncated
    index = torch.minimum(index, size.unsqueeze(-1) - 1).clamp(min=0)            # (1.0 rounds up; negative / NaN -> 0)
    out = torch.searchsorted(mask.long().cumsum(dim=1), index + 1)               # the (index)-th True of the row
    out = torch.where(size.unsqueeze(-1) > 0, out, torch.zeros_like(out))
    return (out, n_free) if return_free else out


def constrained_negatives(keys, anchor, rel, n_rel, n_node, rand, sets=None, set_of=None, min_free=1, return_free=False):
    """Type-constrained strict negatives (``ultra_constrained_negative``; the contract is in ``include/ultra_rspmm.h``, DESIGN.md
    section 22): row ``q`` draws ``rand.shape[1]`` entities from the list of set ``set_of[q]`` of ``sets`` (a
    ``data.CandidateSets`` over ``n_node`` entities; ``-1`` = every entity; ``set_of=None``: ``-1`` for all rows) minus the
    entities that complete ``(anchor[q], rel[q], ?)`` in ``keys`` -- ``F[min((rand * n_free).long(), n_free - 1)]`` with ``F``
    ascending, the draw of :func:`strict_negatives`.  A row with fewer than ``min_free`` free entities in its set, an empty
    set or a set id outside ``[-1, S)`` falls back to the row :func:`strict_negatives` returns for the same ``rand``.
    ``anchor`` / ``rel`` / ``set_of`` int64 ``(B,)`` may be views that share one positive stride (the columns of ``batch.t()``);
    ``rand`` contiguous fp32 ``(B, S)`` on the device.  Returns int64 ``(B, S)`` and, with ``return_free``, ``n_free`` int64
    ``(B,)``: the SET-SIDE count of every row (a row fell back iff ``n_free < min_free``).  One launch, no ``(B, N)`` mask, no
    host synchronisation.  CPU tensors take :func:`dense_constrained_negatives`."""
    if not rand.is_cuda:
        return dense_constrained_negatives(keys, anchor, rel, n_rel, n_node, rand, sets, set_of, min_free, return_free)
    anchor, rel, set_of, stride = _negative_arguments("constrained_negatives", keys, anchor, rel, n_rel, n_node, rand, sets,
                                                      set_of, min_free, True)
    rows, n_sample = rand.shape
    ptr, items = (sets.ptr, sets.items) if sets is not None else (None, None)
    if _torch_ext.binding() == "torch":
        out, n_free = _torch_ext.load().constrained_negatives(keys, anchor, rel, set_of, ptr, items, int(n_rel), int(n_node), rand,
                                                              int(min_free))
        return (out, n_free) if return_free else out
    out = torch.empty(rows, n_sample, dtype=torch.int64, device=rand.device)
    n_free = torch.empty(rows, dtype=torch.int64, device=rand.device) if return_free else None
    if rows:
        _launch(rand.device, "ultra_constrained_negative", keys, keys.numel(), anchor, rel, set_of, stride, rows, int(n_rel),
                int(n_node), ptr, items, ptr.numel() - 1 if ptr is not None else 0, items.numel() if items is not None else 0,
                rand, n_sample, int(min_free), out, n_free)
    return (out, n_free) if return_free else out


def dense_set_boundary(member, query, floor=None, with_count=False):
    """:func:`set_boundary` in torch ops, in the dtype of ``query`` (the host twin, and the form the fp64 ATen definition of a
    projection uses): entity ``v`` is kept for query ``q`` iff ``member[q, v] > 0`` and ``member[q, v] >= floor[q]`` (a NaN is
    never kept); kept rows hold ``member[q, v] * query[q]``, every other row ``+0.0`` whatever ``query`` holds.
    Differentiable as it stands: ``torch.where``'s own backward hands the product ``where(keep, d_boundary, 0)``, so on FINITE
    ``d_boundary`` and ``query`` (memberships may hold NaN) its gradients equal the definition of
    ``ultra_set_boundary_backward_f32`` entry for entry (a zero times a finite number is the selected-away zero;
    tests/test_query_train_cpu.py holds it to that).  Only the device entry also keeps the zeros under non-finite
    ``d_boundary`` / ``query`` values at entries that are not kept."""
    m = member.to(query.dtype)
    keep = m > 0
    if floor is not None:
        keep = keep & (m >= floor.to(query.dtype).unsqueeze(-1))
    keep_t = keep.t().unsqueeze(-1)                                      # (N, Q, 1)
    # (the product is taken of the KEPT memberships: the same forward values, and in backward a NaN membership that is not kept
    # meets its zero gradient as 0 * 0, not as 0 * NaN)
    kept = torch.where(keep, m, m.new_zeros(()))
    boundary = torch.where(keep_t, kept.t().unsqueeze(-1) * query.unsqueeze(0), query.new_zeros(()))
    return (boundary, keep.sum(dim=1).to(torch.int32)) if with_count else boundary


def set_boundary(member, query, floor=None, with_count=False):
    """The boundary condition of a projection from fuzzy entity SETS (``ultra_set_boundary_f32``, the contract is in
    ``include/ultra_rspmm.h``): ``member`` fp32 ``(Q, N)`` memberships, ``query`` fp32 ``(Q, D)``, ``floor`` fp32 ``(Q,)`` or
    ``None``.  Entity ``v`` is kept for query ``q`` iff ``member[q, v] > 0`` and ``member[q, v] >= floor[q]``; returns the
    ``(N, Q, D)`` tensor ``member[q, v] * query[q]`` with ``+0.0`` rows for everything not kept, and with ``with_count`` also the
    int32 ``(Q,)`` numbers of kept entities.  One launch that reads the memberships once and writes the boundary once; no host
    synchronisation (capturable).  The rows of ``member`` may be strided (a view of a wider matrix) but not overlap.  CPU tensors
    take :func:`dense_set_boundary`."""
    if member.dim() != 2 or query.dim() != 2 or member.dtype != torch.float32 or query.dtype != torch.float32:
        raise RuntimeError("set_boundary: member must be fp32 (Q, N) and query fp32 (Q, D), got %s %s and %s %s"
                           % (member.dtype, tuple(member.shape), query.dtype, tuple(query.shape)))
    n_query, n_node = member.shape
    dim = query.shape[1]
    if n_query < 1 or n_node < 1 or dim < 1 or query.shape[0] != n_query:
        raise RuntimeError("set_boundary: member (Q, N) and query (Q, D) must share Q >= 1 with N, D >= 1, got %s and %s"
                           % (tuple(member.shape), tuple(query.shape)))
    if n_node > 1 and member.stride(1) != 1:
        raise RuntimeError("set_boundary: the rows of member must be contiguous")
    if n_query > 1 and member.stride(0) < n_node:
        raise RuntimeError("set_boundary: the rows of member overlap")
    if query.device != member.device:
        raise RuntimeError("set_boundary: member is on %s, query on %s" % (member.device, query.device))
    if floor is not None and (floor.dtype != torch.float32 or floor.shape != (n_query,) or floor.device != member.device):
        raise RuntimeError("set_boundary: floor must be fp32 (%d,) on %s" % (n_query, member.device))
    if not member.is_cuda:
        return dense_set_boundary(member, query, floor, with_count)
    if torch.is_grad_enabled() and (member.requires_grad or query.requires_grad):
        boundary, count = _SetBoundaryFunction.apply(member, query, floor, bool(with_count))
        return (boundary, count) if with_count else boundary
    return _set_boundary_launch(member, query, floor, with_count)


def _set_boundary_launch(member, query, floor, with_count):
    """The one launch of :func:`set_boundary` behind its checks."""
    n_query, n_node = member.shape
    dim = query.shape[1]
    query = query.contiguous()
    floor = None if floor is None else floor.contiguous()
    boundary = torch.empty(n_node, n_query, dim, dtype=torch.float32, device=member.device)
    count = torch.empty(n_query, dtype=torch.int32, device=member.device) if with_count else None
    _launch(member.device, "ultra_set_boundary_f32", member, n_query, n_node, member.stride(0) if n_query > 1 else n_node,
            floor, query, dim, boundary, count)
    return (boundary, count) if with_count else boundary


def set_boundary_backward(d_boundary, member, query, floor=None, want_query=True):
    """``ultra_set_boundary_backward_f32`` (the contract is in ``include/ultra_rspmm.h``): ``(d_member (Q, N), d_query (Q, D) or
    None)`` for the gradient ``d_boundary`` fp32 ``(N, Q, D)`` of :func:`set_boundary`'s result.  An entity that is not kept is
    selected away: ``+0.0`` in ``d_member`` and nothing in ``d_query``, whatever ``d_boundary`` and ``query`` hold there.  The
    rows of ``member`` may be strided, as in the forward.  Deterministic; two launches, capturable."""
    if (member.dim() != 2 or query.dim() != 2 or d_boundary.dim() != 3
            or _not_fp32_on(member.device, (member, query, d_boundary) + (() if floor is None else (floor,)))):
        raise RuntimeError("set_boundary_backward needs fp32 member (Q, N), query (Q, D), d_boundary (N, Q, D) on one HIP device")
    n_query, n_node = member.shape
    dim = query.shape[1]
    if n_query < 1 or n_node < 1 or dim < 1 or query.shape[0] != n_query or tuple(d_boundary.shape) != (n_node, n_query, dim):
        raise RuntimeError("set_boundary_backward: member %s, query %s and d_boundary %s do not fit"
                           % (tuple(member.shape), tuple(query.shape), tuple(d_boundary.shape)))
    if (n_node > 1 and member.stride(1) != 1) or (n_query > 1 and member.stride(0) < n_node):
        raise RuntimeError("set_boundary_backward: the rows of member must be contiguous and must not overlap")
    if floor is not None and floor.shape != (n_query,):
        raise RuntimeError("set_boundary_backward: floor must be fp32 (%d,)" % n_query)
    dev = member.device
    d_boundary, query = d_boundary.contiguous(), query.contiguous()
    floor = None if floor is None else floor.contiguous()
    d_member = torch.empty(n_query, n_node, dtype=torch.float32, device=dev)
    d_query = workspace = None
    ws_bytes = 0
    if want_query:
        d_query = torch.empty(n_query, dim, dtype=torch.float32, device=dev)
        ws_bytes = int(_lib.load().ultra_set_boundary_backward_workspace(n_query, n_node, dim))
        workspace = torch.empty(max(ws_bytes // 4, 1), dtype=torch.float32, device=dev)
    _launch(dev, "ultra_set_boundary_backward_f32", d_boundary, member, n_query, n_node,
            member.stride(0) if n_query > 1 else n_node, floor, query, dim, d_member, d_query, workspace, ws_bytes)
    return d_member, d_query


class _SetBoundaryFunction(torch.autograd.Function):
    """:func:`set_boundary` under autograd: today's launch forward, ``ultra_set_boundary_backward_f32`` backward.  ``count`` is
    not differentiable, ``floor`` (a cut, hence a mask) gets no gradient."""

    @staticmethod
    def forward(ctx, member, query, floor, with_count):
        query = query.contiguous()
        result = _set_boundary_launch(member, query, floor, with_count)
        boundary, count = result if with_count else (result, None)
        ctx.save_for_backward(member, query, floor)
        if count is not None:
            ctx.mark_non_differentiable(count)
        return boundary, count

    @staticmethod
    def backward(ctx, d_boundary, _d_count):
        member, query, floor = ctx.saved_tensors
        d_member, d_query = set_boundary_backward(d_boundary, member.detach(), query.detach(), floor, ctx.needs_input_grad[1])
        return (d_member if ctx.needs_input_grad[0] else None), d_query, None, None


# The divergence guard's record (``include/ultra_rspmm.h``): int32 fields ``step`` (committed steps; they are numbered from 1),
# ``tripped_step`` (-1 until the first trip, then the number of that step; sticky), ``tripped_tensor`` (the lowest index among
# the tensors that tripped in that step), ``pending`` (the lowest index that tripped since the last commit; GUARD_CLEAN = none).
GUARD_STEP, GUARD_TRIPPED_STEP, GUARD_TRIPPED_TENSOR, GUARD_PENDING, GUARD_FIELDS = 0, 1, 2, 3, 4
GUARD_CLEAN = 0x7fffffff
_NONFINITE_BITS = 0x7f800000


def nonfinite_record(device, step=0):
    """A fresh record ``[step, -1, -1, GUARD_CLEAN]`` on ``device`` (created by the host, outside any capture)."""
    return torch.tensor([int(step), -1, -1, GUARD_CLEAN], dtype=torch.int32).to(device)


def _check_record(record, device):
    if (record.dtype != torch.int32 or record.dim() != 1 or record.numel() != GUARD_FIELDS or not record.is_contiguous()
            or record.device != device):
        raise RuntimeError("the guard's record must be a contiguous int32 vector of %d fields on %s" % (GUARD_FIELDS, device))


def nonfinite_scan(tensors, record, first_index=0):
    """Tensor ``i`` of ``tensors`` has the index ``first_index + i``; every one that holds a non-finite element -- exponent
    bits all ones: ``inf`` and ``NaN`` of either sign and any payload, not denormals, ``+-FLT_MAX`` or ``-0.0`` -- lowers
    ``record[GUARD_PENDING]`` to its index (``ultra_nonfinite_scan_f32``: the whole list in a few launches, the addresses in the
    kernel arguments; kernels only, capturable, nothing is read back).  A ``None`` entry is skipped and keeps its index.  The
    tensors are fp32 and contiguous (a view may start at any element) on the record's device; CPU tensors take a dense torch
    path of the same definition."""
    device = record.device
    _check_record(record, device)
    first_index = int(first_index)
    if first_index < 0:
        raise RuntimeError("nonfinite_scan: first_index must not be negative, got %d" % first_index)
    tensors = [None if t is None else t.detach() for t in tensors]
    for i, t in enumerate(tensors):
        if t is None:
            continue
        if t.dtype != torch.float32:
            raise RuntimeError("nonfinite_scan: tensor %d is %s; the scan reads fp32 bit patterns" % (first_index + i, t.dtype))
        if t.device != device:
            raise RuntimeError("nonfinite_scan: tensor %d is on %s, the record on %s" % (first_index + i, t.device, device))
        if not t.is_contiguous():
            raise RuntimeError("nonfinite_scan: tensor %d is not contiguous" % (first_index + i))
    if not record.is_cuda:
        for i, t in enumerate(tensors):
            if t is not None and t.numel() and bool(((t.view(torch.int32) & _NONFINITE_BITS) == _NONFINITE_BITS).any()):
                record[GUARD_PENDING] = min(int(record[GUARD_PENDING]), first_index + i)
        return
    if not tensors:
        return
    ptrs = _pointer_array([t if t is not None and t.numel() else None for t in tensors])
    numel = (ctypes.c_int64 * len(tensors))(*[0 if t is None else t.numel() for t in tensors])
    _launch(device, "ultra_nonfinite_scan_f32", ptrs, numel, len(tensors), first_index, record)


def nonfinite_commit(record, advance=True):
    """Ends a step of the guard, behind its scans (``ultra_nonfinite_commit``, one thread): if nothing tripped before and
    ``pending`` is not clean, ``tripped_step = step + 1`` and ``tripped_tensor = pending``; then ``pending`` is reset and
    ``step`` counted.  ``advance=False`` only latches, in the middle of a step: what was scanned so far is reported ahead of
    whatever is scanned later in the step."""
    _check_record(record, record.device)
    if record.is_cuda:
        _launch(record.device, "ultra_nonfinite_commit", record, int(bool(advance)))
        return
    step, tripped, _, pending = record.tolist()
    if tripped < 0 and pending != GUARD_CLEAN:
        record[GUARD_TRIPPED_STEP], record[GUARD_TRIPPED_TENSOR] = step + 1, pending
    record[GUARD_PENDING], record[GUARD_STEP] = GUARD_CLEAN, step + int(bool(advance))


# Training, opt-in (ULTRA_KEEP_PRE_NORM=1): the fused epilogue's forward keeps z = Linear(cat[input, update]) (one more
# (N, B, 64) tensor per layer) and the fused backward loads it instead of recomputing it -- a third of that kernel's matrix
# work, identical gradients.  Measured on an MI355X it only moves the backward kernel 380 -> 365 us at 655 k rows (the kernel
# waits on memory 38 % of its cycles, PMC; its matrix cores are busy 44 %) and the forward pays 12 us for writing z: no gain
# per step, hence off by default.
KEEP_PRE_NORM = _env_bool("ULTRA_KEEP_PRE_NORM", False)


def _epilogue_gradients(input_c, update_c, has_ln, zero_update=False):
    """Outputs of the one-pass epilogue backward: ``[d_input, d_update, d_weight, d_bias, d_gamma, d_beta]`` (the LayerNorm
    pair ``None`` without LayerNorm)."""
    dev = input_c.device
    d_input = torch.empty_like(input_c)
    d_update = torch.zeros_like(update_c) if zero_update else torch.empty_like(update_c)
    d_weight = torch.empty(64, 128, dtype=torch.float32, device=dev)
    d_bias = torch.empty(64, dtype=torch.float32, device=dev)
    d_g = torch.empty(64, dtype=torch.float32, device=dev) if has_ln else None
    d_b = torch.empty(64, dtype=torch.float32, device=dev) if has_ln else None
    return [d_input, d_update, d_weight, d_bias, d_g, d_b]


def _combine_backward_fused(input_c, update_c, epilogue, grad_out, z, grads, tiles=None):
    """``ultra_combine_backward_fused_f32`` into ``grads`` (:func:`_epilogue_gradients`): one pass over the rows -- recompute z
    (or load ``z``), LayerNorm / ReLU backward, d_weight, d_input | d_update (3 row-sized reads + 2 writes); parameter gradients
    come out finished.  ``epilogue``: the layer's :func:`_epilogue` run; ``tiles``: see :func:`candidate_tiles`."""
    dev = input_c.device
    rows = input_c.numel() // 64
    n_waves = ctypes.c_int(0)
    _lib.check(_lib.load().ultra_combine_backward_fused_waves(dev.index or 0, rows, ctypes.byref(n_waves)))
    ws = torch.empty(n_waves.value * (64 * 128 + 192), dtype=torch.float32, device=dev)
    _launch(dev, "ultra_combine_backward_fused_f32", input_c, update_c, *epilogue, grad_out, z, *grads, ws, ws.numel() * 4, tiles,
            tiles.numel() if tiles is not None else 0, rows, 64)


# The one-pass backward addresses its rows through 32-bit buffer offsets: ``(rows + a tile) * 256 B < 4 GiB``
# (csrc/combine_fused_bwd.inc; the entry returns ULTRA_ERR_BAD_SHAPE beyond).  Above it the three-kernel form, whose addresses
# are 64-bit, runs whatever ULTRA_COMBINE_BWD says.
FUSED_BACKWARD_MAX_ROWS = (1 << 24) - 64


def _combine_backward_split(input_c, update_c, weight, bias, ln_weight, ln_bias, ln_eps, relu, shortcut, grad_out, grads=None,
                            needs=(True,) * 6):
    """The three-kernel epilogue backward (csrc/combine_train.inc): d_z and the per-wave partial parameter sums,
    ``d_input | d_update`` from d_z -- written into ``grads[0]`` and ``grads[1]`` (:func:`_epilogue_gradients`) where the caller
    brings them and wants both --, the partial sums added.  ``needs``: which of the six gradients the caller wants; the others
    come back as ``None``.  Returns the six."""
    dev = input_c.device
    rows = input_c.numel() // 64
    has_ln = ln_weight is not None
    n_ln, n_wg = ctypes.c_int(0), ctypes.c_int(0)
    _lib.check(_lib.load().ultra_combine_backward_waves(dev.index or 0, rows, ctypes.byref(n_ln), ctypes.byref(n_wg)))
    d_z = torch.empty(rows, 64, dtype=torch.float32, device=dev)
    dg_p = torch.empty(n_ln.value, 64, dtype=torch.float32, device=dev) if has_ln else None
    db_p = torch.empty(n_ln.value, 64, dtype=torch.float32, device=dev) if has_ln else None
    dw_p = torch.empty(n_wg.value, 64 * 128, dtype=torch.float32, device=dev)
    dbias_p = torch.empty(n_wg.value, 64, dtype=torch.float32, device=dev) if needs[3] else None
    _launch(dev, "ultra_combine_backward_f32", input_c, update_c, *_epilogue(weight, bias, ln_weight, ln_bias, ln_eps, relu),
            grad_out, d_z, dg_p, db_p, dw_p, dbias_p, rows, 64)
    d_input = d_update = d_weight = d_bias = d_g = d_b = None
    if needs[0] and needs[1]:       # both activation gradients: one pass over d_z instead of two GEMMs
        d_input, d_update = (torch.empty_like(input_c), torch.empty_like(update_c)) if grads is None else (grads[0], grads[1])
        _launch(dev, "ultra_combine_dxdu_f32", d_z, weight.contiguous(), grad_out if shortcut else None, d_input, d_update,
                rows, 64)
    elif needs[0]:
        if shortcut:        # d_input = grad_out + d_z . W[:, :64] in one GEMM call (beta = 1)
            d_input = torch.addmm(grad_out.view(rows, 64), d_z, weight[:, :64]).view_as(input_c)
        else:
            d_input = torch.mm(d_z, weight[:, :64]).view_as(input_c)
    if needs[1] and d_update is None:
        d_update = torch.mm(d_z, weight[:, 64:]).view_as(update_c)
    if needs[2]:
        d_weight = dw_p.sum(0).view(64, 128)
    if needs[3]:
        d_bias = dbias_p.sum(0)
    if has_ln and needs[4]:
        d_g = dg_p.sum(0)
    if has_ln and needs[5]:
        d_b = db_p.sum(0)
    return d_input, d_update, d_weight, d_bias, d_g, d_b


class _CombineFunction(torch.autograd.Function):
    """Fused epilogue with a fused backward (training).  Forward = ``combine_forward``; only the layer's inputs are
    saved.  Backward: ``libultra_rspmm`` recomputes z, applies the ReLU mask and LayerNorm-backward and reduces
    ``d_weight`` on the matrix cores; ``d_input`` / ``d_update`` are two 64x64 GEMMs."""

    @staticmethod
    def forward(ctx, input, update, weight, bias, ln_weight, ln_bias, ln_eps, relu, shortcut):
        z = torch.empty_like(input, memory_format=torch.contiguous_format) if KEEP_PRE_NORM else None
        out = combine_forward(input, update, weight, bias, ln_weight, ln_bias, ln_eps, relu, shortcut, z_out=z)
        ctx.save_for_backward(input, update, weight, bias, ln_weight, ln_bias, z)
        ctx.flags = (float(ln_eps), bool(relu), bool(shortcut))
        return out

    @staticmethod
    def backward(ctx, grad_out):
        input, update, weight, bias, ln_weight, ln_bias, z = ctx.saved_tensors
        ln_eps, relu, shortcut = ctx.flags
        grad_out = grad_out.contiguous()
        input_c, update_c = input.contiguous(), update.contiguous()
        rows = input.numel() // 64
        needs = ctx.needs_input_grad
        has_ln = ln_weight is not None
        if os.environ.get("ULTRA_COMBINE_BWD", "fused") == "fused" and rows <= FUSED_BACKWARD_MAX_ROWS:
            # the one-pass form (_combine_backward_fused).  ULTRA_COMBINE_BWD=split, and every input beyond that form's 32-bit
            # offsets: the three-kernel form.
            grads = _epilogue_gradients(input_c, update_c, has_ln)
            _combine_backward_fused(input_c, update_c, _epilogue(weight, bias, ln_weight, ln_bias, ln_eps, relu, shortcut), grad_out,
                                    z, grads)
            d_input, d_update, d_weight, d_bias, d_g, d_b = grads
            return (d_input.view_as(input) if needs[0] else None, d_update.view_as(update) if needs[1] else None,
                    d_weight if needs[2] else None, d_bias if needs[3] else None, d_g if (has_ln and needs[4]) else None,
                    d_b if (has_ln and needs[5]) else None, None, None, None)
        d_input, d_update, d_weight, d_bias, d_g, d_b = _combine_backward_split(
            input_c, update_c, weight, bias, ln_weight, ln_bias, ln_eps, relu, shortcut, grad_out, needs=needs[:6])
        d_input = d_input.view_as(input) if d_input is not None else None
        d_update = d_update.view_as(update) if d_update is not None else None
        return d_input, d_update, d_weight, d_bias, d_g, d_b, None, None, None


# The fused inference fast paths of model.py / rel_model.py (one query-preparation kernel, projection tables computed once
# for both sides, the first layer's boundary never materialised) run on this backend; the oracle-backed backend of the
# tests keeps the reference's op-by-op path, so the two are compared against each other.
FAST_INFERENCE = _env_bool("ULTRA_FAST_INFERENCE", True)


def combine(input, update, weight, bias, ln_weight=None, ln_bias=None, ln_eps=1e-5, relu=True, shortcut=False,
            reuse_update=False):
    """``combine`` + shortcut of one layer (``ultra/layer.py:386-392``, ``ultra/model.py:126-127``) as fused HIP
    kernels, differentiable: same forward as :func:`combine_forward`, fused backward.  ``reuse_update`` (inference
    only): see :func:`combine_forward`."""
    tensors = [t for t in (input, update, weight, bias, ln_weight, ln_bias) if t is not None]
    if torch.is_grad_enabled() and any(t.requires_grad for t in tensors):
        return _CombineFunction.apply(input, update, weight, bias, ln_weight, ln_bias, ln_eps, relu, shortcut)
    return combine_forward(input, update, weight, bias, ln_weight, ln_bias, ln_eps, relu, shortcut,
                           reuse_update=reuse_update and update.is_contiguous())


class _RSPMMFunction(torch.autograd.Function):
    """Counterpart of torchdrug's ``RSPMM{Add,Min,Max}{Mul,Add}Function`` autograd classes."""

    @staticmethod
    def forward(ctx, sparse, relation, input, csr, sum, mul, add_rows=None, b_node=None, b_value=None, edge_weight=None):
        # add_rows (sum only): `update + boundary` of layer.py:156,358 inside the kernel; its gradient is grad_out.
        # (b_node, b_value): the same boundary in sparse form -- the gradient of b_value[b] is row b_node[b] of
        # query block b of grad_out (what scatter_add_'s backward would gather from the dense gradient)
        # edge_weight: fp32 (csr.n_edges,) weights of the COALESCED edges (forward-plan order) that replace csr's own; its
        # gradient is rspmm_backward_weight's d_w (TransferNBFNet.visualize: per-layer edge gradients without an (E, F) tensor)
        # a 2-D edge_weight (B, E): one weight vector per query block of F / B columns, every row EQUAL to the coalesced weights
        # (the caller's precondition) -- the forward runs on row 0, the gradient is rspmm_backward_weight_blocks' (B, E)
        ctx.weight_blocks = None
        if edge_weight is not None:
            if edge_weight.dim() == 2:
                ctx.weight_blocks = edge_weight.shape[0]
                csr = csr.with_coalesced_weights(edge_weight.detach()[0])
            else:
                csr = csr.with_coalesced_weights(edge_weight.detach())
        boundary = None if b_node is None else (b_node, b_value.detach())
        out = rspmm_forward(csr, relation, input, sum, mul, add_rows=add_rows, boundary=boundary)
        ctx.has_add_rows = add_rows is not None
        ctx.b_node = b_node
        ctx.csr, ctx.sum, ctx.mul = csr, sum, mul
        ctx.sparse_shape = None
        if sparse is not None and sparse.requires_grad:
            ctx.sparse_shape = tuple(sparse.shape)
        ctx.save_for_backward(relation, input, out if (sum != "add") else None)
        return out

    @staticmethod
    def backward(ctx, output_grad):
        relation, input, out = ctx.saved_tensors
        need_rel, need_in = ctx.needs_input_grad[1], ctx.needs_input_grad[2]
        d_input, d_relation = rspmm_backward(ctx.csr, relation, input, out, output_grad, ctx.sum, ctx.mul,
                                             need_input=need_in, need_relation=need_rel)
        d_sparse = None
        if ctx.sparse_shape is not None and ctx.needs_input_grad[0]:
            d_w = rspmm_backward_weight(ctx.csr, relation, input, out, output_grad, ctx.sum, ctx.mul)
            # one entry per COALESCED edge ((dst, src, rel) order: a coalesced COO tensor), so that every duplicate of a triple
            # receives its gradient once: autograd coalesces the gradient of a sparse constructor before it reads the values'
            # share, and an entry per ORIGINAL edge would hand each duplicate the gradient times the triple's multiplicity
            csr = ctx.csr
            d_sparse = torch.sparse_coo_tensor(torch.stack([csr.dst, csr.src, csr.rel_id]), d_w, ctx.sparse_shape,
                                               is_coalesced=True)
        d_add = output_grad if (ctx.has_add_rows and ctx.needs_input_grad[6]) else None
        d_value = None
        if ctx.b_node is not None and ctx.needs_input_grad[8]:
            d_value = _boundary_value_grad(output_grad, ctx.b_node)
        d_edge = None
        if len(ctx.needs_input_grad) > 9 and ctx.needs_input_grad[9]:
            if ctx.weight_blocks is not None:
                d_edge = rspmm_backward_weight_blocks(ctx.csr, relation, input, out, output_grad, ctx.sum, ctx.mul,
                                                      input.shape[1] // ctx.weight_blocks)
            else:
                d_edge = rspmm_backward_weight(ctx.csr, relation, input, out, output_grad, ctx.sum, ctx.mul)
        return d_sparse, d_relation, d_input, None, None, None, d_add, None, d_value, d_edge


# Training, first layer (the caller's `input_is_boundary` promise): the edge gradient of `input` only at the boundary rows
# While a hipGraph is being captured nothing can be read back, so the shortcuts whose precondition is a FINITE relation table
# (first-layer frontier, sparse first layer, dense relation-graph form) take it on trust.  engine.capture_semantics() tests the
# model's parameters once per capture and clears this for a model that holds a non-finite one: the capture then records the
# full kernels, whose NaN propagation is the reference's.
CAPTURE_ASSUMES_FINITE = True


def tables_finite(relation):
    """Eager: one reduction and a host read; under capture: :data:`CAPTURE_ASSUMES_FINITE`."""
    if relation.is_cuda and torch.cuda.is_current_stream_capturing():
        return CAPTURE_ASSUMES_FINITE
    return bool(torch.isfinite(relation).all())


# (see rspmm_backward_boundary_rows).  ULTRA_BOUNDARY_ROWS_BACKWARD=0: the full d_input pass.
BOUNDARY_ROWS_BACKWARD = _env_bool("ULTRA_BOUNDARY_ROWS_BACKWARD", True)


# Training, last layer: the epilogue's backward over the candidate rows' tiles only (see sum_layer).  ULTRA_SPARSE_LAST_LAYER=0: all tiles.
SPARSE_LAST_LAYER_BACKWARD = _env_bool("ULTRA_SPARSE_LAST_LAYER", True)


def candidate_tiles(t_index, n_query, n_node=None):
    """The 32-row tiles of an ``(N, B, 64)`` activation (rows ``(node, query)``, query fastest) that hold the rows
    ``(t_index[b, j], b)`` -- where the gradient of ``hidden[t_index, arange(B)]`` (``ultra/model.py:177-183`` with the
    candidates first, ``model.forward``) is non-zero.  int32 ``(B * K,)``, ascending, ``-1`` padding; static shapes, no host
    synchronisation (capturable).  ``None`` when the sparse backward is switched off."""
    if not SPARSE_LAST_LAYER_BACKWARD:
        return None
    if n_node is not None:
        n_rows = int(n_node) * int(n_query)
        # worth it only where the candidates' tiles are a small part of all tiles (the rest is zero-filled: two passes)
        if t_index.numel() * 8 > (n_rows + 31) // 32:
            return None
        if t_index.is_cuda and t_index.dtype == torch.int64 and t_index.dim() == 2 and n_rows <= (32 << 20):
            t_index = t_index.contiguous()
            out = torch.empty(t_index.numel(), dtype=torch.int32, device=t_index.device)
            _launch(t_index.device, "ultra_candidate_tiles", t_index, t_index.shape[0], t_index.shape[1], int(n_query), n_rows,
                    out)
            return out
    rows = t_index.long() * int(n_query) + torch.arange(t_index.shape[0], device=t_index.device).unsqueeze(-1)
    tiles = torch.div(rows.reshape(-1), 32, rounding_mode="floor")
    ordered, _ = torch.sort(tiles)
    first = torch.ones_like(ordered, dtype=torch.bool)
    first[1:] = ordered[1:] != ordered[:-1]
    # distinct tiles first (ascending), padding behind: a stable sort on the "duplicate" flag keeps the ascending order
    keyed = torch.where(first, ordered, torch.full_like(ordered, torch.iinfo(torch.int64).max))
    keyed, _ = torch.sort(keyed)
    return torch.where(keyed == torch.iinfo(torch.int64).max, torch.full_like(keyed, -1), keyed).to(torch.int32)


class _SumLayerFunction(torch.autograd.Function):
    """One Bellman-Ford layer with summed messages as ONE autograd node:
    ``out = combine(input, rspmm(adjacency, relation, input, sum="add") + boundary)``
    (``ultra/layer.py:298-392`` + the caller's shortcut, ``ultra/model.py:126-127``).  Forward: the rspmm kernel with the
    boundary epilogue, then the fused epilogue kernel.  Backward: the one-pass epilogue backward, then the rspmm
    backward, which adds its edge gradient INTO the epilogue's ``d_input`` inside its row epilogue -- as separate
    autograd nodes the two gradients of ``input`` meet in an extra add pass over an ``(N, B, 64)`` tensor per layer."""

    @staticmethod
    def forward(ctx, csr, relation, input, add_rows, b_node, b_value, mul, weight, bias, ln_weight, ln_bias, ln_eps,
                relu, shortcut, input_is_boundary=False, grad_tiles=None, grad_rows=None):
        shape = input.shape                                      # (N, B, 64)
        flat = input.flatten(1)
        boundary = None if b_node is None else (b_node, b_value.detach())
        # what BOTH first-layer shortcuts need (frontier forward, boundary-rows backward): the caller's promise, a square
        # adjacency, one 64-column block per query, a query count the backward's grid can take -- decided HERE, so that a
        # layer outside those limits takes the full kernels in both directions instead of failing in backward
        first_layer = bool(input_is_boundary and boundary is not None and BOUNDARY_ROWS_BACKWARD
                           and frontier_supported("add", mul, flat.shape[1]) and csr.shape[0] == csr.shape[1]
                           and flat.shape[1] == 64 * b_node.shape[0] and b_node.shape[0] <= 65535)
        sparse = None
        if first_layer and tables_finite(relation):
            # first layer: only the boundary nodes' out-edges carry a message (same bits as the full kernel, finite tables:
            # see rspmm_frontier) -- as in inference; and the epilogue runs on the rows they reach only (first_layer_train_forward)
            # (only where the backward takes d_relation from the boundary nodes' out-edges: every other d_relation kernel multiplies
            # ALL d_update rows, which the sparse backward writes at the listed rows only -- ADVICE r5)
            if (mul == "mul" and grad_tiles is None and not KEEP_PRE_NORM and BOUNDARY_DRELATION
                    and not csr.kernel_order("add", "mul", flat.shape[1])[1]):
                sparse = first_layer_train_forward(csr, relation.detach(), boundary, weight, bias, ln_weight, ln_bias, ln_eps, relu,
                                                   shortcut)
            update = rspmm_frontier(csr, relation.detach(), boundary) if sparse is None else sparse[0].flatten(1)
        else:
            update = rspmm_forward(csr, relation, flat, "add", mul, add_rows=None if add_rows is None else add_rows.flatten(1),
                                   boundary=boundary)
        update = update.view(shape)
        z = torch.empty_like(update) if KEEP_PRE_NORM else None
        if sparse is None:
            out = combine_forward(input, update, weight, bias, ln_weight, ln_bias, ln_eps, relu, shortcut, z_out=z)
        else:
            out = sparse[1].view(shape)
        ctx.first_rows = None if sparse is None else (sparse[2], sparse[3])
        ctx.csr, ctx.mul, ctx.b_node, ctx.has_add = csr, mul, b_node, add_rows is not None
        # first layer: `input` is the boundary, whose gradient is consumed at row (b_node[q], q) only
        ctx.boundary_rows_only = first_layer
        # last layer: the caller's word that the output's gradient is zero outside these 32-row tiles (see sum_layer)
        ctx.grad_tiles = grad_tiles if (grad_tiles is not None and SPARSE_LAST_LAYER_BACKWARD) else None
        # ... and outside these (node, query) rows (candidate_rows): the rspmm backward gathers d_update rows there only
        ctx.grad_rows = grad_rows
        ctx.flags = (float(ln_eps), bool(relu), bool(shortcut))
        ctx.save_for_backward(relation, input, update, weight, bias, ln_weight, ln_bias, z)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        relation, input, update, weight, bias, ln_weight, ln_bias, z = ctx.saved_tensors
        ln_eps, relu, shortcut = ctx.flags
        needs = ctx.needs_input_grad
        tiles = ctx.grad_tiles
        shape = input.shape
        dev = input.device
        grad_out = grad_out.contiguous()
        input_c, update_c = input.contiguous(), update.contiguous()
        rows = input.numel() // 64
        has_ln = ln_weight is not None
        epilogue = _epilogue(weight, bias, ln_weight, ln_bias, ln_eps, relu, shortcut)
        first_rows = getattr(ctx, "first_rows", None)
        # first layer: d_relation from the boundary nodes' out-edges (reads d_update at the rows those edges reach only)?
        drel_boundary = bool(ctx.boundary_rows_only and needs[2] and needs[1] and BOUNDARY_DRELATION and ctx.mul == "mul"
                             and not ctx.csr.kernel_order("add", "mul", update_c[0].numel())[1])
        # The sparse first-layer backward writes d_update at the LISTED rows only.  Any other consumer than the boundary kernels
        # (a knob or switch flipped between forward and backward: the full / masked d_relation kernels multiply every d_update row
        # by the zero input row, and 0 * NaN of uninitialised memory is NaN) gets zeros elsewhere.
        grads = _epilogue_gradients(input_c, update_c, has_ln, zero_update=not (first_rows is None or drel_boundary))
        d_input, d_update, d_weight, d_bias, d_g, d_b = grads
        if first_rows is not None:
            # sparse first layer (csrc/first_layer_train.inc): the listed rows compacted and run through the one-pass backward, every
            # other row's share of d_bias / d_gamma / d_beta from the column sums of grad_out; d_update is written (and later read) at
            # the listed rows only, d_input -- which leaves this node -- is zero elsewhere
            row_list, list_count = first_rows
            ws1 = torch.empty(int(_lib.load().ultra_first_layer_epilogue_backward_workspace(dev.index or 0, row_list.numel())) // 4,
                              dtype=torch.float32, device=dev)
            _launch(dev, "ultra_first_layer_epilogue_backward_f32", input_c, update_c, grad_out, row_list, list_count,
                    row_list.numel(), *epilogue, *grads, ws1, ws1.numel() * 4, rows)
        elif rows <= FUSED_BACKWARD_MAX_ROWS:
            _combine_backward_fused(input_c, update_c, epilogue, grad_out, z, grads, tiles)
        else:
            # beyond the one-pass form's 32-bit offsets: the three-kernel form over every row (`tiles` is a promise of zeros
            # outside them, which the full computation keeps), d_input | d_update into the same tensors
            _, _, d_weight, d_bias, d_g, d_b = _combine_backward_split(input_c, update_c, weight, bias, ln_weight, ln_bias, ln_eps,
                                                                       relu, shortcut, grad_out, grads)
        # the edge gradient accumulates into the epilogue's d_input (same buffer) inside the rspmm backward
        flat_du = d_update.flatten(1)
        if ctx.boundary_rows_only and needs[2]:
            # first layer: the input is zero outside row b_node[q] of block q -- d_relation needs that node's out-edges only
            if drel_boundary:
                d_relation = rspmm_drelation_boundary(ctx.csr, input_c.flatten(1), flat_du, ctx.b_node)
            else:
                _, d_relation = rspmm_backward(ctx.csr, relation, input_c.flatten(1), None, flat_du, "add", ctx.mul,
                                               need_input=False, need_relation=needs[1], active_dst=ctx.grad_rows,
                                               active_src=ctx.b_node)
            d_in = rspmm_backward_boundary_rows(ctx.csr, relation.contiguous(), flat_du, ctx.b_node, d_input.flatten(1), ctx.mul)
        else:
            d_in, d_relation = rspmm_backward(ctx.csr, relation, input_c.flatten(1), None, flat_du, "add", ctx.mul,
                                              need_input=needs[2], need_relation=needs[1],
                                              d_input_add=d_input.flatten(1) if needs[2] else None, active_dst=ctx.grad_rows)
        d_add = d_update if (ctx.has_add and needs[3]) else None
        d_value = None
        if ctx.b_node is not None and needs[5]:
            n_query = ctx.b_node.shape[0]
            d_value = torch.empty(n_query, 64, dtype=torch.float32, device=dev)
            _launch(dev, "ultra_gather_boundary_rows_f32", d_update, ctx.b_node, n_query, d_value)
        return (None, d_relation, d_in.view(shape) if d_in is not None else None, d_add, None, d_value, None,
                d_weight if needs[7] else None, d_bias if needs[8] else None, d_g if (has_ln and needs[9]) else None,
                d_b if (has_ln and needs[10]) else None, None, None, None, None, None, None)


def sum_layer(csr, relation, input, boundary_dense, boundary_sparse, mul, weight, bias, ln_weight=None, ln_bias=None,
              ln_eps=1e-5, relu=True, shortcut=False, input_is_boundary=False, grad_tiles=None, grad_rows=None):
    """A whole sum-aggregation layer for TRAINING as one autograd node (see :class:`_SumLayerFunction`):
    ``[input +] relu(LN(Linear(cat[input, rspmm(csr, relation, input) + boundary])))``.  ``input``: ``(N, B, 64)``;
    ``relation``: ``(R, B * 64)``; the boundary either dense ``(N, B, 64)`` or sparse ``(node int32 (B,), value (B, 64))``.
    ``input_is_boundary``: the caller's word that ``input`` is the boundary (first layer).  ``grad_tiles``: int32 tile ids
    (row ``// 32`` of the ``(N * B, 64)`` view, ascending, ``-1`` padding) -- the caller's word that the gradient arriving at
    this layer's OUTPUT is zero outside those tiles (the last layer, whose output is read at the candidate entities' rows only,
    ``ultra/model.py:177-183``; see :func:`candidate_tiles`): the epilogue's backward then computes those tiles alone.
    ``grad_rows``: the same promise per (node, query) row as bitmaps (:func:`candidate_rows`): the rspmm backward of the layer
    then gathers gradient rows at those destinations only."""
    _check_dense(csr, relation, input.flatten(1))
    b_node, b_value = (None, None) if boundary_sparse is None else boundary_sparse
    add_rows = boundary_dense if boundary_sparse is None else None
    return _SumLayerFunction.apply(csr, relation, input, add_rows, b_node, b_value, mul, weight, bias, ln_weight, ln_bias,
                                   ln_eps, relu, shortcut, input_is_boundary, grad_tiles, grad_rows)


def _check_edge_weight(csr, sparse_leaf, edge_weight, input, block=None):
    """The 2-D form ``(B, E)`` needs ``B`` to divide ``F``; ``block`` (rotate): the query width, ``B * block == F``."""
    if edge_weight is None:
        return
    if sparse_leaf is not None:
        raise RuntimeError("give the edge weights either as the values of a sparse tensor that requires grad or as "
                           "edge_weight, not both")
    batched = (edge_weight.dim() == 2 and edge_weight.shape[0] >= 1 and edge_weight.shape[1] == csr.n_edges
               and input.shape[1] % edge_weight.shape[0] == 0
               and (block is None or input.shape[1] == edge_weight.shape[0] * block))
    if (edge_weight.dtype != torch.float32 or (tuple(edge_weight.shape) != (csr.n_edges,) and not batched)
            or edge_weight.device != input.device):
        raise RuntimeError("edge_weight must be fp32 (%d,) -- one weight per coalesced edge -- or (B, %d) with equal rows, one per "
                           "query block of F / B columns, on %s, got %s %s on %s"
                           % (csr.n_edges, csr.n_edges, input.device, edge_weight.dtype, tuple(edge_weight.shape),
                              edge_weight.device))


def rspmm_sum_plus(sparse, relation, input, add_rows, mul="mul", boundary=None, edge_weight=None):
    """``generalized_rspmm(..., sum="add") + add_rows`` with the addition inside the kernel (differentiable).
    ``boundary = (node, value)`` instead of ``add_rows``: the boundary in sparse form (see :func:`rspmm_forward`),
    differentiable in ``value``.  ``edge_weight``: see :func:`generalized_rspmm`."""
    csr, sparse_leaf = _as_relcsr(sparse)
    _check_dense(csr, relation, input)
    _check_edge_weight(csr, sparse_leaf, edge_weight, input)
    if boundary is not None:
        if add_rows is not None:
            raise RuntimeError("give the boundary either dense (add_rows) or sparse (boundary), not both")
        return _RSPMMFunction.apply(sparse_leaf, relation, input, csr, "add", mul, None, boundary[0], boundary[1], edge_weight)
    return _RSPMMFunction.apply(sparse_leaf, relation, input, csr, "add", mul, add_rows, None, None, edge_weight)


def _rspmm_host(csr, relation, input, sum_op, mul_op):
    """CPU tensors: the raw-CSR dispatcher operator (CPU key of ``torch.ops.ultra_mi.rspmm_fwd``; its Autograd key
    reaches ``rspmm_bwd``'s CPU kernel).  Every row strictly sequentially in (src, rel) order: the reference's order."""
    row_ptr, src, rel, w = csr.csr_arrays
    return _torch_ext.load().rspmm_fwd(row_ptr, src, rel, w, relation, input, sum_op, mul_op)


def generalized_rspmm(sparse, relation, input, sum="add", mul="mul", edge_weight=None):
    r"""Generalized relational sparse-dense product (drop-in for torchdrug's function of the same name).

    .. math::  out_{v,:} = \bigoplus_{(v, u, r) \in sparse} w_{vur} \cdot (relation_{r,:} \otimes input_{u,:})

    with :math:`\oplus` = ``sum`` in {add, min, max} and :math:`\otimes` = ``mul`` in {mul, add}.

    Parameters: ``sparse`` -- 3-D sparse COO tensor ``(N_dst, N_src, R)`` (any order, duplicates are merged by
    summing their values, as ``coalesce()`` does) or a :class:`RelCSR`; ``relation`` -- ``(R, F)`` fp32;
    ``input`` -- ``(N_src, F)`` fp32 (a 1-D ``input`` is treated as ``(N_src, 1)``).  Returns ``(N_dst, F)``.
    ``edge_weight`` (MI355X only; an extension): fp32 ``(n_edges,)`` weights of the COALESCED edges in forward-plan order
    (``RelCSR.dst / src / rel_id``) used instead of the adjacency's own; differentiable -- its gradient is
    :func:`rspmm_backward_weight` (duplicate triples of a COO input share one coalesced edge, ``RelCSR.edge_of_input``).
    A 2-D ``edge_weight`` ``(B, n_edges)`` is one weight vector per query block of ``F / B`` columns; PRECONDITION: every row
    equals the coalesced weights in use.  The forward runs on row 0 (the bits of the 1-D form) and the gradient is the ``(B,
    n_edges)`` result of :func:`rspmm_backward_weight_blocks` (``TransferNBFNet.edge_gradients_batch``).
    """
    _ops(sum, mul)
    csr, sparse_leaf = _as_relcsr(sparse)
    squeeze = input.dim() == 1
    if squeeze:
        input = input.unsqueeze(-1)
        if relation.dim() == 1:
            relation = relation.unsqueeze(-1)
    _check_dense(csr, relation, input, require_hip=False)
    _check_edge_weight(csr, sparse_leaf, edge_weight, input)
    if not input.is_cuda:
        if edge_weight is not None:
            raise RuntimeError("generalized_rspmm: edge_weight runs on an MI355X (HIP) device only")
        if sparse_leaf is not None:
            raise RuntimeError("generalized_rspmm on CPU tensors has no gradient for the sparse values "
                               "(the reference takes its scatter path then, ultra/layer.py:299)")
        out = _rspmm_host(csr, relation, input, *_ops(sum, mul))
    else:
        out = _RSPMMFunction.apply(sparse_leaf, relation, input, csr, sum, mul, None, None, None, edge_weight)
    return out.squeeze(-1) if squeeze else out


def _rotate_ops(csr, relation, input, sum, block, require_hip):
    """Validates a rotate call: ``(sum_op, block)``.  Unknown ``sum`` names raise ``ValueError``; a ``block`` that is not even,
    positive and a divisor of ``F`` raises ``RuntimeError`` (a shape problem)."""
    if sum not in _lib.SUM_OPS:
        raise ValueError("Can't find a rotate rspmm operator for sum=`%s` (expected add, min or max)" % sum)
    _check_dense(csr, relation, input, require_hip=require_hip)
    block, F = int(block), input.shape[1]
    if block <= 0 or block % 2 or F % block:
        raise RuntimeError("rotate messages need an even block width that divides F = %d, got block = %d" % (F, block))
    return _lib.SUM_OPS[sum], block


def rotate_rspmm_forward(csr, relation, input, sum="add", block=64, add_rows=None, boundary=None):
    """Forward of :func:`rotate_rspmm` without autograd (``ultra_rspmm_rotate_forward_f32``).  ``add_rows`` / ``boundary =
    (node, value)``: the epilogue ``(+ | min | max) boundary`` inside the kernel, as in :func:`rspmm_forward`."""
    sum_op, block = _rotate_ops(csr, relation, input, sum, block, True)
    relation, input = relation.contiguous(), input.contiguous()
    F = input.shape[1]
    out = torch.empty(csr.shape[0], F, dtype=torch.float32, device=input.device)
    add_rows, b_node, b_value = _check_boundary_epilogue(out, add_rows, boundary, block)
    if out.numel() == 0:
        return out
    seg = csr.fwd
    if _torch_ext.binding() == "torch":
        return _torch_ext.load().rspmm_rotate_plan_fwd(seg.plan_tensor, relation, input, add_rows, b_node, b_value, csr.shape[1],
                                                       block, sum_op)
    ws, ws_bytes = _workspace(seg, F, input.device)
    _launch(input.device, "ultra_rspmm_rotate_forward_f32", seg.pointer, relation, input, add_rows, b_node, b_value, out, ws,
            ws_bytes, csr.shape[1], csr.shape[2], F, block, sum_op)
    return out


def rotate_rspmm_backward(csr, relation, input, output, output_grad, sum="add", block=64, need_input=True, need_relation=True):
    """``(d_input, d_relation)`` of :func:`rotate_rspmm_forward` (``ultra_rspmm_rotate_backward_f32``); ``output`` is the forward
    result without the epilogue (read for min / max only)."""
    sum_op, block = _rotate_ops(csr, relation, input, sum, block, True)
    relation, input, output_grad = relation.contiguous(), input.contiguous(), output_grad.contiguous()
    output = output.contiguous() if output is not None else None
    F, dev = input.shape[1], input.device
    if not need_input and not need_relation:
        return None, None
    by_src = csr.by_src if need_input else None
    by_rel = csr.by_rel if need_relation else None
    if _torch_ext.binding() == "torch":
        d_input, d_relation = _torch_ext.load().rspmm_rotate_plan_bwd(
            by_src.plan_tensor if by_src is not None else None, by_rel.plan_tensor if by_rel is not None else None,
            relation, input, output, output_grad, csr.shape[1], csr.shape[0], block, sum_op)
        return (d_input if need_input else None), (d_relation if need_relation else None)
    d_input = torch.empty_like(input) if need_input else None
    d_relation = torch.empty_like(relation) if need_relation else None
    ws, ws_bytes = _backward_workspace(by_src, by_rel, F, dev)
    _launch(dev, "ultra_rspmm_rotate_backward_f32", _plan(by_src), _plan(by_rel), relation, input, output, output_grad, d_input,
            d_relation, ws, ws_bytes, csr.shape[1], csr.shape[0], csr.shape[2], F, block, sum_op)
    return d_input, d_relation


def rotate_rspmm_backward_weight(csr, relation, input, output, output_grad, sum="add", block=64):
    """d(weights) of the coalesced edges (forward-plan order) of :func:`rotate_rspmm_forward`
    (``ultra_rspmm_rotate_backward_weight_f32``); ``output`` is the forward result without the epilogue (read for min / max only)."""
    sum_op, block = _rotate_ops(csr, relation, input, sum, block, True)
    relation, input, output_grad = relation.contiguous(), input.contiguous(), output_grad.contiguous()
    output = output.contiguous() if output is not None else None
    if _torch_ext.binding() == "torch":
        return _torch_ext.load().rspmm_rotate_plan_bwd_weight(csr.fwd.plan_tensor, relation, input, output, output_grad, block,
                                                              sum_op)
    d_w = torch.empty(csr.n_edges, dtype=torch.float32, device=input.device)
    if csr.n_edges == 0:
        return d_w
    _launch(input.device, "ultra_rspmm_rotate_backward_weight_f32", csr.fwd.pointer, relation, input, output, output_grad, d_w,
            csr.shape[2], input.shape[1], block, sum_op)
    return d_w


def rotate_rspmm_backward_weight_blocks(csr, relation, input, output, output_grad, sum="add", block=64):
    """:func:`rotate_rspmm_backward_weight` per query block: fp32 ``(F / block, n_edges)``, row ``b`` the gradient over the pairs
    of query block ``b`` alone -- bit for bit :func:`rotate_rspmm_backward_weight` on a contiguous copy of that block's columns
    (``ultra_rspmm_rotate_backward_weight_blocks_f32``)."""
    sum_op, block = _rotate_ops(csr, relation, input, sum, block, True)
    relation, input, output_grad = relation.contiguous(), input.contiguous(), output_grad.contiguous()
    output = output.contiguous() if output is not None else None
    d_w = torch.empty(input.shape[1] // block, csr.n_edges, dtype=torch.float32, device=input.device)   # written completely
    if csr.n_edges == 0:
        return d_w
    _launch(input.device, "ultra_rspmm_rotate_backward_weight_blocks_f32", csr.fwd.pointer, relation, input, output, output_grad,
            d_w, csr.shape[2], input.shape[1], block, sum_op)
    return d_w


class _RotateFunction(torch.autograd.Function):
    """Autograd of :func:`rotate_rspmm` on device tensors; ``add_rows`` / ``(b_node, b_value)`` / ``edge_weight`` as in
    :class:`_RSPMMFunction`."""

    @staticmethod
    def forward(ctx, relation, input, csr, sum, block, add_rows=None, b_node=None, b_value=None, edge_weight=None):
        # edge_weight: fp32 (csr.n_edges,) weights of the COALESCED edges (forward-plan order) that replace csr's own; its
        # gradient is rotate_rspmm_backward_weight's d_w
        # (B, E): one weight vector per query block, rows equal; the gradient is rotate_rspmm_backward_weight_blocks' (B, E)
        ctx.weight_blocks = None
        if edge_weight is not None:
            if edge_weight.dim() == 2:
                ctx.weight_blocks = edge_weight.shape[0]
                csr = csr.with_coalesced_weights(edge_weight.detach()[0])
            else:
                csr = csr.with_coalesced_weights(edge_weight.detach())
        boundary = None if b_node is None else (b_node, b_value.detach())
        out = rotate_rspmm_forward(csr, relation, input, sum, block, add_rows=add_rows, boundary=boundary)
        ctx.csr, ctx.sum, ctx.block = csr, sum, block
        ctx.has_add_rows, ctx.b_node = add_rows is not None, b_node
        ctx.save_for_backward(relation, input, out if sum != "add" else None)
        return out

    @staticmethod
    def backward(ctx, output_grad):
        relation, input, out = ctx.saved_tensors
        d_input, d_relation = rotate_rspmm_backward(ctx.csr, relation, input, out, output_grad, ctx.sum, ctx.block,
                                                    need_input=ctx.needs_input_grad[1], need_relation=ctx.needs_input_grad[0])
        d_add = output_grad if (ctx.has_add_rows and ctx.needs_input_grad[5]) else None
        d_value = None
        if ctx.b_node is not None and ctx.needs_input_grad[7]:
            d_value = _boundary_value_grad(output_grad, ctx.b_node)
        d_edge = None
        if len(ctx.needs_input_grad) > 8 and ctx.needs_input_grad[8]:
            if ctx.weight_blocks is not None:
                d_edge = rotate_rspmm_backward_weight_blocks(ctx.csr, relation, input, out, output_grad, ctx.sum, ctx.block)
            else:
                d_edge = rotate_rspmm_backward_weight(ctx.csr, relation, input, out, output_grad, ctx.sum, ctx.block)
        return d_relation, d_input, None, None, None, d_add, None, d_value, d_edge


def rotate_rspmm(sparse, relation, input, sum="add", block=64, add_rows=None, boundary=None, edge_weight=None):
    r"""Relational sparse-dense product with RotatE messages (the ``message_func="rotate"`` layers without an ``(E, F)`` tensor).

    .. math::  out_{v,:} = \bigoplus_{(v, u, r) \in sparse} w_{vur} \cdot (input_{u,:} \circledast relation_{r,:})

    where every query block of ``block`` columns holds ``block / 2`` complex numbers, real parts first, and
    :math:`\circledast` is their element-wise complex product (``layer.message``'s rotate branch); :math:`\oplus` = ``sum``
    in {add, min, max}.  ``sparse``: as in :func:`generalized_rspmm` (duplicate triples merged by summing their weights);
    differentiable in ``relation`` and ``input``, on CPU tensors (``torch.ops.ultra_mi.rspmm_rotate_fwd``, every row strictly
    sequentially) or MI355X tensors (the plan kernels of ``csrc/rotate.inc``).  The sparse values may not require grad.
    Extension (device tensors, ``sum="add"``): ``add_rows`` / ``boundary = (node, value)`` -- the epilogue ``+ boundary`` inside
    the kernel, differentiable in ``add_rows`` / ``value`` (see :func:`rspmm_forward`).  ``edge_weight`` (MI355X only): fp32
    ``(n_edges,)`` weights of the COALESCED edges in forward-plan order used instead of the adjacency's own, as in
    :func:`generalized_rspmm`; differentiable -- its gradient is :func:`rotate_rspmm_backward_weight` (2-D ``(F / block,
    n_edges)`` with equal rows: :func:`rotate_rspmm_backward_weight_blocks`, as there)."""
    if sum not in _lib.SUM_OPS:
        raise ValueError("Can't find a rotate rspmm operator for sum=`%s` (expected add, min or max)" % sum)
    csr, sparse_leaf = _as_relcsr(sparse)
    if sparse_leaf is not None:
        raise RuntimeError("rotate_rspmm has no gradient for the sparse values (the reference takes its message + "
                           "aggregate path then, ultra/layer.py:299)")
    if (add_rows is not None or boundary is not None) and sum != "add":
        raise RuntimeError("rotate_rspmm: the fused boundary is for sum aggregation (max: torch.max after the call)")
    sum_op, block = _rotate_ops(csr, relation, input, sum, block, False)
    _check_edge_weight(csr, sparse_leaf, edge_weight, input, block)
    if not input.is_cuda:
        if edge_weight is not None:
            raise RuntimeError("rotate_rspmm: edge_weight runs on an MI355X (HIP) device only")
        if add_rows is not None or boundary is not None:
            raise RuntimeError("rotate_rspmm: the fused boundary runs on an MI355X (HIP) device only")
        row_ptr, src, rel, w = csr.csr_arrays
        return _torch_ext.load().rspmm_rotate_fwd(row_ptr, src, rel, w, relation, input, block, sum_op)
    b_node, b_value = boundary if boundary is not None else (None, None)
    return _RotateFunction.apply(relation, input, csr, sum, block, add_rows, b_node, b_value, edge_weight)


BEAM_MAX = 32        # beams per node the beam-search step takes (csrc/beam_search.hip: register top-K of at most 32)


def beam_search_step(row_ptr, src, edge_grad, input, tail):
    """One layer of the path beam search of :meth:`TransferNBFNet.visualize` (``torch.ops.ultra_mi.beam_search_step``: the
    HIP kernel of ``csrc/beam_search.hip`` for device tensors, its CPU twin for host tensors -- same bits).

    ``row_ptr`` int32 ``(N + 1,)`` / ``src`` int32 ``(E,)``: the coalesced dst-CSR (:attr:`RelCSR.csr_arrays`); ``edge_grad``
    fp32 ``(E,)``: this layer's edge gradients in the same order; ``input`` fp32 ``(N, K)``: the previous layer's beams
    (``-inf`` = empty); ``tail``: the explained triple's tail, whose out-edges are masked.  Returns ``(distance fp32 (N, K),
    back_edge int32 (N, K), back_rank int32 (N, K))`` -- semantics in DESIGN.md ("Explaining a prediction")."""
    if input.dim() != 2 or not 1 <= input.shape[1] <= BEAM_MAX:
        raise ValueError("beam_search_step: input must be (N, K) with 1 <= K <= %d, got %s" % (BEAM_MAX, tuple(input.shape)))
    return _torch_ext.load().beam_search_step(row_ptr, src, edge_grad, input, int(tail))


def beam_search_step_batch(row_ptr, src, edge_grad, input, tails):
    """:func:`beam_search_step` for ``B`` queries over one graph in one launch (``torch.ops.ultra_mi.beam_search_step_batch``):
    ``edge_grad`` fp32 ``(B, E)``, ``input`` fp32 ``(B, N, K)``, ``tails`` int32 ``(B,)`` on the tensors' device (never read on
    the host beyond the one validity check).  Returns ``(distance, back_edge, back_rank)``, each ``(B, N, K)``; query ``b``'s
    slices are exactly :func:`beam_search_step` on ``(edge_grad[b], input[b], tails[b])``."""
    if input.dim() != 3 or input.shape[0] < 1 or not 1 <= input.shape[2] <= BEAM_MAX:
        raise ValueError("beam_search_step_batch: input must be (B, N, K) with B >= 1 and 1 <= K <= %d, got %s"
                         % (BEAM_MAX, tuple(input.shape)))
    return _torch_ext.load().beam_search_step_batch(row_ptr, src, edge_grad, input, tails)


HOP_ITERS = 100      # the reference's num_iters (ultra/model.py:302): the cap is part of the definition


def _hop_csr(csr):
    if isinstance(csr, RelCSR):
        row_ptr, src, _, w = csr.csr_arrays
        return row_ptr, src, w
    if isinstance(csr, (tuple, list)) and len(csr) == 3:
        return tuple(csr)
    raise TypeError("hop_distance: csr must be a RelCSR or a (row_ptr, src, w) triple, got %s" % type(csr).__name__)


def hop_distance(csr, sources, num_iters=HOP_ITERS, targets=None, poll=None):
    """Hop distances from many sources at once (``torch.ops.ultra_mi.hop_distance``: the bit-parallel multi-source BFS of
    ``csrc/hop_distance.hip`` for device tensors, a queue BFS on the host for CPU tensors -- the same integers; the contract is
    in ``include/ultra_rspmm.h``).

    ``csr``: a :class:`RelCSR` or ``(row_ptr int32 (N + 1,), src int32 (E,), w fp32 (E,) | None)``, the coalesced dst-CSR
    (:attr:`RelCSR.csr_arrays` without its relation column); ``sources`` int64 ``(B,)``.  Returns int32 ``(N, B)``:
    ``dist[v, b]`` = edges on a shortest path ``sources[b] -> v`` along the edge direction if that is ``<= num_iters``, else
    ``N`` (unreachable, or farther than the cap: ``_get_shortest_distance``, ``ultra/model.py:302-314``).  An edge whose
    coalesced weight is exactly 0 does not exist (``Graph.reweighted`` / ``Graph.without_triples`` remove edges that way); other
    weights are ignored.  With ``targets`` int64 ``(B, K)`` the result is int32 ``(B, K)``, ``out[b, j] = dist[targets[b, j],
    b]``, computed without the matrix.  ``poll`` (device only): ``True`` stops each block of 64 sources at the first level that
    adds nothing, by one small host read per level; ``False`` enqueues exactly ``num_iters`` levels and reads nothing;
    ``None``: poll unless the stream is being captured.  The result does not depend on it.  ``ULTRA_BINDING=ctypes`` and an explicit
    ``poll=False`` (an argument of the C entry, not of the operator) go through the C ABI directly."""
    row_ptr, src, w = _hop_csr(csr)
    sources = torch.as_tensor(sources, device=row_ptr.device) if not isinstance(sources, torch.Tensor) else sources
    num_iters = int(num_iters)
    if not row_ptr.is_cuda or (_torch_ext.binding() == "torch" and poll is not False):
        return _torch_ext.load().hop_distance(row_ptr, src, w, sources, num_iters, targets)
    # the C ABI through _launch: the operator's checks, restated (values are read only outside a capture)
    capturing = torch.cuda.is_current_stream_capturing()
    given = [t for t in (row_ptr, src, w, sources, targets) if t is not None]
    if any(not isinstance(t, torch.Tensor) or t.device != row_ptr.device for t in given):
        raise RuntimeError("hop_distance: all tensors must share a device")
    if num_iters < 0:
        raise ValueError("hop_distance: num_iters must not be negative, got %d" % num_iters)
    if row_ptr.dtype != torch.int32 or src.dtype != torch.int32 or row_ptr.dim() != 1 or src.dim() != 1 or not row_ptr.numel():
        raise RuntimeError("hop_distance: row_ptr (N + 1,) and src (E,) must be int32")
    n_node, n_edges = row_ptr.numel() - 1, src.numel()
    if w is not None and (w.dtype != torch.float32 or tuple(w.shape) != (n_edges,)):
        raise RuntimeError("hop_distance: w must be fp32 (E,)")
    if sources.dtype != torch.int64 or sources.dim() != 1:
        raise RuntimeError("hop_distance: sources must be int64 (B,)")
    n_source = sources.numel()
    if targets is not None and (targets.dtype != torch.int64 or targets.dim() != 2 or targets.shape[0] != n_source):
        raise RuntimeError("hop_distance: targets must be int64 (B, K), got %s %s" % (targets.dtype, tuple(targets.shape)))
    if not capturing:
        for name, ids in (("sources", sources), ("targets", targets)):
            if ids is not None and ids.numel() and (int(ids.min()) < 0 or int(ids.max()) >= n_node):
                raise RuntimeError("hop_distance: %s outside [0, %d)" % (name, n_node))
        rp = row_ptr.long()
        bad = int(rp[0]) != 0 or int(rp[-1]) != n_edges or bool((rp[1:] < rp[:-1]).any())
        if bad or (n_edges and (int(src.min()) < 0 or int(src.max()) >= n_node)):
            raise RuntimeError("hop_distance: malformed CSR (row_ptr must run from 0 to E without decreasing, src must lie in "
                               "[0, N))")
    per_source = targets.shape[1] if targets is not None else 0
    out = torch.empty((n_source, per_source) if targets is not None else (n_node, n_source), dtype=torch.int32,
                      device=row_ptr.device)
    if out.numel() == 0:
        return out
    ws_bytes = int(_lib.load().ultra_hop_distance_workspace(n_node))
    ws = torch.empty((ws_bytes + 7) // 8, dtype=torch.int64, device=row_ptr.device)
    poll = (not capturing) if poll is None else bool(poll)
    _launch(row_ptr.device, "ultra_hop_distance", row_ptr.contiguous(), src.contiguous() if n_edges else None,
            w.contiguous() if (w is not None and n_edges) else None, n_node, n_edges, sources.contiguous(), n_source, num_iters,
            targets.contiguous() if targets is not None else None, per_source, None if targets is not None else out,
            out if targets is not None else None, int(poll), ws, ws_bytes)
    return out


# ---------------------------------------------------------------------------------------------------- exact (crisp) sets
# A batch of Q entity sets over N entities, packed: int64 ``bits (N, W)``, ``W = ceil(Q / 64)``; bit ``q % 64`` of
# ``bits[v, q // 64]`` says "v is in set q" (``include/ultra_rspmm.h``).  Bits of columns ``>= Q`` are
# always 0.  Intersection and union are ``&`` and ``|``; a complement is ``~bits & column_mask(Q)``.
SET_WORD = 64
SET_PROJECT_SEGMENT = 1024  # edges of a row its lane group walks in ultra_sets_project; the rest goes to the tail launch (kSeg)
SET_RANK_TARGETS = 256      # targets a block of ultra_sets_rank takes at once (kTargets of csrc/query_exact.hip)
SET_RANK_TILE = 1024        # entities per LDS tile of ultra_sets_rank (kTile)


def _bit_values(device):
    return torch.ones(SET_WORD, dtype=torch.int64, device=device) << torch.arange(SET_WORD, device=device)


def column_mask(n_query, device=None):
    """int64 ``(W,)``: the bits of the columns ``< n_query`` of every word -- what a complement is ANDed with."""
    n_query = int(n_query)
    words = (n_query + SET_WORD - 1) // SET_WORD
    mask = torch.full((words,), -1, dtype=torch.int64, device=device)
    if n_query % SET_WORD:
        mask[-1] = (1 << (n_query % SET_WORD)) - 1
    return mask


def pack_sets(member):
    """bool ``(Q, N)`` memberships as packed sets int64 ``(N, W)``."""
    if member.dim() != 2 or member.dtype != torch.bool:
        raise RuntimeError("pack_sets: member must be bool (Q, N), got %s %s" % (member.dtype, tuple(member.shape)))
    n_query, n_node = member.shape
    words = (n_query + SET_WORD - 1) // SET_WORD
    padded = torch.zeros(n_node, words * SET_WORD, dtype=torch.int64, device=member.device)
    padded[:, :n_query] = member.t()
    # distinct powers of two: the int64 sum is the OR (bit 63 is the sign bit, and wraps to it exactly)
    return (padded.view(n_node, words, SET_WORD) * _bit_values(member.device)).sum(dim=2)


def unpack_sets(bits, n_query):
    """Packed sets int64 ``(N, W)`` as bool ``(Q, N)``."""
    n_query = int(n_query)
    if bits.dim() != 2 or bits.dtype != torch.int64 or bits.shape[1] != (n_query + SET_WORD - 1) // SET_WORD:
        raise RuntimeError("unpack_sets: %d sets are int64 (N, %d), got %s %s"
                           % (n_query, (n_query + SET_WORD - 1) // SET_WORD, bits.dtype, tuple(bits.shape)))
    each = (bits.unsqueeze(-1) >> torch.arange(SET_WORD, device=bits.device)) & 1
    return each.view(bits.shape[0], -1)[:, :n_query].t().bool()


def seed_sets(nodes, n_node):
    """One-hot packed sets: set ``q`` = ``{nodes[q]}``, ``nodes`` int64 ``(Q,)`` in ``[0, n_node)``.  Nodes may repeat across
    queries: every (word, bit) is added at most once, so the accumulate-add of distinct powers of two is the OR, exactly."""
    if nodes.dim() != 1 or nodes.dtype != torch.int64:
        raise RuntimeError("seed_sets: nodes must be int64 (Q,), got %s %s" % (nodes.dtype, tuple(nodes.shape)))
    n_query, n_node = nodes.numel(), int(n_node)
    words = (n_query + SET_WORD - 1) // SET_WORD
    bits = torch.zeros(n_node * words, dtype=torch.int64, device=nodes.device)
    if n_query:
        if not (nodes.is_cuda and torch.cuda.is_current_stream_capturing()) and (int(nodes.min()) < 0 or int(nodes.max()) >= n_node):
            raise RuntimeError("seed_sets: nodes outside [0, %d)" % n_node)
        q = torch.arange(n_query, device=nodes.device)
        bits.index_add_(0, nodes * words + q // SET_WORD, _bit_values(nodes.device)[q % SET_WORD])
    return bits.view(n_node, words)


def _exact_csr(csr, n_relation):
    if isinstance(csr, RelCSR):
        return csr.csr_arrays + (csr.shape[2],)
    if isinstance(csr, (tuple, list)) and len(csr) == 4 and n_relation is not None:
        return tuple(csr) + (int(n_relation),)
    raise TypeError("project_sets_exact: csr must be a RelCSR, or a (row_ptr, src, rel, w) tuple with n_relation given, got %s"
                    % type(csr).__name__)


def dense_project_sets_exact(csr, bits, relation, n_relation=None):
    """:func:`project_sets_exact` in torch ops (the host twin of the same definition): a ``(Q, E)`` boolean per call."""
    row_ptr, src, rel, w, n_rel = _exact_csr(csr, n_relation)
    n_node, n_query = row_ptr.numel() - 1, relation.numel()
    member = unpack_sets(bits, n_query)                                                  # (Q, N)
    dst = torch.repeat_interleave(torch.arange(n_node, device=row_ptr.device), row_ptr.long().diff())
    passes = member[:, src.long()] & (rel.long().unsqueeze(0) == relation.unsqueeze(1))  # (Q, E)
    if w is not None:
        passes = passes & (w != 0).unsqueeze(0)
    reached = torch.zeros(n_query, n_node, dtype=torch.int32, device=row_ptr.device)
    reached.index_add_(1, dst, passes.to(torch.int32))
    return pack_sets(reached > 0)


def project_sets_exact(csr, bits, relation, n_relation=None):
    """One relation projection of packed crisp sets (``ultra_sets_project``, ``csrc/query_exact.hip``; the contract is in
    ``include/ultra_rspmm.h``).

    ``csr``: a :class:`RelCSR`, or ``(row_ptr int32 (N + 1,), src int32 (E,), rel int32 (E,), w fp32 (E,) | None)`` with
    ``n_relation`` -- the coalesced dst-CSR of a graph with inverse edges (:attr:`RelCSR.csr_arrays`); ``bits`` int64 ``(N,
    W)``; ``relation`` int64 ``(Q,)`` in ``[0, n_relation)``.  Returns int64 ``(N, W)``: entity ``v`` is in set ``q`` of the
    result iff some edge ``u -> v`` of relation ``relation[q]`` and non-zero weight leaves a member ``u`` of set ``q``.  Bits of
    columns ``>= Q`` come out 0 whatever ``bits`` holds there.  Two small launches, one pull over the CSR and one launch for the
    tails of rows longer than 1024 edges; the values are not read while the stream is being captured.  CPU tensors take :func:`dense_project_sets_exact`."""
    row_ptr, src, rel, w, n_rel = _exact_csr(csr, n_relation)
    given = [t for t in (row_ptr, src, rel, w, bits, relation) if t is not None]
    if any(not isinstance(t, torch.Tensor) or t.device != row_ptr.device for t in given):
        raise RuntimeError("project_sets_exact: all tensors must share a device")
    if (row_ptr.dtype != torch.int32 or src.dtype != torch.int32 or rel.dtype != torch.int32 or row_ptr.dim() != 1
            or src.dim() != 1 or not row_ptr.numel() or rel.shape != src.shape):
        raise RuntimeError("project_sets_exact: row_ptr (N + 1,), src (E,) and rel (E,) must be int32")
    n_node, n_edges = row_ptr.numel() - 1, src.numel()
    if w is not None and (w.dtype != torch.float32 or tuple(w.shape) != (n_edges,)):
        raise RuntimeError("project_sets_exact: w must be fp32 (E,)")
    if relation.dtype != torch.int64 or relation.dim() != 1:
        raise RuntimeError("project_sets_exact: relation must be int64 (Q,)")
    n_query = relation.numel()
    words = (n_query + SET_WORD - 1) // SET_WORD
    if bits.dtype != torch.int64 or tuple(bits.shape) != (n_node, words):
        raise RuntimeError("project_sets_exact: %d sets over %d entities are int64 (%d, %d), got %s %s"
                           % (n_query, n_node, n_node, words, bits.dtype, tuple(bits.shape)))
    if n_rel < 0:
        raise RuntimeError("project_sets_exact: n_relation must not be negative, got %d" % n_rel)
    capturing = row_ptr.is_cuda and torch.cuda.is_current_stream_capturing()
    if not capturing and n_query and (int(relation.min()) < 0 or int(relation.max()) >= n_rel):
        raise RuntimeError("project_sets_exact: relations outside [0, %d)" % n_rel)
    if not row_ptr.is_cuda:
        return dense_project_sets_exact((row_ptr, src, rel, w), bits, relation, n_rel)
    out = torch.empty(n_node, words, dtype=torch.int64, device=row_ptr.device)
    if out.numel() == 0:
        return out
    ws_bytes = int(_lib.load().ultra_sets_project_workspace(n_rel, n_query))
    ws = torch.empty(max(ws_bytes // 8, 1), dtype=torch.int64, device=row_ptr.device)
    _launch(row_ptr.device, "ultra_sets_project", row_ptr.contiguous(), src.contiguous() if n_edges else None,
            rel.contiguous() if n_edges else None, w.contiguous() if (w is not None and n_edges) else None, n_node, n_edges,
            n_rel, bits.contiguous(), relation.contiguous(), n_query, out, ws, ws_bytes)
    return out


def dense_set_ranks(pred, excluded_bits, target_ptr, target_entity):
    """:func:`set_ranks` in torch ops (the host twin of the same definition): a ``(T, N)`` boolean per call."""
    n_query, n_node = pred.shape
    query = torch.repeat_interleave(torch.arange(n_query, device=pred.device), target_ptr.diff())
    counted = pred[query] >= pred[query, target_entity].unsqueeze(1)                     # (T, N); false for a NaN
    if excluded_bits is not None:
        counted = counted & ~unpack_sets(excluded_bits, n_query)[query]
    return 1 + counted.sum(dim=1)


def set_ranks(pred, excluded_bits, target_ptr, target_entity):
    """Filtered ranks of many targets per query (``ultra_sets_rank``, ``csrc/query_exact.hip``; the contract is in
    ``include/ultra_rspmm.h``): ``pred`` fp32 ``(Q, N)`` (the rows may be strided, not overlap), ``excluded_bits`` int64 ``(N,
    W)`` packed sets or ``None``, ``target_ptr`` int64 ``(Q + 1,)`` ascending from 0 to ``T``, ``target_entity`` int64 ``(T,)``:
    the targets of query ``q`` are ``target_entity[target_ptr[q]:target_ptr[q + 1]]``.  Returns int64 ``(T,)``,
    ``rank[t] = 1 + #{v : v not excluded for q_t and pred[q_t, v] >= pred[q_t, target_entity[t]]}``: pessimistic on ties, false for
    NaN (``ultra/task.py:311``), and a target that is not excluded counts itself.  One launch, no ``(T, N)`` temporary; the
    values are not read while the stream is being captured.  CPU tensors take :func:`dense_set_ranks`."""
    if pred.dim() != 2 or pred.dtype != torch.float32 or (pred.shape[1] > 1 and pred.stride(1) != 1):
        raise RuntimeError("set_ranks: pred must be fp32 (Q, N) with contiguous rows")
    n_query, n_node = pred.shape
    if n_query > 1 and pred.stride(0) < n_node:
        raise RuntimeError("set_ranks: the rows of pred overlap")
    words = (n_query + SET_WORD - 1) // SET_WORD
    if excluded_bits is not None and (excluded_bits.dtype != torch.int64 or tuple(excluded_bits.shape) != (n_node, words)
                                      or excluded_bits.device != pred.device):
        raise RuntimeError("set_ranks: excluded_bits must be int64 (%d, %d) on %s" % (n_node, words, pred.device))
    if (target_ptr.dtype != torch.int64 or tuple(target_ptr.shape) != (n_query + 1,) or target_entity.dtype != torch.int64
            or target_entity.dim() != 1 or target_ptr.device != pred.device or target_entity.device != pred.device):
        raise RuntimeError("set_ranks: target_ptr must be int64 (%d,) and target_entity int64 (T,) on %s"
                           % (n_query + 1, pred.device))
    n_target = target_entity.numel()
    capturing = pred.is_cuda and torch.cuda.is_current_stream_capturing()
    if not capturing:
        if int(target_ptr[0]) != 0 or int(target_ptr[-1]) != n_target or bool((target_ptr[1:] < target_ptr[:-1]).any()):
            raise RuntimeError("set_ranks: target_ptr must run from 0 to T = %d without decreasing" % n_target)
        if n_target and (int(target_entity.min()) < 0 or int(target_entity.max()) >= n_node):
            raise RuntimeError("set_ranks: targets outside [0, %d)" % n_node)
    if not pred.is_cuda:
        return dense_set_ranks(pred, excluded_bits, target_ptr, target_entity)
    rank = torch.empty(n_target, dtype=torch.int64, device=pred.device)
    if n_target:
        _launch(pred.device, "ultra_sets_rank", pred, n_query, n_node, pred.stride(0) if n_query > 1 else n_node,
                None if excluded_bits is None else excluded_bits.contiguous(), target_ptr.contiguous(),
                target_entity.contiguous(), n_target, rank)
    return rank

"""ctypes binding of ``libultra_rspmm.so`` (C ABI: ``include/ultra_rspmm.h``).

The shared object is the product: there is no Python, PyTorch or CPU fallback behind it.  If it is missing or
cannot be loaded every operator of this package raises immediately.
"""
import ctypes
import os

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
# ULTRA_RSPMM_LIB: load another build of the same ABI (kernel A/B runs, tools/kbench.py)
LIB_PATH = os.environ.get("ULTRA_RSPMM_LIB") or os.path.join(_HERE, "libultra_rspmm.so")
ABI_VERSION = 8

SUM_OPS = {"add": 0, "min": 1, "max": 2}
MUL_OPS = {"mul": 0, "add": 1}


class UltraSegments(ctypes.Structure):
    """``struct ultra_segments`` of include/ultra_rspmm.h (device pointers as integers).  A new instance carries the fence
    of ABI 8: ``struct_bytes`` = the size of THIS declaration, ``abi_version`` = the version this binding was written for;
    the library refuses a struct whose two leading fields are not its own (``ULTRA_ERR_ABI``)."""
    _fields_ = [
        ("struct_bytes", ctypes.c_uint32),
        ("abi_version", ctypes.c_uint32),
        ("n_rows", ctypes.c_int64),
        ("n_edges", ctypes.c_int64),
        ("row", ctypes.c_void_p),
        ("node_a", ctypes.c_void_p),
        ("node_b", ctypes.c_void_p),
        ("rel", ctypes.c_void_p),
        ("weight", ctypes.c_void_p),
        ("n_chunks", ctypes.c_int64),
        ("chunks", ctypes.c_void_p),
        ("n_long_rows", ctypes.c_int64),
        ("long_rows", ctypes.c_void_p),
        ("n_pieces", ctypes.c_int64),
        ("piece_len", ctypes.c_int64),
        ("packed", ctypes.c_void_p),
        ("packed_src_shift", ctypes.c_int64),
        ("n_hot", ctypes.c_int64),
        ("hot_nodes", ctypes.c_void_p),
        ("row_ptr", ctypes.c_void_p),
        ("dense", ctypes.c_void_p),
        ("dense_rows", ctypes.c_int64),
        ("dense_cols", ctypes.c_int64),
        ("packed_dead", ctypes.c_void_p),
    ]

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        if not self.struct_bytes:
            self.struct_bytes = ctypes.sizeof(type(self))
        if not self.abi_version:
            self.abi_version = ABI_VERSION


# The binding as data: exported function of include/ultra_rspmm.h -> (restype, argtypes).  load() applies it;
# tests/test_host_logic.py compares every row's argument count and kinds with the header's prototype.
vp, i64, i32, sz, f32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_size_t, ctypes.c_float
seg = ctypes.POINTER(UltraSegments)
SIGNATURES = {
    "ultra_rspmm_abi_version": (i32, []),
    "ultra_segments_bytes": (sz, []),
    "ultra_rspmm_status_string": (ctypes.c_char_p, [i32]),
    "ultra_rspmm_last_hip_error": (i32, []),
    "ultra_rspmm_device_info": (i32, [i32, ctypes.POINTER(i32), ctypes.POINTER(i32), ctypes.c_char_p, sz]),
    "ultra_rspmm_profile_next": (i32, [vp, vp]),
    "ultra_rspmm_event_create": (i32, [ctypes.POINTER(vp)]),
    "ultra_rspmm_event_destroy": (i32, [vp]),
    "ultra_rspmm_event_elapsed_ms": (i32, [vp, vp, ctypes.POINTER(f32)]),
    "ultra_rspmm_launch_records_clear": (i32, []),
    "ultra_rspmm_launch_records": (i32, [vp, i32]),
    "ultra_rspmm_launch_record_fields": (ctypes.c_char_p, []),
    "ultra_combine_forward_last_form": (i32, []),
    "ultra_rspmm_force_general_path": (i32, [i32]),
    "ultra_rspmm_reserve_cus": (i32, [i32]),
    "ultra_rspmm_workspace_bytes": (sz, [seg, i64]),
    "ultra_rspmm_forward_f32": (i32, [seg, vp, vp, vp, vp, vp, sz, i64, i64, i64, i32, i32, vp]),
    "ultra_rspmm_fwd_f32": (i32, [vp, vp, vp, vp, vp, vp, vp, i64, i64, i64, i64, i32, i32, vp]),
    "ultra_rspmm_forward_boundary_f32": (i32, [seg, vp, vp, vp, vp, i64, vp, vp, sz, i64, i64, i64, i32, i32, vp]),
    "ultra_rspmm_frontier_f32": (i32, [seg, vp, vp, vp, vp, vp, i64, vp, i64, i64, i64, vp]),
    "ultra_first_layer_sparse_supported": (i32, [i64, i64, i64]),
    "ultra_first_layer_sparse_f32": (i32, [seg, vp, vp, vp, vp, vp, vp, i64, vp, vp, vp, vp, f32, i32, i32, vp, vp, i64, i64, vp, i64,
                                          i64, vp]),
    "ultra_rspmm_backward_boundary_rows_f32": (i32, [seg, vp, vp, vp, vp, vp, vp, sz, i64, i64, i64, i32, vp]),
    "ultra_rspmm_backward_boundary_rows_workspace": (sz, [i64]),
    "ultra_rspmm_backward_f32": (i32, [seg, seg, vp, vp, vp, vp, vp, vp, vp, sz, i64, i64, i64, i64, i32, i32, vp]),
    "ultra_rspmm_backward_accumulate_f32": (i32, [seg, seg, vp, vp, vp, vp, vp, vp, vp, vp, sz, i64, i64, i64, i64, i32, i32, vp]),
    "ultra_rspmm_backward_weight_f32": (i32, [seg, vp, vp, vp, vp, vp, i64, i64, i32, i32, vp]),
    "ultra_rspmm_backward_weight_blocks_f32": (i32, [seg, vp, vp, vp, vp, vp, i64, i64, i64, i32, i32, vp]),
    "ultra_beam_search_step_f32": (i32, [vp, vp, vp, vp, i64, i64, i64, i64, vp, vp, vp, vp]),
    "ultra_beam_search_step_batch_f32": (i32, [vp, vp, vp, vp, vp, i64, i64, i64, i64, vp, vp, vp, vp]),
    "ultra_hop_distance_workspace": (sz, [i64]),
    "ultra_hop_distance": (i32, [vp, vp, vp, i64, i64, vp, i64, i64, vp, i64, vp, vp, i32, vp, sz, vp]),
    "ultra_rspmm_backward_active_f32": (i32, [seg, seg, vp, vp, vp, vp, vp, vp, vp, sz, i64, i64, i64, i64, i32, vp, i64, vp, vp]),
    "ultra_node_bitmap": (i32, [vp, i64, i64, i64, vp, vp]),
    "ultra_rspmm_drelation_boundary_f32": (i32, [seg, vp, i64, vp, vp, vp, vp, vp, vp, vp, sz, i64, i64, i64, vp]),
    "ultra_combine_forward_f32": (i32, [vp, vp, vp, vp, vp, vp, f32, i32, i32, vp, vp, i64, i64, vp]),
    "ultra_combine_forward_boundary_f32": (i32, [vp, vp, i64, vp, vp, vp, vp, vp, f32, i32, i32, vp, i64, i64, vp]),
    "ultra_combine_backward_waves": (i32, [i32, i64, ctypes.POINTER(i32), ctypes.POINTER(i32)]),
    "ultra_combine_backward_f32": (i32, [vp, vp, vp, vp, vp, vp, f32, i32, vp, vp, vp, vp, vp, vp, i64, i64, vp]),
    "ultra_combine_dxdu_f32": (i32, [vp, vp, vp, vp, vp, i64, i64, vp]),
    "ultra_combine_backward_fused_waves": (i32, [i32, i64, ctypes.POINTER(i32)]),
    "ultra_combine_backward_fused_f32": (i32, [vp, vp, vp, vp, vp, vp, f32, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, sz, vp, i64,
                                              i64, i64, vp]),
    "ultra_linear_forward_f32": (i32, [vp, vp, vp, vp, i64, i64, i64, i32, vp]),
    "ultra_score_forward_f32": (i32, [vp, vp, vp, vp, vp, vp, vp, vp, i64, i64, vp]),
    "ultra_relation_project_f32": (i32, [vp, i64, i64, vp, vp, vp, vp, vp, i64, i64, i64, i64, i64, vp]),
    "ultra_relation_project_backward_blocks": (i32, [i32, i64, i64, i64, vp]),
    "ultra_relation_project_backward_f32": (i32, [vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, sz, i64, i64, i64, i64, vp]),
    "ultra_query_tables_f32": (i32, [vp, i64, vp, vp, vp, vp, i64, i64, i64, i64, vp]),
    "ultra_query_tables_backward_workspace": (sz, [i64, i64, i64, vp, i64]),
    "ultra_query_tables_backward_f32": (i32, [vp, i64, vp, vp, vp, vp, vp, vp, sz, vp, i64, i64, i64, i64, vp]),
    "ultra_filtered_rank": (i32, [vp, i64, i64, i64, vp, vp, vp, vp, vp]),
    "ultra_filtered_rank_keys": (i32, [vp, i64, i64, i64, vp, i64, vp, i64, vp, vp, i64, i64, vp, i64, vp]),
    "ultra_strict_negative": (i32, [vp, i64, vp, vp, i64, i64, i64, vp, i64, vp, vp]),
    "ultra_filter_counts": (i32, [vp, i64, vp, vp, i64, i64, i64, i64, vp, vp]),
    "ultra_sampled_rank_keys": (i32, [vp, i64, i64, i64, vp, i64, vp, i64, vp, vp, i64, i64, vp, i64, vp, vp, vp, vp]),
    "ultra_topk_keys_workspace": (sz, [i64, i64, i64]),
    "ultra_topk_keys": (i32, [vp, i64, i64, i64, i64, vp, i64, vp, vp, i64, i64, vp, vp, vp, sz, vp]),
    "ultra_relation_select_limit": (i32, []),
    "ultra_relation_select_f32": (i32, [vp, i64, i64, i64, vp, vp, i64, vp, i64, vp, vp, i64, vp, i64, i64, i64, i64, vp, vp, vp, vp,
                                       vp, vp]),
    "ultra_candidate_select_workspace": (sz, [i64, i64, i64]),
    "ultra_candidate_select_f32": (i32, [vp, i64, i64, i64, vp, vp, i64, i64, vp, i64, vp, i64, vp, vp, i64, i64, vp, i64, i64, vp, vp,
                                        vp, vp, vp, vp, sz, vp]),
    "ultra_constrained_negative": (i32, [vp, i64, vp, vp, vp, i64, i64, i64, i64, vp, vp, i64, i64, vp, i64, i64, vp, vp, vp]),
    "ultra_set_boundary_f32": (i32, [vp, i64, i64, i64, vp, vp, i64, vp, vp, vp]),
    "ultra_set_boundary_backward_workspace": (sz, [i64, i64, i64]),
    "ultra_set_boundary_backward_f32": (i32, [vp, vp, i64, i64, i64, vp, vp, i64, vp, vp, vp, sz, vp]),
    "ultra_score_backward_workspace": (sz, [i64, i64]),
    "ultra_score_backward_f32": (i32, [vp, vp, vp, vp, vp, vp, i64, vp, vp, vp, vp, vp, vp, vp, sz, i64, i64, vp]),
    "ultra_sets_project_workspace": (sz, [i64, i64]),
    "ultra_sets_project": (i32, [vp, vp, vp, vp, i64, i64, i64, vp, vp, i64, vp, vp, sz, vp]),
    "ultra_sets_rank": (i32, [vp, i64, i64, i64, vp, vp, vp, i64, vp, vp]),
    "ultra_nonfinite_scan_tensors": (i32, []),
    "ultra_nonfinite_scan_chunk": (i32, []),
    "ultra_nonfinite_scan_f32": (i32, [vp, vp, i64, i64, vp, vp]),
    "ultra_nonfinite_commit": (i32, [vp, i32, vp]),
    "ultra_edge_removal_weights": (i32, [seg, seg, seg, vp, vp, vp, i64, i64, vp, vp, vp, i64, vp]),
    "ultra_edge_removal_marks": (i32, [seg, seg, seg, vp, vp, vp, i64, i64, vp, vp, vp, i64, vp, vp, vp, i64, vp]),
    "ultra_pair_removal": (i32, [seg, seg, seg, vp, vp, i64, vp, vp, vp, i64, vp, vp, vp, i64, vp]),
    "ultra_prepare_queries": (i32, [vp, vp, i64, i64, i64, i64, i64, vp, vp, vp, vp, vp]),
    "ultra_relation_stack_inputs": (i32, [vp, i64, i64, i64, vp, i64, vp, vp, vp, vp]),
    "ultra_statistics_blocks": (i32, [i64]),
    "ultra_statistics_f32": (i32, [vp, i64, vp, i64, i64, vp, vp, vp]),
    "ultra_bce_adversarial_f32": (i32, [vp, i64, i64, f32, vp, vp, vp]),
    "ultra_candidate_tiles": (i32, [vp, i64, i64, i64, i64, vp, vp]),
    "ultra_score_rows_forward_f32": (i32, [vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, i64, i64, vp]),
    "ultra_score_rows_backward_f32": (i32, [vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, i64, i64, i64, vp]),
    "ultra_gather_boundary_rows_f32": (i32, [vp, vp, i64, vp, vp]),
    "ultra_relcsr_coalesce_temp_bytes": (sz, [i64]),
    "ultra_relcsr_coalesce": (i32, [vp, vp, vp, vp, i64, i64, i64, i64, vp, vp, vp, vp, vp, ctypes.POINTER(i64), ctypes.POINTER(i32), vp,
                                   sz, vp]),
    "ultra_relcsr_plan_temp_bytes": (sz, [i64, i64, i64]),
    "ultra_relcsr_plan": (i32, [vp, vp, vp, i64, i64, i64, i64, i32, i32, i32, i64, i64, i64, vp, i64, vp, i64, vp, i64,
                               ctypes.POINTER(i64), vp, sz, vp]),
    "ultra_relcsr_dense_bytes": (sz, [i64, i64, i32]),
    "ultra_relcsr_dense": (i32, [seg, i64, i64, i32, vp, vp]),
    "ultra_relation_graph_marks": (i32, [vp, vp, vp, vp, i64, i64, vp, vp]),
    "ultra_calibrate_gather_f32": (i32, [vp, i64, vp, i64, vp, ctypes.POINTER(i64), vp]),
    "ultra_first_layer_sparse_train_f32": (i32, [seg, vp, vp, vp, vp, vp, vp, i64, vp, vp, vp, vp, f32, i32, i32, vp, vp, vp, i64, i64,
                                                vp, i64, i64, vp]),
    "ultra_first_layer_epilogue_backward_workspace": (sz, [i32, i64]),
    "ultra_first_layer_epilogue_backward_f32": (i32, [vp, vp, vp, vp, vp, i64, vp, vp, vp, vp, f32, i32, i32, vp, vp, vp, vp, vp, vp, vp,
                                                     sz, i64, vp]),
    "ultra_column_sum_blocks": (i32, []),
    "ultra_column_sum_f32": (i32, [vp, i64, vp, vp, vp, vp]),
    "ultra_dense_layer_supported": (i32, [seg, i64]),
    "ultra_dense_layer_forward_f32": (i32, [seg, vp, vp, vp, vp, i64, vp, vp, vp, vp, f32, i32, i32, vp, vp]),
    "ultra_layer_forward_supported": (i32, [seg, i64, i64]),
    "ultra_layer_forward_f32": (i32, [seg, vp, vp, vp, vp, i64, vp, vp, vp, vp, f32, i32, i32, vp, i64, vp]),
    "ultra_second_layer_sources": (i32, [vp, i64, i64, vp, vp, i64, i64, i64, vp, vp, vp, vp]),
    "ultra_layer_forward_sources_f32": (i32, [seg, vp, vp, vp, vp, vp, i64, vp, vp, vp, vp, f32, i32, i32, vp, i64, vp]),
    "ultra_layer_score_supported": (i32, [seg, i64, i64]),
    "ultra_layer_score_forward_f32": (i32, [seg, vp, vp, vp, vp, i64, vp, vp, vp, vp, f32, i32, i32, vp, vp, vp, vp, vp, vp, vp, i64, vp]),
    "ultra_rspmm_rotate_forward_f32": (i32, [seg, vp, vp, vp, vp, vp, vp, vp, sz, i64, i64, i64, i64, i32, vp]),
    "ultra_rspmm_rotate_backward_f32": (i32, [seg, seg, vp, vp, vp, vp, vp, vp, vp, sz, i64, i64, i64, i64, i64, i32, vp]),
    "ultra_rspmm_rotate_backward_weight_f32": (i32, [seg, vp, vp, vp, vp, vp, i64, i64, i64, i32, vp]),
    "ultra_rspmm_rotate_backward_weight_blocks_f32": (i32, [seg, vp, vp, vp, vp, vp, i64, i64, i64, i32, vp]),
    "ultra_rspmm_pna_workspace_bytes": (sz, [seg, i64]),
    "ultra_rspmm_pna_forward_f32": (i32, [seg, vp, vp, vp, vp, vp, i64, vp, vp, vp, vp, vp, sz, i64, i64, i64, i32, vp]),
    "ultra_pna_combine_forward_f32": (i32, [vp, vp, vp, vp, vp, vp, i64, vp, vp, vp, vp, f32, f32, i32, i32, vp, i64, i64, vp]),
}
EXPORTS = tuple(SIGNATURES)

_lib = None


class UltraLibraryError(RuntimeError):
    pass


def load():
    """Load the HIP library once; raise :class:`UltraLibraryError` if it is absent (no fallback exists)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise UltraLibraryError(
            "%s not found: build it with `make -C ultra_torchdrug_amd/csrc` (hipcc --offload-arch=gfx950) or "
            "`python -c 'import __graft_entry__ as g; g.build()'`. There is no CPU/PyTorch fallback." % LIB_PATH)
    try:
        lib = ctypes.CDLL(LIB_PATH)
    except OSError as err:  # missing libamdhip64 etc.
        raise UltraLibraryError("cannot load %s: %s" % (LIB_PATH, err)) from err
    missing = [name for name in EXPORTS if not hasattr(lib, name)]
    if missing:
        raise UltraLibraryError("%s lacks symbols %s" % (LIB_PATH, missing))

    for name, (restype, argtypes) in SIGNATURES.items():
        getattr(lib, name).restype, getattr(lib, name).argtypes = restype, argtypes
    if lib.ultra_rspmm_abi_version() != ABI_VERSION:
        raise UltraLibraryError("ABI mismatch: library %d, binding %d" % (lib.ultra_rspmm_abi_version(), ABI_VERSION))
    if lib.ultra_segments_bytes() != ctypes.sizeof(UltraSegments):
        raise UltraLibraryError("struct ultra_segments: library %d bytes, binding %d bytes"
                                % (lib.ultra_segments_bytes(), ctypes.sizeof(UltraSegments)))
    _lib = lib
    return lib


def check(status):
    """Turn a non-zero ``ultra_status`` into a RuntimeError (TORCH_CHECK-like behaviour of the reference op)."""
    if status != 0:
        lib = load()
        msg = lib.ultra_rspmm_status_string(status).decode()
        if status == 5:
            msg += " [hipError_t=%d]" % lib.ultra_rspmm_last_hip_error()
        raise RuntimeError("libultra_rspmm: %s" % msg)


def ptr(tensor):
    """The device address of ``tensor`` as it is (``data_ptr()``: never a copy), NULL for ``None``."""
    return None if tensor is None else tensor.data_ptr()


def launch(device, name, *args):
    """Run the exported launch ``name`` on ``device``: tensors among ``args`` become their ``data_ptr()`` and ``None`` NULL, the
    current HIP stream is appended and a non-zero status raises (:func:`check`).  A tensor is passed as it is -- an output that
    got copied here would be written into a temporary and lost -- so the caller makes its inputs contiguous and passes the
    copies, which ``args`` keeps alive until the C call has returned."""
    entry = getattr(load(), name)
    if len(args) + 1 != len(entry.argtypes):        # (ctypes itself lets surplus arguments of a cdecl function pass)
        raise TypeError("%s takes %d arguments and the stream, got %d" % (name, len(entry.argtypes) - 1, len(args)))
    with torch.cuda.device(device):
        check(entry(*[a.data_ptr() if isinstance(a, torch.Tensor) else a for a in args],
                    torch.cuda.current_stream().cuda_stream))


def launch_records_clear():
    """Forget this thread's launch records (``ultra_rspmm_launch_records_clear``)."""
    check(load().ultra_rspmm_launch_records_clear())


def launch_records():
    """``(count, records)``: how many plan runs of THIS thread reached a launch since the last clear, and the newest (at most
    8) of them, oldest first, as dicts keyed by the library's own field names (``ultra_rspmm_launch_record_fields``)."""
    lib = load()
    names = lib.ultra_rspmm_launch_record_fields().decode().split()
    rows = (ctypes.c_int32 * (8 * len(names)))()
    count = int(lib.ultra_rspmm_launch_records(ctypes.cast(rows, vp), 8))
    kept = min(count, 8)
    return count, [dict(zip(names, rows[i * len(names):(i + 1) * len(names)])) for i in range(kept)]


COMBINE_FORMS = {0: None, 1: "combine_kernel", 2: "combine_paired_kernel", 3: "combine_paired_kernel_lds"}


def combine_forward_last_form():
    """Name of the kernel the last layer-epilogue forward of THIS thread launched (``ultra_combine_forward_last_form``)."""
    return COMBINE_FORMS[int(load().ultra_combine_forward_last_form())]


def device_info(device=0):
    lib = load()
    n_cu, lds = ctypes.c_int(0), ctypes.c_int(0)
    arch = ctypes.create_string_buffer(64)
    check(lib.ultra_rspmm_device_info(int(device), ctypes.byref(n_cu), ctypes.byref(lds), arch, 64))
    return {"n_cu": n_cu.value, "lds_bytes": lds.value, "arch": arch.value.decode()}

// ultra_torchdrug_amd/csrc/plan_rotate.hip -- rspmm with rotate messages (rotate.inc): its kernels, run_rotate_plan and the
// ultra_rspmm_rotate_* entries.  Dispatches outside plan_path(); the fix-up pass over split rows is launch_fixup's.
#include <hip/hip_runtime.h>
#include <type_traits>

#include <cstdint>

#include "device_common.h"
#include "plan_kernels.h"

namespace {

using namespace ultra_detail;

#include "rotate.inc"

}  // namespace

extern "C" {

int ultra_rspmm_rotate_forward_f32(const ultra_segments *fwd, const float *relation, const float *input,
                                   const float *add_rows, const int32_t *boundary_node, const float *boundary_value,
                                   float *out, void *workspace, size_t workspace_bytes, int64_t n_src, int64_t n_rel,
                                   int64_t F, int64_t block, int sum_op, void *stream) {
    (void)n_src;
    if (fwd == nullptr) return ULTRA_ERR_NULL_POINTER;
    if (!segments_abi_ok(fwd)) return ULTRA_ERR_ABI;
    if (fwd->n_rows > 0 && out == nullptr) return ULTRA_ERR_NULL_POINTER;
    if (fwd->n_edges > 0 && (relation == nullptr || input == nullptr)) return ULTRA_ERR_NULL_POINTER;
    if ((boundary_node == nullptr) != (boundary_value == nullptr)) return ULTRA_ERR_NULL_POINTER;
    if (boundary_node != nullptr && add_rows != nullptr) return ULTRA_ERR_BAD_SHAPE;
    RotParams p{};
    p.relation = relation;
    p.input = input;
    p.add_rows = add_rows;
    p.bnode = boundary_node;
    p.bvec = boundary_value;
    p.out = out;
    return run_rotate_plan<KIND_FWD>(fwd, p, n_rel, F, block, sum_op, workspace, workspace_bytes,
                                     static_cast<hipStream_t>(stream));
}

int ultra_rspmm_rotate_backward_f32(const ultra_segments *by_src, const ultra_segments *by_rel, const float *relation,
                                    const float *input, const float *output, const float *output_grad, float *d_input,
                                    float *d_relation, void *workspace, size_t workspace_bytes, int64_t n_src,
                                    int64_t n_dst, int64_t n_rel, int64_t F, int64_t block, int sum_op, void *stream) {
    (void)n_src;
    (void)n_dst;
    if (by_src != nullptr && !segments_abi_ok(by_src)) return ULTRA_ERR_ABI;
    if (by_rel != nullptr && !segments_abi_ok(by_rel)) return ULTRA_ERR_ABI;
    if (block <= 0 || block % 2 != 0 || F <= 0 || F % block != 0) return ULTRA_ERR_BAD_SHAPE;
    if (sum_op < 0 || sum_op > 2) return ULTRA_ERR_BAD_OP;
    if (output_grad == nullptr || relation == nullptr || input == nullptr) return ULTRA_ERR_NULL_POINTER;
    if (sum_op != ULTRA_SUM_ADD && output == nullptr) return ULTRA_ERR_NULL_POINTER;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (d_input != nullptr) {
        if (by_src == nullptr) return ULTRA_ERR_NULL_POINTER;
        RotParams p{};
        p.relation = relation; p.input = input; p.output = output; p.grad = output_grad; p.out = d_input;
        int rc = run_rotate_plan<KIND_DX>(by_src, p, n_rel, F, block, sum_op, workspace, workspace_bytes, s);
        if (rc) return rc;
    }
    if (d_relation != nullptr) {
        if (by_rel == nullptr) return ULTRA_ERR_NULL_POINTER;
        if (by_rel->n_edges > 0 && by_rel->node_b == nullptr) return ULTRA_ERR_NULL_POINTER;
        RotParams p{};
        p.relation = relation; p.input = input; p.output = output; p.grad = output_grad; p.out = d_relation;
        int rc = run_rotate_plan<KIND_DREL>(by_rel, p, n_rel, F, block, sum_op, workspace, workspace_bytes, s);
        if (rc) return rc;
    }
    return ULTRA_OK;
}

int ultra_rspmm_rotate_backward_weight_f32(const ultra_segments *fwd, const float *relation, const float *input,
                                           const float *output, const float *output_grad, float *d_weight, int64_t n_rel,
                                           int64_t F, int64_t block, int sum_op, void *stream) {
    int rc = check_segments(fwd);
    if (rc) return rc;
    (void)n_rel;
    if (F <= 0 || F > 0x7ffffffeLL || block <= 0 || block % 2 != 0 || F % block != 0) return ULTRA_ERR_BAD_SHAPE;
    if (sum_op < 0 || sum_op > 2) return ULTRA_ERR_BAD_OP;
    if (fwd->n_edges == 0) return ULTRA_OK;
    if (relation == nullptr || input == nullptr || output_grad == nullptr || d_weight == nullptr)
        return ULTRA_ERR_NULL_POINTER;
    if (sum_op != ULTRA_SUM_ADD && output == nullptr) return ULTRA_ERR_NULL_POINTER;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int half = (int)(block / 2);
    return with_sum(sum_op, [&](auto sum) {
        return launch_rotate_weight_grad<decltype(sum)::value>(fwd, relation, input, output, output_grad, d_weight, F, half, s);
    });
}

int ultra_rspmm_rotate_backward_weight_blocks_f32(const ultra_segments *fwd, const float *relation, const float *input,
                                                  const float *output, const float *output_grad, float *d_weight,
                                                  int64_t n_rel, int64_t F, int64_t block, int sum_op, void *stream) {
    int rc = check_segments(fwd);
    if (rc) return rc;
    (void)n_rel;
    if (F <= 0 || F > 0x7ffffffeLL || block <= 0 || block % 2 != 0 || F % block != 0) return ULTRA_ERR_BAD_SHAPE;
    if (sum_op < 0 || sum_op > 2) return ULTRA_ERR_BAD_OP;
    if (fwd->n_edges == 0) return ULTRA_OK;
    if (relation == nullptr || input == nullptr || output_grad == nullptr || d_weight == nullptr)
        return ULTRA_ERR_NULL_POINTER;
    if (sum_op != ULTRA_SUM_ADD && output == nullptr) return ULTRA_ERR_NULL_POINTER;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int half = (int)(block / 2);
    return with_sum(sum_op, [&](auto sum) {
        return launch_rotate_weight_grad_blocks<decltype(sum)::value>(fwd, relation, input, output, output_grad, d_weight, F, half, s);
    });
}

}  // extern "C"

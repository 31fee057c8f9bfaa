// host_common.h -- what the translation units of libultra_rspmm.so share on the host side (internal: the library is built
// with -fvisibility=hidden, nothing here is exported).  The state behind these declarations lives in runtime.hip;
// dense_launch in relgraph_dense.hip.  Beside it: device_common.h (what kernels share) and plan_kernels.h (the plan families).
#ifndef ULTRA_HOST_COMMON_H
#define ULTRA_HOST_COMMON_H

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <type_traits>

#include "plan_path.h"
#include "ultra_rspmm.h"

// hipError_t of the last failing HIP call on this thread (ultra_rspmm_last_hip_error)
extern thread_local int ultra_detail_last_hip_error;

#define HIP_TRY(expr)                                   \
    do {                                                \
        hipError_t _e = (expr);                         \
        if (_e != hipSuccess) {                         \
            ultra_detail_last_hip_error = (int)_e;      \
            (void)hipGetLastError();                    \
            return ULTRA_ERR_HIP;                       \
        }                                               \
    } while (0)

namespace ultra_detail {

// ultra_rspmm_force_general_path (process-wide)
extern Knobs g_knobs;

// one-shot profiling events (ultra_rspmm_profile_next): bracket the next plan's segment kernel, or the next frontier call,
// on its stream; whoever takes them clears them
extern thread_local hipEvent_t g_prof_start;
extern thread_local hipEvent_t g_prof_stop;

struct DeviceInfo {
    bool valid = false;
    int n_cu = 0;            // compute units the persistent grids are sized for (= n_cu_total - ultra_rspmm_reserve_cus)
    int n_cu_total = 0;
    int lds_bytes = 0;
    char arch[64] = {0};
};
int device_info(int device, DeviceInfo **out);
int current_device_info(DeviceInfo **out);      // ... of hipGetDevice()

// The fence of the boundary (ABI 8): the caller's struct must be THIS header's, field for field.  Only the two leading
// fields are read before that is known.
inline bool segments_abi_ok(const ultra_segments *s) {
    return s->struct_bytes == (uint32_t)sizeof(ultra_segments) && s->abi_version == (uint32_t)ULTRA_RSPMM_ABI_VERSION;
}

inline int check_segments(const ultra_segments *s) {
    if (s == nullptr) return ULTRA_ERR_NULL_POINTER;
    if (!segments_abi_ok(s)) return ULTRA_ERR_ABI;
    if (s->n_rows < 0 || s->n_edges < 0 || s->n_chunks < 0 || s->n_pieces < 0 || s->n_long_rows < 0)
        return ULTRA_ERR_BAD_SHAPE;
    if (s->n_rows > 0x7fffffffLL || s->n_edges > 0x7fffffffLL || s->n_chunks > 0x7fffffffLL) return ULTRA_ERR_BAD_SHAPE;
    if (s->n_edges > 0 && (s->row == nullptr || s->node_a == nullptr || s->rel == nullptr)) return ULTRA_ERR_NULL_POINTER;
    if (s->n_chunks > 0 && s->chunks == nullptr) return ULTRA_ERR_NULL_POINTER;
    if (s->n_long_rows > 0 && s->long_rows == nullptr) return ULTRA_ERR_NULL_POINTER;
    return ULTRA_OK;
}

// hipFuncAttributeMaxDynamicSharedMemorySize is a property of ONE kernel function, and kernel instances of one template share
// a pointer type, so the "already set" table is keyed on the kernel's address (per device) and guarded by a mutex.  Launches
// of at most 48 KiB need no attribute.  max_bytes: what the attribute is set to -- kernels with static LDS of their own pass
// their own cap.
int ensure_lds_attribute(const void *kern, size_t lds, int max_bytes = kMaxLdsBytes);

template <typename Kern, typename Params>
int launch_with_lds(Kern kern, const Params &p, int grid, size_t lds, hipStream_t stream, int block, int max_bytes = kMaxLdsBytes) {
    const int rc = ensure_lds_attribute(reinterpret_cast<const void *>(kern), lds, max_bytes);
    if (rc) return rc;
    hipLaunchKernelGGL(kern, dim3(grid), dim3(block), lds, stream, p);
    HIP_TRY(hipGetLastError());
    return ULTRA_OK;
}

// Runtime value -> template argument: fn(std::integral_constant<int, V>{}) for the V among Vs that equals v, else
// ULTRA_ERR_BAD_OP.  Kernels are instantiated where fn names them, for the combinations fn's own `if constexpr` lets through,
// so a dispatch written with these instantiates what a call can reach and nothing else.
template <int... Vs, typename Fn>
int with_int(int v, Fn &&fn) {
    int rc = ULTRA_ERR_BAD_OP;
    (void)((v == Vs && ((rc = fn(std::integral_constant<int, Vs>{})), true)) || ...);
    return rc;
}
template <typename Fn>
int with_bool(bool b, Fn &&fn) {
    return b ? fn(std::true_type{}) : fn(std::false_type{});
}
template <typename Fn>
int with_sum(int sum_op, Fn &&fn) {
    return with_int<ULTRA_SUM_ADD, ULTRA_SUM_MIN, ULTRA_SUM_MAX>(sum_op, fn);
}
template <typename Fn>
int with_mul(int mul_op, Fn &&fn) {
    return with_int<ULTRA_MUL_MUL, ULTRA_MUL_ADD>(mul_op, fn);
}
template <typename Fn>
int with_sum_mul(int sum_op, int mul_op, Fn &&fn) {
    return with_sum(sum_op, [&](auto sum) { return with_mul(mul_op, [&](auto mul) { return fn(sum, mul); }); });
}

// one sum-aggregation call over a plan in its dense form (relgraph_dense.hip); plan_path() has said that it applies
struct DenseCall {
    const ultra_segments *seg;
    int kind, mul_op;
    const float *relation;      // [n_rel, F]
    const float *input;         // [n_src, F]
    const float *grad;          // backward: output_grad [n_dst, F]
    const float *add_rows;      // forward: fused boundary rows; d_input: the gradient to accumulate into (may alias out)
    const int32_t *bnode;       // forward: sparse boundary
    const float *bvec;
    int bdim;
    float *out;
    void *workspace;
    int64_t F;
};
int dense_launch(const DenseCall &call, hipStream_t stream);

}  // namespace ultra_detail

#endif

// ultra_torchdrug_amd/csrc/rspmm_kernels.hip -- the rspmm entries of libultra_rspmm.so's C ABI and the dispatch behind them
//
// Replaces the native operator behind torchdrug.layers.functional.generalized_rspmm, which the reference
// calls at /root/reference/ultra/layer.py:134-167 and :336-369 (see include/ultra_rspmm.h).
//
// run_plan validates a call, lets plan_path() (plan_path.h) decide, fills the parameter block of the chosen family and calls
// that family's launcher (plan_kernels.h): the plan kernels themselves live in plan_general.hip, plan_packed.hip,
// plan_quad.hip and plan_rowgroup.hip, the dense form in relgraph_dense.hip, the fix-up pass over split rows in epilogue.hip.
// The only kernels here are the per-edge weight gradients.  DESIGN.md has the design and its numbers.
#include <hip/hip_runtime.h>
#include <type_traits>

#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <cstring>

#include "device_common.h"
#include "plan_kernels.h"

namespace {

using namespace ultra_detail;        // kTile, kXcd, kMaxLdsBytes, kLdsHeader, Kind (plan_path.h) and the host helpers

// d_weight[e] = sum_f (grad[dst,f] * dmask) * (relation[rel,f] MUL input[src,f]); one wave per edge.
template <int SUM, int MUL, bool UNIT_W>
__global__ __launch_bounds__(256) void weight_grad_kernel(const int32_t *row, const int32_t *src, const int32_t *rel,
                                                          const float *weight, const float *relation,
                                                          const float *input, const float *output, const float *grad,
                                                          float *d_weight, long long F, long long n_edges) {
    const int lane = threadIdx.x & 63;
    const long long waves_total = ((long long)gridDim.x * blockDim.x) >> 6;
    long long e = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    for (; e < n_edges; e += waves_total) {
        const int v = row[e], u = src[e], r = rel[e];
        float wk = 1.0f;
        if constexpr (!UNIT_W) wk = weight[e];
        float acc = 0.0f;
        for (long long f = lane; f < F; f += 64) {
            const float m = binary<MUL>(relation[(long long)r * F + f], input[(long long)u * F + f]);
            float g = grad[(long long)v * F + f];
            if constexpr (SUM != ULTRA_SUM_ADD) {
                float y = m;
                if constexpr (!UNIT_W) y = wk * m;
                g = g * ((output[(long long)v * F + f] == y) ? 1.0f : 0.0f);
            }
            acc = acc + g * m;
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
        if (lane == 0) d_weight[e] = acc;
    }
}

// weight_grad_kernel per query block: d_weight[b][e] = the sum above over columns b * block .. (b + 1) * block - 1 alone
// (ultra_rspmm_backward_weight_blocks_f32).  Still one wave per edge -- ids and weight are read once -- walking the blocks;
// within a block lane l takes columns l, l + 64, ... of the block, then the same __shfl_down tree: slice [b] carries the bits
// weight_grad_kernel gives on a contiguous copy of the block's columns.
template <int SUM, int MUL, bool UNIT_W>
__global__ __launch_bounds__(256) void weight_grad_blocks_kernel(const int32_t *row, const int32_t *src, const int32_t *rel,
                                                                 const float *weight, const float *relation,
                                                                 const float *input, const float *output, const float *grad,
                                                                 float *d_weight, long long F, long long block,
                                                                 long long n_blocks, long long n_edges) {
    const int lane = threadIdx.x & 63;
    const long long waves_total = ((long long)gridDim.x * blockDim.x) >> 6;
    long long e = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    for (; e < n_edges; e += waves_total) {
        const int v = row[e], u = src[e], r = rel[e];
        float wk = 1.0f;
        if constexpr (!UNIT_W) wk = weight[e];
        for (long long b = 0; b < n_blocks; ++b) {
            const long long c0 = b * block;
            float acc = 0.0f;
            for (long long f = lane; f < block; f += 64) {
                const float m = binary<MUL>(relation[(long long)r * F + c0 + f], input[(long long)u * F + c0 + f]);
                float g = grad[(long long)v * F + c0 + f];
                if constexpr (SUM != ULTRA_SUM_ADD) {
                    float y = m;
                    if constexpr (!UNIT_W) y = wk * m;
                    g = g * ((output[(long long)v * F + c0 + f] == y) ? 1.0f : 0.0f);
                }
                acc = acc + g * m;
            }
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
            if (lane == 0) d_weight[b * n_edges + e] = acc;
        }
    }
}

// ------------------------------------------------------------------------------------------------ host side

void fill_tiling(RowGroupParams &q, const PlanPath &path) {
    q.n_tiles = path.geo.n_tiles;
    q.split = path.geo.split;
    q.n_slots = path.geo.n_slots;
    q.blocks_per_label = path.geo.blocks_per_label;
    q.n_rel_lds = path.n_rel_lds;
}

inline bool aligned16(const void *ptr) { return (reinterpret_cast<uintptr_t>(ptr) & 15u) == 0; }

// packed_kernel / quad_kernel over the plan's packed words
template <int KIND>
int launch_words(const ultra_segments *seg, const KParams &p, const PlanPath &path, int64_t gather_rows, int64_t gather2_rows,
                 int64_t n_rel, int64_t F, int sum_op, int mul_op, hipStream_t stream) {
    const bool big = seg->packed_src_shift >= 32;          // node ids live in node_a, not in the packed word
    const bool quad = path.family == FAM_QUAD;
    const unsigned long long relation_bytes = (unsigned long long)n_rel * (unsigned long long)F * 4ull;
    const unsigned long long meta_bytes = ((unsigned long long)seg->n_edges + 16ull) * 4ull;   // PACK_SLACK words follow
    const unsigned long long out_bytes = (unsigned long long)seg->n_rows * (unsigned long long)F * 4ull;
    PParams q{};
    q.meta = path.dead ? seg->packed_dead : seg->packed;
    q.meta2 = reinterpret_cast<const uint32_t *>(big ? seg->node_a : seg->node_b);
    q.weight = path.dead ? nullptr : seg->weight;
    q.chunks = p.chunks;
    q.relation = p.relation;
    q.gather = (KIND == KIND_DX) ? p.grad : p.input;
    q.gather2 = p.grad;
    q.add_rows = p.add_rows;
    q.bnode = p.bnode;
    q.bvec = p.bvec;
    q.bdim = p.bdim;
    q.out = p.out;
    q.partial = p.partial;
    q.F = F;
    q.gather_bytes = (uint32_t)((unsigned long long)gather_rows * (unsigned long long)F * 4ull);
    q.gather2_bytes = (uint32_t)((unsigned long long)gather2_rows * (unsigned long long)F * 4ull);
    q.relation_bytes = (uint32_t)(relation_bytes < 0xffff0000ull ? relation_bytes : 0);
    q.meta_bytes = (uint32_t)(meta_bytes < 0xffff0000ull ? meta_bytes : 0);
    q.meta2_bytes = (uint32_t)((unsigned long long)seg->n_edges * 4ull);
    q.out_bytes = (uint32_t)(out_bytes < 0xffff0000ull ? out_bytes : 0);
    q.row_bytes = (uint32_t)(F * 4);
    q.src_shift = (uint32_t)seg->packed_src_shift;
    q.rel_mask = big ? 0xffffff00u : ((1u << (seg->packed_src_shift - 8)) - 1u) << 8;
    q.n_gather_rows = (int)gather_rows;
    if (!big && seg->n_hot > 0) {
        q.hot_nodes = seg->hot_nodes;
        q.n_hot = (int)seg->n_hot;
    }
    q.n_chunks = p.n_chunks;
    q.n_rel = p.n_rel;
    q.n_tiles = p.n_tiles;
    q.split = p.split;
    q.n_slots = p.n_slots;
    q.blocks_per_label = p.blocks_per_label;
    if (quad) {
        q.concurrent = path.concurrent;
        if (path.act == ACT_BITS) {
            q.act_bits = p.act_bits;
            q.act_words = p.act_words;
        } else if (path.act == ACT_NODE) {
            q.act_node = p.act_node;
        }
    }
    return quad ? launch_quad(KIND, sum_op, mul_op, q, path, stream) : launch_packed(KIND, sum_op, mul_op, q, path, stream);
}

// Runs one plan: validate, decide (plan_path.h), fill the parameters of the chosen family, launch, then fixup_kernel over the
// split rows.
template <int KIND>
int run_plan(const ultra_segments *seg, KParams p, int64_t gather_rows, int64_t gather2_rows, int64_t n_rel, int64_t F,
             int sum_op, int mul_op, void *workspace, size_t workspace_bytes, hipStream_t stream) {
    int rc = check_segments(seg);
    if (rc) return rc;
    if (F <= 0 || n_rel < 0 || n_rel > 0x7fffffffLL) return ULTRA_ERR_BAD_SHAPE;
    if (sum_op < 0 || sum_op > 2 || mul_op < 0 || mul_op > 1) return ULTRA_ERR_BAD_OP;
    const size_t need = ultra_rspmm_workspace_bytes(seg, F);
    if (need > 0 && (workspace == nullptr || workspace_bytes < need)) return ULTRA_ERR_WORKSPACE;
    if (seg->n_rows == 0) return ULTRA_OK;

    DeviceInfo *di = nullptr;
    rc = current_device_info(&di);
    if (rc) return rc;

    p.partial = static_cast<float *>(workspace);
    PlanInput in;
    in.kind = KIND; in.sum_op = sum_op; in.mul_op = mul_op;
    in.F = F; in.n_rel = n_rel; in.gather_rows = gather_rows; in.gather2_rows = gather2_rows;
    in.has_weight = seg->weight != nullptr; in.has_node_b = seg->node_b != nullptr; in.has_row_ptr = seg->row_ptr != nullptr;
    in.has_packed = seg->packed != nullptr; in.has_packed_dead = seg->packed_dead != nullptr; in.has_dense = seg->dense != nullptr;
    in.packed_src_shift = seg->packed_src_shift; in.n_rows = seg->n_rows; in.n_edges = seg->n_edges;
    in.n_long_rows = seg->n_long_rows; in.n_pieces = seg->n_pieces; in.n_hot = seg->n_hot;
    in.dense_rows = seg->dense_rows; in.dense_cols = seg->dense_cols;
    in.has_add_rows = p.add_rows != nullptr; in.has_bnode = p.bnode != nullptr; in.bdim = p.bdim;
    in.has_act_bits = p.act_bits != nullptr; in.has_act_node = p.act_node != nullptr; in.act_words = p.act_words;
    in.has_workspace = workspace != nullptr; in.workspace_bytes = workspace_bytes;
    in.aligned = (aligned16(p.input) ? AL_INPUT : 0) | (aligned16(p.grad) ? AL_GRAD : 0) | (aligned16(p.out) ? AL_OUT : 0) |
                 (aligned16(p.relation) ? AL_RELATION : 0) | (aligned16(p.add_rows) ? AL_ADD_ROWS : 0) |
                 (aligned16(p.partial) ? AL_PARTIAL : 0) | (aligned16(p.bvec) ? AL_BVEC : 0);
    in.knobs = g_knobs;
    in.n_cu = di->n_cu;
    in.gfx950 = std::strncmp(di->arch, "gfx950", 6) == 0;
    PlanPath path = plan_path(in);
    if (path.family == FAM_QUAD) {
        if (const char *force = getenv("ULTRA_CONC")) {      // experiments (tools/conc_ab.sh)
            const char *min_rows = getenv("ULTRA_CONC_MIN_ROWS");
            force_concurrent(path, atoi(force), min_rows != nullptr, min_rows != nullptr ? atoll(min_rows) : 0, gather_rows);
        }
    }

    hipEvent_t ev_start = g_prof_start, ev_stop = g_prof_stop;
    g_prof_start = g_prof_stop = nullptr;
    // (not while the stream is being captured: the ROCm 7.0 runtime bundled with PyTorch rejects external
    // event-record nodes, so the hook is simply ignored inside a hipGraph capture)
    if (ev_start != nullptr || ev_stop != nullptr) {
        hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
        HIP_TRY(hipStreamIsCapturing(stream, &cs));
        if (cs != hipStreamCaptureStatusNone) ev_start = ev_stop = nullptr;
    }
    if (ev_start != nullptr) HIP_TRY(hipEventRecord(ev_start, stream));
    if (path.status) return path.status;

    p.row = seg->row;
    p.node_a = seg->node_a;
    p.node_b = seg->node_b;
    p.rel = seg->rel;
    p.weight = seg->weight;
    p.chunks = reinterpret_cast<const int4 *>(seg->chunks);
    p.F = F;
    p.n_chunks = (int)seg->n_chunks;
    p.n_rel = (int)n_rel;
    p.n_tiles = path.geo.n_tiles;
    p.split = path.geo.split;
    p.n_slots = path.geo.n_slots;
    p.blocks_per_label = path.geo.blocks_per_label;
    switch (path.family) {
        case FAM_DENSE: {
            const DenseCall call{seg, KIND, mul_op, p.relation, p.input, p.grad, p.add_rows, p.bnode, p.bvec, p.bdim, p.out, workspace, F};
            rc = dense_launch(call, stream);
            {       // (relgraph_dense.hip picks its own kernels: the record says that the dense form ran, and for which call)
                LaunchRecord rec;
                rec.family = FAM_DENSE; rec.kind = KIND; rec.sum = sum_op; rec.mul = mul_op; rec.unit_w = 1;
                g_launches.push(rec).status = rc;
            }
            break;
        }
        case FAM_ROWGROUP:
            if constexpr (KIND != KIND_DREL) {
                RowGroupParams q{};
                q.row_ptr = seg->row_ptr;
                q.col = seg->node_a;
                q.rel = seg->rel;
                q.weight = seg->weight;
                q.relation = p.relation;
                q.gather = (KIND == KIND_DX) ? p.grad : p.input;
                q.add_rows = p.add_rows;
                q.bnode = p.bnode;
                q.bvec = p.bvec;
                q.bdim = p.bdim;
                q.out = p.out;
                q.F = F;
                q.n_rows = (int)seg->n_rows;
                q.n_rel = (int)n_rel;
                fill_tiling(q, path);
                rc = launch_rowgroup(sum_op, mul_op, KIND == KIND_DX, q, path, stream);
            }
            break;
        case FAM_QUAD:
        case FAM_PACKED:
            rc = launch_words<KIND>(seg, p, path, gather_rows, gather2_rows, n_rel, F, sum_op, mul_op, stream);
            break;
        default:
            rc = launch_general(KIND, sum_op, mul_op, p, path, stream);
    }
    if (rc) return rc;
    if (ev_stop != nullptr) HIP_TRY(hipEventRecord(ev_stop, stream));

    if (path.fixup != FIX_NONE) {
        FixParams fp;
        fp.long_rows = seg->long_rows;
        fp.partial = p.partial;
        fp.add_rows = p.add_rows;
        fp.bnode = p.bnode;
        fp.bvec = p.bvec;
        fp.bdim = p.bdim;
        fp.out = p.out;
        fp.F = F;
        fp.n_long = (int)seg->n_long_rows;
        fp.n_tiles = path.geo.n_tiles;
        return launch_fixup(fp, (KIND == KIND_FWD) ? sum_op : ULTRA_SUM_ADD, path.fixup == FIX_MANY, path.fixup_grid, stream);
    }
    return ULTRA_OK;
}

}  // namespace

extern "C" {

size_t ultra_rspmm_workspace_bytes(const ultra_segments *seg, int64_t F) {
    if (seg == nullptr || F <= 0 || !segments_abi_ok(seg)) return 0;     // (the call over a foreign struct then fails with ULTRA_ERR_ABI)
    int64_t rows = seg->n_pieces > 0 ? seg->n_pieces : 0;
    // d_relation plan in its dense form: one tile sum per 16 destination nodes and relation type (relgraph_dense.hip)
    if (seg->dense != nullptr && seg->n_rows == 4 && seg->node_b != nullptr) rows = std::max<int64_t>(rows, 4 * ((seg->dense_rows + 15) / 16));
    return (size_t)rows * (size_t)F * sizeof(float);
}

int ultra_rspmm_forward_f32(const ultra_segments *fwd, const float *relation, const float *input, const float *add_rows,
                            float *out, void *workspace, size_t workspace_bytes, int64_t n_src, int64_t n_rel, int64_t F,
                            int sum_op, int mul_op, void *stream) {
    if (fwd == nullptr) return ULTRA_ERR_NULL_POINTER;
    if (!segments_abi_ok(fwd)) return ULTRA_ERR_ABI;
    if (fwd->n_rows > 0 && out == nullptr) return ULTRA_ERR_NULL_POINTER;
    if (fwd->n_edges > 0 && (relation == nullptr || input == nullptr)) return ULTRA_ERR_NULL_POINTER;
    KParams p{};
    p.relation = relation;
    p.input = input;
    p.add_rows = add_rows;
    p.out = out;
    return run_plan<KIND_FWD>(fwd, p, n_src, 0, n_rel, F, sum_op, mul_op, workspace, workspace_bytes,
                              static_cast<hipStream_t>(stream));
}

int ultra_rspmm_fwd_f32(const int32_t *row_ptr, const int32_t *src, const int32_t *rel, const float *w,
                        const float *relation, const float *x, float *out, int64_t N, int64_t E, int64_t R, int64_t F,
                        int sum_op, int mul_op, void *stream) {
    if (N < 0 || E < 0 || R < 0 || F <= 0 || N > 0x7fffffffLL || E > 0x7fffffffLL || (F % 4) != 0) return ULTRA_ERR_BAD_SHAPE;
    if (sum_op < 0 || sum_op > 2 || mul_op < 0 || mul_op > 1) return ULTRA_ERR_BAD_OP;
    if (N == 0) return ULTRA_OK;
    if (row_ptr == nullptr || out == nullptr) return ULTRA_ERR_NULL_POINTER;
    if (E > 0 && (src == nullptr || rel == nullptr || relation == nullptr || x == nullptr)) return ULTRA_ERR_NULL_POINTER;
    if ((reinterpret_cast<uintptr_t>(out) | reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(relation)) & 15u)
        return ULTRA_ERR_BAD_SHAPE;
    if (F >= (1LL << 30)) return ULTRA_ERR_BAD_SHAPE;         // row bytes are a 32-bit factor of the address arithmetic
    DeviceInfo *di = nullptr;
    int rc = current_device_info(&di);
    if (rc) return rc;
    RowGroupParams q{};
    q.row_ptr = row_ptr;
    q.col = src;
    q.rel = rel;
    q.weight = w;
    q.relation = relation;
    q.gather = x;
    q.out = out;
    q.F = F;
    q.n_rows = (int)N;
    q.n_rel = (int)R;
    // (the rows of x are not part of this signature; N stands in for them in the cache-residency heuristic)
    PlanPath path;
    path.unit_w = w == nullptr;
    set_rowgroup(path, rowgroup_tiling(F, N, N, R, di->n_cu, g_knobs.wide_groups, kLdsHeader, kMaxLdsBytes));
    fill_tiling(q, path);
    return launch_rowgroup(sum_op, mul_op, false, q, path, static_cast<hipStream_t>(stream));
}

int ultra_rspmm_forward_boundary_f32(const ultra_segments *fwd, const float *relation, const float *input,
                                     const int32_t *boundary_node, const float *boundary_value, int64_t block, float *out,
                                     void *workspace, size_t workspace_bytes, int64_t n_src, int64_t n_rel, int64_t F,
                                     int sum_op, int mul_op, void *stream) {
    if (fwd == nullptr) return ULTRA_ERR_NULL_POINTER;
    if (!segments_abi_ok(fwd)) return ULTRA_ERR_ABI;
    if (boundary_node == nullptr || boundary_value == nullptr) return ULTRA_ERR_NULL_POINTER;
    if (fwd->n_rows > 0 && out == nullptr) return ULTRA_ERR_NULL_POINTER;
    if (fwd->n_edges > 0 && (relation == nullptr || input == nullptr)) return ULTRA_ERR_NULL_POINTER;
    if (block <= 0 || block > 0x7fffffffLL || F <= 0 || F % block != 0) return ULTRA_ERR_BAD_SHAPE;
    KParams p{};
    p.relation = relation;
    p.input = input;
    p.bnode = boundary_node;
    p.bvec = boundary_value;
    p.bdim = (int)block;
    p.out = out;
    return run_plan<KIND_FWD>(fwd, p, n_src, 0, n_rel, F, sum_op, mul_op, workspace, workspace_bytes,
                              static_cast<hipStream_t>(stream));
}

// d_input over the by_src plan and d_relation over the by_rel plan, each where its output is asked for; the activity
// arguments are ultra_rspmm_backward_active_f32's (NULL: none)
static int backward_plans(const ultra_segments *by_src, const ultra_segments *by_rel, const float *relation, const float *input,
                          const float *output, const float *output_grad, const float *d_input_add, float *d_input,
                          float *d_relation, void *workspace, size_t workspace_bytes, int64_t n_src, int64_t n_dst,
                          int64_t n_rel, int64_t F, int sum_op, int mul_op, const uint32_t *dst_active_bits,
                          int64_t active_words, const int32_t *src_active_node, hipStream_t s) {
    KParams p{};
    p.relation = relation;
    p.input = input;
    p.output = output;
    p.grad = output_grad;
    p.act_bits = dst_active_bits;
    p.act_words = (int)active_words;
    if (d_input != nullptr) {
        if (by_src == nullptr) return ULTRA_ERR_NULL_POINTER;
        p.out = d_input;
        p.add_rows = d_input_add;
        int rc = run_plan<KIND_DX>(by_src, p, n_dst, 0, n_rel, F, sum_op, mul_op, workspace, workspace_bytes, s);
        if (rc) return rc;
    }
    if (d_relation != nullptr) {
        if (by_rel == nullptr) return ULTRA_ERR_NULL_POINTER;
        if (!segments_abi_ok(by_rel)) return ULTRA_ERR_ABI;
        if (by_rel->n_edges > 0 && by_rel->node_b == nullptr) return ULTRA_ERR_NULL_POINTER;
        p.out = d_relation;
        p.add_rows = nullptr;
        p.act_node = src_active_node;
        int rc = run_plan<KIND_DREL>(by_rel, p, n_src, n_dst, n_rel, F, sum_op, mul_op, workspace, workspace_bytes, s);
        if (rc) return rc;
    }
    return ULTRA_OK;
}

int ultra_rspmm_backward_f32(const ultra_segments *by_src, const ultra_segments *by_rel, const float *relation,
                             const float *input, const float *output, const float *output_grad, float *d_input,
                             float *d_relation, void *workspace, size_t workspace_bytes, int64_t n_src, int64_t n_dst,
                             int64_t n_rel, int64_t F, int sum_op, int mul_op, void *stream) {
    return ultra_rspmm_backward_accumulate_f32(by_src, by_rel, relation, input, output, output_grad, nullptr, d_input,
                                               d_relation, workspace, workspace_bytes, n_src, n_dst, n_rel, F, sum_op,
                                               mul_op, stream);
}

int ultra_rspmm_backward_accumulate_f32(const ultra_segments *by_src, const ultra_segments *by_rel, const float *relation,
                                        const float *input, const float *output, const float *output_grad,
                                        const float *d_input_add, float *d_input, float *d_relation, void *workspace,
                                        size_t workspace_bytes, int64_t n_src, int64_t n_dst, int64_t n_rel, int64_t F,
                                        int sum_op, int mul_op, void *stream) {
    if (output_grad == nullptr || relation == nullptr || input == nullptr) return ULTRA_ERR_NULL_POINTER;
    if (d_input_add != nullptr && sum_op != ULTRA_SUM_ADD) return ULTRA_ERR_BAD_OP;       // the sum-aggregation kernels carry the epilogue
    if (sum_op != ULTRA_SUM_ADD && output == nullptr) return ULTRA_ERR_NULL_POINTER;
    return backward_plans(by_src, by_rel, relation, input, output, output_grad, d_input_add, d_input, d_relation, workspace,
                          workspace_bytes, n_src, n_dst, n_rel, F, sum_op, mul_op, nullptr, 0, nullptr, static_cast<hipStream_t>(stream));
}

// Backward of sum-aggregation with the caller's knowledge of WHICH rows carry gradient (see include/ultra_rspmm.h).
int ultra_rspmm_backward_active_f32(const ultra_segments *by_src, const ultra_segments *by_rel, const float *relation,
                                    const float *input, const float *output_grad, const float *d_input_add, float *d_input,
                                    float *d_relation, void *workspace, size_t workspace_bytes, int64_t n_src, int64_t n_dst,
                                    int64_t n_rel, int64_t F, int mul_op, const uint32_t *dst_active_bits, int64_t active_words,
                                    const int32_t *src_active_node, void *stream) {
    if (output_grad == nullptr || relation == nullptr || input == nullptr) return ULTRA_ERR_NULL_POINTER;
    if (dst_active_bits != nullptr && (active_words < (n_dst + 31) / 32 || active_words > 0x7fffffffLL)) return ULTRA_ERR_BAD_SHAPE;
    if ((dst_active_bits != nullptr || src_active_node != nullptr) && F % kTile != 0) return ULTRA_ERR_BAD_SHAPE;
    return backward_plans(by_src, by_rel, relation, input, nullptr, output_grad, d_input_add, d_input, d_relation, workspace,
                          workspace_bytes, n_src, n_dst, n_rel, F, ULTRA_SUM_ADD, mul_op, dst_active_bits, active_words,
                          src_active_node, static_cast<hipStream_t>(stream));
}

int ultra_rspmm_backward_weight_f32(const ultra_segments *fwd, const float *relation, const float *input,
                                    const float *output, const float *output_grad, float *d_weight, int64_t n_rel,
                                    int64_t F, int sum_op, int mul_op, void *stream) {
    int rc = check_segments(fwd);
    if (rc) return rc;
    (void)n_rel;
    if (F <= 0) return ULTRA_ERR_BAD_SHAPE;
    if (sum_op < 0 || sum_op > 2 || mul_op < 0 || mul_op > 1) return ULTRA_ERR_BAD_OP;
    if (fwd->n_edges == 0) return ULTRA_OK;
    if (relation == nullptr || input == nullptr || output_grad == nullptr || d_weight == nullptr)
        return ULTRA_ERR_NULL_POINTER;
    if (sum_op != ULTRA_SUM_ADD && output == nullptr) return ULTRA_ERR_NULL_POINTER;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const bool unit = fwd->weight == nullptr;
    long long blocks = (fwd->n_edges + 3) / 4;
    if (blocks > 8192) blocks = 8192;
    return with_sum_mul(sum_op, mul_op, [&](auto sum, auto mul) {
        return with_bool(unit, [&](auto uw) -> int {
            hipLaunchKernelGGL((weight_grad_kernel<decltype(sum)::value, decltype(mul)::value, decltype(uw)::value>), dim3((int)blocks),
                               dim3(256), 0, s, fwd->row, fwd->node_a, fwd->rel, fwd->weight, relation, input, output, output_grad,
                               d_weight, (long long)F, (long long)fwd->n_edges);
            HIP_TRY(hipGetLastError());
            return ULTRA_OK;
        });
    });
}

int ultra_rspmm_backward_weight_blocks_f32(const ultra_segments *fwd, const float *relation, const float *input,
                                           const float *output, const float *output_grad, float *d_weight, int64_t n_rel,
                                           int64_t F, int64_t block, int sum_op, int mul_op, void *stream) {
    int rc = check_segments(fwd);
    if (rc) return rc;
    (void)n_rel;
    if (F <= 0 || block <= 0 || F % block != 0) return ULTRA_ERR_BAD_SHAPE;
    if (sum_op < 0 || sum_op > 2 || mul_op < 0 || mul_op > 1) return ULTRA_ERR_BAD_OP;
    if (fwd->n_edges == 0) return ULTRA_OK;
    if (relation == nullptr || input == nullptr || output_grad == nullptr || d_weight == nullptr)
        return ULTRA_ERR_NULL_POINTER;
    if (sum_op != ULTRA_SUM_ADD && output == nullptr) return ULTRA_ERR_NULL_POINTER;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const bool unit = fwd->weight == nullptr;
    long long blocks = (fwd->n_edges + 3) / 4;
    if (blocks > 8192) blocks = 8192;
    return with_sum_mul(sum_op, mul_op, [&](auto sum, auto mul) {
        return with_bool(unit, [&](auto uw) -> int {
            hipLaunchKernelGGL((weight_grad_blocks_kernel<decltype(sum)::value, decltype(mul)::value, decltype(uw)::value>),
                               dim3((int)blocks), dim3(256), 0, s, fwd->row, fwd->node_a, fwd->rel, fwd->weight, relation, input,
                               output, output_grad, d_weight, (long long)F, (long long)block, (long long)(F / block),
                               (long long)fwd->n_edges);
            HIP_TRY(hipGetLastError());
            return ULTRA_OK;
        });
    });
}

}  // extern "C"

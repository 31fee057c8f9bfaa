// score_backward.hip -- backward of the score head over ALL entities (a translation unit of libultra_rspmm.so; C ABI:
// ultra_score_backward_f32 in include/ultra_rspmm.h).
//
//     score[b, v] = w2 . relu( W1 . cat[ hidden[v, b, :], query[b, :] ] + b1 ) + b2            (ultra_score_forward_f32)
//
// Nothing of the forward is kept but its inputs.  With  c[b] = b1 + W1[:, 64:] . query[b]  (once per query, as the forward
// does) a row (v, b) is
//     pre    = c[b] + W1[:, :64] . hidden[v, b]                         product 1   (32 rows x 64) . (64 x 128)
//     d_pre  = pre > 0 ? grad[b, v] * w2 : 0                            the mask of ultra_score_rows_backward_f32
//     d_hidden[v, b] = d_pre . W1[:, :64]                               product 2   (32 rows x 128) . (128 x 64)
//     d_W1[:, :64]  += d_pre^T . hidden[v, b]                           product 3   (128 x 32 rows) . (32 rows x 64)
// and everything the query half needs is ONE vector per query, S[b] = sum_v d_pre[v, b]:
//     d_query[b] = S[b] . W1[:, 64:]      d_W1[:, 64:] = sum_b S[b]^T query[b]      d_b1 = sum_b S[b]
// so the three 128-wide products of a row shrink to three 64 x 128 ones (49 kFLOP a row).  They run on the exact-f32 matrix
// cores (v_mfma_f32_32x32x2_f32), W1[:, :64] as an LDS image, a wave-private tile of 32 rows of ONE query (blockIdx.y = b; rows
// v0 .. v0 + 31, 256 contiguous bytes each).  d_pre never leaves the CU: no (N * B, 128) activation exists anywhere.
//   score_backward_query_kernel    c[b]
//   score_backward_kernel          the three products; per WORKGROUP one record {d_W1[:, :64], S, d_w2, d_b2} of partial sums: the
//                                  four waves' registers are added in wave order through LDS
//   score_backward_reduce_kernel   records added in block order: d_W1[:, :64], d_w2, d_b2, S[b]
//   score_backward_query_grad_kernel  d_query, d_W1[:, 64:], d_b1 from S
// Every sum has a fixed order: the same bits on every call.  A row's d_hidden depends on the row's own operands alone (its
// place in the tile picks the lane, not the arithmetic).  All offsets are 64-bit.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "device_common.h"
#include "host_common.h"

namespace {

using namespace ultra_detail;

constexpr int kSbWaves = 4;
constexpr int kSbRows = 32;                     // rows of a tile
constexpr int kXs = 64 + 4;                     // tile of hidden rows / W1 image: row stride in floats
constexpr int kDs = 128 + 4;                    // tile of d_pre rows
constexpr int kSbWaveFloats = kSbRows * kXs + kSbRows * kDs + kSbRows;
constexpr int kSbLdsFloats = 128 * kXs + kSbWaves * kSbWaveFloats;
constexpr int kSbRecord = 128 * 64 + 128 + 128 + 4;       // floats of a workgroup's record: d_W1[:, :64] | S | d_w2 | d_b2, pad
static_assert(128 * 64 + kSbWaves * 260 <= kSbLdsFloats, "the block's fold fits the tiles it reuses");

struct ScoreBwdParams {
    const float *hidden;      // [n_node, B, 64]
    const float *query;       // [B, 64]
    const float *w1;          // [128, 128]
    const float *b1;          // [128]
    const float *w2;          // [128]
    const float *grad;        // [B] rows of n_node at grad_stride
    float *c;                 // [B, 128]      workspace
    float *records;           // [B * blocks_per_query, kSbRecord]
    float *s_total;           // [B, 128]
    float *d_hidden, *d_query, *d_w1, *d_b1, *d_w2, *d_b2;
    long long n_node, n_batch, grad_stride;
    int blocks_per_query;
};

__global__ __launch_bounds__(128) void score_backward_query_kernel(const ScoreBwdParams p) {
    const long long b = blockIdx.x;
    const int o = threadIdx.x;
    float acc = p.b1[o];
    for (int j = 0; j < 32; ++j) {              // k = 64, 96, 65, 97, ...: the chain of ultra_score_forward_f32's query share
        acc = __builtin_fmaf(p.w1[o * 128 + 64 + j], p.query[b * 64 + j], acc);
        acc = __builtin_fmaf(p.w1[o * 128 + 96 + j], p.query[b * 64 + 32 + j], acc);
    }
    p.c[b * 128 + o] = acc;
}

__global__ __launch_bounds__(kSbWaves * 64, 1) void score_backward_kernel(const ScoreBwdParams p) {
    extern __shared__ __attribute__((aligned(16))) float sb_lds[];
    float *w_lds = sb_lds;                                                    // [128 o][kXs]: W1[o][:64]
    const int lane = threadIdx.x & 63;
    const int wl = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    float *xt = sb_lds + 128 * kXs + wl * kSbWaveFloats;                      // [32 rows][kXs]   hidden rows
    float *dt = xt + kSbRows * kXs;                                           // [32 rows][kDs]   d_pre rows
    float *gt = dt + kSbRows * kDs;                                           // [32]             grad of the rows
    const int i = lane & 31, h = lane >> 5;
    const long long b = blockIdx.y, B = p.n_batch, N = p.n_node;
    for (int idx = threadIdx.x; idx < 128 * 16; idx += kSbWaves * 64) {
        const int o = idx >> 4, c4 = (idx & 15) * 4;
        *reinterpret_cast<f32x4 *>(w_lds + o * kXs + c4) = *reinterpret_cast<const f32x4 *>(p.w1 + o * 128 + c4);
    }
    __syncthreads();
    float cq[4], w2v[4], s_acc[4], w2_acc[4];
#pragma unroll
    for (int tt = 0; tt < 4; ++tt) {
        cq[tt] = p.c[b * 128 + 32 * tt + i];
        w2v[tt] = p.w2[32 * tt + i];
        s_acc[tt] = 0.0f;
        w2_acc[tt] = 0.0f;
    }
    float g_acc = 0.0f;
    f32x16 dw[4][2];                                                          // d_W1[32 tt + row(r, h)][32 kt + i]
#pragma unroll
    for (int tt = 0; tt < 4; ++tt)
#pragma unroll
        for (int kt = 0; kt < 2; ++kt)
#pragma unroll
            for (int r = 0; r < 16; ++r) dw[tt][kt][r] = 0.0f;
    const bool want_hidden = p.d_hidden != nullptr, want_w1 = p.d_w1 != nullptr;
    const long long n_tiles = (N + kSbRows - 1) / kSbRows;
    for (long long t = (long long)blockIdx.x * kSbWaves + wl; t < n_tiles; t += (long long)gridDim.x * kSbWaves) {
        const long long v0 = t * kSbRows;
        // ---- stage: 32 rows of 64 floats (rows past the end are zeros: they add nothing anywhere), their grad
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const int r = 4 * q + (lane >> 4), c = (lane & 15) * 4;
            f32x4 x = {0.0f, 0.0f, 0.0f, 0.0f};
            if (v0 + r < N) x = *reinterpret_cast<const f32x4 *>(p.hidden + ((v0 + r) * B + b) * 64 + c);
            *reinterpret_cast<f32x4 *>(xt + r * kXs + c) = x;
        }
        if (lane < kSbRows) {
            const float g = v0 + lane < N ? p.grad[b * p.grad_stride + v0 + lane] : 0.0f;
            gt[lane] = g;
            g_acc = g_acc + g;
        }
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
        // ---- product 1: pre[row][o] = c[o] + sum_k hidden[row][k] W1[o][k]
        f32x16 acc[4];
#pragma unroll
        for (int tt = 0; tt < 4; ++tt)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[tt][r] = cq[tt];
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const f32x4 av = *reinterpret_cast<const f32x4 *>(xt + i * kXs + 32 * h + 4 * q);
#pragma unroll
            for (int tt = 0; tt < 4; ++tt) {
                const f32x4 wv = *reinterpret_cast<const f32x4 *>(w_lds + (32 * tt + i) * kXs + 32 * h + 4 * q);
                acc[tt] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.x, wv.x, acc[tt], 0, 0, 0);
                acc[tt] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.y, wv.y, acc[tt], 0, 0, 0);
                acc[tt] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.z, wv.z, acc[tt], 0, 0, 0);
                acc[tt] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.w, wv.w, acc[tt], 0, 0, 0);
            }
        }
        // ---- d_pre from the accumulators: register r of lane (i, h) is row (r & 3) + 8 (r >> 2) + 4 h, column 32 tt + i
        float gr[16];
#pragma unroll
        for (int g4 = 0; g4 < 4; ++g4) {
            const f32x4 gv = *reinterpret_cast<const f32x4 *>(gt + 8 * g4 + 4 * h);
            gr[4 * g4 + 0] = gv.x; gr[4 * g4 + 1] = gv.y; gr[4 * g4 + 2] = gv.z; gr[4 * g4 + 3] = gv.w;
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = (r & 3) + 8 * (r >> 2) + 4 * h;
            const bool valid = v0 + row < N;
#pragma unroll
            for (int tt = 0; tt < 4; ++tt) {
                const float pre = acc[tt][r];
                const bool on = valid && pre > 0.0f;                          // (false for a NaN)
                const float d = on ? gr[r] * w2v[tt] : 0.0f;
                const float gh = on ? gr[r] * pre : 0.0f;
                s_acc[tt] = s_acc[tt] + d;
                w2_acc[tt] = w2_acc[tt] + gh;
                dt[row * kDs + 32 * tt + i] = d;
            }
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        // ---- product 2: d_hidden[row][k] = sum_o d_pre[row][o] W1[o][k]
        if (want_hidden) {
            f32x16 a2[2];
#pragma unroll
            for (int kt = 0; kt < 2; ++kt)
#pragma unroll
                for (int r = 0; r < 16; ++r) a2[kt][r] = 0.0f;
#pragma unroll 4
            for (int q = 0; q < 16; ++q) {
                const f32x4 av = *reinterpret_cast<const f32x4 *>(dt + i * kDs + 64 * h + 4 * q);
                const float *wrow = w_lds + (64 * h + 4 * q) * kXs + i;
#pragma unroll
                for (int kt = 0; kt < 2; ++kt) {
                    a2[kt] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.x, wrow[0 * kXs + 32 * kt], a2[kt], 0, 0, 0);
                    a2[kt] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.y, wrow[1 * kXs + 32 * kt], a2[kt], 0, 0, 0);
                    a2[kt] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.z, wrow[2 * kXs + 32 * kt], a2[kt], 0, 0, 0);
                    a2[kt] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.w, wrow[3 * kXs + 32 * kt], a2[kt], 0, 0, 0);
                }
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = (r & 3) + 8 * (r >> 2) + 4 * h;
                if (v0 + row < N) {
                    float *out = p.d_hidden + ((v0 + row) * B + b) * 64 + i;
                    out[0] = a2[0][r];
                    out[32] = a2[1][r];
                }
            }
        }
        // ---- product 3: d_W1[o][k] += sum_rows d_pre[row][o] hidden[row][k]
        if (want_w1) {
#pragma unroll 4
            for (int s = 0; s < 16; ++s) {
                const int row = 2 * s + h;
                float a[4], x[2];
#pragma unroll
                for (int tt = 0; tt < 4; ++tt) a[tt] = dt[row * kDs + 32 * tt + i];
#pragma unroll
                for (int kt = 0; kt < 2; ++kt) x[kt] = xt[row * kXs + 32 * kt + i];
#pragma unroll
                for (int tt = 0; tt < 4; ++tt)
#pragma unroll
                    for (int kt = 0; kt < 2; ++kt)
                        dw[tt][kt] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[tt], x[kt], dw[tt][kt], 0, 0, 0);
            }
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");                    // the next tile restages xt / dt / gt
    }
    // ---- the workgroup's record: the four waves' sums added in wave order through LDS (the tiles are done with)
    __syncthreads();
    float *fold = sb_lds;                                                     // [128 o][64 k]
    float *small = sb_lds + 128 * 64;                                         // [4 waves][260]: S | d_w2 | d_b2
    for (int w = 0; w < kSbWaves; ++w) {
        if (wl == w) {
#pragma unroll
            for (int tt = 0; tt < 4; ++tt)
#pragma unroll
                for (int kt = 0; kt < 2; ++kt)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int o = 32 * tt + (r & 3) + 8 * (r >> 2) + 4 * h;
                        float *at = fold + o * 64 + 32 * kt + i;
                        *at = w == 0 ? dw[tt][kt][r] : *at + dw[tt][kt][r];
                    }
        }
        __syncthreads();
    }
    {
        float g = g_acc;
#pragma unroll
        for (int m = 32; m > 0; m >>= 1) g = g + __shfl_xor(g, m, 64);
#pragma unroll
        for (int tt = 0; tt < 4; ++tt) {
            const float s = s_acc[tt] + __shfl_xor(s_acc[tt], 32, 64);        // rows of h = 0 and of h = 1
            const float u = w2_acc[tt] + __shfl_xor(w2_acc[tt], 32, 64);
            if (h == 0) {
                small[wl * 260 + 32 * tt + i] = s;
                small[wl * 260 + 128 + 32 * tt + i] = u;
            }
        }
        if (lane == 0) small[wl * 260 + 256] = g;
    }
    __syncthreads();
    float *rec = p.records + (b * p.blocks_per_query + blockIdx.x) * (long long)kSbRecord;
    for (int idx = threadIdx.x; idx < 128 * 16; idx += kSbWaves * 64)
        reinterpret_cast<f32x4 *>(rec)[idx] = reinterpret_cast<const f32x4 *>(fold)[idx];
    for (int idx = threadIdx.x; idx < 257; idx += kSbWaves * 64) {
        float total = small[idx];
        for (int w = 1; w < kSbWaves; ++w) total = total + small[w * 260 + idx];
        rec[128 * 64 + idx] = total;
    }
}

// records added in block order.  Thread e: e < 8192: d_W1[o][k < 64]; then 128 of d_w2; d_b2; then S[b][o] over the blocks of b.
__global__ __launch_bounds__(256) void score_backward_reduce_kernel(const ScoreBwdParams p) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long n_rec = p.n_batch * p.blocks_per_query;
    if (e < 128 * 64 + 129) {
        float total = 0.0f;
        const long long at = e < 128 * 64 ? e : e + 128;                      // (S lies between d_W1 and d_w2)
#pragma unroll 8
        for (long long r = 0; r < n_rec; ++r) total = total + p.records[r * kSbRecord + at];
        if (e < 128 * 64) {
            if (p.d_w1 != nullptr) p.d_w1[(e >> 6) * 128 + (e & 63)] = total;
        } else if (e < 128 * 64 + 128) {
            if (p.d_w2 != nullptr) p.d_w2[e - 128 * 64] = total;
        } else if (p.d_b2 != nullptr) {
            p.d_b2[0] = total;
        }
        return;
    }
    const long long se = e - (128 * 64 + 129);
    if (se >= p.n_batch * 128) return;
    const long long b = se >> 7;
    const int o = (int)(se & 127);
    float total = 0.0f;
    for (int r = 0; r < p.blocks_per_query; ++r) total = total + p.records[(b * p.blocks_per_query + r) * kSbRecord + 128 * 64 + o];
    p.s_total[se] = total;
}

// what the query half of the first layer gets, from S alone.  Thread e: e < 8192: d_W1[o][64 + k] = sum_b S[b][o] query[b][k];
// then 128 of d_b1[o] = sum_b S[b][o]; then d_query[b][k] = sum_o S[b][o] W1[o][64 + k].
__global__ __launch_bounds__(256) void score_backward_query_grad_kernel(const ScoreBwdParams p) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e < 128 * 64) {
        if (p.d_w1 == nullptr) return;
        const int o = (int)(e >> 6), k = (int)(e & 63);
        float total = 0.0f;
        for (long long b = 0; b < p.n_batch; ++b) total = __builtin_fmaf(p.s_total[b * 128 + o], p.query[b * 64 + k], total);
        p.d_w1[o * 128 + 64 + k] = total;
    } else if (e < 128 * 64 + 128) {
        if (p.d_b1 == nullptr) return;
        const int o = (int)(e - 128 * 64);
        float total = 0.0f;
        for (long long b = 0; b < p.n_batch; ++b) total = total + p.s_total[b * 128 + o];
        p.d_b1[o] = total;
    } else {
        const long long qe = e - (128 * 64 + 128);
        if (p.d_query == nullptr || qe >= p.n_batch * 64) return;
        const long long b = qe >> 6;
        const int k = (int)(qe & 63);
        float total = 0.0f;
        for (int o = 0; o < 128; ++o) total = __builtin_fmaf(p.s_total[b * 128 + o], p.w1[o * 128 + 64 + k], total);
        p.d_query[qe] = total;
    }
}

// workgroups per query: the device's CUs shared among the queries, at most one per four tiles
int blocks_per_query(long long n_node, long long batch, int n_cu) {
    const long long n_tiles = (n_node + kSbRows - 1) / kSbRows;
    long long most = (n_tiles + kSbWaves - 1) / kSbWaves;
    long long want = (n_cu + batch - 1) / batch;
    if (want < 1) want = 1;
    return (int)(want < most ? want : most);
}

size_t workspace_floats(long long batch, int per_query) {
    return (size_t)batch * 128 * 2 + (size_t)batch * per_query * kSbRecord;
}

}  // namespace

extern "C" size_t ultra_score_backward_workspace(int64_t n_node, int64_t batch) {
    if (n_node < 1 || batch < 1 || batch > 65535) return 0;
    DeviceInfo *di = nullptr;
    if (current_device_info(&di)) return 0;
    return workspace_floats(batch, blocks_per_query(n_node, batch, di->n_cu)) * sizeof(float);
}

extern "C" int ultra_score_backward_f32(const float *hidden, const float *query, const float *w1, const float *b1, const float *w2,
                                        const float *grad, int64_t grad_stride, float *d_hidden, float *d_query, float *d_w1,
                                        float *d_b1, float *d_w2, float *d_b2, void *workspace, size_t workspace_bytes,
                                        int64_t n_node, int64_t batch, void *stream) {
    if (n_node < 1 || batch < 1 || batch > 65535 || grad_stride < n_node) return ULTRA_ERR_BAD_SHAPE;
    if (n_node > (1ll << 50) / batch || grad_stride > (1ll << 56) / batch) return ULTRA_ERR_BAD_SHAPE;
    if (hidden == nullptr || query == nullptr || w1 == nullptr || b1 == nullptr || w2 == nullptr || grad == nullptr ||
        workspace == nullptr)
        return ULTRA_ERR_NULL_POINTER;
    if (((reinterpret_cast<uintptr_t>(hidden) | reinterpret_cast<uintptr_t>(w1) | reinterpret_cast<uintptr_t>(workspace)) & 15u) != 0)
        return ULTRA_ERR_BAD_SHAPE;
    DeviceInfo *di = nullptr;
    int rc = current_device_info(&di);
    if (rc) return rc;
    const int per_query = blocks_per_query(n_node, batch, di->n_cu);
    if (workspace_bytes < workspace_floats(batch, per_query) * sizeof(float)) return ULTRA_ERR_WORKSPACE;
    ScoreBwdParams p{};
    p.hidden = hidden; p.query = query; p.w1 = w1; p.b1 = b1; p.w2 = w2; p.grad = grad;
    p.c = static_cast<float *>(workspace);
    p.s_total = p.c + batch * 128;
    p.records = p.s_total + batch * 128;
    p.d_hidden = d_hidden; p.d_query = d_query; p.d_w1 = d_w1; p.d_b1 = d_b1; p.d_w2 = d_w2; p.d_b2 = d_b2;
    p.n_node = n_node; p.n_batch = batch; p.grad_stride = grad_stride; p.blocks_per_query = per_query;
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(score_backward_query_kernel, dim3((unsigned)batch), dim3(128), 0, s, p);
    HIP_TRY(hipGetLastError());
    const size_t lds = (size_t)kSbLdsFloats * sizeof(float);
    rc = ensure_lds_attribute(reinterpret_cast<const void *>(score_backward_kernel), lds);
    if (rc) return rc;
    hipLaunchKernelGGL(score_backward_kernel, dim3((unsigned)per_query, (unsigned)batch), dim3(kSbWaves * 64), lds, s, p);
    HIP_TRY(hipGetLastError());
    if (d_query == nullptr && d_w1 == nullptr && d_b1 == nullptr && d_w2 == nullptr && d_b2 == nullptr) return ULTRA_OK;
    const long long n_reduce = 128 * 64 + 129 + batch * 128;
    hipLaunchKernelGGL(score_backward_reduce_kernel, dim3((unsigned)((n_reduce + 255) / 256)), dim3(256), 0, s, p);
    const long long n_small = 128 * 64 + 128 + batch * 64;
    hipLaunchKernelGGL(score_backward_query_grad_kernel, dim3((unsigned)((n_small + 255) / 256)), dim3(256), 0, s, p);
    HIP_TRY(hipGetLastError());
    return ULTRA_OK;
}

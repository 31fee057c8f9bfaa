// query_tables.hip -- the per-query relation tables of ALL layers of a NeuralBellmanFordNetwork (`dependent=True`,
// ultra/layer.py:48,58-61) in one launch, and their backward (a translation unit of libultra_rspmm.so; C ABI:
// ultra_query_tables_f32, ultra_query_tables_backward_f32 and ultra_query_tables_backward_workspace in include/ultra_rspmm.h;
// DESIGN.md section 23).
//
//     out[l][r, b, d] = bias[l][r*D + d] + sum_k w[l][r*D + d, k] * query[b, k]        l < n_layers, r < n_rel, b < batch, d < D_l
//
// = relation_linear(query).view(B, R, D).transpose(0, 1) of every layer, written straight into the (n_rel, batch * D) layout the
// rspmm reads.  A weight row j = r*D + d belongs to ONE thread: a workgroup of kRows = 128 threads owns 128 consecutive rows of
// one layer (blockIdx.y), stages their weights (a contiguous run of memory) into LDS with coalesced loads, and the query block
// -- kQB = 32 queries at a time, transposed so that a thread reads the 32 values of one k as eight broadcast 16-byte loads --
// beside them.  A thread then keeps 32 accumulators, one per query, and walks k ASCENDING: acc[b] = fmaf(w[j][k], query[b][k],
// acc[b]) from acc[b] = bias[j].  That is the order the header states; K above kKC = 64 is walked in chunks of 64 columns with
// the same accumulators, so the chain is the same whatever K is.  With K <= 64 the weight tile is staged once and stays in LDS
// over all query blocks.  The stores of a wave are 64 consecutive floats (one d-run of a relation, or several for narrow layers).
//
// Backward, three kernels in one call, no atomics:
//   dw_kernel       the forward's tiling; a thread keeps the 64 entries d_w[j][k0 .. k0+64) of its row in registers and walks
//                   b ASCENDING: d_w[j][k] = fmaf(grad[j][b], query[b][k], d_w[j][k]) from +0.0, d_bias[j] += grad[j][b]; the
//                   rows leave through LDS so that the stores are coalesced.  A NULL grad[l] writes zeros.
//   dquery_kernel   a workgroup owns kTilesB = 4 row tiles of one layer and computes its partial [batch][K] block of
//                   d_query = grad^T . w: thread (k, half) keeps 16 queries' sums for its column, rows ascending.  One partial
//                   block per workgroup goes to the workspace; the workgroups of a layer whose grad is NULL do nothing.
//   dquery_reduce   d_query[b][k] = the partial blocks added in ASCENDING block order (layer by layer, tile by tile); the
//                   layers without a gradient are skipped, not read.
// All addressing is 64-bit.  Grids follow from the shapes alone.  Rows past the end of a layer are never loaded or stored.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "host_common.h"

namespace {

constexpr int kRows = 128;           // threads of a workgroup = weight rows of a tile
constexpr int kKC = 64;              // columns of k per chunk
constexpr int kQB = 32;              // queries per block of the batch
constexpr int kTilesB = 4;           // row tiles per workgroup of dquery_kernel
constexpr int kMaxLayers = 8;

struct TableParams {
    const float *query;
    long long stride_q;
    const float *w[kMaxLayers];
    const float *bias[kMaxLayers];       // backward: unused
    float *out[kMaxLayers];              // backward: unused
    const float *grad[kMaxLayers];       // backward only (NULL: zeros)
    float *d_w[kMaxLayers];
    float *d_bias[kMaxLayers];
    int dims[kMaxLayers];
    long long first_block[kMaxLayers];   // dquery: the layer's first partial block
    long long n_blocks[kMaxLayers];      // dquery: its partial blocks
    int n_layers;
    long long batch, n_rel, K;
    float *partial;
    float *d_query;
};

// rows [j0, j0 + n_rows) x columns [k0, k0 + nk) of a (rows, K) matrix -> tile[row][k], coalesced along k
template <int VEC>
__device__ __forceinline__ void stage_rows(float (*tile)[kKC + 1], const float *__restrict__ w, long long j0, int n_rows,
                                           long long K, long long k0, int nk, int t) {
    if constexpr (VEC == 4) {
        const int per = nk / 4;
        for (int idx = t; idx < n_rows * per; idx += kRows) {
            const int row = idx / per, k = (idx % per) * 4;
            const float4 v = *reinterpret_cast<const float4 *>(w + (j0 + row) * K + k0 + k);
            tile[row][k] = v.x; tile[row][k + 1] = v.y; tile[row][k + 2] = v.z; tile[row][k + 3] = v.w;
        }
    } else {
        for (int idx = t; idx < n_rows * nk; idx += kRows) {
            const int row = idx / nk, k = idx % nk;
            tile[row][k] = w[(j0 + row) * K + k0 + k];
        }
    }
}

template <int VEC>
__global__ __launch_bounds__(kRows) void query_tables_kernel(TableParams p) {
    __shared__ float w_lds[kRows][kKC + 1];
    __shared__ __attribute__((aligned(16))) float q_lds[kKC][kQB];          // transposed: [k][b]
    const int l = (int)blockIdx.y;
    const long long D = p.dims[l];
    const long long rows = p.n_rel * D;
    const long long j0 = (long long)blockIdx.x * kRows;
    if (j0 >= rows) return;                                                  // (the grid is sized for the widest layer)
    const int t = (int)threadIdx.x;
    const long long j = j0 + t;
    const bool live = j < rows;
    const int n_rows = (int)(rows - j0 < kRows ? rows - j0 : kRows);
    const float *__restrict__ w = p.w[l];
    const float *__restrict__ query = p.query;
    const float start = live ? p.bias[l][j] : 0.0f;
    const bool one_chunk = p.K <= kKC;
    for (long long q0 = 0; q0 < p.batch; q0 += kQB) {
        const int nq = (int)(p.batch - q0 < kQB ? p.batch - q0 : kQB);
        float acc[kQB];
#pragma unroll
        for (int b = 0; b < kQB; ++b) acc[b] = start;
        for (long long k0 = 0; k0 < p.K; k0 += kKC) {
            const int nk = (int)(p.K - k0 < kKC ? p.K - k0 : kKC);
            __syncthreads();                                                 // the readers of the last chunk are done
            if (!(one_chunk && q0 > 0)) stage_rows<VEC>(w_lds, w, j0, n_rows, p.K, k0, nk, t);
            for (int idx = t; idx < kQB * nk; idx += kRows) {                // queries past the batch: +0.0, never stored
                const int b = idx / nk, k = idx % nk;
                q_lds[k][b] = b < nq ? query[(q0 + b) * p.stride_q + k0 + k] : 0.0f;
            }
            __syncthreads();
            if (live) {
                for (int k = 0; k < nk; ++k) {                               // k ascending: the documented order
                    const float wv = w_lds[t][k];
#pragma unroll
                    for (int b4 = 0; b4 < kQB; b4 += 4) {
                        const float4 q = *reinterpret_cast<const float4 *>(&q_lds[k][b4]);
                        acc[b4] = fmaf(wv, q.x, acc[b4]);
                        acc[b4 + 1] = fmaf(wv, q.y, acc[b4 + 1]);
                        acc[b4 + 2] = fmaf(wv, q.z, acc[b4 + 2]);
                        acc[b4 + 3] = fmaf(wv, q.w, acc[b4 + 3]);
                    }
                }
            }
        }
        if (live) {
            const long long r = j / D, d = j % D;
            float *__restrict__ o = p.out[l] + (r * p.batch + q0) * D + d;
#pragma unroll
            for (int b = 0; b < kQB; ++b)
                if (b < nq) o[(long long)b * D] = acc[b];
        }
    }
}

template <int VEC>
__global__ __launch_bounds__(kRows) void query_tables_dw_kernel(TableParams p) {
    __shared__ float w_lds[kRows][kKC + 1];                                 // the rows of d_w on their way out
    __shared__ __attribute__((aligned(16))) float q_lds[kQB][kKC];          // [b][k]
    const int l = (int)blockIdx.y;
    const long long D = p.dims[l];
    const long long rows = p.n_rel * D;
    const long long j0 = (long long)blockIdx.x * kRows;
    if (j0 >= rows) return;
    const int t = (int)threadIdx.x;
    const long long j = j0 + t;
    const bool live = j < rows;
    const int n_rows = (int)(rows - j0 < kRows ? rows - j0 : kRows);
    const float *__restrict__ query = p.query;
    const float *__restrict__ grad = p.grad[l];
    const long long r = live ? j / D : 0, d = live ? j % D : 0;
    const bool read = live && grad != nullptr;
    for (long long k0 = 0; k0 < p.K; k0 += kKC) {
        const int nk = (int)(p.K - k0 < kKC ? p.K - k0 : kKC);
        float dw[kKC];
#pragma unroll
        for (int k = 0; k < kKC; ++k) dw[k] = 0.0f;
        float db = 0.0f;
        for (long long q0 = 0; q0 < p.batch; q0 += kQB) {
            const int nq = (int)(p.batch - q0 < kQB ? p.batch - q0 : kQB);
            __syncthreads();
            for (int idx = t; idx < nq * kKC; idx += kRows) {                // columns past K: +0.0, never stored
                const int b = idx / kKC, k = idx % kKC;
                q_lds[b][k] = k < nk ? query[(q0 + b) * p.stride_q + k0 + k] : 0.0f;
            }
            __syncthreads();
            if (read) {
                const float *__restrict__ g = grad + (r * p.batch + q0) * D + d;
                for (int b = 0; b < nq; ++b) {                               // b ascending
                    const float gv = g[(long long)b * D];
                    db = db + gv;
#pragma unroll
                    for (int k4 = 0; k4 < kKC; k4 += 4) {
                        const float4 q = *reinterpret_cast<const float4 *>(&q_lds[b][k4]);
                        dw[k4] = fmaf(gv, q.x, dw[k4]);
                        dw[k4 + 1] = fmaf(gv, q.y, dw[k4 + 1]);
                        dw[k4 + 2] = fmaf(gv, q.z, dw[k4 + 2]);
                        dw[k4 + 3] = fmaf(gv, q.w, dw[k4 + 3]);
                    }
                }
            }
        }
        if (live && k0 == 0) p.d_bias[l][j] = db;
        __syncthreads();                                                     // the stores of the last chunk have read w_lds
#pragma unroll
        for (int k = 0; k < kKC; ++k) w_lds[t][k] = dw[k];
        __syncthreads();
        float *__restrict__ out = p.d_w[l];
        if constexpr (VEC == 4) {
            const int per = nk / 4;
            for (int idx = t; idx < n_rows * per; idx += kRows) {
                const int row = idx / per, k = (idx % per) * 4;
                *reinterpret_cast<float4 *>(out + (j0 + row) * p.K + k0 + k) =
                    make_float4(w_lds[row][k], w_lds[row][k + 1], w_lds[row][k + 2], w_lds[row][k + 3]);
            }
        } else {
            for (int idx = t; idx < n_rows * nk; idx += kRows) {
                const int row = idx / nk, k = idx % nk;
                out[(j0 + row) * p.K + k0 + k] = w_lds[row][k];
            }
        }
    }
}

template <int VEC>
__global__ __launch_bounds__(kRows) void query_tables_dquery_kernel(TableParams p) {
    __shared__ float w_lds[kRows][kKC + 1];
    __shared__ float g_lds[kQB][kRows];                                      // [b][row]
    const int l = (int)blockIdx.y;
    if ((long long)blockIdx.x >= p.n_blocks[l] || p.grad[l] == nullptr) return;
    const long long D = p.dims[l];
    const long long rows = p.n_rel * D;
    const int t = (int)threadIdx.x;
    const int k = t % kKC, half = t / kKC;                                   // 16 queries per half
    constexpr int kPer = kQB / (kRows / kKC);
    const float *__restrict__ w = p.w[l];
    const float *__restrict__ grad = p.grad[l];
    float *__restrict__ partial = p.partial + (p.first_block[l] + blockIdx.x) * (p.batch * p.K);
    for (long long q0 = 0; q0 < p.batch; q0 += kQB) {
        const int nq = (int)(p.batch - q0 < kQB ? p.batch - q0 : kQB);
        for (long long k0 = 0; k0 < p.K; k0 += kKC) {
            const int nk = (int)(p.K - k0 < kKC ? p.K - k0 : kKC);
            float acc[kPer];
#pragma unroll
            for (int i = 0; i < kPer; ++i) acc[i] = 0.0f;
            for (int tile = 0; tile < kTilesB; ++tile) {
                const long long j0 = ((long long)blockIdx.x * kTilesB + tile) * kRows;
                if (j0 >= rows) break;                                       // (uniform over the workgroup)
                const int n_rows = (int)(rows - j0 < kRows ? rows - j0 : kRows);
                __syncthreads();
                stage_rows<VEC>(w_lds, w, j0, n_rows, p.K, k0, nk, t);
                for (int idx = t; idx < kQB * n_rows; idx += kRows) {        // queries past the batch: +0.0
                    const int b = idx / n_rows, row = idx % n_rows;
                    const long long j = j0 + row;
                    g_lds[b][row] = b < nq ? grad[(j / D * p.batch + q0 + b) * D + j % D] : 0.0f;
                }
                __syncthreads();
                if (k < nk) {
                    for (int row = 0; row < n_rows; ++row) {                 // rows ascending
                        const float wv = w_lds[row][k];
#pragma unroll
                        for (int i = 0; i < kPer; ++i) acc[i] = fmaf(g_lds[half * kPer + i][row], wv, acc[i]);
                    }
                }
            }
            if (k < nk) {
#pragma unroll
                for (int i = 0; i < kPer; ++i) {
                    const int b = half * kPer + i;
                    if (b < nq) partial[(q0 + b) * p.K + k0 + k] = acc[i];
                }
            }
        }
    }
}

__global__ __launch_bounds__(256) void query_tables_dquery_reduce_kernel(TableParams p) {
    const long long n = p.batch * p.K;
    const long long at = (long long)blockIdx.x * 256 + threadIdx.x;
    if (at >= n) return;
    float total = 0.0f;
    for (int l = 0; l < p.n_layers; ++l) {
        if (p.grad[l] == nullptr) continue;
        const float *__restrict__ src = p.partial + p.first_block[l] * n + at;
        for (long long b = 0; b < p.n_blocks[l]; ++b) total = total + src[b * n];
    }
    p.d_query[at] = total;
}

// what every entry checks of the shape; fills the block table of the d_query partials
int check_shape(int64_t n_layers, int64_t batch, int64_t n_rel, const int64_t *dims, int64_t K, TableParams *p,
                long long *total_blocks, long long *widest) {
    if (n_layers < 1 || n_layers > kMaxLayers || batch < 0 || n_rel < 0 || K < 1) return ULTRA_ERR_BAD_SHAPE;
    if (dims == nullptr) return ULTRA_ERR_NULL_POINTER;
    // sizes the 64-bit offsets and the 31-bit grids hold (far beyond any device memory)
    if (K > (1ll << 30) || batch > (1ll << 30) || n_rel > (1ll << 30)) return ULTRA_ERR_BAD_SHAPE;
    long long blocks = 0, most = 0;
    for (int l = 0; l < n_layers; ++l) {
        const long long D = dims[l];
        if (D < 1 || D > (1ll << 30)) return ULTRA_ERR_BAD_SHAPE;
        const long long rows = n_rel * D;
        if (rows > (1ll << 36) || (rows > 0 && (batch > (1ll << 60) / rows || K > (1ll << 60) / rows))) return ULTRA_ERR_BAD_SHAPE;
        p->dims[l] = (int)D;
        p->first_block[l] = blocks;
        p->n_blocks[l] = (rows + (long long)kRows * kTilesB - 1) / ((long long)kRows * kTilesB);
        blocks += p->n_blocks[l];
        most = rows > most ? rows : most;
    }
    if (batch > 0 && K > 0 && blocks > (1ll << 60) / (batch * K)) return ULTRA_ERR_BAD_SHAPE;
    p->n_layers = (int)n_layers;
    p->batch = batch;
    p->n_rel = n_rel;
    p->K = K;
    *total_blocks = blocks;
    *widest = most;
    return ULTRA_OK;
}

bool aligned16(const void *ptr) { return (reinterpret_cast<uintptr_t>(ptr) & 15u) == 0; }

}  // namespace

extern "C" int ultra_query_tables_f32(const float *query, int64_t stride_q, const float *const *w, const float *const *bias,
                                      float *const *out, const int64_t *dims, int64_t n_layers, int64_t batch, int64_t n_rel,
                                      int64_t K, void *stream) {
    TableParams p = {};
    long long blocks = 0, widest = 0;
    const int rc = check_shape(n_layers, batch, n_rel, dims, K, &p, &blocks, &widest);
    if (rc) return rc;
    if (stride_q < K) return ULTRA_ERR_BAD_SHAPE;
    if (query == nullptr || w == nullptr || bias == nullptr || out == nullptr) return ULTRA_ERR_NULL_POINTER;
    bool wide = K % 4 == 0;                  // (the weights alone are loaded 16 bytes at a time; the query block is small)
    for (int l = 0; l < n_layers; ++l) {
        if (w[l] == nullptr || bias[l] == nullptr || out[l] == nullptr) return ULTRA_ERR_NULL_POINTER;
        p.w[l] = w[l];
        p.bias[l] = bias[l];
        p.out[l] = out[l];
        wide = wide && aligned16(w[l]);
    }
    if (batch == 0 || n_rel == 0) return ULTRA_OK;
    p.query = query;
    p.stride_q = stride_q;
    const dim3 grid((unsigned)((widest + kRows - 1) / kRows), (unsigned)n_layers);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (wide)
        hipLaunchKernelGGL(query_tables_kernel<4>, grid, dim3(kRows), 0, s, p);
    else
        hipLaunchKernelGGL(query_tables_kernel<1>, grid, dim3(kRows), 0, s, p);
    HIP_TRY(hipGetLastError());
    return ULTRA_OK;
}

// the d_query partial blocks of ultra_query_tables_backward_f32: one [batch][K] block per workgroup of dquery_kernel
extern "C" size_t ultra_query_tables_backward_workspace(int64_t n_layers, int64_t batch, int64_t n_rel, const int64_t *dims,
                                                        int64_t K) {
    TableParams p = {};
    long long blocks = 0, widest = 0;
    if (check_shape(n_layers, batch, n_rel, dims, K, &p, &blocks, &widest) != ULTRA_OK) return 0;
    return (size_t)blocks * (size_t)batch * (size_t)K * sizeof(float);
}

extern "C" int ultra_query_tables_backward_f32(const float *query, int64_t stride_q, const float *const *w,
                                               const float *const *grad, float *const *d_w, float *const *d_bias, float *d_query,
                                               void *workspace, size_t workspace_bytes, const int64_t *dims, int64_t n_layers,
                                               int64_t batch, int64_t n_rel, int64_t K, void *stream) {
    TableParams p = {};
    long long blocks = 0, widest = 0;
    const int rc = check_shape(n_layers, batch, n_rel, dims, K, &p, &blocks, &widest);
    if (rc) return rc;
    if (stride_q < K) return ULTRA_ERR_BAD_SHAPE;
    if (query == nullptr || w == nullptr || grad == nullptr || d_w == nullptr || d_bias == nullptr || d_query == nullptr)
        return ULTRA_ERR_NULL_POINTER;
    bool wide = K % 4 == 0;
    for (int l = 0; l < n_layers; ++l) {
        if (w[l] == nullptr || d_w[l] == nullptr || d_bias[l] == nullptr) return ULTRA_ERR_NULL_POINTER;
        p.w[l] = w[l];
        p.grad[l] = grad[l];
        p.d_w[l] = d_w[l];
        p.d_bias[l] = d_bias[l];
        wide = wide && aligned16(w[l]) && aligned16(d_w[l]);
    }
    const size_t need = (size_t)blocks * (size_t)batch * (size_t)K * sizeof(float);
    if (need > 0 && workspace == nullptr) return ULTRA_ERR_NULL_POINTER;
    if (workspace_bytes < need) return ULTRA_ERR_WORKSPACE;
    if (batch == 0 || n_rel == 0) return ULTRA_OK;
    p.query = query;
    p.stride_q = stride_q;
    p.partial = static_cast<float *>(workspace);
    p.d_query = d_query;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const dim3 grid_w((unsigned)((widest + kRows - 1) / kRows), (unsigned)n_layers);
    const dim3 grid_q((unsigned)((widest + (long long)kRows * kTilesB - 1) / ((long long)kRows * kTilesB)), (unsigned)n_layers);
    if (wide) {
        hipLaunchKernelGGL(query_tables_dw_kernel<4>, grid_w, dim3(kRows), 0, s, p);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(query_tables_dquery_kernel<4>, grid_q, dim3(kRows), 0, s, p);
    } else {
        hipLaunchKernelGGL(query_tables_dw_kernel<1>, grid_w, dim3(kRows), 0, s, p);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(query_tables_dquery_kernel<1>, grid_q, dim3(kRows), 0, s, p);
    }
    HIP_TRY(hipGetLastError());
    const long long n = batch * K;
    hipLaunchKernelGGL(query_tables_dquery_reduce_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, p);
    HIP_TRY(hipGetLastError());
    return ULTRA_OK;
}

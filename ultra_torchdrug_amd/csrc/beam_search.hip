// beam_search.hip -- one step of the path beam search behind TransferNBFNet.visualize / visualize_batch (a translation unit
// of libultra_rspmm.so; C ABI: ultra_beam_search_step_f32 and ultra_beam_search_step_batch_f32 in include/ultra_rspmm.h).
//
// For every destination row v of the coalesced dst-CSR, the K best of the row's (in-edge, source beam) candidates
//     m = input[u, k] + g[e]          (e = u -> v, u != tail, m finite; one f32 add)
// after the per-edge de-duplication of near-equal beams ("Explaining a prediction"):
//     prev(k) = smallest candidate beam k' of the same edge with m_k == m_k' || |m_k - m_k'| <= 1e-8f + 1e-5f * |m_k'|
//     beam k is dropped when beam k - 1 is a candidate too and prev(k) == prev(k - 1)
// ordered by value (descending), then edge position, then k.  Slots without a candidate: -inf, back_edge = back_rank = -1.
// The CPU kernel of torch.ops.ultra_mi.beam_search_step (csrc/torch_ext.cpp) is the same definition, bit for bit.
//
// Shape: one group of G lanes (16 / 32 / 64, from the mean degree) per destination row.  Lane j walks the row's edges
// j, j + G, ... and keeps a private sorted top-K of (value, tie key) in registers (KMAX = K rounded up to 4 / 8 / 16 / 32:
// fully unrolled arrays, no scratch).  The group then emits the row's K results in K rounds of a butterfly arg-max over
// the lanes' heads (__shfl_xor within the group); the winning lane pops its head.  A hub row costs deg / G edges per lane
// -- every lane works on its own edges, nothing is serialised per candidate; there is no split pass.
// The row bounds are clamped to [0, n_edges] and sources outside [0, n_node) are skipped, so malformed arrays cannot make
// the kernel read out of bounds (the torch operator rejects them before the launch); writes go to rows < n_node only.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "host_common.h"

namespace {

constexpr int kThreads = 256;
constexpr unsigned long long kNoKey = ~0ull;

// tie key: (edge position, beam) order; the low 5 bits carry prev(k), which never decides (edge, beam) pairs are distinct
__device__ __forceinline__ unsigned long long make_key(long long e, int k, int prev) {
    return ((unsigned long long)e << 10) | ((unsigned long long)k << 5) | (unsigned long long)prev;
}

__device__ __forceinline__ bool better(float av, unsigned long long ak, float bv, unsigned long long bk) {
    return av > bv || (av == bv && ak < bk);
}

// torch.isclose(a, b, rtol=1e-5, atol=1e-8) in f32 (the library is built with -ffp-contract=off: no fused multiply-add)
__device__ __forceinline__ bool near_equal(float a, float b) {
    if (a == b) return true;
    const float d = fabsf(a - b);
    const float tol = 1e-8f + 1e-5f * fabsf(b);
    return d <= tol;
}

// One destination row of one query: the row code of both kernels below (`grad`, `input` and the outputs are the query's own).
template <int G, int KMAX>
__device__ __forceinline__ void beam_row(const int32_t *__restrict__ row_ptr, const int32_t *__restrict__ src,
                                         const float *__restrict__ grad, const float *__restrict__ input, long long n_node,
                                         long long n_edges, long long tail, int K, float *__restrict__ distance,
                                         int32_t *__restrict__ back_edge, int32_t *__restrict__ back_rank) {
    const long long v = ((long long)blockIdx.x * kThreads + threadIdx.x) / G;
    const int lane = (int)(threadIdx.x % G);
    if (v >= n_node) return;            // whole groups leave together (G divides the block)

    float tv[KMAX];
    unsigned long long tk[KMAX];
#pragma unroll
    for (int i = 0; i < KMAX; ++i) {
        tv[i] = -INFINITY;
        tk[i] = kNoKey;
    }
    long long e0 = row_ptr[v], e1 = row_ptr[v + 1];
    e0 = e0 < 0 ? 0 : e0;
    e1 = e1 > n_edges ? n_edges : e1;
    for (long long e = e0 + lane; e < e1; e += G) {
        const int u = src[e];
        if (u == tail || u < 0 || (long long)u >= n_node) continue;
        const float ge = grad[e];
        const float *in = input + (long long)u * K;
        float m[KMAX];
        bool cand[KMAX];
#pragma unroll
        for (int k = 0; k < KMAX; ++k) {
            m[k] = k < K ? in[k] + ge : -INFINITY;
            cand[k] = k < K && isfinite(m[k]);
        }
        bool last_cand = false;
        int last_prev = -1;
#pragma unroll
        for (int k = 0; k < KMAX; ++k) {
            if (cand[k]) {
                int p = k;
#pragma unroll
                for (int j = KMAX - 1; j >= 0; --j)           // downwards: the smallest matching j is written last
                    if (j < k && cand[j] && near_equal(m[k], m[j])) p = j;
                if (!(last_cand && p == last_prev)) {
                    float cv = m[k];
                    unsigned long long ck = make_key(e, k, p);
#pragma unroll
                    for (int i = 0; i < KMAX; ++i) {            // insertion into the sorted private list
                        if (better(cv, ck, tv[i], tk[i])) {
                            const float sv = tv[i];
                            const unsigned long long sk = tk[i];
                            tv[i] = cv;
                            tk[i] = ck;
                            cv = sv;
                            ck = sk;
                        }
                    }
                }
                last_cand = true;
                last_prev = p;
            } else {
                last_cand = false;
            }
        }
    }

    // K rounds of a group-wide arg-max over the lanes' heads
    for (int r = 0; r < K; ++r) {
        float bv = tv[0];
        unsigned long long bk = tk[0];
#pragma unroll
        for (int off = G / 2; off > 0; off >>= 1) {
            const float ov = __shfl_xor(bv, off, G);
            const unsigned lo = __shfl_xor((unsigned)(bk & 0xffffffffull), off, G);
            const unsigned hi = __shfl_xor((unsigned)(bk >> 32), off, G);
            const unsigned long long ok = ((unsigned long long)hi << 32) | lo;
            if (better(ov, ok, bv, bk)) {
                bv = ov;
                bk = ok;
            }
        }
        if (bk != kNoKey && tk[0] == bk) {      // the winner pops its head
#pragma unroll
            for (int i = 0; i < KMAX - 1; ++i) {
                tv[i] = tv[i + 1];
                tk[i] = tk[i + 1];
            }
            tv[KMAX - 1] = -INFINITY;
            tk[KMAX - 1] = kNoKey;
        }
        if (lane == 0) {
            const long long o = v * K + r;
            const bool none = bk == kNoKey;
            distance[o] = none ? -INFINITY : bv;
            back_edge[o] = none ? -1 : (int32_t)(bk >> 10);
            back_rank[o] = none ? -1 : (int32_t)(bk & 31ull);
        }
    }
}

template <int G, int KMAX>
__global__ __launch_bounds__(kThreads) void beam_step_kernel(const int32_t *__restrict__ row_ptr,
                                                             const int32_t *__restrict__ src,
                                                             const float *__restrict__ grad,
                                                             const float *__restrict__ input, long long n_node,
                                                             long long n_edges, long long tail, int K,
                                                             float *__restrict__ distance, int32_t *__restrict__ back_edge,
                                                             int32_t *__restrict__ back_rank) {
    beam_row<G, KMAX>(row_ptr, src, grad, input, n_node, n_edges, tail, K, distance, back_edge, back_rank);
}

// The same step for n_query queries over one graph: blockIdx.y is the query, whose slices of the batched arrays start at
// 64-bit offsets (q * n_edges, q * n_node * K); its tail comes from device memory.  B groups stand on every row at once, so
// the tail of a hub row is shared by the batch instead of paid once per query.
template <int G, int KMAX>
__global__ __launch_bounds__(kThreads) void beam_step_batch_kernel(const int32_t *__restrict__ row_ptr,
                                                                   const int32_t *__restrict__ src,
                                                                   const float *__restrict__ grad,
                                                                   const float *__restrict__ input,
                                                                   const int32_t *__restrict__ tails, long long n_node,
                                                                   long long n_edges, int K, float *__restrict__ distance,
                                                                   int32_t *__restrict__ back_edge,
                                                                   int32_t *__restrict__ back_rank) {
    const long long q = blockIdx.y;
    const long long eo = q * n_edges, no = q * n_node * K;
    beam_row<G, KMAX>(row_ptr, src, grad + eo, input + no, n_node, n_edges, (long long)tails[q], K, distance + no,
                      back_edge + no, back_rank + no);
}

template <int G>
int launch_g(const int32_t *row_ptr, const int32_t *src, const float *grad, const float *input, long long n_node,
             long long n_edges, long long tail, int K, float *distance, int32_t *back_edge, int32_t *back_rank,
             hipStream_t s) {
    const long long blocks = (n_node * G + kThreads - 1) / kThreads;
    if (blocks > 0x7fffffffll) return ULTRA_ERR_BAD_SHAPE;
    const dim3 grid((unsigned)blocks), block(kThreads);
#define ULTRA_BEAM_LAUNCH(KM)                                                                                           \
    hipLaunchKernelGGL((beam_step_kernel<G, KM>), grid, block, 0, s, row_ptr, src, grad, input, n_node, n_edges, tail, \
                       K, distance, back_edge, back_rank)
    if (K <= 4) ULTRA_BEAM_LAUNCH(4);
    else if (K <= 8) ULTRA_BEAM_LAUNCH(8);
    else if (K <= 16) ULTRA_BEAM_LAUNCH(16);
    else ULTRA_BEAM_LAUNCH(32);
#undef ULTRA_BEAM_LAUNCH
    HIP_TRY(hipGetLastError());
    return ULTRA_OK;
}

template <int G>
int launch_batch_g(const int32_t *row_ptr, const int32_t *src, const float *grad, const float *input, const int32_t *tails,
                   long long n_node, long long n_edges, long long n_query, int K, float *distance, int32_t *back_edge,
                   int32_t *back_rank, hipStream_t s) {
    const long long blocks = (n_node * G + kThreads - 1) / kThreads;
    if (blocks > 0x7fffffffll) return ULTRA_ERR_BAD_SHAPE;
    const dim3 grid((unsigned)blocks, (unsigned)n_query), block(kThreads);
#define ULTRA_BEAM_LAUNCH(KM)                                                                                             \
    hipLaunchKernelGGL((beam_step_batch_kernel<G, KM>), grid, block, 0, s, row_ptr, src, grad, input, tails, n_node,     \
                       n_edges, K, distance, back_edge, back_rank)
    if (K <= 4) ULTRA_BEAM_LAUNCH(4);
    else if (K <= 8) ULTRA_BEAM_LAUNCH(8);
    else if (K <= 16) ULTRA_BEAM_LAUNCH(16);
    else ULTRA_BEAM_LAUNCH(32);
#undef ULTRA_BEAM_LAUNCH
    HIP_TRY(hipGetLastError());
    return ULTRA_OK;
}

}  // namespace

extern "C" int ultra_beam_search_step_f32(const int32_t *row_ptr, const int32_t *src, const float *edge_grad,
                                          const float *input, int64_t n_node, int64_t n_edges, int64_t tail, int64_t K,
                                          float *distance, int32_t *back_edge, int32_t *back_rank, void *stream) {
    if (K < 1 || K > 32 || n_node < 0 || n_edges < 0 || n_edges > 0x7fffffffll || n_node > 0x7fffffffll)
        return ULTRA_ERR_BAD_SHAPE;
    if (n_node == 0) return ULTRA_OK;
    if (row_ptr == nullptr || input == nullptr || distance == nullptr || back_edge == nullptr || back_rank == nullptr ||
        (n_edges > 0 && (src == nullptr || edge_grad == nullptr)))
        return ULTRA_ERR_NULL_POINTER;
    hipStream_t s = static_cast<hipStream_t>(stream);
    // lanes per row from the mean degree (as rowgroup.inc sizes its groups)
    const long long mean = n_edges / n_node;
    if (mean >= 48)
        return launch_g<64>(row_ptr, src, edge_grad, input, n_node, n_edges, tail, (int)K, distance, back_edge, back_rank, s);
    if (mean >= 24)
        return launch_g<32>(row_ptr, src, edge_grad, input, n_node, n_edges, tail, (int)K, distance, back_edge, back_rank, s);
    return launch_g<16>(row_ptr, src, edge_grad, input, n_node, n_edges, tail, (int)K, distance, back_edge, back_rank, s);
}

extern "C" int ultra_beam_search_step_batch_f32(const int32_t *row_ptr, const int32_t *src, const float *edge_grad,
                                                const float *input, const int32_t *tails, int64_t n_node, int64_t n_edges,
                                                int64_t n_query, int64_t K, float *distance, int32_t *back_edge,
                                                int32_t *back_rank, void *stream) {
    if (K < 1 || K > 32 || n_query < 1 || n_query > 65535 || n_node < 0 || n_edges < 0 || n_edges > 0x7fffffffll ||
        n_node > 0x7fffffffll)
        return ULTRA_ERR_BAD_SHAPE;                  // (the query is the grid's y dimension)
    if (n_node == 0) return ULTRA_OK;
    if (row_ptr == nullptr || input == nullptr || tails == nullptr || distance == nullptr || back_edge == nullptr ||
        back_rank == nullptr || (n_edges > 0 && (src == nullptr || edge_grad == nullptr)))
        return ULTRA_ERR_NULL_POINTER;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const long long mean = n_edges / n_node;         // lanes per row: as the single step
    if (mean >= 48)
        return launch_batch_g<64>(row_ptr, src, edge_grad, input, tails, n_node, n_edges, n_query, (int)K, distance, back_edge, back_rank, s);
    if (mean >= 24)
        return launch_batch_g<32>(row_ptr, src, edge_grad, input, tails, n_node, n_edges, n_query, (int)K, distance, back_edge, back_rank, s);
    return launch_batch_g<16>(row_ptr, src, edge_grad, input, tails, n_node, n_edges, n_query, (int)K, distance, back_edge, back_rank, s);
}

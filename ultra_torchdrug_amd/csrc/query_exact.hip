// query_exact.hip -- exact (crisp) answer sets of logical queries: a relation-restricted set expansion for many queries at once,
// and the filtered rank of many targets per query (a translation unit of libultra_rspmm.so; C ABI: ultra_sets_project /
// ultra_sets_project_workspace / ultra_sets_rank in include/ultra_rspmm.h).
//
// A batch of Q entity sets over N entities is bits[N][W], W = ceil(Q / 64) 64-bit words a node: bit q % 64 of word q / 64 of
// node v = "v is in set q".
//
// ---- ultra_sets_project
//     out[v] bit q  =  OR over the in-edges e = (u -> v) of row v with rel[e] == relation[q] and w[e] != 0  of  in[u] bit q
// A small launch pair first builds relmask[n_rel][W]: bit q of row relation[q] (cleared by a kernel -- not a memset node, see
// ultra_rspmm_frontier_f32 -- then one integer atomicOr per query, as hop_seed_kernel seeds its bitmaps; a relation outside
// [0, n_rel) sets nothing, so its set comes out empty).  Columns >= Q have no bit in relmask: whatever the input holds there never
// reaches the output.  Then ONE pull over the dst-CSR, the walk of hop_level_kernel with a relation test per edge: a group of G
// lanes (16 / 32 / 64 from the mean degree) owns destination row v and a tile of up to kWordTile = 4 words (blockIdx.y); lane j
// ORs  in[src[e]][word] & relmask[rel[e]][word]  over the row's edges j, j + G, ... (an edge whose weight is exactly 0 does not
// exist), the group ORs its lanes' words with a butterfly and lane 0 stores them.  Every word of every row is stored, so nothing
// is cleared.  The rows are handed out grid-stride over at most 2048 blocks.
// A group walks at most the first kSeg = 1024 edges of its row: on a graph with hubs one group on a row of 30 000 edges was the
// whole launch (0.38 ms on S-fb15k237, whose other rows take a few rounds).  The rest of such a row is taken by a second launch
// over the EDGE array in pieces of kSeg edges, one block a piece: only the row that holds a piece's first edge can have edges
// beyond its first kSeg inside that piece (a row that starts inside the piece has its first kSeg edges reach past the piece's
// end), so the block finds that row by bisection of row_ptr, ORs the part of the piece that lies in the row's tail and adds it
// to the stored word with one integer atomicOr per wave and word.  Pieces without such a part -- all of them on a graph without
// long rows -- end after the bisection.
// OR is associative, commutative and idempotent: every schedule gives the same bits.
// Row bounds are clamped to [0, n_edges]; an edge whose source is outside [0, n_node) or whose relation is outside [0, n_rel) is
// skipped, so malformed arrays cannot make the kernel touch memory out of bounds.  All index arithmetic is 64-bit.
//
// ---- ultra_sets_rank
//     rank[t] = 1 + #{ v in [0, N) : bit (v, q_t) of excluded clear  and  pred[q_t][v] >= pred[q_t][target_entity[t]] }
// (pessimistic on ties, false for a NaN on either side: the comparison of ultra_filtered_rank_keys).  A workgroup takes one query
// (blockIdx.x) and blocks of kTargets = 256 of its targets, one target per thread (blockIdx.y strides over the blocks).  The
// row's scores go through LDS in tiles of kTile = 1024 entities: thread i stages scores i, i + 256, ... of the tile, an excluded
// entity -- and the slots past N of the last tile -- as NaN, which no threshold is <=; after the barrier every thread compares
// its own threshold with the whole tile (all lanes read the same LDS address: a broadcast) and counts.  Nothing of size (T, N)
// exists; the counts are integers and each thread owns its target, so every schedule gives the same ranks.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "host_common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWordTile = 4;         // words of a row a lane group carries at once
constexpr int kMaxBlocks = 2048;     // grid-stride beyond
constexpr int kSeg = 1024;           // edges of a row its lane group walks; the rest: sets_project_tail_kernel, in pieces of kSeg
constexpr int kTargets = 256;        // targets per block of ultra_sets_rank = its threads
constexpr int kTile = 1024;          // entities per LDS tile of ultra_sets_rank
constexpr int kTargetBlocks = 16;    // grid.y of ultra_sets_rank at most: a query with more target blocks strides
using word_t = unsigned long long;

__device__ __forceinline__ word_t shfl_xor_word(word_t x, int off, int width) {
    const unsigned lo = __shfl_xor((unsigned)(x & 0xffffffffull), off, width);
    const unsigned hi = __shfl_xor((unsigned)(x >> 32), off, width);
    return ((word_t)hi << 32) | lo;
}

__global__ __launch_bounds__(kThreads) void sets_relmask_clear_kernel(word_t *__restrict__ relmask, long long n) {
    const long long stride = (long long)gridDim.x * kThreads;
    for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < n; i += stride) relmask[i] = 0;
}

// bit q of row relation[q] (relations repeat across queries: integer OR)
__global__ __launch_bounds__(kThreads) void sets_relmask_seed_kernel(const int64_t *__restrict__ relation, long long n_query,
                                                                     long long n_rel, long long W, word_t *__restrict__ relmask) {
    const long long stride = (long long)gridDim.x * kThreads;
    for (long long q = (long long)blockIdx.x * kThreads + threadIdx.x; q < n_query; q += stride) {
        const long long r = relation[q];
        if (r < 0 || r >= n_rel) continue;
        atomicOr(&relmask[r * W + (q >> 6)], (word_t)1 << (q & 63));
    }
}

template <int G, bool HAS_W>
__global__ __launch_bounds__(kThreads) void sets_project_kernel(const int32_t *__restrict__ row_ptr, const int32_t *__restrict__ src,
                                                                const int32_t *__restrict__ rel, const float *__restrict__ w,
                                                                long long n_node, long long n_edges, long long n_rel, long long W,
                                                                const word_t *__restrict__ in, const word_t *__restrict__ relmask,
                                                                word_t *__restrict__ out) {
    constexpr int kGroups = kThreads / G;          // rows a block takes per round
    const int lane = (int)(threadIdx.x % G);
    const long long w0 = (long long)blockIdx.y * kWordTile;
    const int n_live = (int)(W - w0 < kWordTile ? W - w0 : kWordTile);       // (uniform over the block; >= 1 by the grid)
    const long long stride = (long long)gridDim.x * kGroups;
    // grid-stride over the rows; the bound is the block's first row, so every lane of a wave runs the same rounds (the shuffles
    // below want the whole wave)
    for (long long base = (long long)blockIdx.x * kGroups; base < n_node; base += stride) {
        const long long v = base + threadIdx.x / G;
        const bool live = v < n_node;
        word_t acc[kWordTile];
#pragma unroll
        for (int i = 0; i < kWordTile; ++i) acc[i] = 0;
        if (live) {
            long long e0 = row_ptr[v], e1 = row_ptr[v + 1];
            e0 = e0 < 0 ? 0 : e0;
            e1 = e1 > n_edges ? n_edges : e1;
            e1 = e1 - e0 > kSeg ? e0 + kSeg : e1;                       // (the tail of a longer row: sets_project_tail_kernel)
#pragma unroll 2
            for (long long e = e0 + lane; e < e1; e += G) {
                const int u = src[e], r = rel[e];
                bool ok = u >= 0 && (long long)u < n_node && r >= 0 && (long long)r < n_rel;
                if (HAS_W) ok = ok && w[e] != 0.0f;
                const word_t *in_row = in + (ok ? (long long)u : 0) * W + w0;           // (n_node, n_rel >= 1 here: row 0 exists)
                const word_t *mask_row = relmask + (ok ? (long long)r : 0) * W + w0;
#pragma unroll
                for (int i = 0; i < kWordTile; ++i)
                    if (i < n_live) {
                        const word_t f = in_row[i] & mask_row[i];
                        acc[i] |= ok ? f : 0;
                    }
            }
        }
#pragma unroll
        for (int i = 0; i < kWordTile; ++i)
            if (i < n_live) {
#pragma unroll
                for (int off = G / 2; off > 0; off >>= 1) acc[i] |= shfl_xor_word(acc[i], off, G);
            }
        if (live && lane == 0) {
            word_t *row = out + v * W + w0;
#pragma unroll
            for (int i = 0; i < kWordTile; ++i)
                if (i < n_live) row[i] = acc[i];
        }
    }
}

// piece blockIdx.x = edges [p0, p0 + kSeg) of the edge array: the part of it that lies beyond the first kSeg edges of the row
// holding edge p0 is ORed into that row's stored words
template <bool HAS_W>
__global__ __launch_bounds__(kThreads) void sets_project_tail_kernel(const int32_t *__restrict__ row_ptr, const int32_t *__restrict__ src,
                                                                     const int32_t *__restrict__ rel, const float *__restrict__ w,
                                                                     long long n_node, long long n_edges, long long n_rel, long long W,
                                                                     const word_t *__restrict__ in, const word_t *__restrict__ relmask,
                                                                     word_t *__restrict__ out) {
    const long long p0 = (long long)blockIdx.x * kSeg;
    const long long w0 = (long long)blockIdx.y * kWordTile;
    const int n_live = (int)(W - w0 < kWordTile ? W - w0 : kWordTile);
    // the last row v with row_ptr[v] <= p0: the row that holds edge p0 (every thread bisects the same way: all below is uniform)
    long long lo = 0, hi = n_node - 1;
    while (lo < hi) {
        const long long mid = (lo + hi + 1) >> 1;
        if ((long long)row_ptr[mid] <= p0) lo = mid; else hi = mid - 1;
    }
    const long long v = lo;
    long long e0 = row_ptr[v], e1 = row_ptr[v + 1];
    e0 = e0 < 0 ? 0 : e0;
    e1 = e1 > n_edges ? n_edges : e1;
    const long long a = p0 > e0 + kSeg ? p0 : e0 + kSeg;
    const long long b = p0 + kSeg < e1 ? p0 + kSeg : e1;
    if (a >= b) return;
    word_t acc[kWordTile];
#pragma unroll
    for (int i = 0; i < kWordTile; ++i) acc[i] = 0;
    for (long long e = a + threadIdx.x; e < b; e += kThreads) {
        const int u = src[e], r = rel[e];
        bool ok = u >= 0 && (long long)u < n_node && r >= 0 && (long long)r < n_rel;
        if (HAS_W) ok = ok && w[e] != 0.0f;
        const word_t *in_row = in + (ok ? (long long)u : 0) * W + w0;
        const word_t *mask_row = relmask + (ok ? (long long)r : 0) * W + w0;
#pragma unroll
        for (int i = 0; i < kWordTile; ++i)
            if (i < n_live) {
                const word_t f = in_row[i] & mask_row[i];
                acc[i] |= ok ? f : 0;
            }
    }
#pragma unroll
    for (int i = 0; i < kWordTile; ++i)
        if (i < n_live) {
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) acc[i] |= shfl_xor_word(acc[i], off, 64);
            if ((threadIdx.x & 63) == 0 && acc[i] != 0) atomicOr(&out[v * W + w0 + i], acc[i]);
        }
}

struct ProjectCall {
    const int32_t *row_ptr, *src, *rel;
    const float *w;
    long long n_node, n_edges, n_rel, W;
    const word_t *in, *relmask;
    word_t *out;
};

template <int G>
int launch_project(const ProjectCall &c, hipStream_t s) {
    const long long row_blocks = (c.n_node * G + kThreads - 1) / kThreads;
    const dim3 grid((unsigned)(row_blocks > kMaxBlocks ? kMaxBlocks : row_blocks), (unsigned)((c.W + kWordTile - 1) / kWordTile));
    if (c.w != nullptr)
        hipLaunchKernelGGL((sets_project_kernel<G, true>), grid, dim3(kThreads), 0, s, c.row_ptr, c.src, c.rel, c.w, c.n_node,
                           c.n_edges, c.n_rel, c.W, c.in, c.relmask, c.out);
    else
        hipLaunchKernelGGL((sets_project_kernel<G, false>), grid, dim3(kThreads), 0, s, c.row_ptr, c.src, c.rel, c.w, c.n_node,
                           c.n_edges, c.n_rel, c.W, c.in, c.relmask, c.out);
    HIP_TRY(hipGetLastError());
    if (c.n_edges <= kSeg) return ULTRA_OK;                                      // no row is longer than a group walks
    const dim3 pieces((unsigned)((c.n_edges + kSeg - 1) / kSeg), grid.y);
    if (c.w != nullptr)
        hipLaunchKernelGGL((sets_project_tail_kernel<true>), pieces, dim3(kThreads), 0, s, c.row_ptr, c.src, c.rel, c.w, c.n_node,
                           c.n_edges, c.n_rel, c.W, c.in, c.relmask, c.out);
    else
        hipLaunchKernelGGL((sets_project_tail_kernel<false>), pieces, dim3(kThreads), 0, s, c.row_ptr, c.src, c.rel, c.w, c.n_node,
                           c.n_edges, c.n_rel, c.W, c.in, c.relmask, c.out);
    HIP_TRY(hipGetLastError());
    return ULTRA_OK;
}

__global__ __launch_bounds__(kTargets) void sets_rank_kernel(const float *__restrict__ pred, long long n_query, long long n_node,
                                                             long long row_stride, const word_t *__restrict__ excluded,
                                                             long long W, const int64_t *__restrict__ target_ptr,
                                                             const int64_t *__restrict__ target_entity, long long n_target,
                                                             int64_t *__restrict__ rank) {
    __shared__ __align__(16) float tile[kTile];          // (read back 16 bytes at a time)
    const long long q = blockIdx.x;
    const int t = (int)threadIdx.x;
    long long t0 = target_ptr[q], t1 = target_ptr[q + 1];
    t0 = t0 < 0 ? 0 : t0;
    t1 = t1 > n_target ? n_target : t1;
    const float *row = pred + q * row_stride;
    const word_t *ex = excluded != nullptr ? excluded + (q >> 6) : nullptr;
    const int bit = (int)(q & 63);
    // (t0, t1 and so the number of rounds are uniform over the block: the barriers below are met by every thread)
    for (long long first = t0 + (long long)blockIdx.y * kTargets; first < t1; first += (long long)gridDim.y * kTargets) {
        const long long mine = first + t;
        const bool have = mine < t1;
        const long long entity = have ? target_entity[mine] : -1;
        const bool valid = entity >= 0 && entity < n_node;
        const float threshold = valid ? row[entity] : nanf("");
        long long count = 0;
        for (long long v0 = 0; v0 < n_node; v0 += kTile) {
#pragma unroll
            for (int i = t; i < kTile; i += kTargets) {
                const long long v = v0 + i;
                float score = nanf("");
                if (v < n_node) {
                    const bool out = ex != nullptr && ((ex[v * W] >> bit) & 1ull);
                    if (!out) score = row[v];
                }
                tile[i] = score;
            }
            __syncthreads();
            int here = 0;
#pragma unroll 8
            for (int i = 0; i < kTile; i += 4) {
                const float4 s4 = *reinterpret_cast<const float4 *>(&tile[i]);
                here += (s4.x >= threshold) + (s4.y >= threshold) + (s4.z >= threshold) + (s4.w >= threshold);
            }
            count += here;
            __syncthreads();                                        // the next tile overwrites this one
        }
        if (have) rank[mine] = valid ? 1 + count : 0;
    }
}

}  // namespace

extern "C" size_t ultra_sets_project_workspace(int64_t n_rel, int64_t n_query) {
    if (n_rel <= 0 || n_query <= 0) return 0;
    return (size_t)n_rel * (size_t)((n_query + 63) / 64) * sizeof(word_t);
}

extern "C" int ultra_sets_project(const int32_t *row_ptr, const int32_t *src, const int32_t *rel, const float *w, int64_t n_node,
                                  int64_t n_edges, int64_t n_rel, const uint64_t *bits, const int64_t *relation, int64_t n_query,
                                  uint64_t *out, void *workspace, size_t workspace_bytes, void *stream) {
    if (n_node < 0 || n_edges < 0 || n_rel < 0 || n_query < 0 || n_edges > 0x7fffffffll || n_node >= 0x7fffffffll ||
        n_rel > 0x7fffffffll)
        return ULTRA_ERR_BAD_SHAPE;
    const long long W = (n_query + 63) / 64;
    if ((W + kWordTile - 1) / kWordTile > 65535) return ULTRA_ERR_BAD_SHAPE;     // (the word tiles are grid.y: Q <= 16 776 960)
    if (n_query == 0 || n_node == 0) return ULTRA_OK;                              // the output is empty
    if (row_ptr == nullptr || bits == nullptr || relation == nullptr || out == nullptr) return ULTRA_ERR_NULL_POINTER;
    if (n_edges > 0 && (src == nullptr || rel == nullptr)) return ULTRA_ERR_NULL_POINTER;
    if (bits == out) return ULTRA_ERR_BAD_SHAPE;                                   // rows are read while others are written
    if (n_rel > 0 && workspace == nullptr) return ULTRA_ERR_NULL_POINTER;
    if (workspace_bytes < ultra_sets_project_workspace(n_rel, n_query)) return ULTRA_ERR_WORKSPACE;
    hipStream_t s = static_cast<hipStream_t>(stream);
    ProjectCall c;
    c.row_ptr = row_ptr;
    c.src = src;
    c.rel = rel;
    c.w = n_edges > 0 ? w : nullptr;
    c.n_node = n_node;
    c.n_edges = n_rel > 0 ? n_edges : 0;            // without relations no edge passes the test: every row is empty
    c.n_rel = n_rel;
    c.W = W;
    c.in = reinterpret_cast<const word_t *>(bits);
    c.relmask = static_cast<const word_t *>(workspace);
    c.out = reinterpret_cast<word_t *>(out);
    if (n_rel > 0) {
        const long long words = n_rel * W;
        const long long clear_blocks = (words + kThreads - 1) / kThreads, seed_blocks = (n_query + kThreads - 1) / kThreads;
        hipLaunchKernelGGL(sets_relmask_clear_kernel, dim3((unsigned)(clear_blocks > kMaxBlocks ? kMaxBlocks : clear_blocks)),
                           dim3(kThreads), 0, s, static_cast<word_t *>(workspace), words);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(sets_relmask_seed_kernel, dim3((unsigned)(seed_blocks > kMaxBlocks ? kMaxBlocks : seed_blocks)),
                           dim3(kThreads), 0, s, relation, (long long)n_query, (long long)n_rel, W,
                           static_cast<word_t *>(workspace));
        HIP_TRY(hipGetLastError());
    }
    // lanes per row from the mean degree (as hop_distance.hip and beam_search.hip size their groups)
    const long long mean = n_edges / n_node;
    if (mean >= 48) return launch_project<64>(c, s);
    if (mean >= 24) return launch_project<32>(c, s);
    return launch_project<16>(c, s);
}

extern "C" int ultra_sets_rank(const float *pred, int64_t n_query, int64_t n_node, int64_t row_stride, const uint64_t *excluded,
                               const int64_t *target_ptr, const int64_t *target_entity, int64_t n_target, int64_t *rank,
                               void *stream) {
    if (n_query < 0 || n_node < 0 || n_target < 0 || n_query > 0x7fffffffll || n_node >= 0x7fffffffll) return ULTRA_ERR_BAD_SHAPE;
    if (n_query > 0 && row_stride < n_node) return ULTRA_ERR_BAD_SHAPE;
    if (n_query > 1 && row_stride > (1ll << 60) / n_query) return ULTRA_ERR_BAD_SHAPE;
    if (n_target == 0 || n_query == 0) return ULTRA_OK;                            // no rank to write
    if (target_ptr == nullptr || target_entity == nullptr || rank == nullptr) return ULTRA_ERR_NULL_POINTER;
    if (n_node > 0 && pred == nullptr) return ULTRA_ERR_NULL_POINTER;
    const long long blocks = (n_target + kTargets - 1) / kTargets;
    const dim3 grid((unsigned)n_query, (unsigned)(blocks > kTargetBlocks ? kTargetBlocks : blocks));
    hipLaunchKernelGGL(sets_rank_kernel, grid, dim3(kTargets), 0, static_cast<hipStream_t>(stream), pred, (long long)n_query,
                       (long long)n_node, (long long)row_stride, reinterpret_cast<const word_t *>(excluded),
                       (long long)((n_query + 63) / 64), target_ptr, target_entity, (long long)n_target, rank);
    HIP_TRY(hipGetLastError());
    return ULTRA_OK;
}

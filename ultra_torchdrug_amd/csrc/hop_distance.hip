// hop_distance.hip -- hop distances from many sources at once: bit-parallel multi-source BFS over the coalesced dst-CSR (a
// translation unit of libultra_rspmm.so; C ABI: ultra_hop_distance / ultra_hop_distance_workspace in include/ultra_rspmm.h;
// DESIGN.md section 14).
//
//     dist[v][b] = edges on a shortest path sources[b] -> v along the edge direction, if that is <= num_iters;  n_node otherwise
//
// Sources are processed 64 at a time (a "source block"): one 64-bit word per node holds, bit j = source j of the block,
//     visited[v]   the sources that have reached v,
//     frontier[v]  the sources that reached v at the previous level,
//     next[v]      the sources that reach v at this level.
// One level is one launch that PULLS over the dst-CSR: a group of G lanes (16 / 32 / 64, from the mean degree, as
// beam_search.hip sizes its groups) owns destination row v.  A row every source of the block has reached is left without a look
// at its edges (at later levels that is most rows); otherwise lane j ORs frontier[src[e]] over the row's edges j, j + G, ...
// (an edge whose weight is exactly 0 does not exist), the group ORs its lanes' words with a butterfly, and
//     fresh = acc & ~visited[v];   visited[v] |= fresh;   next[v] = fresh
// are plain stores: the group owns its row (the rows are handed out grid-stride over at most 2048 blocks).  next is written for
// EVERY row, so nothing is cleared between levels.  For every set bit of fresh the level goes to dist[v][column] when the matrix
// is asked for (lane j writes columns j, j + G, ...).  OR is associative, commutative and idempotent: every schedule gives the
// same bits.
// The targets form never builds the matrix: after each level a small kernel over the block's (source, target) pairs writes the
// level where the pair's entry still holds n_node and the target's visited word has the source's bit.
// Termination: with poll the fresh bits of a level are counted into a 64-bit device word -- one integer atomic per wave of the
// capped grid, a few thousand a level; one per wave of an uncapped grid (2.5 M on 10 M nodes) took longer than the level -- that
// the host reads after the level; the first level that adds nothing ends the block.  Without poll -- or while the stream is
// being captured -- exactly num_iters levels are enqueued and nothing is read; the surplus levels change nothing.
// Row bounds are clamped to [0, n_edges]; edge sources, BFS sources and targets outside [0, n_node) are skipped, so malformed
// arrays cannot make a kernel touch memory out of bounds (the torch operator rejects them before the launch).
#include <hip/hip_runtime.h>

#include <cstdint>

#include "host_common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWord = 64;            // sources per block = bits of a bitmap word
using word_t = unsigned long long;

__device__ __forceinline__ word_t shfl_xor_word(word_t x, int off, int width) {
    const unsigned lo = __shfl_xor((unsigned)(x & 0xffffffffull), off, width);
    const unsigned hi = __shfl_xor((unsigned)(x >> 32), off, width);
    return ((word_t)hi << 32) | lo;
}

// every entry of an int32 array = value (the sentinel n_node)
__global__ __launch_bounds__(kThreads) void hop_fill_kernel(int32_t *__restrict__ out, long long n, int32_t value) {
    const long long stride = (long long)gridDim.x * kThreads;
    for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < n; i += stride) out[i] = value;
}

// visited = frontier = 0 for every node; both counter words = 0
__global__ __launch_bounds__(kThreads) void hop_clear_kernel(word_t *__restrict__ visited, word_t *__restrict__ frontier,
                                                             long long n_node, word_t *__restrict__ counter) {
    const long long stride = (long long)gridDim.x * kThreads;
    for (long long v = (long long)blockIdx.x * kThreads + threadIdx.x; v < n_node; v += stride) {
        visited[v] = 0;
        frontier[v] = 0;
    }
    if (blockIdx.x == 0 && threadIdx.x < 2) counter[threadIdx.x] = 0;
}

// level 0: bit j of visited / frontier at the node of source j (sources may repeat: integer OR), dist[source][column] = 0
__global__ __launch_bounds__(kWord) void hop_seed_kernel(const int64_t *__restrict__ sources, int n_cols, long long col0,
                                                         long long n_node, long long n_source, word_t *__restrict__ visited,
                                                         word_t *__restrict__ frontier, int32_t *__restrict__ dist) {
    const int j = (int)threadIdx.x;
    if (j >= n_cols) return;
    const long long s = sources[col0 + j];
    if (s < 0 || s >= n_node) return;
    atomicOr(&visited[s], (word_t)1 << j);
    atomicOr(&frontier[s], (word_t)1 << j);
    if (dist != nullptr) dist[s * n_source + col0 + j] = 0;
}

template <int G, bool HAS_W>
__global__ __launch_bounds__(kThreads) void hop_level_kernel(const int32_t *__restrict__ row_ptr, const int32_t *__restrict__ src,
                                                             const float *__restrict__ w, long long n_node, long long n_edges,
                                                             const word_t *__restrict__ frontier, word_t *__restrict__ next,
                                                             word_t *__restrict__ visited, word_t col_mask, int32_t level,
                                                             int32_t *__restrict__ dist, long long n_source, long long col0,
                                                             word_t *__restrict__ counter) {
    constexpr int kGroups = kThreads / G;          // rows a block takes per round
    const int lane = (int)(threadIdx.x % G);
    const long long stride = (long long)gridDim.x * kGroups;
    word_t n_new = 0;
    // grid-stride over the rows; the bound is the block's first row, so every lane of a wave runs the same rounds (the shuffles
    // below want the whole wave) and a wave reports its fresh bits once, however many rows it took
    for (long long base = (long long)blockIdx.x * kGroups; base < n_node; base += stride) {
        const long long v = base + threadIdx.x / G;
        const bool live = v < n_node;
        const word_t seen = live ? visited[v] : ~(word_t)0;
        const word_t want = ~seen & col_mask;       // the same for the whole group
        word_t acc = 0;
        if (want != 0) {
            long long e0 = row_ptr[v], e1 = row_ptr[v + 1];
            e0 = e0 < 0 ? 0 : e0;
            e1 = e1 > n_edges ? n_edges : e1;
#pragma unroll 4
            for (long long e = e0 + lane; e < e1; e += G) {
                const int u = src[e];
                bool ok = u >= 0 && (long long)u < n_node;
                if (HAS_W) ok = ok && w[e] != 0.0f;
                const word_t f = frontier[ok ? u : 0];      // (n_node >= 1 here: word 0 exists)
                acc |= ok ? f : 0;
            }
        }
#pragma unroll
        for (int off = G / 2; off > 0; off >>= 1) acc |= shfl_xor_word(acc, off, G);
        const word_t fresh = acc & want;
        if (live && lane == 0) {
            if (fresh != 0) visited[v] = seen | fresh;
            next[v] = fresh;
            n_new += (word_t)__popcll(fresh);
        }
        if (dist != nullptr && fresh != 0) {
            int32_t *row = dist + v * n_source + col0;
#pragma unroll
            for (int b = lane; b < kWord; b += G)
                if ((fresh >> b) & 1ull) row[b] = level;
        }
    }
    if (counter != nullptr) {                       // (uniform over the launch)
#pragma unroll
        for (int off = kWord / 2; off > 0; off >>= 1) n_new += shfl_xor_word(n_new, off, kWord);
        if ((threadIdx.x & (kWord - 1)) == 0 && n_new != 0) atomicAdd(&counter[level & 1], n_new);
        if (blockIdx.x == 0 && threadIdx.x == 0) counter[(level + 1) & 1] = 0;      // the next level's word
    }
}

// targets form: pair (column j of the block, slot k) takes `level` when it still holds the sentinel and source j has reached it
__global__ __launch_bounds__(kThreads) void hop_targets_kernel(const int64_t *__restrict__ targets, long long per_source,
                                                               int n_cols, long long col0, long long n_node,
                                                               const word_t *__restrict__ visited, int32_t level,
                                                               int32_t *__restrict__ out) {
    const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (i >= (long long)n_cols * per_source) return;
    const int j = (int)(i / per_source);
    const long long o = col0 * per_source + i;
    const long long t = targets[o];
    if (t < 0 || t >= n_node) return;
    if (out[o] == (int32_t)n_node && ((visited[t] >> j) & 1ull)) out[o] = level;
}

int grid_for(long long n) {
    const long long blocks = (n + kThreads - 1) / kThreads;
    return (int)(blocks < 1 ? 1 : (blocks > 2048 ? 2048 : blocks));       // grid-stride beyond 2048 blocks
}

struct HopCall {
    const int32_t *row_ptr, *src;
    const float *w;
    long long n_node, n_edges, n_source, per_source;
    const int64_t *sources, *targets;
    int32_t *dist_matrix, *dist_targets;
    word_t *visited, *frontier, *next;
    word_t *counter;
};

template <int G, bool HAS_W>
int launch_level(const HopCall &c, const word_t *frontier, word_t *next, word_t col_mask, int32_t level, long long col0,
                 bool count, hipStream_t s) {
    hipLaunchKernelGGL((hop_level_kernel<G, HAS_W>), dim3(grid_for(c.n_node * G)), dim3(kThreads), 0, s, c.row_ptr, c.src, c.w,
                       c.n_node, c.n_edges, frontier, next, c.visited, col_mask, level, c.dist_matrix, c.n_source, col0,
                       count ? c.counter : nullptr);
    HIP_TRY(hipGetLastError());
    return ULTRA_OK;
}

int launch_targets(const HopCall &c, int n_cols, long long col0, int32_t level, hipStream_t s) {
    const long long pairs = (long long)n_cols * c.per_source;
    if (c.dist_targets == nullptr || pairs == 0) return ULTRA_OK;
    hipLaunchKernelGGL(hop_targets_kernel, dim3((unsigned)((pairs + kThreads - 1) / kThreads)), dim3(kThreads), 0, s, c.targets,
                       c.per_source, n_cols, col0, c.n_node, c.visited, level, c.dist_targets);
    HIP_TRY(hipGetLastError());
    return ULTRA_OK;
}

template <int G, bool HAS_W>
int run(const HopCall &c, long long num_iters, bool poll, hipStream_t s) {
    if (c.dist_matrix != nullptr) {
        hipLaunchKernelGGL(hop_fill_kernel, dim3(grid_for(c.n_node * c.n_source)), dim3(kThreads), 0, s, c.dist_matrix,
                           c.n_node * c.n_source, (int32_t)c.n_node);
        HIP_TRY(hipGetLastError());
    }
    if (c.dist_targets != nullptr && c.n_source * c.per_source > 0) {
        hipLaunchKernelGGL(hop_fill_kernel, dim3(grid_for(c.n_source * c.per_source)), dim3(kThreads), 0, s, c.dist_targets,
                           c.n_source * c.per_source, (int32_t)c.n_node);
        HIP_TRY(hipGetLastError());
    }
    for (long long col0 = 0; col0 < c.n_source; col0 += kWord) {
        const int n_cols = (int)(c.n_source - col0 < kWord ? c.n_source - col0 : kWord);
        const word_t col_mask = n_cols == kWord ? ~(word_t)0 : (((word_t)1 << n_cols) - 1);
        word_t *frontier = c.frontier, *next = c.next;
        hipLaunchKernelGGL(hop_clear_kernel, dim3(grid_for(c.n_node)), dim3(kThreads), 0, s, c.visited, frontier, c.n_node,
                           c.counter);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(hop_seed_kernel, dim3(1), dim3(kWord), 0, s, c.sources, n_cols, col0, c.n_node, c.n_source, c.visited,
                           frontier, c.dist_matrix);
        HIP_TRY(hipGetLastError());
        int rc = launch_targets(c, n_cols, col0, 0, s);
        if (rc) return rc;
        for (long long level = 1; level <= num_iters; ++level) {
            rc = launch_level<G, HAS_W>(c, frontier, next, col_mask, (int32_t)level, col0, poll, s);
            if (rc) return rc;
            if (poll) {
                word_t fresh = 0;
                HIP_TRY(hipMemcpyAsync(&fresh, c.counter + (level & 1), sizeof(fresh), hipMemcpyDeviceToHost, s));
                HIP_TRY(hipStreamSynchronize(s));
                if (fresh == 0) break;              // nothing new at this level: nothing new ever after
            }
            rc = launch_targets(c, n_cols, col0, (int32_t)level, s);
            if (rc) return rc;
            word_t *t = frontier;
            frontier = next;
            next = t;
        }
    }
    return ULTRA_OK;
}

template <int G>
int run_g(const HopCall &c, long long num_iters, bool poll, hipStream_t s) {
    return c.w != nullptr ? run<G, true>(c, num_iters, poll, s) : run<G, false>(c, num_iters, poll, s);
}

constexpr size_t kCounterBytes = 2 * sizeof(word_t);        // the two counter words

}  // namespace

extern "C" size_t ultra_hop_distance_workspace(int64_t n_node) {
    if (n_node <= 0) return 0;
    return (size_t)n_node * 3 * sizeof(word_t) + kCounterBytes;
}

extern "C" int ultra_hop_distance(const int32_t *row_ptr, const int32_t *src, const float *w, int64_t n_node, int64_t n_edges,
                                  const int64_t *sources, int64_t n_source, int64_t num_iters, const int64_t *targets,
                                  int64_t per_source, int32_t *dist_matrix, int32_t *dist_targets, int poll, void *workspace,
                                  size_t workspace_bytes, void *stream) {
    if (n_node < 0 || n_edges < 0 || n_source < 0 || num_iters < 0 || per_source < 0 || n_edges > 0x7fffffffll ||
        n_node >= 0x7fffffffll || n_source > 0x7fffffffll || per_source > 0x7fffffffll)
        return ULTRA_ERR_BAD_SHAPE;
    if (dist_matrix == nullptr && dist_targets == nullptr) return ULTRA_ERR_BAD_SHAPE;
    if (dist_targets != nullptr && targets == nullptr && n_source * per_source > 0) return ULTRA_ERR_NULL_POINTER;
    if (n_source == 0 || n_node == 0) return ULTRA_OK;            // every output is empty
    if (row_ptr == nullptr || sources == nullptr || (n_edges > 0 && src == nullptr)) return ULTRA_ERR_NULL_POINTER;
    if (workspace == nullptr) return ULTRA_ERR_NULL_POINTER;
    if (workspace_bytes < ultra_hop_distance_workspace(n_node)) return ULTRA_ERR_WORKSPACE;
    hipStream_t s = static_cast<hipStream_t>(stream);
    bool read_back = poll != 0;
    if (read_back) {                                // a capturing stream cannot be read: the fixed number of levels
        hipStreamCaptureStatus status = hipStreamCaptureStatusNone;
        HIP_TRY(hipStreamIsCapturing(s, &status));
        if (status != hipStreamCaptureStatusNone) read_back = false;
    }
    HopCall c;
    c.row_ptr = row_ptr;
    c.src = src;
    c.w = n_edges > 0 ? w : nullptr;
    c.n_node = n_node;
    c.n_edges = n_edges;
    c.n_source = n_source;
    c.per_source = per_source;
    c.sources = sources;
    c.targets = targets;
    c.dist_matrix = dist_matrix;
    c.dist_targets = dist_targets;
    c.visited = static_cast<word_t *>(workspace);
    c.frontier = c.visited + n_node;
    c.next = c.frontier + n_node;
    c.counter = c.next + n_node;
    // lanes per row from the mean degree (as beam_search.hip and rowgroup.inc size their groups)
    const long long mean = n_edges / n_node;
    if (mean >= 48) return run_g<64>(c, num_iters, read_back, s);
    if (mean >= 24) return run_g<32>(c, num_iters, read_back, s);
    return run_g<16>(c, num_iters, read_back, s);
}

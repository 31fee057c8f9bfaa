// sampler.inc -- the per-step index work of training and evaluation, on the device, from SORTED KEY ARRAYS instead of
// dense (B, N) boolean masks.  (included by step_index.hip)
//
// The reference builds, per batch,
//   * filter masks   mask[b, n] = not (anchor_b, r_b, n) in graph             (ultra/task.py:65-100)   (B, N) bool
//   * strict negatives: mask.nonzero() + variadic_sample over the surviving candidates   (ultra/task.py:102-118)
//   * the batch's own positive edges, removed from the graph (a new graph + a re-sort)   (ultra/model.py:57-74)
// all of them lookups "which entities complete (anchor, relation, ?)" / "where is edge (h, t, r)".  Here a graph keeps
// one sorted array of DISTINCT 64-bit keys per direction,
//       key = (anchor * n_rel + rel) * n_node + other,
// and every kernel below finds its completions by binary search: no (B, N) tensor, no nonzero(), no host
// synchronisation, static shapes -- so a training step or an evaluation batch can be captured whole into a hipGraph.

namespace {

// (lower_bound_i64, the binary search of every kernel below, is in select_keys.h)

// rank[q] = 1 + #{c : pos <= pred[q, c]} - #{c in completions(anchor_q, rel_q) : pos <= pred[q, c]}
// SLICED = false: one workgroup per query does all of it.  SLICED = true (rows of many candidates): this launch leaves
// rank[q] = 1 - (filtered count) and rank_slices_kernel adds the candidates' count slice by slice.
template <bool SLICED>
__global__ __launch_bounds__(256) void filtered_rank_keys_kernel(const float *pred, long long row_stride, long long n_cand,
                                                                 const int64_t *target, long long target_stride,
                                                                 const int64_t *keys, long long n_keys,
                                                                 const int64_t *anchor, const int64_t *rel,
                                                                 long long index_stride, long long n_rel,
                                                                 int64_t *rank, long long rank_stride) {
    __shared__ long long part[4];
    __shared__ long long range[2];
    const long long q = blockIdx.x;
    const float *row = pred + q * row_stride;
    const float pos = row[target[q * target_stride]];
    long long count = 0;
    if constexpr (!SLICED)
        for (long long c = threadIdx.x; c < n_cand; c += blockDim.x) count += (pos <= row[c]) ? 1 : 0;
    if (keys != nullptr) {
        const int64_t base = (anchor[q * index_stride] * n_rel + rel[q * index_stride]) * n_cand;
        if (threadIdx.x < 2) range[threadIdx.x] = lower_bound_i64(keys, n_keys, base + (threadIdx.x ? n_cand : 0));
        __syncthreads();
        for (long long k = range[0] + threadIdx.x; k < range[1]; k += blockDim.x)
            count -= (pos <= row[keys[k] - base]) ? 1 : 0;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) count += __shfl_down(count, off, 64);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = count;
    __syncthreads();
    if (threadIdx.x == 0) rank[q * rank_stride] = part[0] + part[1] + part[2] + part[3] + 1;
}

constexpr long long kRankSlice = 32768;       // candidates per workgroup of the sliced count (128 per thread)

// rank[q] += #{c in slice : pos <= pred[q, c]}; grid (slices, queries).  Integer atomics: the sum does not depend on the order.
__global__ __launch_bounds__(256) void rank_slices_kernel(const float *pred, long long row_stride, long long n_cand,
                                                          const int64_t *target, long long target_stride, int64_t *rank,
                                                          long long rank_stride) {
    __shared__ int part[4];
    const long long q = blockIdx.y;
    const float *row = pred + q * row_stride;
    const float pos = row[target[q * target_stride]];
    const long long c0 = (long long)blockIdx.x * kRankSlice;
    const long long c1 = c0 + kRankSlice < n_cand ? c0 + kRankSlice : n_cand;
    int count = 0;
    long long c = c0 + threadIdx.x;
    for (; c + 3 * 256 < c1; c += 4 * 256) {                  // four independent loads in flight per thread
        const float v0 = row[c], v1 = row[c + 256], v2 = row[c + 512], v3 = row[c + 768];
        count += (pos <= v0) + (pos <= v1) + (pos <= v2) + (pos <= v3);
    }
    for (; c < c1; c += 256) count += (pos <= row[c]) ? 1 : 0;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) count += __shfl_down(count, off, 64);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = count;
    __syncthreads();
    if (threadIdx.x == 0) {
        const int total = part[0] + part[1] + part[2] + part[3];
        if (total) atomicAdd(reinterpret_cast<unsigned long long *>(rank + q * rank_stride), (unsigned long long)total);
    }
}

// out[q, s] = the floor(rand[q, s] * n_free_q)-th entity (ascending) that is NOT a completion of (anchor_q, rel_q, ?):
// exactly the entity `variadic_sample(mask.nonzero()[:, 1], mask.sum(-1), n_sample)` returns for the same uniform
// numbers (ultra/task.py:105-108: index = (rand * size).long() into the row's surviving candidates), found as the
// "k-th missing number" of the sorted completion list L:  smallest j with L[j] - j > k  ->  candidate = k + j.
__global__ __launch_bounds__(256) void strict_negative_kernel(const int64_t *keys, long long n_keys,
                                                              const int64_t *anchor, const int64_t *rel,
                                                              long long n_query, long long n_rel, long long n_node,
                                                              const float *rand, long long n_sample, int64_t *out) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_query * n_sample) return;
    const long long q = i / n_sample;
    const int64_t base = (anchor[q] * n_rel + rel[q]) * n_node;
    const long long first = lower_bound_i64(keys, n_keys, base);
    const long long last = lower_bound_i64(keys, n_keys, base + n_node);
    const long long n_excl = last - first;
    const long long n_free = n_node - n_excl;
    if (n_free <= 0) {          // every entity is a known completion: the reference would index an empty list
        out[i] = 0;
        return;
    }
    // fp32 product, truncated, as torch computes `(rand * sizes).long()`; clamped where rounding reaches n_free
    long long k = (long long)(rand[i] * (float)n_free);
    if (k >= n_free) k = n_free - 1;
    if (k < 0) k = 0;
    long long lo = 0, hi = n_excl;      // smallest j in [0, n_excl] with L[j] - j > k   (L[n_excl] = +infinity)
    while (lo < hi) {
        const long long mid = (lo + hi) >> 1;
        if ((keys[first + mid] - base) - mid > k) hi = mid; else lo = mid + 1;
    }
    out[i] = k + lo;
}

// n_free[q] = n_node - #{keys in [(anchor_q * n_rel + rel_q) * n_node, ... + n_node)}: `mask.sum(-1)` of the filter mask
// (ultra/task.py:65-100; the keys are distinct), the denominator of the sampled metrics (ultra/task.py:498).  Two
// binary searches per query, one thread each.
__global__ __launch_bounds__(256) void filter_counts_kernel(const int64_t *keys, long long n_keys, const int64_t *anchor,
                                                            const int64_t *rel, long long index_stride, long long n_query,
                                                            long long n_rel, long long n_node, int64_t *n_free) {
    const long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= n_query) return;
    long long n_excl = 0;
    if (keys != nullptr) {
        const int64_t base = (anchor[q * index_stride] * n_rel + rel[q * index_stride]) * n_node;
        n_excl = lower_bound_i64(keys, n_keys, base + n_node) - lower_bound_i64(keys, n_keys, base);
    }
    n_free[q] = n_node - n_excl;
}

constexpr int kSampledMax = 64;               // draws per query: one lane each
constexpr int kSampledWaves = 4;              // queries per workgroup: one wave each

// toy_eval of the reference (ultra/task.py:474-484): S_eff = min(S, n_free) DISTINCT entities that do not complete
// (anchor_q, rel_q, ?), drawn without replacement, and the positive ranked among their scores:
//     optimistic[q] = #{pos < pred[q, e]},  pessimistic[q] = #{pos <= pred[q, e]}.
// The draw is defined by the uniform numbers rand[q, 0..S) (torch.multinomial's stream cannot be restated):
//     for j = 0 .. S_eff - 1, m = n_free - j:   k = min((long long)(rand[q, j] * (float)m), m - 1)       fp32 product, truncated
//         for every earlier chosen free-rank c in ASCENDING order: if (c <= k) ++k                     k-th of those left
//     k is the j-th chosen free-rank; its entity is the k-th missing number of the sorted completion list (as above).
// One wave per query: lane 0 runs the dependent draw steps over a sorted list in LDS (at most 64 * 64 / 2 steps), then
// lane j maps rank j, gathers one score and compares; the counts are a shuffle tree; plain stores, no atomics.
__global__ __launch_bounds__(64 * kSampledWaves) void sampled_rank_keys_kernel(
        const float *pred, long long row_stride, long long n_cand, long long n_query, const int64_t *target,
        long long target_stride, const int64_t *keys, long long n_keys, const int64_t *anchor, const int64_t *rel,
        long long index_stride, long long n_rel, const float *rand, int n_sample, int64_t *optimistic, int64_t *pessimistic,
        int64_t *samples) {
    __shared__ long long sorted[kSampledWaves][kSampledMax];       // chosen free-ranks, ascending
    __shared__ long long chosen[kSampledWaves][kSampledMax];       // ... in draw order
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const long long q = (long long)blockIdx.x * kSampledWaves + wave;
    const bool live = q < n_query;
    int64_t base = 0;
    long long first = 0, n_excl = 0;
    if (live && keys != nullptr) {
        base = (anchor[q * index_stride] * n_rel + rel[q * index_stride]) * n_cand;
        first = lower_bound_i64(keys, n_keys, base);
        n_excl = lower_bound_i64(keys, n_keys, base + n_cand) - first;
    }
    const long long n_free = n_cand - n_excl;
    const int s_eff = !live ? 0 : (n_free < (long long)n_sample ? (int)(n_free < 0 ? 0 : n_free) : n_sample);
    if (lane == 0) {
        for (int j = 0; j < s_eff; ++j) {
            const long long m = n_free - j;
            long long k = (long long)(rand[q * n_sample + j] * (float)m);
            if (k > m - 1) k = m - 1;
            if (k < 0) k = 0;
            int at = 0;                                            // (the list ascends and k only grows: the first c > k ends it)
            while (at < j && sorted[wave][at] <= k) { ++k; ++at; }
            for (int i = j; i > at; --i) sorted[wave][i] = sorted[wave][i - 1];
            sorted[wave][at] = k;
            chosen[wave][j] = k;
        }
    }
    __syncthreads();                                               // (every wave of the workgroup arrives: no early return above)
    if (!live) return;
    int opt = 0, pess = 0;
    long long entity = -1;
    if (lane < s_eff) {
        const long long k = chosen[wave][lane];
        long long lo = 0, hi = n_excl;      // smallest j in [0, n_excl] with L[j] - j > k   (L[n_excl] = +infinity)
        while (lo < hi) {
            const long long mid = (lo + hi) >> 1;
            if ((keys[first + mid] - base) - mid > k) hi = mid; else lo = mid + 1;
        }
        entity = k + lo;
        if (entity >= n_cand) entity = n_cand - 1;                 // (keys of another graph: a wrong answer, not a wild read)
        const float *row = pred + q * row_stride;
        const float pos = row[target[q * target_stride]];
        const float neg = row[entity];
        opt = pos < neg ? 1 : 0;
        pess = pos <= neg ? 1 : 0;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        opt += __shfl_down(opt, off, 64);
        pess += __shfl_down(pess, off, 64);
    }
    if (lane == 0) {
        optimistic[q] = opt;
        pessimistic[q] = pess;
    }
    if (samples != nullptr && lane < n_sample) samples[q * n_sample + lane] = entity;       // unused slots: -1
}

// ---------------------------------------------------------------------------------------- top-K answers of a query
// topk_keys_kernel: the K best candidates of a score row that do NOT complete (anchor_q, rel_q, ?), best first (the contract is in
// include/ultra_rspmm.h).  Candidate c with score v becomes one 64-bit SORT KEY (topk_key of select_keys.h, with kTopkMax and
// kTopkEmpty)
//       high half: order-preserving map of v (-0.0 folded into +0.0; every NaN in one class BELOW -inf)     low half: ~c
// so that "better" is "larger key" -- equal scores go by ascending index -- and all keys of a row are distinct.  0 is no
// candidate's key (the NaN class is 1): it marks an empty slot.
// A workgroup keeps its K best keys, sorted, in LDS [0, 128) and their smallest as the THRESHOLD.  It walks its candidates in
// tiles of 1024 (four independent loads per thread, the next tile's in flight across the barriers); a candidate that beats the
// threshold is looked up in the query's range of the completion keys (binary search) and, when it is none of them, appended to
// LDS [128, 2048) through an LDS counter (one atomic per wave).  When the next tile might not fit, and at the end, best + appended
// are sorted (bitonic, descending, over the next power of two) and cut to K.  The threshold only changes there, between barriers.
// (kTopkLds, kTopkTile, TopkShared, topk_push and topk_flush are in select_keys.h, shared with candidate_select.hip)
enum { kTopkRow = 0, kTopkSlice = 1, kTopkCombine = 2 };

// MODE kTopkRow:     grid (queries): the whole row, value / index written.
// MODE kTopkSlice:   grid (slices, queries): candidates [slice * kRankSlice, ...), the slice's K keys -> ws[q, slice, 0 .. K).
// MODE kTopkCombine: grid (queries): the best K of ws[q, 0 .. n_slices * K), value / index written.
template <int MODE>
__global__ __launch_bounds__(256) void topk_keys_kernel(const float *pred, long long row_stride, long long n_cand, int K,
                                                        const int64_t *keys, long long n_keys, const int64_t *anchor,
                                                        const int64_t *rel, long long index_stride, long long n_rel,
                                                        unsigned long long *ws, long long n_slices, float *value, int64_t *index) {
    __shared__ TopkShared sh;
    const int tid = threadIdx.x;
    const long long q = MODE == kTopkSlice ? blockIdx.y : blockIdx.x;
    const float *row = pred + q * row_stride;
    long long c0 = 0, c1 = n_cand;
    if constexpr (MODE == kTopkSlice) {
        c0 = (long long)blockIdx.x * kRankSlice;
        c1 = c0 + kRankSlice < n_cand ? c0 + kRankSlice : n_cand;
    }
    if constexpr (MODE == kTopkCombine) c1 = n_slices * K;
    const unsigned long long *src = ws + q * n_slices * K;         // (kTopkCombine reads it, kTopkSlice writes behind it)
    const bool filtered = MODE != kTopkCombine && keys != nullptr;
    int64_t base = 0;
    if (tid < kTopkMax) sh.arr[tid] = kTopkEmpty;
    if (tid == 0) {
        sh.thr = kTopkEmpty;
        sh.count = 0;
    }
    if (filtered) {
        base = (anchor[q * index_stride] * n_rel + rel[q * index_stride]) * n_cand;
        if (tid < 2) sh.range[tid] = lower_bound_i64(keys, n_keys, base + (tid ? c1 : c0));     // the slice's part of the range
    }
    __syncthreads();
    const long long lo = filtered ? sh.range[0] : 0, hi = filtered ? sh.range[1] : 0;

    unsigned long long cur[4], nxt[4] = {0ull, 0ull, 0ull, 0ull};
    auto load_tile = [&](unsigned long long (&out)[4], long long c) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const long long cc = c + tid + 256 * i;
            if constexpr (MODE == kTopkCombine) out[i] = cc < c1 ? src[cc] : kTopkEmpty;
            else out[i] = cc < c1 ? (unsigned long long)__float_as_uint(row[cc]) : 0ull;          // raw bits: the key is formed later
        }
    };
    load_tile(cur, c0);
    for (long long c = c0; c < c1; c += kTopkTile) {
        if (c + kTopkTile < c1) load_tile(nxt, c + kTopkTile);
        const unsigned long long thr = sh.thr;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const long long cc = c + tid + 256 * i;
            unsigned long long key = kTopkEmpty;
            if (cc < c1) key = MODE == kTopkCombine ? cur[i] : topk_key(__uint_as_float((unsigned)cur[i]), cc);
            bool pass = key > thr;
            if (pass && lo < hi) {
                const long long at = lo + lower_bound_i64(keys + lo, hi - lo, base + cc);
                if (at < hi && keys[at] == base + cc) pass = false;                                // a known completion
            }
            topk_push(sh, key, pass);
        }
        __syncthreads();
        const int cnt = sh.count;
        __syncthreads();                                           // (nobody appends to the next tile before everybody has read cnt)
        if (cnt > kTopkLds - kTopkMax - kTopkTile) topk_flush(sh, K);
#pragma unroll
        for (int i = 0; i < 4; ++i) cur[i] = nxt[i];
    }
    topk_flush(sh, K);
    if (tid < K) {
        const unsigned long long key = sh.arr[tid];
        if constexpr (MODE == kTopkSlice) {
            ws[(q * n_slices + blockIdx.x) * K + tid] = key;
        } else {
            const long long e = key == kTopkEmpty ? -1 : (long long)(~(unsigned)key);
            index[q * K + tid] = e;
            value[q * K + tid] = e < 0 ? -INFINITY : row[e];       // the score's own bits, not the key's
        }
    }
}

// Lexicographic lower bound over three sorted int32 columns.
__device__ __forceinline__ long long lower_bound_3(const int32_t *a, const int32_t *b, const int32_t *c, long long n,
                                                   int va, int vb, int vc) {
    long long lo = 0, hi = n;
    while (lo < hi) {
        const long long mid = (lo + hi) >> 1;
        const int xa = a[mid], xb = b[mid], xc = c[mid];
        const bool less = xa < va || (xa == va && (xb < vb || (xb == vb && xc < vc)));
        if (less) lo = mid + 1; else hi = mid;
    }
    return lo;
}

struct RemovalParams {
    // the three plans of the graph WITH inverse edges; each sorted by its own (row, second, third) key
    const int32_t *f_row, *f_a, *f_rel;          // forward:    (dst, src, rel)
    const int32_t *s_row, *s_a, *s_rel;          // d_input:    (src, dst, rel)
    const int32_t *r_row, *r_b, *r_a;            // d_relation: (rel, dst, src)
    long long n_edges;
    const int64_t *h, *t, *r;                    // [n_pattern] triples to remove (h -> t, relation r) and their inverses
    long long n_pattern;
    long long n_base_rel;                        // inverse of relation r is r + n_base_rel
    float *w_fwd, *w_src, *w_rel;                // [n_edges + slack], pre-filled with the plans' own weights
    uint32_t *m_fwd, *m_src, *m_rel;             // optional marked copies of the plans' packed words (bit 31 = removed), or NULL
};

__global__ __launch_bounds__(256) void edge_removal_kernel(const RemovalParams p) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= 2 * p.n_pattern) return;
    const long long k = i >> 1;
    const bool inverse = (i & 1) != 0;
    // undirected(add_inverse=True): edge (h, t, r) and its flipped copy (t, h, r + R)   (ultra/model.py:166)
    const int src = (int)(inverse ? p.t[k] : p.h[k]);
    const int dst = (int)(inverse ? p.h[k] : p.t[k]);
    const int rel = (int)(p.r[k] + (inverse ? p.n_base_rel : 0));
    long long e = lower_bound_3(p.f_row, p.f_a, p.f_rel, p.n_edges, dst, src, rel);
    if (e >= p.n_edges || p.f_row[e] != dst || p.f_a[e] != src || p.f_rel[e] != rel) return;   // not an edge (a negative)
    p.w_fwd[e] = 0.0f;
    if (p.m_fwd != nullptr) atomicOr(p.m_fwd + e, 0x80000000u);       // (a triple listed twice marks the same word twice)
    e = lower_bound_3(p.s_row, p.s_a, p.s_rel, p.n_edges, src, dst, rel);
    p.w_src[e] = 0.0f;
    if (p.m_src != nullptr) atomicOr(p.m_src + e, 0x80000000u);
    e = lower_bound_3(p.r_row, p.r_b, p.r_a, p.n_edges, rel, dst, src);
    p.w_rel[e] = 0.0f;
    if (p.m_rel != nullptr) atomicOr(p.m_rel + e, 0x80000000u);
}

// The one-hop rule (ultra/model.py:57-74 with remove_one_hop = True): EVERY edge between the heads and the tails of a batch goes,
// in either direction and under any relation.  An ordered pair (src, dst) is a range lookup where a triple is a point lookup:
//   forward plan    (dst, src, rel): its edges are ONE run, found by the lower bound of (dst, src, 0);
//   d_input plan    (src, dst, rel): a run of the same length in the same relation order, from the lower bound of (src, dst, 0);
//   d_relation plan (rel, dst, src): one point lookup per edge of the run, with the relation read from the forward run.
// One lane searches one ordered pair -- most pairs of a batch are negatives that no edge connects and end there; the runs that
// exist (0 .. 2R edges each) are then walked by the whole wave, one after the other, lane l taking the edges l, l + 64, ...
// Every write is a store of 0.0f or an atomicOr of bit 31: a pair listed twice, (u, v) beside (v, u) with u == v, or another
// split of the work over lanes and waves write the same words with the same values.
struct PairRemovalParams {
    const int32_t *f_row, *f_a, *f_rel;          // forward:    (dst, src, rel)
    const int32_t *s_row, *s_a, *s_rel;          // d_input:    (src, dst, rel)
    const int32_t *r_row, *r_b, *r_a;            // d_relation: (rel, dst, src)
    long long n_edges;
    const int64_t *h, *t;                        // [n_pattern] node pairs; both orders are removed
    long long n_pattern;
    long long n_node;                            // ids outside [0, n_node) match nothing
    float *w_fwd, *w_src, *w_rel;                // [n_edges + slack], pre-filled with the plans' own weights
    uint32_t *m_fwd, *m_src, *m_rel;             // optional marked copies of the plans' packed words (bit 31 = removed), or NULL
};

__global__ __launch_bounds__(256) void pair_removal_kernel(const PairRemovalParams p) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const long long E = p.n_edges;                                    // < 2^31 (check_segments): positions fit an int
    int src = 0, dst = 0, f0 = 0, s0 = 0;
    bool found = false;
    if (i < 2 * p.n_pattern) {
        const long long k = i >> 1;
        const long long a = (i & 1) ? p.t[k] : p.h[k], b = (i & 1) ? p.h[k] : p.t[k];
        if (a >= 0 && a < p.n_node && b >= 0 && b < p.n_node) {
            src = (int)a;
            dst = (int)b;
            const long long e = lower_bound_3(p.f_row, p.f_a, p.f_rel, E, dst, src, 0);     // relations are >= 0: the run's start
            found = e < E && p.f_row[e] == dst && p.f_a[e] == src;
            if (found) {
                f0 = (int)e;
                s0 = (int)lower_bound_3(p.s_row, p.s_a, p.s_rel, E, src, dst, 0);
            }
        }
    }
    // (no lane has left: the shuffles below read every lane of the wave)
    unsigned long long todo = __ballot(found ? 1 : 0);
    while (todo != 0ull) {
        const int owner = __ffsll((long long)todo) - 1;
        todo &= todo - 1ull;
        const int u = __shfl(src, owner, 64), v = __shfl(dst, owner, 64);
        const long long fb = __shfl(f0, owner, 64), sb = __shfl(s0, owner, 64);
        for (long long j = lane;; j += 64) {
            const long long ef = fb + j;
            if (ef >= E || p.f_row[ef] != v || p.f_a[ef] != u) break;                       // past the run
            const int rel = p.f_rel[ef];
            p.w_fwd[ef] = 0.0f;
            if (p.m_fwd != nullptr) atomicOr(p.m_fwd + ef, 0x80000000u);
            // the same edge in the other two orders; the comparisons hold for plans of one edge set and keep every write inside
            // the arrays for any others
            const long long es = sb + j;
            if (es < E && p.s_row[es] == u && p.s_a[es] == v && p.s_rel[es] == rel) {
                p.w_src[es] = 0.0f;
                if (p.m_src != nullptr) atomicOr(p.m_src + es, 0x80000000u);
            }
            const long long er = lower_bound_3(p.r_row, p.r_b, p.r_a, E, rel, v, u);
            if (er < E && p.r_row[er] == rel && p.r_b[er] == v && p.r_a[er] == u) {
                p.w_rel[er] = 0.0f;
                if (p.m_rel != nullptr) atomicOr(p.m_rel + er, 0x80000000u);
            }
        }
    }
}

// the weight arrays (ones) and the word copies of the three plans in one launch: blockIdx.y picks the array
struct RemovalFillParams {
    float *w[3];
    uint32_t *m[3];
    const uint32_t *words[3];
    long long n_total;
};
__global__ __launch_bounds__(256) void removal_fill_kernel(const RemovalFillParams p) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= p.n_total) return;
    const int k = blockIdx.y;
    p.w[k][i] = 1.0f;
    if (p.m[k] != nullptr) p.m[k][i] = p.words[k][i];
}

__global__ __launch_bounds__(256) void fill_weights_kernel(const float *base, float *out, long long n_edges, long long n_total) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_total) return;
    out[i] = (base != nullptr && i < n_edges) ? base[i] : 1.0f;
}

}  // namespace

extern "C" {

int ultra_filtered_rank_keys(const float *pred, int64_t n_query, int64_t n_cand, int64_t row_stride, const int64_t *target,
                             int64_t target_stride, const int64_t *keys, int64_t n_keys, const int64_t *anchor,
                             const int64_t *rel, int64_t index_stride, int64_t n_rel, int64_t *rank, int64_t rank_stride,
                             void *stream) {
    if (n_query < 0 || n_cand <= 0 || row_stride < n_cand || n_keys < 0) return ULTRA_ERR_BAD_SHAPE;
    if (n_query == 0) return ULTRA_OK;
    if (pred == nullptr || target == nullptr || rank == nullptr) return ULTRA_ERR_NULL_POINTER;
    if (keys != nullptr && (anchor == nullptr || rel == nullptr || n_rel <= 0)) return ULTRA_ERR_NULL_POINTER;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const bool sliced = n_cand > 2 * kRankSlice;
    if (n_query > 65535 && sliced) return ULTRA_ERR_BAD_SHAPE;                // grid.y
    if (sliced) {
        hipLaunchKernelGGL(filtered_rank_keys_kernel<true>, dim3((unsigned)n_query), dim3(256), 0, s, pred, (long long)row_stride,
                           (long long)n_cand, target, (long long)target_stride, keys, (long long)n_keys, anchor, rel,
                           (long long)index_stride, (long long)n_rel, rank, (long long)rank_stride);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(rank_slices_kernel, dim3((unsigned)((n_cand + kRankSlice - 1) / kRankSlice), (unsigned)n_query), dim3(256),
                           0, s, pred, (long long)row_stride, (long long)n_cand, target, (long long)target_stride, rank,
                           (long long)rank_stride);
    } else {
        hipLaunchKernelGGL(filtered_rank_keys_kernel<false>, dim3((unsigned)n_query), dim3(256), 0, s, pred, (long long)row_stride,
                           (long long)n_cand, target, (long long)target_stride, keys, (long long)n_keys, anchor, rel,
                           (long long)index_stride, (long long)n_rel, rank, (long long)rank_stride);
    }
    HIP_TRY(hipGetLastError());
    return ULTRA_OK;
}

int ultra_strict_negative(const int64_t *keys, int64_t n_keys, const int64_t *anchor, const int64_t *rel, int64_t n_query,
                          int64_t n_rel, int64_t n_node, const float *rand, int64_t n_sample, int64_t *out, void *stream) {
    if (n_query < 0 || n_sample < 0 || n_keys < 0 || n_rel <= 0 || n_node <= 0) return ULTRA_ERR_BAD_SHAPE;
    const long long total = (long long)n_query * n_sample;
    if (total == 0) return ULTRA_OK;
    if (anchor == nullptr || rel == nullptr || rand == nullptr || out == nullptr) return ULTRA_ERR_NULL_POINTER;
    if (n_keys > 0 && keys == nullptr) return ULTRA_ERR_NULL_POINTER;
    hipLaunchKernelGGL(strict_negative_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0,
                       static_cast<hipStream_t>(stream), keys, (long long)n_keys, anchor, rel, (long long)n_query,
                       (long long)n_rel, (long long)n_node, rand, (long long)n_sample, out);
    HIP_TRY(hipGetLastError());
    return ULTRA_OK;
}

int ultra_filter_counts(const int64_t *keys, int64_t n_keys, const int64_t *anchor, const int64_t *rel, int64_t index_stride,
                        int64_t n_query, int64_t n_rel, int64_t n_node, int64_t *n_free, void *stream) {
    if (n_query < 0 || n_keys < 0 || n_node <= 0 || index_stride < 0) return ULTRA_ERR_BAD_SHAPE;
    if (n_query == 0) return ULTRA_OK;
    if (n_free == nullptr) return ULTRA_ERR_NULL_POINTER;
    if (keys != nullptr && (anchor == nullptr || rel == nullptr)) return ULTRA_ERR_NULL_POINTER;
    if (keys != nullptr && n_rel <= 0) return ULTRA_ERR_BAD_SHAPE;
    hipLaunchKernelGGL(filter_counts_kernel, dim3((unsigned)((n_query + 255) / 256)), dim3(256), 0,
                       static_cast<hipStream_t>(stream), keys, (long long)n_keys, anchor, rel, (long long)index_stride,
                       (long long)n_query, (long long)n_rel, (long long)n_node, n_free);
    HIP_TRY(hipGetLastError());
    return ULTRA_OK;
}

int ultra_sampled_rank_keys(const float *pred, int64_t n_query, int64_t n_cand, int64_t row_stride, const int64_t *target,
                            int64_t target_stride, const int64_t *keys, int64_t n_keys, const int64_t *anchor,
                            const int64_t *rel, int64_t index_stride, int64_t n_rel, const float *rand, int64_t n_sample,
                            int64_t *optimistic, int64_t *pessimistic, int64_t *samples, void *stream) {
    if (n_query < 0 || n_cand <= 0 || row_stride < n_cand || n_keys < 0 || target_stride < 0 || index_stride < 0)
        return ULTRA_ERR_BAD_SHAPE;
    if (n_sample < 1 || n_sample > kSampledMax) return ULTRA_ERR_BAD_SHAPE;
    if (n_query == 0) return ULTRA_OK;
    if (pred == nullptr || target == nullptr || rand == nullptr || optimistic == nullptr || pessimistic == nullptr)
        return ULTRA_ERR_NULL_POINTER;
    if (keys != nullptr && (anchor == nullptr || rel == nullptr)) return ULTRA_ERR_NULL_POINTER;
    if (keys != nullptr && n_rel <= 0) return ULTRA_ERR_BAD_SHAPE;
    hipLaunchKernelGGL(sampled_rank_keys_kernel, dim3((unsigned)((n_query + kSampledWaves - 1) / kSampledWaves)),
                       dim3(64 * kSampledWaves), 0, static_cast<hipStream_t>(stream), pred, (long long)row_stride,
                       (long long)n_cand, (long long)n_query, target, (long long)target_stride, keys, (long long)n_keys, anchor,
                       rel, (long long)index_stride, (long long)n_rel, rand, (int)n_sample, optimistic, pessimistic, samples);
    HIP_TRY(hipGetLastError());
    return ULTRA_OK;
}

size_t ultra_topk_keys_workspace(int64_t n_query, int64_t n_cand, int64_t k) {
    if (n_query <= 0 || n_cand <= kRankSlice || k < 1 || k > kTopkMax) return 0;           // short rows: one launch, no workspace
    return (size_t)n_query * (size_t)((n_cand + kRankSlice - 1) / kRankSlice) * (size_t)k * sizeof(unsigned long long);
}

int ultra_topk_keys(const float *pred, int64_t n_query, int64_t n_cand, int64_t row_stride, int64_t k, const int64_t *keys,
                    int64_t n_keys, const int64_t *anchor, const int64_t *rel, int64_t index_stride, int64_t n_rel, float *value,
                    int64_t *index, void *workspace, size_t workspace_bytes, void *stream) {
    if (n_query < 0 || n_cand <= 0 || n_cand > 0x7fffffffLL || row_stride < n_cand || n_keys < 0 || index_stride < 0)
        return ULTRA_ERR_BAD_SHAPE;
    if (k < 1 || k > kTopkMax) return ULTRA_ERR_BAD_SHAPE;
    if (n_query == 0) return ULTRA_OK;
    if (pred == nullptr || value == nullptr || index == nullptr) return ULTRA_ERR_NULL_POINTER;
    if (keys != nullptr && (anchor == nullptr || rel == nullptr)) return ULTRA_ERR_NULL_POINTER;
    if (keys != nullptr && n_rel <= 0) return ULTRA_ERR_BAD_SHAPE;
    const bool sliced = n_cand > kRankSlice;
    if (n_query > (sliced ? 65535 : 0x7fffffffLL)) return ULTRA_ERR_BAD_SHAPE;              // grid.y / grid.x
    const size_t need = ultra_topk_keys_workspace(n_query, n_cand, k);
    if (need > 0 && (workspace == nullptr || workspace_bytes < need)) return ULTRA_ERR_WORKSPACE;
    hipStream_t s = static_cast<hipStream_t>(stream);
    unsigned long long *ws = static_cast<unsigned long long *>(workspace);
    if (sliced) {
        const long long n_slices = (n_cand + kRankSlice - 1) / kRankSlice;
        hipLaunchKernelGGL(topk_keys_kernel<kTopkSlice>, dim3((unsigned)n_slices, (unsigned)n_query), dim3(256), 0, s, pred,
                           (long long)row_stride, (long long)n_cand, (int)k, keys, (long long)n_keys, anchor, rel,
                           (long long)index_stride, (long long)n_rel, ws, n_slices, value, index);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(topk_keys_kernel<kTopkCombine>, dim3((unsigned)n_query), dim3(256), 0, s, pred, (long long)row_stride,
                           (long long)n_cand, (int)k, keys, (long long)n_keys, anchor, rel, (long long)index_stride,
                           (long long)n_rel, ws, n_slices, value, index);
    } else {
        hipLaunchKernelGGL(topk_keys_kernel<kTopkRow>, dim3((unsigned)n_query), dim3(256), 0, s, pred, (long long)row_stride,
                           (long long)n_cand, (int)k, keys, (long long)n_keys, anchor, rel, (long long)index_stride,
                           (long long)n_rel, ws, 0LL, value, index);
    }
    HIP_TRY(hipGetLastError());
    return ULTRA_OK;
}

int ultra_edge_removal_weights(const ultra_segments *fwd, const ultra_segments *by_src, const ultra_segments *by_rel,
                               const int64_t *h, const int64_t *t, const int64_t *r, int64_t n_pattern,
                               int64_t n_base_rel, float *w_fwd, float *w_src, float *w_rel, int64_t slack, void *stream) {
    int rc = check_segments(fwd);
    if (!rc) rc = check_segments(by_src);
    if (!rc) rc = check_segments(by_rel);
    if (rc) return rc;
    if (fwd->n_edges != by_src->n_edges || fwd->n_edges != by_rel->n_edges || n_pattern < 0 || slack < 0)
        return ULTRA_ERR_BAD_SHAPE;
    if (w_fwd == nullptr || w_src == nullptr || w_rel == nullptr) return ULTRA_ERR_NULL_POINTER;
    if (n_pattern > 0 && (h == nullptr || t == nullptr || r == nullptr)) return ULTRA_ERR_NULL_POINTER;
    if (fwd->n_edges > 0 && by_rel->node_b == nullptr) return ULTRA_ERR_NULL_POINTER;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const long long E = fwd->n_edges, total = E + slack;
    if (total > 0) {
        const unsigned blocks = (unsigned)((total + 255) / 256);
        hipLaunchKernelGGL(fill_weights_kernel, dim3(blocks), dim3(256), 0, s, fwd->weight, w_fwd, E, total);
        hipLaunchKernelGGL(fill_weights_kernel, dim3(blocks), dim3(256), 0, s, by_src->weight, w_src, E, total);
        hipLaunchKernelGGL(fill_weights_kernel, dim3(blocks), dim3(256), 0, s, by_rel->weight, w_rel, E, total);
    }
    if (n_pattern > 0 && E > 0) {
        RemovalParams p;
        p.f_row = fwd->row; p.f_a = fwd->node_a; p.f_rel = fwd->rel;
        p.s_row = by_src->row; p.s_a = by_src->node_a; p.s_rel = by_src->rel;
        p.r_row = by_rel->row; p.r_b = by_rel->node_b; p.r_a = by_rel->node_a;
        p.n_edges = E;
        p.h = h; p.t = t; p.r = r;
        p.n_pattern = n_pattern;
        p.n_base_rel = n_base_rel;
        p.w_fwd = w_fwd; p.w_src = w_src; p.w_rel = w_rel;
        p.m_fwd = nullptr; p.m_src = nullptr; p.m_rel = nullptr;
        hipLaunchKernelGGL(edge_removal_kernel, dim3((unsigned)((2 * n_pattern + 255) / 256)), dim3(256), 0, s, p);
    }
    HIP_TRY(hipGetLastError());
    return ULTRA_OK;
}

int ultra_edge_removal_marks(const ultra_segments *fwd, const ultra_segments *by_src, const ultra_segments *by_rel,
                             const int64_t *h, const int64_t *t, const int64_t *r, int64_t n_pattern, int64_t n_base_rel,
                             float *w_fwd, float *w_src, float *w_rel, int64_t slack, uint32_t *words_fwd, uint32_t *words_src,
                             uint32_t *words_rel, int64_t n_node, void *stream) {
    int rc = check_segments(fwd);
    if (!rc) rc = check_segments(by_src);
    if (!rc) rc = check_segments(by_rel);
    if (rc) return rc;
    if (fwd->n_edges != by_src->n_edges || fwd->n_edges != by_rel->n_edges || n_pattern < 0 || slack < 0 || slack > 16 || n_node <= 0)
        return ULTRA_ERR_BAD_SHAPE;
    if (w_fwd == nullptr || w_src == nullptr || w_rel == nullptr) return ULTRA_ERR_NULL_POINTER;
    if (n_pattern > 0 && (h == nullptr || t == nullptr || r == nullptr)) return ULTRA_ERR_NULL_POINTER;
    if (fwd->n_edges > 0 && by_rel->node_b == nullptr) return ULTRA_ERR_NULL_POINTER;
    const ultra_segments *plans[3] = {fwd, by_src, by_rel};
    uint32_t *marks[3] = {words_fwd, words_src, words_rel};
    for (int k = 0; k < 3; ++k) {
        if (plans[k]->weight != nullptr) return ULTRA_ERR_BAD_SHAPE;               // ones only: the marks replace the weights
        if (marks[k] == nullptr) continue;
        // bit 31 must be free: the node field [packed_src_shift, 32) holds ids below n_node
        if (plans[k]->packed == nullptr || plans[k]->packed_src_shift >= 31 ||
            ((unsigned long long)(n_node - 1) >> (31 - plans[k]->packed_src_shift)) != 0ull)
            return ULTRA_ERR_BAD_SHAPE;
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    const long long E = fwd->n_edges, total = E + slack;
    if (total > 0) {
        RemovalFillParams f;
        f.w[0] = w_fwd; f.w[1] = w_src; f.w[2] = w_rel;
        for (int k = 0; k < 3; ++k) { f.m[k] = marks[k]; f.words[k] = plans[k]->packed; }
        f.n_total = total;
        hipLaunchKernelGGL(removal_fill_kernel, dim3((unsigned)((total + 255) / 256), 3), dim3(256), 0, s, f);
    }
    if (n_pattern > 0 && E > 0) {
        RemovalParams p;
        p.f_row = fwd->row; p.f_a = fwd->node_a; p.f_rel = fwd->rel;
        p.s_row = by_src->row; p.s_a = by_src->node_a; p.s_rel = by_src->rel;
        p.r_row = by_rel->row; p.r_b = by_rel->node_b; p.r_a = by_rel->node_a;
        p.n_edges = E;
        p.h = h; p.t = t; p.r = r;
        p.n_pattern = n_pattern;
        p.n_base_rel = n_base_rel;
        p.w_fwd = w_fwd; p.w_src = w_src; p.w_rel = w_rel;
        p.m_fwd = words_fwd; p.m_src = words_src; p.m_rel = words_rel;
        hipLaunchKernelGGL(edge_removal_kernel, dim3((unsigned)((2 * n_pattern + 255) / 256)), dim3(256), 0, s, p);
    }
    HIP_TRY(hipGetLastError());
    return ULTRA_OK;
}

int ultra_pair_removal(const ultra_segments *fwd, const ultra_segments *by_src, const ultra_segments *by_rel, const int64_t *h,
                       const int64_t *t, int64_t n_pattern, float *w_fwd, float *w_src, float *w_rel, int64_t slack,
                       uint32_t *words_fwd, uint32_t *words_src, uint32_t *words_rel, int64_t n_node, void *stream) {
    int rc = check_segments(fwd);
    if (!rc) rc = check_segments(by_src);
    if (!rc) rc = check_segments(by_rel);
    if (rc) return rc;
    if (fwd->n_edges != by_src->n_edges || fwd->n_edges != by_rel->n_edges || n_pattern < 0 || slack < 0 || n_node <= 0)
        return ULTRA_ERR_BAD_SHAPE;
    if (n_pattern > (1LL << 37)) return ULTRA_ERR_BAD_SHAPE;                           // grid.x: one lane per ordered pair
    if (w_fwd == nullptr || w_src == nullptr || w_rel == nullptr) return ULTRA_ERR_NULL_POINTER;
    if (n_pattern > 0 && (h == nullptr || t == nullptr)) return ULTRA_ERR_NULL_POINTER;
    if (fwd->n_edges > 0 && by_rel->node_b == nullptr) return ULTRA_ERR_NULL_POINTER;
    const ultra_segments *plans[3] = {fwd, by_src, by_rel};
    uint32_t *marks[3] = {words_fwd, words_src, words_rel};
    const bool marked = words_fwd != nullptr || words_src != nullptr || words_rel != nullptr;
    if (marked) {                                                                      // as ultra_edge_removal_marks
        if (slack > 16) return ULTRA_ERR_BAD_SHAPE;
        for (int k = 0; k < 3; ++k) {
            if (plans[k]->weight != nullptr) return ULTRA_ERR_BAD_SHAPE;               // ones only: the marks replace the weights
            if (marks[k] == nullptr) continue;
            if (plans[k]->packed == nullptr || plans[k]->packed_src_shift >= 31 ||
                ((unsigned long long)(n_node - 1) >> (31 - plans[k]->packed_src_shift)) != 0ull)
                return ULTRA_ERR_BAD_SHAPE;
        }
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    const long long E = fwd->n_edges, total = E + slack;
    if (total > 0) {
        const unsigned blocks = (unsigned)((total + 255) / 256);
        if (marked) {
            RemovalFillParams f;
            f.w[0] = w_fwd; f.w[1] = w_src; f.w[2] = w_rel;
            for (int k = 0; k < 3; ++k) { f.m[k] = marks[k]; f.words[k] = plans[k]->packed; }
            f.n_total = total;
            hipLaunchKernelGGL(removal_fill_kernel, dim3(blocks, 3), dim3(256), 0, s, f);
        } else {
            hipLaunchKernelGGL(fill_weights_kernel, dim3(blocks), dim3(256), 0, s, fwd->weight, w_fwd, E, total);
            hipLaunchKernelGGL(fill_weights_kernel, dim3(blocks), dim3(256), 0, s, by_src->weight, w_src, E, total);
            hipLaunchKernelGGL(fill_weights_kernel, dim3(blocks), dim3(256), 0, s, by_rel->weight, w_rel, E, total);
        }
    }
    if (n_pattern > 0 && E > 0) {
        PairRemovalParams p;
        p.f_row = fwd->row; p.f_a = fwd->node_a; p.f_rel = fwd->rel;
        p.s_row = by_src->row; p.s_a = by_src->node_a; p.s_rel = by_src->rel;
        p.r_row = by_rel->row; p.r_b = by_rel->node_b; p.r_a = by_rel->node_a;
        p.n_edges = E;
        p.h = h; p.t = t;
        p.n_pattern = n_pattern;
        p.n_node = n_node;
        p.w_fwd = w_fwd; p.w_src = w_src; p.w_rel = w_rel;
        p.m_fwd = words_fwd; p.m_src = words_src; p.m_rel = words_rel;
        hipLaunchKernelGGL(pair_removal_kernel, dim3((unsigned)((2 * n_pattern + 255) / 256)), dim3(256), 0, s, p);
    }
    HIP_TRY(hipGetLastError());
    return ULTRA_OK;
}

}  // extern "C"

// ---------------------------------------------------------------------------------------- queries of an evaluation batch
// prepare_queries_kernel: the index glue between the relation stack and the entity stack of task.predict, in ONE launch.
// The reference (ultra/task.py:249-259, ultra/model.py:76-83,101-114) builds for a batch of B triples (h, t, r) the 2B
// tail-form queries -- (h, r, ?) and (t, r + R, ?) -- with cat / add / arange / advanced-index / int32-cast kernels of a
// few microseconds each (nine launches per batch here before this kernel existed); the results are plain copies:
//     anchor[q]   = h[q]           (q < B)      t[q - B]            (q >= B)
//     relation[q] = r[q]           (q < B)      r[q - B] + n_base_rel
//     query[q, :] = rel_rep[q mod B, relation[q], :]                        (the conditioned relation representation)
namespace {
__global__ __launch_bounds__(256) void prepare_queries_kernel(const long long *batch, const float *rel_rep, long long stride_b,
                                                              long long stride_r, int B, int n_rel2, int n_base_rel,
                                                              long long *anchor, int32_t *anchor32, long long *relation,
                                                              float *query) {
    const int q = blockIdx.x;                       // 0 .. 2B - 1
    const int b = q < B ? q : q - B;
    const long long h = batch[3 * b + 0], t = batch[3 * b + 1], r = batch[3 * b + 2];
    const long long a = q < B ? h : t, rr = q < B ? r : r + n_base_rel;
    if (threadIdx.x == 0) {
        anchor[q] = a;
        anchor32[q] = (int32_t)a;
        relation[q] = rr;
    }
    if (threadIdx.x < 64) query[(long long)q * 64 + threadIdx.x] = rel_rep[b * stride_b + rr * stride_r + threadIdx.x];
}

// relation_stack_inputs_kernel: what the relation stack needs before its first layer, in ONE launch (the reference builds
// them with ones / expand / stack / cast kernels, ultra/rel_model.py:351-378, ultra/layer.py:143-151):
//     tables[l, r, q, :] = weight_l[r, :]      the layers' relation embeddings (4 edge types x 64) tiled over the queries
//     ones[q, :] = 1                           the boundary value of every query (rel_model.py:355)
//     node32[q] = (int32) h_index[q]           the boundary nodes for the frontier kernel and the sparse epilogue
constexpr int kRelStackMaxLayers = 8;
struct RelStackParams {
    const float *weight[kRelStackMaxLayers];     // each [n_rel, 64]
    const long long *h_index;                    // n_query indices, h_stride elements apart
    long long h_stride;
    float *tables;                               // [n_layers, n_rel, n_query, 64]
    float *ones;                                 // [n_query, 64]
    int32_t *node32;                             // [n_query]
    int n_layers, n_rel, n_query;
};

__global__ __launch_bounds__(256) void relation_stack_inputs_kernel(const RelStackParams p) {
    const long long per_layer = (long long)p.n_rel * p.n_query * 16;             // float4 items
    const long long total = per_layer * p.n_layers;
    const long long stride = (long long)gridDim.x * blockDim.x;
    const long long tid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    typedef float f4 __attribute__((ext_vector_type(4)));
    for (long long i = tid; i < total; i += stride) {
        const int l = (int)(i / per_layer);
        const long long j = i - l * per_layer;
        const int c = (int)(j & 15);
        const int r = (int)((j >> 4) / p.n_query);
        reinterpret_cast<f4 *>(p.tables)[i] = reinterpret_cast<const f4 *>(p.weight[l])[r * 16 + c];
    }
    const f4 one = {1.0f, 1.0f, 1.0f, 1.0f};
    for (long long i = tid; i < (long long)p.n_query * 16; i += stride) reinterpret_cast<f4 *>(p.ones)[i] = one;
    for (long long i = tid; i < p.n_query; i += stride) p.node32[i] = (int32_t)p.h_index[i * p.h_stride];
}
}  // namespace

extern "C" int ultra_relation_stack_inputs(const float *const *weights, int64_t n_layers, int64_t n_rel, int64_t n_query,
                                           const int64_t *h_index, int64_t h_stride, float *tables, float *ones, int32_t *node32,
                                           void *stream) {
    if (n_layers < 0 || n_layers > kRelStackMaxLayers || n_rel < 0 || n_query < 0 || n_rel > 0x7fffffffLL || n_query > 0x7fffffffLL ||
        h_stride < 0)
        return ULTRA_ERR_BAD_SHAPE;
    if (n_query == 0) return ULTRA_OK;
    if (h_index == nullptr || ones == nullptr || node32 == nullptr || (n_layers > 0 && n_rel > 0 && (weights == nullptr || tables == nullptr)))
        return ULTRA_ERR_NULL_POINTER;
    RelStackParams p{};
    for (int l = 0; l < (int)n_layers; ++l) {
        if (n_rel > 0 && weights[l] == nullptr) return ULTRA_ERR_NULL_POINTER;
        p.weight[l] = weights[l];
    }
    p.h_index = reinterpret_cast<const long long *>(h_index); p.h_stride = h_stride; p.tables = tables; p.ones = ones; p.node32 = node32;
    p.n_layers = (int)n_layers; p.n_rel = (int)n_rel; p.n_query = (int)n_query;
    const long long items = n_layers * n_rel * n_query * 16 + n_query * 16;
    long long blocks = (items + 255) / 256;
    if (blocks > 1024) blocks = 1024;
    if (blocks < 1) blocks = 1;
    hipLaunchKernelGGL(relation_stack_inputs_kernel, dim3((unsigned)blocks), dim3(256), 0, static_cast<hipStream_t>(stream), p);
    HIP_TRY(hipGetLastError());
    return ULTRA_OK;
}

extern "C" int ultra_prepare_queries(const int64_t *batch, const float *rel_rep, int64_t stride_b, int64_t stride_r,
                                     int64_t n_batch, int64_t n_rel2, int64_t n_base_rel, int64_t *anchor, int32_t *anchor32,
                                     int64_t *relation, float *query, void *stream) {
    if (n_batch < 0 || n_rel2 <= 0 || n_base_rel < 0 || 2 * n_base_rel > n_rel2 || n_batch > 0x3fffffffLL || stride_b < 0 || stride_r < 0)
        return ULTRA_ERR_BAD_SHAPE;
    if (n_batch == 0) return ULTRA_OK;
    if (batch == nullptr || rel_rep == nullptr || anchor == nullptr || anchor32 == nullptr || relation == nullptr || query == nullptr)
        return ULTRA_ERR_NULL_POINTER;
    hipLaunchKernelGGL(prepare_queries_kernel, dim3((unsigned)(2 * n_batch)), dim3(256), 0, static_cast<hipStream_t>(stream),
                       reinterpret_cast<const long long *>(batch), rel_rep, (long long)stride_b, (long long)stride_r, (int)n_batch,
                       (int)n_rel2, (int)n_base_rel,
                       reinterpret_cast<long long *>(anchor), anchor32, reinterpret_cast<long long *>(relation), query);
    HIP_TRY(hipGetLastError());
    return ULTRA_OK;
}

// ---------------------------------------------------------------------------------------- training metrics
// statistics kernels: norm / mean / unbiased std of the multiset { a[0 .. n_a) } U { every b[0 .. n_b) taken `b_repeat`
// times } in two launches (partial sums in double, then one block that adds them in a fixed order).  The reference logs
// `query_norm / query_mean / query_std` of the relation representations and `output_norm / output_mean / output_std`
// of node_feature = cat[hidden, query] in every training forward (ultra/model.py:158-160,178-181): as ATen reductions
// that is ~45 launches of a few microseconds (and, for tensors this size, multi-block reductions whose semaphore memset
// does not replay reliably inside a captured step); node_feature itself is never materialised here -- its query half is
// B vectors repeated for every node (b, b_repeat).
namespace {
constexpr int kStatThreads = 256;

__device__ inline void stat_block_reduce(double &sum, double &sq, double *lds) {
    lds[threadIdx.x] = sum;
    lds[kStatThreads + threadIdx.x] = sq;
    __syncthreads();
    for (int step = kStatThreads / 2; step > 0; step >>= 1) {
        if ((int)threadIdx.x < step) {
            lds[threadIdx.x] += lds[threadIdx.x + step];
            lds[kStatThreads + threadIdx.x] += lds[kStatThreads + threadIdx.x + step];
        }
        __syncthreads();
    }
    sum = lds[0];
    sq = lds[kStatThreads];
}

__global__ __launch_bounds__(kStatThreads) void statistics_partial_kernel(const float *a, long long n_a, double *partials) {
    __shared__ double lds[2 * kStatThreads];
    typedef float f4 __attribute__((ext_vector_type(4)));
    const long long n4 = n_a >> 2;
    const long long per = (n4 + gridDim.x - 1) / gridDim.x;
    const long long lo = (long long)blockIdx.x * per, hi = lo + per < n4 ? lo + per : n4;
    double sum = 0.0, sq = 0.0;
    for (long long i = lo + threadIdx.x; i < hi; i += kStatThreads) {
        const f4 v = reinterpret_cast<const f4 *>(a)[i];
        sum += ((double)v.x + (double)v.y) + ((double)v.z + (double)v.w);
        sq += ((double)v.x * v.x + (double)v.y * v.y) + ((double)v.z * v.z + (double)v.w * v.w);
    }
    if (blockIdx.x == gridDim.x - 1)                       // the last n_a % 4 elements
        for (long long i = (n4 << 2) + threadIdx.x; i < n_a; i += kStatThreads) {
            sum += (double)a[i];
            sq += (double)a[i] * a[i];
        }
    stat_block_reduce(sum, sq, lds);
    if (threadIdx.x == 0) {
        partials[2 * blockIdx.x] = sum;
        partials[2 * blockIdx.x + 1] = sq;
    }
}

__global__ __launch_bounds__(kStatThreads) void statistics_final_kernel(const double *partials, int n_partials, long long n_a,
                                                                        const float *b, long long n_b, long long b_repeat,
                                                                        float *out) {
    __shared__ double lds[2 * kStatThreads];
    double sum = 0.0, sq = 0.0;
    for (int i = threadIdx.x; i < n_partials; i += kStatThreads) {
        sum += partials[2 * i];
        sq += partials[2 * i + 1];
    }
    double sum_b = 0.0, sq_b = 0.0;
    for (long long i = threadIdx.x; i < n_b; i += kStatThreads) {
        sum_b += (double)b[i];
        sq_b += (double)b[i] * b[i];
    }
    sum += sum_b * (double)b_repeat;
    sq += sq_b * (double)b_repeat;
    stat_block_reduce(sum, sq, lds);
    if (threadIdx.x == 0) {
        const double n = (double)n_a + (double)n_b * (double)b_repeat;
        const double mean = n > 0.0 ? sum / n : 0.0;
        double var = n > 1.0 ? (sq - mean * mean * n) / (n - 1.0) : __builtin_nan("");     // torch.std of one element: nan
        if (var < 0.0) var = 0.0;
        out[0] = (float)__builtin_sqrt(sq);
        out[1] = (float)mean;
        out[2] = (float)__builtin_sqrt(var);
    }
}
}  // namespace

extern "C" int ultra_statistics_blocks(int64_t n_a) {
    long long blocks = (n_a / 4 + 4LL * kStatThreads - 1) / (4LL * kStatThreads);
    if (blocks > 1024) blocks = 1024;
    return (int)(blocks < 1 ? 1 : blocks);
}

extern "C" int ultra_statistics_f32(const float *a, int64_t n_a, const float *b, int64_t n_b, int64_t b_repeat, double *partials,
                                    float *out, void *stream) {
    if (n_a < 0 || n_b < 0 || b_repeat < 0) return ULTRA_ERR_BAD_SHAPE;
    if ((n_a > 0 && a == nullptr) || (n_b > 0 && b == nullptr) || partials == nullptr || out == nullptr) return ULTRA_ERR_NULL_POINTER;
    if (n_a > 0 && (reinterpret_cast<uintptr_t>(a) & 15u)) return ULTRA_ERR_BAD_SHAPE;
    const int blocks = ultra_statistics_blocks(n_a);
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(statistics_partial_kernel, dim3((unsigned)blocks), dim3(kStatThreads), 0, st, a, (long long)n_a, partials);
    hipLaunchKernelGGL(statistics_final_kernel, dim3(1), dim3(kStatThreads), 0, st, partials, blocks, (long long)n_a, b,
                       (long long)n_b, (long long)b_repeat, out);
    HIP_TRY(hipGetLastError());
    return ULTRA_OK;
}

// ---------------------------------------------------------------------------------------- training loss
// bce_adversarial_kernel: the reference's training criterion for one batch of (positive | K negatives) logits
// (ultra/task.py:169-180) and its gradient in one launch (about forty ATen launches of a few microseconds otherwise):
//     l_j   = (1 - t_j) x_j - log_sigmoid(x_j)                 t_0 = 1, t_j = 0     (binary_cross_entropy_with_logits)
//     w_0   = 1,  w_j = softmax_j(x_{1..K} / T)  (no gradient through w, task.py:175-177)   or 1 / K when T <= 0
//     loss  = sum_j w_j l_j / sum_j w_j                         per row
//     d loss / d x_j = w_j (sigmoid(x_j) - t_j) / sum_j w_j
// One workgroup per row; reductions as fixed trees in LDS (deterministic).
namespace {
constexpr int kBceThreads = 256;

__device__ inline float bce_block_reduce(float v, float *lds, bool take_max) {
    lds[threadIdx.x] = v;
    __syncthreads();
    for (int step = kBceThreads / 2; step > 0; step >>= 1) {
        if ((int)threadIdx.x < step) {
            const float a = lds[threadIdx.x], b = lds[threadIdx.x + step];
            lds[threadIdx.x] = take_max ? (a > b ? a : b) : a + b;
        }
        __syncthreads();
    }
    const float out = lds[0];
    __syncthreads();
    return out;
}

__global__ __launch_bounds__(kBceThreads) void bce_adversarial_kernel(const float *pred, long long cols, float temperature,
                                                                      float *loss_rows, float *dpred) {
    __shared__ float lds[kBceThreads];
    const float *x = pred + (long long)blockIdx.x * cols;
    float *dx = dpred + (long long)blockIdx.x * cols;
    const long long K = cols - 1;
    const bool adversarial = temperature > 0.0f && K > 0;
    float m = -INFINITY;
    if (adversarial)
        for (long long j = 1 + threadIdx.x; j < cols; j += kBceThreads) { const float z = x[j] / temperature; m = z > m ? z : m; }
    m = adversarial ? bce_block_reduce(m, lds, true) : 0.0f;
    float se = 0.0f;
    if (adversarial)
        for (long long j = 1 + threadIdx.x; j < cols; j += kBceThreads) se += expf(x[j] / temperature - m);
    se = adversarial ? bce_block_reduce(se, lds, false) : 1.0f;
    float sw = 0.0f, swl = 0.0f;
    for (long long j = threadIdx.x; j < cols; j += kBceThreads) {
        const float v = x[j];
        const float w = j == 0 ? 1.0f : (adversarial ? expf(v / temperature - m) / se : 1.0f / (float)K);
        const float t = j == 0 ? 1.0f : 0.0f;
        const float log_sig = (v < 0.0f ? v : 0.0f) - log1pf(expf(-fabsf(v)));
        const float l = (1.0f - t) * v - log_sig;
        sw += w;
        swl += w * l;
    }
    sw = bce_block_reduce(sw, lds, false);
    swl = bce_block_reduce(swl, lds, false);
    if (threadIdx.x == 0) loss_rows[blockIdx.x] = swl / sw;
    for (long long j = threadIdx.x; j < cols; j += kBceThreads) {
        const float v = x[j];
        const float w = j == 0 ? 1.0f : (adversarial ? expf(v / temperature - m) / se : 1.0f / (float)K);
        const float t = j == 0 ? 1.0f : 0.0f;
        const float sig = 1.0f / (1.0f + expf(-v));
        dx[j] = w * (sig - t) / sw;
    }
}
}  // namespace

extern "C" int ultra_bce_adversarial_f32(const float *pred, int64_t rows, int64_t cols, float temperature, float *loss_rows,
                                         float *dpred, void *stream) {
    if (rows < 0 || cols < 1 || rows > 0x7fffffffLL) return ULTRA_ERR_BAD_SHAPE;
    if (rows == 0) return ULTRA_OK;
    if (pred == nullptr || loss_rows == nullptr || dpred == nullptr) return ULTRA_ERR_NULL_POINTER;
    hipLaunchKernelGGL(bce_adversarial_kernel, dim3((unsigned)rows), dim3(kBceThreads), 0, static_cast<hipStream_t>(stream), pred,
                       (long long)cols, temperature, loss_rows, dpred);
    HIP_TRY(hipGetLastError());
    return ULTRA_OK;
}

// ---------------------------------------------------------------------------------------- training, last layer
// candidate_tiles_kernel: the distinct 32-row tiles of an (N, B, 64) activation that hold the rows (t_index[b, j], b) -- where
// the gradient of `hidden[t_index, arange(B)]` (ultra/model.py:177-183) is non-zero -- ascending, -1 padded, in ONE launch
// (as ATen ops: two sorts and a dozen elementwise kernels, ~80 us inside a captured step).  One workgroup: a bitmap of the
// tiles in LDS, a block-wide exclusive scan of the words' popcounts, ordered emission.
namespace {
constexpr int kTilesThreads = 1024;
constexpr int kTilesMaxWords = 32768;                  // 1 Mi tiles = 32 Mi rows

__global__ __launch_bounds__(kTilesThreads) void candidate_tiles_kernel(const long long *t_index, int n_batch, int per_row,
                                                                        int n_query, int n_words, int32_t *out) {
    extern __shared__ uint32_t tiles_lds[];            // [n_words] bitmap, then [kTilesThreads] scan
    uint32_t *bitmap = tiles_lds;
    uint32_t *scan = tiles_lds + n_words;
    const int tid = threadIdx.x;
    for (int i = tid; i < n_words; i += kTilesThreads) bitmap[i] = 0u;
    __syncthreads();
    const int total_in = n_batch * per_row;
    for (int i = tid; i < total_in; i += kTilesThreads) {
        const int b = i / per_row;
        const long long tile = (t_index[i] * n_query + b) >> 5;
        atomicOr(&bitmap[tile >> 5], 1u << (tile & 31));
    }
    __syncthreads();
    const int wpt = (n_words + kTilesThreads - 1) / kTilesThreads;
    const int w0 = tid * wpt, w1 = min(w0 + wpt, n_words);
    uint32_t mine = 0;
    for (int w = w0; w < w1; ++w) mine += __builtin_popcount(bitmap[w]);
    scan[tid] = mine;
    __syncthreads();
    for (int step = 1; step < kTilesThreads; step <<= 1) {       // inclusive Hillis-Steele scan
        const uint32_t add = tid >= step ? scan[tid - step] : 0u;
        __syncthreads();
        scan[tid] += add;
        __syncthreads();
    }
    uint32_t pos = scan[tid] - mine;
    const uint32_t total = scan[kTilesThreads - 1];
    for (int w = w0; w < w1; ++w) {
        uint32_t bits = bitmap[w];
        while (bits) {
            const int bit = __builtin_ctz(bits);
            bits &= bits - 1;
            out[pos++] = w * 32 + bit;
        }
    }
    for (int i = (int)total + tid; i < total_in; i += kTilesThreads) out[i] = -1;
}
}  // namespace

extern "C" int ultra_candidate_tiles(const int64_t *t_index, int64_t n_batch, int64_t per_row, int64_t n_query, int64_t n_rows,
                                     int32_t *out, void *stream) {
    if (n_batch < 0 || per_row < 0 || n_query <= 0 || n_rows < 0 || n_batch * per_row > 0x7fffffffLL) return ULTRA_ERR_BAD_SHAPE;
    if (n_batch * per_row == 0) return ULTRA_OK;
    if (t_index == nullptr || out == nullptr) return ULTRA_ERR_NULL_POINTER;
    const long long n_tiles = (n_rows + 31) / 32;
    const long long n_words = (n_tiles + 31) / 32;
    if (n_words > kTilesMaxWords) return ULTRA_ERR_BAD_SHAPE;          // the caller takes its ATen path
    const size_t lds = (size_t)(n_words + kTilesThreads) * sizeof(uint32_t);
    int rc = ensure_lds_attribute(reinterpret_cast<const void *>(candidate_tiles_kernel), lds);
    if (rc) return rc;
    hipLaunchKernelGGL(candidate_tiles_kernel, dim3(1), dim3(kTilesThreads), lds, static_cast<hipStream_t>(stream),
                       reinterpret_cast<const long long *>(t_index), (int)n_batch, (int)per_row, (int)n_query, (int)n_words, out);
    HIP_TRY(hipGetLastError());
    return ULTRA_OK;
}

// node_bitmap_kernel: per query b the set of nodes t_index[b, :] as a bitmap over the nodes -- which rows of the last layer's
// output receive a gradient (ultra/model.py:177-183: the score head reads hidden[t_index[b, j], b]).  One workgroup per query,
// bitmap in LDS, written out whole (every word, every launch).
namespace {
constexpr int kNodeBitmapMaxWords = 16384;             // 512 Ki nodes

__global__ __launch_bounds__(256) void node_bitmap_kernel(const long long *t_index, int per_row, int n_node, int n_words,
                                                          uint32_t *out) {
    extern __shared__ uint32_t nb_lds[];
    const int b = blockIdx.x;
    for (int i = threadIdx.x; i < n_words; i += 256) nb_lds[i] = 0u;
    __syncthreads();
    for (int j = threadIdx.x; j < per_row; j += 256) {
        const long long t = t_index[(long long)b * per_row + j];
        if (t >= 0 && t < n_node) atomicOr(&nb_lds[t >> 5], 1u << (t & 31));
    }
    __syncthreads();
    for (int i = threadIdx.x; i < n_words; i += 256) out[(long long)b * n_words + i] = nb_lds[i];
}
}  // namespace

extern "C" int ultra_node_bitmap(const int64_t *t_index, int64_t n_batch, int64_t per_row, int64_t n_node, uint32_t *bits,
                                 void *stream) {
    if (n_batch < 0 || per_row < 0 || n_node < 0 || n_batch > 0x7fffffffLL || per_row > 0x7fffffffLL) return ULTRA_ERR_BAD_SHAPE;
    const long long n_words = (n_node + 31) / 32;
    if (n_words > kNodeBitmapMaxWords) return ULTRA_ERR_BAD_SHAPE;       // the caller goes without the mask
    if (n_batch == 0 || n_words == 0) return ULTRA_OK;
    if (t_index == nullptr || bits == nullptr) return ULTRA_ERR_NULL_POINTER;
    const size_t lds = (size_t)n_words * sizeof(uint32_t);
    int rc = ensure_lds_attribute(reinterpret_cast<const void *>(node_bitmap_kernel), lds);
    if (rc) return rc;
    hipLaunchKernelGGL(node_bitmap_kernel, dim3((unsigned)n_batch), dim3(256), lds, static_cast<hipStream_t>(stream),
                       reinterpret_cast<const long long *>(t_index), (int)per_row, (int)n_node, (int)n_words, bits);
    HIP_TRY(hipGetLastError());
    return ULTRA_OK;
}

// gather_boundary_rows_kernel: out[q, :] = rows[node[q], q, :] -- the gradient of the boundary VALUE of query q out of a
// layer's (N, Q, 64) d_update (the sparse boundary epilogue's backward; as ATen ops: a cast, an arange and an index kernel
// per layer).
namespace {
__global__ __launch_bounds__(64) void gather_boundary_rows_kernel(const float *rows, const int32_t *node, int n_query, float *out) {
    const int q = blockIdx.x, lane = threadIdx.x;
    out[(long long)q * 64 + lane] = rows[((long long)node[q] * n_query + q) * 64 + lane];
}
}  // namespace

extern "C" int ultra_gather_boundary_rows_f32(const float *rows, const int32_t *node, int64_t n_query, float *out, void *stream) {
    if (n_query < 0 || n_query > 0x7fffffffLL) return ULTRA_ERR_BAD_SHAPE;
    if (n_query == 0) return ULTRA_OK;
    if (rows == nullptr || node == nullptr || out == nullptr) return ULTRA_ERR_NULL_POINTER;
    hipLaunchKernelGGL(gather_boundary_rows_kernel, dim3((unsigned)n_query), dim3(64), 0, static_cast<hipStream_t>(stream), rows, node,
                       (int)n_query, out);
    HIP_TRY(hipGetLastError());
    return ULTRA_OK;
}

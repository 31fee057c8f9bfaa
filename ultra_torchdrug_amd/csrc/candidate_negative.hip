// candidate_negative.hip -- type-constrained strict negatives: every row draws its corrupted entities from a LIST of admissible
// entities minus the known completions (a translation unit of libultra_rspmm.so; C ABI: ultra_constrained_negative in
// include/ultra_rspmm.h).
//
// ultra_strict_negative finds "the k-th entity outside a sorted list" with one binary search.  Here the admissible entities of
// row q are the ascending, distinct ids of set s = set_of[q] in CSR form, items[ptr[s] .. ptr[s + 1]) (s == -1: every entity),
// minus the completions of (anchor_q, rel_q, ?) -- the sorted 64-bit keys
//       key = (anchor * n_rel + rel) * n_node + entity
// of ultra_strict_negative / ultra_candidate_select_f32 -- and the k-th survivor is only known once the intersection has been
// counted.  One workgroup of 256 threads owns one row:
//   * two threads narrow the keys to the row's range -- two lower bounds, once per workgroup;
//   * the list is walked in chunks of kChunk = 32768 positions: every thread looks its items up in that range, four at a time
//     (free_at4: binary searches of one uniform trip count, so each step is four independent loads), the free flags of a wave
//     become two words of an LDS bitmap through a ballot (4 KB, no atomics), and the per-word popcounts are scanned (a shuffle
//     scan per wave, four waves through LDS; 4 KB);
//   * a sample whose k = min((long long)(rand * (float)n_free), n_free - 1) lies in the chunk's [base, base + count) finds its word
//     by binary search in the scanned counts and the bit inside the word, then reads the entity at that position;
//   * n_free must be known before any k is: a list longer than one chunk is walked twice in the same launch -- the first walk
//     counts, the second redoes the lookups chunk by chunk; a list of at most 32768 positions is looked up once;
//   * rows with s == -1, and rows whose n_free is below min_free (the FALLBACK), take the k-th-missing-number search of
//     strict_negative_kernel (sampler.inc) over all entities: one binary search per sample.
// Every branch around a barrier is taken by the whole workgroup (list, lengths and counts are the same in every thread).  Counts
// are integers and every sample is independent: every schedule, eager or replayed from a hipGraph, gives the same words.  All
// address arithmetic is 64-bit.  Nothing read from device memory addresses anything without a range check: a set id outside
// [-1, n_sets) is the empty list, ptr values are clamped to [0, n_items], an item outside [0, n_node) is skipped, keys are only
// ever addressed through positions inside [0, n_keys), and a rand of 1.0, a negative one or a NaN gives an in-range k.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "host_common.h"
#include "select_keys.h"

namespace {
using namespace ultra_detail;

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr long long kChunk = 32768;                        // list positions per bitmap (128 per thread)
constexpr int kWords = (int)(kChunk / 32);                 // 1024 words of 32 free-bits

struct NegativeParams {
    const int64_t *keys;
    long long n_keys;
    const int64_t *anchor, *rel, *set_of;                  // set_of NULL: every row takes all entities
    long long index_stride;                                // of anchor, rel and set_of
    long long n_rel, n_node;
    const int64_t *ptr;                                    // [n_sets + 1]
    const int32_t *items;                                  // [n_items]
    long long n_sets, n_items;
    const float *rand;                                     // [n_query, n_sample]
    long long n_sample, min_free;
    int64_t *out;                                          // [n_query, n_sample]
    int64_t *n_free;                                       // [n_query] or NULL
};

struct NegativeShared {
    unsigned bits[kWords];                                 // free-bit of every position of the chunk
    unsigned incl[kWords];                                 // inclusive scan of the words' popcounts
    long long range[2];
    unsigned wave_sum[kWaves];
    long long part[kWaves];
};

__device__ __forceinline__ long long clamp_ll(long long v, long long lo, long long hi) { return v < lo ? lo : (v > hi ? hi : v); }

// fp32 product, truncated, as torch computes `(rand * sizes).long()`; clamped where rounding reaches n_free; a negative product
// or a NaN gives 0 (n_free >= 1)
__device__ __forceinline__ long long draw_of(float r, long long n_free) {
    const float x = r * (float)n_free;
    long long k = 0;
    if (x >= 0.0f) k = x < 9.0e18f ? (long long)x : n_free - 1;
    if (k >= n_free) k = n_free - 1;
    return k;
}

// are positions c, c + 256, c + 512, c + 768 of the list (those below c1) free entities?  The four ids are loaded first, then
// four lookups in keys[lo, hi) run side by side: a search for the LAST key <= base + e whose trip count depends on hi - lo
// alone, so every step is four independent loads in every lane.  Every address is inside [lo, hi).
__device__ __forceinline__ void free_at4(const NegativeParams &p, long long begin, long long c, long long c1, int64_t base,
                                         long long lo, long long hi, bool (&is_free)[4]) {
    int64_t v[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const long long cc = c + (long long)kThreads * i;
        const long long e = cc < c1 ? (long long)p.items[begin + cc] : -1;
        is_free[i] = e >= 0 && e < p.n_node;               // anything else is not an entity: skipped
        v[i] = base + e;
    }
    if (lo >= hi) return;
    long long at[4] = {lo, lo, lo, lo};
    for (long long len = hi - lo; len > 1;) {
        const long long half = len >> 1;
#pragma unroll
        for (int i = 0; i < 4; ++i) at[i] += p.keys[at[i] + half] <= v[i] ? half : 0;
        len -= half;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) is_free[i] = is_free[i] && p.keys[at[i]] != v[i];     // not a known completion
}

// The bitmap and the scanned counts of positions [c0, c0 + kChunk) of the list; returns the chunk's number of free entities.
// Ends behind a barrier: bits and incl are complete for every thread.
__device__ __forceinline__ unsigned build_chunk(NegativeShared &sh, const NegativeParams &p, long long begin, long long len,
                                                long long c0, int64_t base, long long lo, long long hi) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long c1 = c0 + kChunk < len ? c0 + kChunk : len;
    const int n_tiles = (int)((c1 - c0 + kThreads - 1) / kThreads);               // <= 128; each writes 8 words
    for (int tile = 0; tile < n_tiles; tile += 4) {        // four tiles' lookups in flight together
        bool is_free[4];
        free_at4(p, begin, c0 + (long long)tile * kThreads + tid, c1, base, lo, hi, is_free);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if (tile + i < n_tiles) {                      // (the same in every thread)
                const unsigned long long mask = __ballot(is_free[i] ? 1 : 0);
                if (lane == 0) {
                    sh.bits[(tile + i) * 8 + wave * 2] = (unsigned)mask;
                    sh.bits[(tile + i) * 8 + wave * 2 + 1] = (unsigned)(mask >> 32);
                }
            }
        }
    }
    __syncthreads();
    const int n_words = n_tiles * 8;
    unsigned v[4], local = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int w = 4 * tid + i;
        v[i] = w < n_words ? (unsigned)__popc(sh.bits[w]) : 0u;
        local += v[i];
    }
    unsigned incl = local;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const unsigned t = __shfl_up(incl, off, 64);
        if (lane >= off) incl += t;
    }
    if (lane == 63) sh.wave_sum[wave] = incl;
    __syncthreads();
    unsigned running = incl - local, total = 0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) {
        if (w < wave) running += sh.wave_sum[w];
        total += sh.wave_sum[w];
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        running += v[i];
        sh.incl[4 * tid + i] = running;                    // (words behind n_words repeat the total)
    }
    __syncthreads();
    return total;
}

// the position inside the chunk of its r-th free entity, r < the chunk's count
__device__ __forceinline__ int select_in_chunk(const NegativeShared &sh, unsigned r) {
    int lo = 0, hi = kWords - 1;                           // smallest w with incl[w] > r; incl[kWords - 1] = count > r
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (sh.incl[mid] > r) hi = mid; else lo = mid + 1;
    }
    unsigned within = r - (lo > 0 ? sh.incl[lo - 1] : 0u);
    unsigned word = sh.bits[lo];
    for (; within > 0 && word != 0u; --within) word &= word - 1u;                  // drop the lower set bits
    const int bit = word != 0u ? __ffs((int)word) - 1 : 0;
    return lo * 32 + bit;
}

__global__ __launch_bounds__(kThreads) void constrained_negative_kernel(const NegativeParams p) {
    __shared__ NegativeShared sh;
    const int tid = threadIdx.x;
    const long long q = blockIdx.x;
    const float *rand = p.rand + q * p.n_sample;
    int64_t *out = p.out + q * p.n_sample;

    // the list of the row: `all` (every entity) or items[begin, begin + len)
    const long long s = p.set_of != nullptr ? p.set_of[q * p.index_stride] : -1;
    const bool all = s == -1;
    long long begin = 0, len = 0;
    if (!all && s >= 0 && s < p.n_sets) {
        begin = clamp_ll(p.ptr[s], 0, p.n_items);
        len = clamp_ll(p.ptr[s + 1], begin, p.n_items) - begin;
    }
    const int64_t base = (p.anchor[q * p.index_stride] * p.n_rel + p.rel[q * p.index_stride]) * p.n_node;
    if (tid < 2) sh.range[tid] = p.n_keys > 0 ? lower_bound_i64(p.keys, p.n_keys, base + (tid ? p.n_node : 0)) : 0;
    __syncthreads();
    const long long lo = sh.range[0], hi = sh.range[1] > sh.range[0] ? sh.range[1] : sh.range[0];
    const long long n_excl = hi - lo;
    const long long n_free_all = p.n_node - n_excl;        // of the unconstrained strict draw

    long long n_free = 0;                                  // the set-side count
    const bool one_chunk = !all && len <= kChunk;
    if (all) {
        n_free = n_free_all > 0 ? n_free_all : 0;
    } else if (one_chunk) {
        n_free = len > 0 ? (long long)build_chunk(sh, p, begin, len, 0, base, lo, hi) : 0;
    } else {                                               // the first walk: count
        long long count = 0;
        for (long long c = tid; c < len; c += 4 * kThreads) {
            bool is_free[4];
            free_at4(p, begin, c, len, base, lo, hi, is_free);
            count += (is_free[0] ? 1 : 0) + (is_free[1] ? 1 : 0) + (is_free[2] ? 1 : 0) + (is_free[3] ? 1 : 0);
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) count += __shfl_down(count, off, 64);
        if ((tid & 63) == 0) sh.part[tid >> 6] = count;
        __syncthreads();
        n_free = sh.part[0] + sh.part[1] + sh.part[2] + sh.part[3];
    }
    if (tid == 0 && p.n_free != nullptr) p.n_free[q] = n_free;

    if (all || n_free < p.min_free) {
        // the unconstrained strict draw (strict_negative_kernel): the k-th missing number of the sorted completion list L,
        // smallest j with L[j] - j > k  ->  entity = k + j
        for (long long j = tid; j < p.n_sample; j += kThreads) {
            long long e = 0;                               // every entity is a known completion: 0
            if (n_free_all > 0) {
                const long long k = draw_of(rand[j], n_free_all);
                long long a = 0, b = n_excl;
                while (a < b) {
                    const long long mid = (a + b) >> 1;
                    if ((p.keys[lo + mid] - base) - mid > k) b = mid; else a = mid + 1;
                }
                e = k + a;
                if (e >= p.n_node) e = p.n_node - 1;       // (keys that are not distinct: a wrong answer, not a wild id)
            }
            out[j] = e;
        }
        return;
    }

    if (one_chunk) {
        for (long long j = tid; j < p.n_sample; j += kThreads) {
            const long long k = draw_of(rand[j], n_free);
            out[j] = (long long)p.items[begin + select_in_chunk(sh, (unsigned)k)];
        }
        return;
    }
    long long first = 0;                                   // free entities before the chunk
    for (long long c0 = 0; c0 < len; c0 += kChunk) {       // the second walk
        const long long count = (long long)build_chunk(sh, p, begin, len, c0, base, lo, hi);
        if (count > 0) {
            for (long long j = tid; j < p.n_sample; j += kThreads) {
                const long long k = draw_of(rand[j], n_free);
                if (k >= first && k < first + count)
                    out[j] = (long long)p.items[begin + c0 + select_in_chunk(sh, (unsigned)(k - first))];
            }
        }
        first += count;
        __syncthreads();                                   // (the next chunk overwrites the bitmap)
    }
}

}  // namespace

extern "C" int ultra_constrained_negative(const int64_t *keys, int64_t n_keys, const int64_t *anchor, const int64_t *rel,
                                          const int64_t *set_of, int64_t index_stride, int64_t n_query, int64_t n_rel,
                                          int64_t n_node, const int64_t *ptr, const int32_t *items, int64_t n_sets,
                                          int64_t n_items, const float *rand, int64_t n_sample, int64_t min_free, int64_t *out,
                                          int64_t *n_free, void *stream) {
    if (n_query < 0 || n_query > 0x7fffffffLL || n_node < 1 || n_node > 0x7fffffffLL || n_rel <= 0 || n_keys < 0 || n_sets < 0 ||
        n_items < 0 || index_stride < 0 || n_sample < 1 || min_free < 1)
        return ULTRA_ERR_BAD_SHAPE;
    // the largest key, n_node * n_rel * n_node - 1, must fit 63 bits
    if ((unsigned __int128)n_node * (unsigned __int128)n_rel * (unsigned __int128)n_node > (unsigned __int128)INT64_MAX)
        return ULTRA_ERR_BAD_SHAPE;
    if ((ptr == nullptr && items != nullptr) || (ptr != nullptr && items == nullptr && n_items > 0)) return ULTRA_ERR_NULL_POINTER;
    if (n_query == 0) return ULTRA_OK;
    if (anchor == nullptr || rel == nullptr || rand == nullptr || out == nullptr) return ULTRA_ERR_NULL_POINTER;
    if (n_keys > 0 && keys == nullptr) return ULTRA_ERR_NULL_POINTER;

    NegativeParams p;
    p.keys = keys;
    p.n_keys = n_keys;
    p.anchor = anchor;
    p.rel = rel;
    p.set_of = set_of;
    p.index_stride = index_stride;
    p.n_rel = n_rel;
    p.n_node = n_node;
    p.ptr = ptr;
    p.items = items;
    p.n_sets = ptr != nullptr ? n_sets : 0;
    p.n_items = items != nullptr ? n_items : 0;
    p.rand = rand;
    p.n_sample = n_sample;
    p.min_free = min_free;
    p.out = out;
    p.n_free = n_free;
    hipLaunchKernelGGL(constrained_negative_kernel, dim3((unsigned)n_query), dim3(kThreads), 0, static_cast<hipStream_t>(stream), p);
    HIP_TRY(hipGetLastError());
    return ULTRA_OK;
}

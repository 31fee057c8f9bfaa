// candidate_select.hip -- candidate sets: rank, counts and the K best entities of a query among a LIST of admissible entities
// (a translation unit of libultra_rspmm.so; C ABI: ultra_candidate_select_f32 in include/ultra_rspmm.h).
//
// ultra_topk_keys / ultra_filtered_rank_keys walk every entity [0, n_node) of a score row.  Here query q walks the ascending,
// distinct entity ids of set s = set_of[q] in CSR form, items[ptr[s] .. ptr[s + 1]) (s == -1: every entity), gathers their
// scores from the row and leaves out the known completions of (anchor_q, rel_q, ?) -- the same sorted 64-bit keys
//       key = (anchor * n_rel + rel) * n_node + entity
// as ultra_topk_keys.  One workgroup of 256 threads owns one query (lists of at most kCandSlice = 32768 positions) or one slice
// of 32768 positions of it (longer lists: grid (slices, queries), then one workgroup per query that combines the slices):
//   * two threads narrow the keys to the part of the query's range that the slice's first and last entity span -- two lower
//     bounds, once per workgroup;
//   * the positions are walked in tiles of 1024, four per thread, with the NEXT tile's ids and gathered scores in flight across
//     the barriers (the ids are loaded first, the four gathers that depend on them follow);
//   * a candidate is looked up in that range (binary search) only when its answer is needed: it beats the LDS threshold of the
//     selection (select_keys.h), n_free is asked for, or it takes part in the rank (pos <= score);
//   * the counts are integers (a shuffle tree per wave, four partial sums; slice by slice through the workspace), the sort keys
//     are distinct within a query and the sort is a total order: every schedule gives the same result.
// The sort key carries the ENTITY in its low half (ids < 2^31), so equal scores go by ascending entity -- the order of
// ultra_topk_keys -- wherever the entity stands in its list.  All address arithmetic is 64-bit.  Nothing read from device
// memory addresses anything without a range check: a set id outside [-1, n_sets) is the empty list, ptr values are clamped to
// [0, n_items], an item outside [0, n_node) is skipped, a target outside [0, n_node) is no target.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "host_common.h"
#include "select_keys.h"

namespace {
using namespace ultra_detail;

constexpr int kThreads = 256;
constexpr long long kCandSlice = 32768;                    // list positions per workgroup (128 per thread)
enum { kCandRow = 0, kCandSlices = 1, kCandCombine = 2 };

struct CandSelectParams {
    const float *pred;
    long long row_stride, n_node;
    const int64_t *ptr;                                    // [n_sets + 1]
    const int32_t *items;                                  // [n_items]
    long long n_sets, n_items;
    const int64_t *set_of;                                 // NULL: every query takes all entities
    const int64_t *keys;                                   // NULL: nothing is filtered
    long long n_keys;
    const int64_t *anchor, *rel;
    long long index_stride;                                // of set_of, anchor and rel
    long long n_rel;
    const int64_t *target;                                 // NULL: no rank, no member
    long long target_stride;
    long long max_len;
    int k;                                                 // 0: no top outputs
    int64_t *top_index;
    float *top_value;
    int64_t *rank, *n_free;
    uint8_t *member;
    unsigned long long *ws_keys;                           // [n_query, n_slices, k]
    long long *ws_counts;                                  // [n_query, n_slices, 2]: free, rank
    long long n_slices;
};

__device__ __forceinline__ long long clamp_ll(long long v, long long lo, long long hi) { return v < lo ? lo : (v > hi ? hi : v); }

// the list of query q: `all` (positions are entities) or items[begin, begin + len)
__device__ __forceinline__ void list_of(const CandSelectParams &p, long long q, bool &all, long long &begin, long long &len) {
    const long long s = p.set_of != nullptr ? p.set_of[q * p.index_stride] : -1;
    all = s == -1;
    begin = 0;
    len = 0;
    if (all) {
        len = p.n_node;
    } else if (s >= 0 && s < p.n_sets) {
        begin = clamp_ll(p.ptr[s], 0, p.n_items);
        len = clamp_ll(p.ptr[s + 1], begin, p.n_items) - begin;
    }
    if (len > p.max_len) len = p.max_len;
}

__device__ __forceinline__ long long lower_bound_i32(const int32_t *items, long long n, long long v) {
    long long lo = 0, hi = n;
    while (lo < hi) {
        const long long mid = (lo + hi) >> 1;
        if (items[mid] < v) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// MODE kCandRow:     grid (queries): the whole list, every output written.
// MODE kCandSlices:  grid (slices, queries): positions [slice * kCandSlice, ...), the slice's k keys and two counts -> workspace.
// MODE kCandCombine: grid (queries): the best k of the slices' keys, the sums of their counts, every output written.
template <int MODE>
__global__ __launch_bounds__(kThreads) void candidate_select_kernel(const CandSelectParams p) {
    __shared__ TopkShared sh;
    __shared__ long long part[2][kThreads / 64];
    const int tid = threadIdx.x;
    const long long q = MODE == kCandSlices ? blockIdx.y : blockIdx.x;
    const float *row = p.pred + q * p.row_stride;
    const int K = p.k;
    const bool want_top = K > 0;

    bool all;
    long long begin, len;
    list_of(p, q, all, begin, len);
    long long c0 = 0, c1 = len;
    if constexpr (MODE == kCandSlices) {
        c0 = (long long)blockIdx.x * kCandSlice;
        c1 = c0 + kCandSlice < len ? c0 + kCandSlice : len;
        if (c0 > c1) c0 = c1;                              // a slice behind the end of this query's list
    }
    if constexpr (MODE == kCandCombine) c1 = want_top ? p.n_slices * K : 0;
    const unsigned long long *src = p.ws_keys + q * p.n_slices * K;                // (kCandCombine reads it)

    long long target = -1;
    if (p.target != nullptr) target = p.target[q * p.target_stride];
    if (target < 0 || target >= p.n_node) target = -1;
    const bool ranked = MODE != kCandCombine && target >= 0 && p.rank != nullptr;
    const float pos = ranked ? row[target] : 0.0f;
    const bool want_free = MODE != kCandCombine && (p.n_free != nullptr);

    const bool filtered = MODE != kCandCombine && p.keys != nullptr;
    int64_t base = 0;
    if (tid < kTopkMax) sh.arr[tid] = kTopkEmpty;
    if (tid == 0) {
        sh.thr = kTopkEmpty;
        sh.count = 0;
    }
    if (filtered) {
        base = (p.anchor[q * p.index_stride] * p.n_rel + p.rel[q * p.index_stride]) * p.n_node;
        if (tid < 2) {                                     // the part of the query's range between the slice's end entities
            long long at = 0;
            if (c0 < c1) {
                const long long edge = tid ? c1 - 1 : c0;
                const long long e = all ? edge : (long long)p.items[begin + edge];
                at = lower_bound_i64(p.keys, p.n_keys, base + e + (tid ? 1 : 0));
            }
            sh.range[tid] = at;
        }
    }
    __syncthreads();
    const long long lo = filtered ? sh.range[0] : 0, hi = filtered ? sh.range[1] : 0;

    // a tile: kCandRow / kCandSlices: entity (-1: none) and its score;  kCandCombine: a key of the workspace in `key`
    int cur_e[4], nxt_e[4] = {-1, -1, -1, -1};
    float cur_v[4], nxt_v[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    unsigned long long cur_key[4], nxt_key[4] = {0ull, 0ull, 0ull, 0ull};
    auto load_tile = [&](int (&e)[4], float (&v)[4], unsigned long long (&key)[4], long long c) {
        if constexpr (MODE == kCandCombine) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const long long cc = c + tid + kThreads * i;
                key[i] = cc < c1 ? src[cc] : kTopkEmpty;
            }
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i) {                  // the ids first ...
                const long long cc = c + tid + kThreads * i;
                long long id = -1;
                if (cc < c1) id = all ? cc : (long long)p.items[begin + cc];
                e[i] = (id >= 0 && id < p.n_node) ? (int)id : -1;
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) v[i] = e[i] >= 0 ? row[e[i]] : 0.0f;      // ... then the gathers that depend on them
        }
    };

    long long free_count = 0, rank_count = 0;
    load_tile(cur_e, cur_v, cur_key, c0);
    for (long long c = c0; c < c1; c += kTopkTile) {
        if (c + kTopkTile < c1) load_tile(nxt_e, nxt_v, nxt_key, c + kTopkTile);
        const unsigned long long thr = sh.thr;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            unsigned long long key = kTopkEmpty;
            bool pass = false;
            if constexpr (MODE == kCandCombine) {
                key = cur_key[i];
                pass = key > thr;
            } else {
                const int e = cur_e[i];
                const float v = cur_v[i];
                const bool live = e >= 0;
                if (live && want_top) key = topk_key(v, e);
                pass = key > thr;                          // (kTopkEmpty beats nothing)
                const bool in_rank = live && ranked && pos <= v;
                const bool counted = live && (want_free || in_rank);
                bool known = false;
                if ((pass || counted) && lo < hi) {
                    const long long at = lo + lower_bound_i64(p.keys + lo, hi - lo, base + e);
                    known = at < hi && p.keys[at] == base + e;                     // a known completion
                }
                if (counted && !known) {
                    ++free_count;                          // (exact when want_free: then every live candidate is counted)
                    if (in_rank) ++rank_count;
                }
                pass = pass && !known;
            }
            if (want_top) topk_push(sh, key, pass);
        }
        if (want_top) {
            __syncthreads();
            const int cnt = sh.count;
            __syncthreads();                               // (nobody appends to the next tile before everybody has read cnt)
            if (cnt > kTopkLds - kTopkMax - kTopkTile) topk_flush(sh, K);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            cur_e[i] = nxt_e[i];
            cur_v[i] = nxt_v[i];
            cur_key[i] = nxt_key[i];
        }
    }
    if (want_top) {
        __syncthreads();
        topk_flush(sh, K);
        if (tid < K) {
            const unsigned long long key = sh.arr[tid];
            if constexpr (MODE == kCandSlices) {
                p.ws_keys[(q * p.n_slices + blockIdx.x) * K + tid] = key;
            } else {
                const long long e = key == kTopkEmpty ? -1 : (long long)(~(unsigned)key);
                if (p.top_index != nullptr) p.top_index[q * K + tid] = e;
                if (p.top_value != nullptr) p.top_value[q * K + tid] = e < 0 ? -INFINITY : row[e];   // the score's own bits
            }
        }
    }

    if constexpr (MODE == kCandCombine) {
        const long long *counts = p.ws_counts + q * p.n_slices * 2;
        for (long long s = tid; s < p.n_slices; s += kThreads) {
            free_count += counts[2 * s];
            rank_count += counts[2 * s + 1];
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        free_count += __shfl_down(free_count, off, 64);
        rank_count += __shfl_down(rank_count, off, 64);
    }
    if ((tid & 63) == 0) {
        part[0][tid >> 6] = free_count;
        part[1][tid >> 6] = rank_count;
    }
    __syncthreads();
    if (tid == 0) {
        const long long n_free = part[0][0] + part[0][1] + part[0][2] + part[0][3];
        const long long n_rank = part[1][0] + part[1][1] + part[1][2] + part[1][3];
        if constexpr (MODE == kCandSlices) {
            long long *counts = p.ws_counts + (q * p.n_slices + blockIdx.x) * 2;
            counts[0] = n_free;
            counts[1] = n_rank;
        } else {
            if (p.n_free != nullptr) p.n_free[q] = n_free;
            if (p.rank != nullptr) p.rank[q] = target < 0 ? 0 : 1 + n_rank;
            if (p.member != nullptr) {
                bool in_list = false;
                if (target >= 0) {
                    if (all) {
                        in_list = target < len;
                    } else {
                        const long long at = lower_bound_i32(p.items + begin, len, target);
                        in_list = at < len && p.items[begin + at] == target;
                    }
                }
                p.member[q] = in_list ? 1 : 0;
            }
        }
    }
}

long long slices_of(int64_t max_len) { return max_len > kCandSlice ? (max_len + kCandSlice - 1) / kCandSlice : 0; }

size_t workspace_of(int64_t n_query, int64_t max_len, int64_t k) {
    const long long n_slices = slices_of(max_len);
    if (n_query <= 0 || n_slices == 0) return 0;           // short lists: one launch, no workspace
    const size_t per_slice = (size_t)(k >= 1 && k <= kTopkMax ? k : 0) * sizeof(unsigned long long) + 2 * sizeof(long long);
    return (size_t)n_query * (size_t)n_slices * per_slice;
}

}  // namespace

extern "C" size_t ultra_candidate_select_workspace(int64_t n_query, int64_t max_len, int64_t k) {
    return workspace_of(n_query, max_len, k);
}

extern "C" int ultra_candidate_select_f32(const float *pred, int64_t n_query, int64_t n_node, int64_t row_stride,
                                          const int64_t *ptr, const int32_t *items, int64_t n_sets, int64_t n_items,
                                          const int64_t *set_of, int64_t max_len, const int64_t *keys, int64_t n_keys,
                                          const int64_t *anchor, const int64_t *rel, int64_t index_stride, int64_t n_rel,
                                          const int64_t *target, int64_t target_stride, int64_t k, int64_t *top_index,
                                          float *top_value, int64_t *rank, int64_t *n_free, uint8_t *member, void *workspace,
                                          size_t workspace_bytes, void *stream) {
    const bool want_top = top_index != nullptr || top_value != nullptr;
    if (n_query < 0 || n_query > 0x7fffffffLL || n_node < 1 || n_node > 0x7fffffffLL || row_stride < n_node || n_sets < 0 ||
        n_items < 0 || max_len < 0 || max_len > 0x7fffffffLL || n_keys < 0 || index_stride < 0 || target_stride < 0)
        return ULTRA_ERR_BAD_SHAPE;
    if (want_top && (k < 1 || k > kTopkMax)) return ULTRA_ERR_BAD_SHAPE;
    if (keys != nullptr) {
        if (n_rel <= 0) return ULTRA_ERR_BAD_SHAPE;
        // the largest key, n_node * n_rel * n_node - 1, must fit 63 bits
        if ((unsigned __int128)n_node * (unsigned __int128)n_rel * (unsigned __int128)n_node > (unsigned __int128)INT64_MAX)
            return ULTRA_ERR_BAD_SHAPE;
    }
    const long long n_slices = slices_of(max_len);
    if (n_slices > 0 && n_query > 65535) return ULTRA_ERR_BAD_SHAPE;               // grid.y
    if (n_query == 0) return ULTRA_OK;
    if (!want_top && rank == nullptr && n_free == nullptr && member == nullptr) return ULTRA_ERR_NULL_POINTER;
    if (pred == nullptr) return ULTRA_ERR_NULL_POINTER;
    if (keys != nullptr && (anchor == nullptr || rel == nullptr)) return ULTRA_ERR_NULL_POINTER;
    if (set_of != nullptr && n_sets > 0 && (ptr == nullptr || (n_items > 0 && items == nullptr))) return ULTRA_ERR_NULL_POINTER;
    const int k_top = want_top ? (int)k : 0;
    const size_t need = workspace_of(n_query, max_len, k_top);
    if (need > 0 && (workspace == nullptr || workspace_bytes < need)) return ULTRA_ERR_WORKSPACE;

    CandSelectParams p;
    p.pred = pred;
    p.row_stride = row_stride;
    p.n_node = n_node;
    p.ptr = ptr;
    p.items = items;
    p.n_sets = ptr != nullptr ? n_sets : 0;
    p.n_items = items != nullptr ? n_items : 0;
    p.set_of = set_of;
    p.keys = keys;
    p.n_keys = n_keys;
    p.anchor = anchor;
    p.rel = rel;
    p.index_stride = index_stride;
    p.n_rel = n_rel;
    p.target = target;
    p.target_stride = target_stride;
    p.max_len = max_len;
    p.k = k_top;
    p.top_index = top_index;
    p.top_value = top_value;
    p.rank = rank;
    p.n_free = n_free;
    p.member = member;
    p.ws_keys = static_cast<unsigned long long *>(workspace);
    p.ws_counts = reinterpret_cast<long long *>(p.ws_keys + (size_t)n_query * (size_t)n_slices * (size_t)k_top);
    p.n_slices = n_slices;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (n_slices > 0) {
        hipLaunchKernelGGL(candidate_select_kernel<kCandSlices>, dim3((unsigned)n_slices, (unsigned)n_query), dim3(kThreads), 0, s,
                           p);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(candidate_select_kernel<kCandCombine>, dim3((unsigned)n_query), dim3(kThreads), 0, s, p);
    } else {
        hipLaunchKernelGGL(candidate_select_kernel<kCandRow>, dim3((unsigned)n_query), dim3(kThreads), 0, s, p);
    }
    HIP_TRY(hipGetLastError());
    return ULTRA_OK;
}

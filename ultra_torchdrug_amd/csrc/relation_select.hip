// relation_select.hip -- relation prediction: which relations hold between h and t?  The filter lookup, the filtered rank and
// the K best relations of every (h, t) pair over a row of candidate-relation scores (a translation unit of libultra_rspmm.so;
// C ABI: ultra_relation_select_f32 in include/ultra_rspmm.h).
//
// ultra_topk_keys / ultra_filtered_rank_keys fix one key base (anchor, relation) per row and let the OTHER ENTITY vary along it;
// here both entities of a row are fixed and the RELATION varies: candidate j of pair p is the relation id c = cand[j] in
// [0, 2 * n_rel) (c >= n_rel: the inverse of c - n_rel), and it is KNOWN iff
//       c <  n_rel  and  (h * n_rel + c) * n_node + t            is in keys_head   (the triple (h, c, t)),
//       c >= n_rel  and  (h * n_rel + (c - n_rel)) * n_node + t  is in keys_tail   (the triple (t, c - n_rel, h)).
// One workgroup of 256 threads owns one pair and every output word of it:
//   * four threads narrow the two key arrays to h's slice [h * n_rel * n_node, (h + 1) * n_rel * n_node) -- two lower bounds
//     each, once per workgroup;
//   * the target's position j* = the FIRST position that lists it (an LDS atomicMin over the list; the identity list needs none);
//   * every candidate then takes one binary search inside the slice, writes its known byte, counts into n_free and -- when it is
//     not known and `score[j*] <= score[j]` -- into the rank (integer counts, a shuffle tree per wave, four partial sums), and
//     leaves its 64-bit sort key (topk_key of select_keys.h by POSITION j; 0 when known) in LDS;
//   * the keys are sorted descending in LDS (bitonic) and the first k give top_index = cand[j] / top_value = score[j] re-read.
// kRelSelectLds = 4096 candidates (32 KiB of LDS, so five workgroups fit a CU's 160 KiB) take ONE such pass.  Longer lists take
// the slower multi-pass form in the same kernel: LDS [0, 128) keeps the best 128 so far, [128, 4096) takes the next 3968
// candidates, one sort per pass.  Keys are distinct within a pair and the sort is a total order, so every schedule gives the
// same result.  Ids outside their ranges -- a candidate outside [0, 2 * n_rel), h or t outside [0, n_node) -- are never known,
// and no index read from device memory addresses anything without a range check.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "host_common.h"
#include "select_keys.h"

namespace {
using namespace ultra_detail;

constexpr int kThreads = 256;
constexpr int kRelSelectLds = 4096;                        // sort keys in LDS = the longest list of the one-pass form (L)
constexpr int kRelSelectChunk = kRelSelectLds - kTopkMax;  // candidates per pass of the multi-pass form

struct RelSelectParams {
    const float *score;
    long long row_stride, n_cand;
    const int64_t *cand;                                   // NULL: the identity
    const int64_t *keys_head, *keys_tail;
    long long n_keys_head, n_keys_tail;
    const int64_t *h, *t;
    long long index_stride;
    const int64_t *target;                                 // NULL: no rank
    long long target_stride;
    long long n_rel, n_node;
    int k;
    int64_t *top_index;
    float *top_value;
    int64_t *rank, *n_free;
    uint8_t *known;
};

// arr[0, P) descending; P a power of two; called by every thread, with a barrier behind the last write to arr
__device__ void sort_descending(unsigned long long *arr, int P) {
    const int tid = threadIdx.x;
    for (int k = 2; k <= P; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = tid; t < (P >> 1); t += kThreads) {
                const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));
                const int l = i | j;
                const unsigned long long a = arr[i], b = arr[l];
                if ((a < b) == ((i & k) == 0)) {
                    arr[i] = b;
                    arr[l] = a;
                }
            }
            __syncthreads();
        }
    }
}

__global__ __launch_bounds__(kThreads) void relation_select_kernel(const RelSelectParams p) {
    __shared__ unsigned long long arr[kRelSelectLds];
    __shared__ long long range[4];                         // h's slice of keys_head [0], [1] and of keys_tail [2], [3]
    __shared__ long long part[2][kThreads / 64];
    __shared__ int first_at;
    const int tid = threadIdx.x;
    const long long q = blockIdx.x;
    const long long n_cand = p.n_cand;
    const float *row = p.score + q * p.row_stride;
    const bool want_top = p.top_index != nullptr || p.top_value != nullptr;
    const bool filtered = p.keys_head != nullptr || p.keys_tail != nullptr;
    const long long two_rel = 2 * p.n_rel;

    long long h = 0, t = 0;
    bool pair_ok = false;
    if (filtered) {
        h = p.h[q * p.index_stride];
        t = p.t[q * p.index_stride];
        pair_ok = h >= 0 && h < p.n_node && t >= 0 && t < p.n_node;
    }
    const int64_t slice = pair_ok ? h * p.n_rel * p.n_node : 0;
    if (tid < 4) {
        const int64_t *keys = tid < 2 ? p.keys_head : p.keys_tail;
        const long long n_keys = tid < 2 ? p.n_keys_head : p.n_keys_tail;
        range[tid] = (pair_ok && keys != nullptr) ? lower_bound_i64(keys, n_keys, slice + ((tid & 1) ? p.n_rel * p.n_node : 0)) : 0;
    }
    if (tid == 0) first_at = 0x7fffffff;
    __syncthreads();

    // the target's position: the first one that lists it
    long long target = -1;
    if (p.target != nullptr) target = p.target[q * p.target_stride];
    long long at = -1;
    if (target >= 0) {
        if (p.cand == nullptr) {
            at = target < n_cand ? target : -1;
        } else {
            int mine = 0x7fffffff;
            for (long long j = tid; j < n_cand; j += kThreads)
                if (p.cand[j] == target && (int)j < mine) mine = (int)j;         // (n_cand < 2^31; the first hit is the smallest)
            if (mine != 0x7fffffff) atomicMin(&first_at, mine);
            __syncthreads();
            at = first_at == 0x7fffffff ? -1 : (long long)first_at;
        }
    }
    const float pos = at >= 0 ? row[at] : 0.0f;

    const long long lo_h = range[0], hi_h = range[1], lo_t = range[2], hi_t = range[3];
    const bool one_pass = n_cand <= kRelSelectLds;
    const int offset = one_pass ? 0 : kTopkMax;            // where a pass's candidates start in arr
    const long long per_pass = one_pass ? kRelSelectLds : kRelSelectChunk;
    int P = kRelSelectLds;                                 // sorted length: the next power of two, at least kTopkMax
    if (one_pass) {
        P = kTopkMax;
        while (P < n_cand) P <<= 1;
    } else if (want_top && tid < kTopkMax) {
        arr[tid] = kTopkEmpty;                             // the best so far: nothing
    }
    long long free_count = 0, rank_count = 0;
    for (long long j0 = 0; j0 < n_cand || j0 == 0; j0 += per_pass) {
        const long long left = n_cand - j0;
        const int here = (int)(left < per_pass ? left : per_pass);
        for (int i = tid; i < P - offset; i += kThreads) {
            unsigned long long key = kTopkEmpty;
            if (i < here) {
                const long long j = j0 + i;
                const long long c = p.cand != nullptr ? p.cand[j] : j;
                bool is_known = false;
                if (pair_ok && c >= 0 && c < two_rel) {
                    const bool inverse = c >= p.n_rel;
                    const int64_t *keys = inverse ? p.keys_tail : p.keys_head;
                    const long long lo = inverse ? lo_t : lo_h, hi = inverse ? hi_t : hi_h;
                    if (lo < hi) {
                        const int64_t want = (h * p.n_rel + (inverse ? c - p.n_rel : c)) * p.n_node + t;
                        const long long found = lo + lower_bound_i64(keys + lo, hi - lo, want);
                        is_known = found < hi && keys[found] == want;
                    }
                }
                const float v = row[j];
                if (p.known != nullptr) p.known[q * n_cand + j] = is_known ? 1 : 0;
                if (!is_known) {
                    ++free_count;
                    if (at >= 0 && pos <= v) ++rank_count;
                    key = topk_key(v, j);
                }
            }
            if (want_top) arr[offset + i] = key;
        }
        if (want_top) {
            __syncthreads();
            sort_descending(arr, P);                       // (ends in a barrier)
        }
        if (n_cand == 0) break;
    }

    if (want_top && tid < p.k) {
        const unsigned long long key = tid < P ? arr[tid] : kTopkEmpty;
        const long long j = key == kTopkEmpty ? -1 : (long long)(~(unsigned)key);
        if (p.top_index != nullptr) p.top_index[q * p.k + tid] = j < 0 ? -1 : (p.cand != nullptr ? p.cand[j] : j);
        if (p.top_value != nullptr) p.top_value[q * p.k + tid] = j < 0 ? -INFINITY : row[j];      // the score's own bits
    }
    if (p.rank != nullptr || p.n_free != nullptr) {
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
            if (p.n_free != nullptr) p.n_free[q] = part[0][0] + part[0][1] + part[0][2] + part[0][3];
            if (p.rank != nullptr) p.rank[q] = at < 0 ? 0 : 1 + part[1][0] + part[1][1] + part[1][2] + part[1][3];
        }
    }
}

}  // namespace

extern "C" int ultra_relation_select_limit(void) { return kRelSelectLds; }

extern "C" int ultra_relation_select_f32(const float *score, int64_t n_pair, int64_t n_cand, int64_t row_stride,
                                         const int64_t *cand, const int64_t *keys_head, int64_t n_keys_head,
                                         const int64_t *keys_tail, int64_t n_keys_tail, const int64_t *h, const int64_t *t,
                                         int64_t index_stride, const int64_t *target, int64_t target_stride, int64_t n_rel,
                                         int64_t n_node, int64_t k, int64_t *top_index, float *top_value, int64_t *rank,
                                         int64_t *n_free, uint8_t *known, void *stream) {
    if (n_pair < 0 || n_pair > 0x7fffffffLL || n_cand < 0 || n_cand > 0x7fffffffLL || row_stride < n_cand || n_keys_head < 0 ||
        n_keys_tail < 0 || index_stride < 0 || target_stride < 0 || n_rel <= 0 || n_node <= 0)
        return ULTRA_ERR_BAD_SHAPE;
    if (k < 1 || k > kTopkMax) return ULTRA_ERR_BAD_SHAPE;
    // the largest key, n_node * n_rel * n_node - 1, must fit 63 bits
    if ((unsigned __int128)n_node * (unsigned __int128)n_rel * (unsigned __int128)n_node > (unsigned __int128)INT64_MAX)
        return ULTRA_ERR_BAD_SHAPE;
    if (n_pair == 0) return ULTRA_OK;
    if (top_index == nullptr && top_value == nullptr && rank == nullptr && n_free == nullptr && known == nullptr)
        return ULTRA_ERR_NULL_POINTER;
    if (n_cand > 0 && score == nullptr) return ULTRA_ERR_NULL_POINTER;
    if ((n_keys_head > 0 && keys_head == nullptr) || (n_keys_tail > 0 && keys_tail == nullptr)) return ULTRA_ERR_NULL_POINTER;
    if ((keys_head != nullptr || keys_tail != nullptr) && (h == nullptr || t == nullptr)) return ULTRA_ERR_NULL_POINTER;
    RelSelectParams p;
    p.score = score;
    p.row_stride = row_stride;
    p.n_cand = n_cand;
    p.cand = cand;
    p.keys_head = keys_head;
    p.keys_tail = keys_tail;
    p.n_keys_head = n_keys_head;
    p.n_keys_tail = n_keys_tail;
    p.h = h;
    p.t = t;
    p.index_stride = index_stride;
    p.target = target;
    p.target_stride = target_stride;
    p.n_rel = n_rel;
    p.n_node = n_node;
    p.k = (int)k;
    p.top_index = top_index;
    p.top_value = top_value;
    p.rank = rank;
    p.n_free = n_free;
    p.known = n_cand > 0 ? known : nullptr;
    hipLaunchKernelGGL(relation_select_kernel, dim3((unsigned)n_pair), dim3(kThreads), 0, static_cast<hipStream_t>(stream), p);
    HIP_TRY(hipGetLastError());
    return ULTRA_OK;
}

// select_keys.h -- what the key-based selections share on the device side (internal): the binary search over a graph's sorted
// completion keys, the 64-bit SORT KEY of a scored candidate and the LDS selection of a workgroup's K best keys.  Used by
// sampler.inc (ultra_topk_keys and the per-step index kernels), relation_select.hip (ultra_relation_select_f32) and
// candidate_select.hip (ultra_candidate_select_f32); every unit compiles its own copy.
#ifndef ULTRA_SELECT_KEYS_H
#define ULTRA_SELECT_KEYS_H

#include <hip/hip_runtime.h>

#include <cstdint>

namespace ultra_detail {

__device__ __forceinline__ long long lower_bound_i64(const int64_t *keys, long long n, int64_t v) {
    long long lo = 0, hi = n;
    while (lo < hi) {
        const long long mid = (lo + hi) >> 1;
        if (keys[mid] < v) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// Candidate at position c with score v as one 64-bit sort key
//       high half: order-preserving map of v (-0.0 folded into +0.0; every NaN in one class BELOW -inf)     low half: ~c
// so that "better" is "larger key" -- equal scores go by ascending position -- and all keys of a row are distinct.  0 is no
// candidate's key (the NaN class is 1): it marks an empty slot.
constexpr int kTopkMax = 128;                 // K <= 128
constexpr unsigned long long kTopkEmpty = 0ull;

__device__ __forceinline__ unsigned long long topk_key(float v, long long c) {
    unsigned u = __float_as_uint(v);
    unsigned m = 1u;                                               // NaN: below -inf (which maps to 0x007fffff)
    if (v == v) {
        if (u == 0x80000000u) u = 0u;                              // -0.0 == +0.0
        m = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    }
    return ((unsigned long long)m << 32) | (unsigned long long)(~(unsigned)c);
}

// The LDS selection of a workgroup of 256 threads (topk_keys_kernel of sampler.inc, candidate_select_kernel): the K best keys so
// far, sorted, in arr[0, 128) and their smallest as the THRESHOLD; survivors of the walk are appended to arr[128, 2048) through an
// LDS counter (one atomic per wave) and, when the next tile of kTopkTile candidates might not fit and at the end, best + appended
// are sorted (bitonic, descending, over the next power of two) and cut to K.  The threshold only changes there, between barriers.
constexpr int kTopkLds = 2048;               // keys in LDS (16 KB): [0, 128) the best so far, [128, 2048) survivors
constexpr int kTopkTile = 1024;               // candidates per step of a workgroup

struct TopkShared {
    unsigned long long arr[kTopkLds];
    unsigned long long thr;
    long long range[2];
    int count;
};

// every thread of the workgroup calls it (the ballot and the shuffle are wave-wide)
__device__ __forceinline__ void topk_push(TopkShared &sh, unsigned long long key, bool pass) {
    const unsigned long long mask = __ballot(pass ? 1 : 0);
    if (mask == 0ull) return;
    const int lane = threadIdx.x & 63;
    const int leader = __ffsll((long long)mask) - 1;
    int start = 0;
    if (lane == leader) start = atomicAdd(&sh.count, __popcll(mask));
    start = __shfl(start, leader, 64);
    if (pass) sh.arr[kTopkMax + start + __popcll(mask & ((1ull << lane) - 1ull))] = key;
}

// best K of (best so far + appended) -> arr[0, K) descending, threshold = arr[K - 1], count = 0.  Called by every thread, after a
// barrier behind the last append.
__device__ void topk_flush(TopkShared &sh, int K) {
    const int tid = threadIdx.x;
    const int cnt = sh.count;
    if (cnt == 0) return;
    const int n = kTopkMax + cnt;
    int P = 256;
    while (P < n) P <<= 1;
    for (int j = K + tid; j < kTopkMax; j += 256) sh.arr[j] = kTopkEmpty;        // leftovers of the last sort
    for (int j = n + tid; j < P; j += 256) sh.arr[j] = kTopkEmpty;
    __syncthreads();
    for (int k = 2; k <= P; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = tid; t < (P >> 1); t += 256) {
                const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));
                const int l = i | j;
                const unsigned long long a = sh.arr[i], b = sh.arr[l];
                if ((a < b) == ((i & k) == 0)) {
                    sh.arr[i] = b;
                    sh.arr[l] = a;
                }
            }
            __syncthreads();
        }
    }
    if (tid == 0) {
        sh.thr = sh.arr[K - 1];
        sh.count = 0;
    }
    __syncthreads();
}

}  // namespace ultra_detail

#endif

// select_keys.h -- what the key-based selections share on the device side (internal): the binary search over a graph's sorted
// completion keys and the 64-bit SORT KEY of a scored candidate.  Used by sampler.inc (ultra_topk_keys and the per-step index
// kernels) and relation_select.hip (ultra_relation_select_f32); everything here is inlined into its caller.
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

}  // namespace ultra_detail

#endif

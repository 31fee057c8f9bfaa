// device_common.h -- what the kernels of libultra_rspmm.so's translation units share on the device side (internal; beside
// host_common.h, which is the host side).  Everything here is inlined into its caller: no unit owns any of it.
#ifndef ULTRA_DEVICE_COMMON_H
#define ULTRA_DEVICE_COMMON_H

#include <hip/hip_runtime.h>

#include <cstdint>

#include "ultra_rspmm.h"

namespace ultra_detail {

template <int SUM>
__device__ __forceinline__ float identity() {
    // min / max start from the largest / lowest FINITE float, as torchdrug's NaryMin / NaryMax do
    // (std::numeric_limits<scalar_t>::max() / lowest()), so an empty row never feeds an infinity to the layers after it
    if constexpr (SUM == ULTRA_SUM_ADD) return 0.0f;
    else if constexpr (SUM == ULTRA_SUM_MIN) return 3.402823466e+38f;
    else return -3.402823466e+38f;
}

template <int SUM>
__device__ __forceinline__ float reduce(float acc, float y) {
    if constexpr (SUM == ULTRA_SUM_ADD) return acc + y;
    else if constexpr (SUM == ULTRA_SUM_MIN) return (y < acc) ? y : acc;
    else return (y > acc) ? y : acc;
}

template <int MUL>
__device__ __forceinline__ float binary(float r, float x) {
    if constexpr (MUL == ULTRA_MUL_MUL) return r * x;
    else return r + x;
}

__device__ __forceinline__ int uniform(int v) { return __builtin_amdgcn_readfirstlane(v); }

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

// The 16-lane groups of quad_kernel, rowgroup_kernel and the first-layer kernels: a lane owns four adjacent columns.
typedef float qf4 __attribute__((ext_vector_type(4)));
typedef uint32_t qu4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) const qf4 *lds_qf4_ptr;
typedef __attribute__((address_space(3))) char *lds_char_ptr;

// (the host pass parses these too and finds its pointers wider than the LDS address)
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wint-to-pointer-cast"
// 16-byte LDS read at an integer byte address (dynamic LDS starts at 0 in these kernels: no static __shared__;
// quad_kernel traps if that ever changes) -- keeps table bases in the instruction's immediate offset.
__device__ __forceinline__ qf4 lds_read4(uint32_t byte_addr) { return *(lds_qf4_ptr)byte_addr; }

template <int RED>
__device__ __forceinline__ qf4 reduce4(qf4 a, qf4 y) {
    if constexpr (RED == ULTRA_SUM_ADD) {
        return a + y;
    } else {
        qf4 r;
        r.x = reduce<RED>(a.x, y.x); r.y = reduce<RED>(a.y, y.y); r.z = reduce<RED>(a.z, y.z); r.w = reduce<RED>(a.w, y.w);
        return r;
    }
}

template <int RED>
__device__ __forceinline__ qf4 identity4() {
    const float v = identity<RED>();
    qf4 r = {v, v, v, v};
    return r;
}

typedef __attribute__((address_space(3))) const uint32_t *lds_u32_ptr;
__device__ __forceinline__ uint32_t lds_read1(uint32_t byte_addr) { return *(lds_u32_ptr)byte_addr; }
#pragma clang diagnostic pop

// v_permlane32_swap: lanes 32..63 of `a` change places with lanes 0..31 of `b`.  (The two results go through scalars:
// __builtin_bit_cast applied to an ELEMENT of the returned vector reads element 0 whichever element is named.)
__device__ __forceinline__ void half_swap(float &a, float &b) {
    const auto sw = __builtin_amdgcn_permlane32_swap(__builtin_bit_cast(uint32_t, a), __builtin_bit_cast(uint32_t, b), false, false);
    const uint32_t first = sw[0], second = sw[1];
    a = __builtin_bit_cast(float, first);
    b = __builtin_bit_cast(float, second);
}

// The activation tile of the exact-f32 matrix-core kernels (the layer epilogue and its backwards, the dense layers): one wave
// = 32 consecutive rows, staged through a wave-private LDS tile whose rows are padded by one access width (conflict-free
// ds_read_b128).
constexpr int kCbRows = 32;
constexpr int kCbStride = 132;                 // 128 floats + 4 pad
constexpr int kCbWaves = 4;                    // waves per workgroup
constexpr int kCbTileFloats = kCbRows * kCbStride;

}  // namespace ultra_detail

#endif

// query_set.hip -- the boundary condition of a relation projection whose source is a fuzzy SET of entities instead of one
// anchor (a translation unit of libultra_rspmm.so; C ABI: ultra_set_boundary_f32 in include/ultra_rspmm.h; DESIGN.md
// section 16).
//
//     keep(q, v)        = m > 0  and  (floor == NULL or m >= floor[q]),      m = member[q * row_stride + v]   (a NaN never)
//     boundary[v][q][:] = m * query[q][:]   where keep(q, v),   +0.0 elsewhere -- whatever query holds
//     count[q]          = #{v : keep(q, v)}
//
// memberships are (n_query, n_node), the boundary is (n_node, n_query, dim): the kernel is the transposing broadcast.  A work
// item is a chunk of up to kChunk = 16 queries x `sub` tiles of kTile = 64 nodes; sub = 16 / n_query when all queries fit one
// chunk (two queries: 512 nodes an item, so that an item still writes 16 slots' worth of rows between its barriers), 1 otherwise.
// The blocks take the items grid-stride, chunk fastest, so that items next to each other write memory next to each other.
//   stage:  a slot is one (tile, query) of the item; wave w takes slots w, w + 4, ...: it reads the tile's 64 memberships of the
//           query (contiguous along v), decides keep, and leaves m (kept) or +0.0 (not kept; a kept m is > 0, so the zero IS
//           the flag) in LDS.  The wave's ballot is the slot's count: it goes to an LDS word per slot, and after the barrier ONE
//           integer atomicAdd per (item, query) that kept anything adds the item's tiles to count[q].  Integer adds: every
//           schedule gives the same counts.
//   write:  for a node the chunk's part of its boundary row is one contiguous run of chunk * dim floats.  Lane j of a span of
//           min(run, 256) lanes owns one 16-byte (or, on the scalar path, 4-byte) piece of that run and keeps its piece of the
//           query vector in registers; 256 / span nodes are written side by side, one after the other down the item's nodes.
//           Every store of a wave is contiguous.  Plain stores: the first layer reads the boundary right after this kernel.
// All index arithmetic is 64-bit (n_node * n_query * dim passes 2^31 on large graphs).  Nodes past n_node in the last item are
// staged as +0.0 and never written.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "host_common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kTile = 64;            // nodes per tile = lanes of a wave
constexpr int kChunk = 16;           // (tile, query) slots per item: queries per chunk x tiles
constexpr int kWaves = kThreads / kTile;
constexpr int kMaxBlocks = 2048;     // grid-stride beyond

// count[q] = 0 as a kernel of this library: a memset NODE of a captured graph is not reliably ordered behind earlier kernel
// nodes (see ultra_rspmm_frontier_f32 in rspmm_kernels.hip)
__global__ __launch_bounds__(kThreads) void set_count_clear_kernel(int32_t *__restrict__ count, long long n_query) {
    const long long q = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (q < n_query) count[q] = 0;
}

template <int VEC>
struct Piece;
template <>
struct Piece<4> {
    using type = float4;
    static __device__ __forceinline__ float4 scale(float m, const float4 &q) {
        return m > 0.0f ? make_float4(m * q.x, m * q.y, m * q.z, m * q.w) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    }
};
template <>
struct Piece<1> {
    using type = float;
    static __device__ __forceinline__ float scale(float m, const float &q) { return m > 0.0f ? m * q : 0.0f; }
};

template <int VEC>
__global__ __launch_bounds__(kThreads) void set_boundary_kernel(const float *__restrict__ member, long long n_query,
                                                                long long n_node, long long row_stride,
                                                                const float *__restrict__ floor, const float *__restrict__ query,
                                                                long long dim, float *__restrict__ boundary,
                                                                int32_t *__restrict__ count, long long n_chunks,
                                                                long long n_items, int sub) {
    using piece_t = typename Piece<VEC>::type;
    __shared__ float kept[kChunk][kTile + 1];       // (+1: the write phase reads a column of it per wave)
    __shared__ int tile_count[kChunk];
    const int t = (int)threadIdx.x;
    const int wave = t / kTile, lane = t % kTile;
    for (long long item = blockIdx.x; item < n_items; item += gridDim.x) {
        const long long q0 = (item % n_chunks) * kChunk;
        const long long v0 = (item / n_chunks) * (kTile * sub);
        const int n_q = (int)(n_query - q0 < kChunk ? n_query - q0 : kChunk);
        const int n_v = (int)(n_node - v0 < kTile * sub ? n_node - v0 : kTile * sub);
        const int n_slot = n_q * sub;                               // <= kChunk: sub > 1 only when n_q * sub <= kChunk
        // ---- stage: one wave per (tile, query), contiguous along v
        for (int slot = wave; slot < n_slot; slot += kWaves) {
            const long long q = q0 + slot % n_q;
            const int vl = slot / n_q * kTile + lane;
            float m = 0.0f;
            if (vl < n_v) m = member[q * row_stride + v0 + vl];
            bool keep = m > 0.0f;                                   // (false for a NaN)
            if (floor != nullptr) keep = keep && m >= floor[q];
            kept[slot][lane] = keep ? m : 0.0f;
            const unsigned long long votes = __ballot(keep);
            if (lane == 0) tile_count[slot] = __popcll(votes);
        }
        __syncthreads();
        if (count != nullptr && t < n_q) {
            int kept_here = 0;
            for (int slot = t; slot < n_slot; slot += n_q) kept_here += tile_count[slot];
            if (kept_here != 0) atomicAdd(&count[q0 + t], kept_here);
        }
        // ---- write: the chunk's run of a node's row is n_q * dim floats = run pieces of VEC floats
        const long long run = (long long)n_q * dim / VEC;
        const int span = (int)(run < kThreads ? run : kThreads);     // lanes side by side on one node's run
        const int side = kThreads / span;                            // nodes written side by side
        const int vg = t / span;
        if (vg < side) {
            const long long row_floats = n_query * dim;
            for (long long j = t % span; j < run; j += span) {
                const long long at = j * VEC;                        // float offset inside the run
                const int ql = (int)(at / dim);
                const piece_t qv = *reinterpret_cast<const piece_t *>(query + q0 * dim + at);
                float *out = boundary + v0 * row_floats + q0 * dim + at;
                for (int vl = vg; vl < n_v; vl += side)
                    *reinterpret_cast<piece_t *>(out + (long long)vl * row_floats) =
                        Piece<VEC>::scale(kept[vl / kTile * n_q + ql][vl % kTile], qv);
            }
        }
        __syncthreads();                                             // the next item restages the tile
    }
}

}  // namespace

extern "C" int ultra_set_boundary_f32(const float *member, int64_t n_query, int64_t n_node, int64_t row_stride,
                                      const float *floor, const float *query, int64_t dim, float *boundary, int32_t *count,
                                      void *stream) {
    if (n_query < 1 || n_node < 1 || dim < 1 || row_stride < n_node) return ULTRA_ERR_BAD_SHAPE;
    if (member == nullptr || query == nullptr || boundary == nullptr) return ULTRA_ERR_BAD_SHAPE;
    // sizes the 64-bit offsets and the item count hold (far beyond any device memory)
    if (n_query > (1ll << 40) / dim || n_node > (1ll << 60) / (n_query * dim) || row_stride > (1ll << 60) / n_query)
        return ULTRA_ERR_BAD_SHAPE;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (count != nullptr) {
        hipLaunchKernelGGL(set_count_clear_kernel, dim3((unsigned)((n_query + kThreads - 1) / kThreads)), dim3(kThreads), 0, s,
                           count, (long long)n_query);
        HIP_TRY(hipGetLastError());
    }
    const long long n_chunks = (n_query + kChunk - 1) / kChunk;
    const int sub = n_chunks == 1 ? kChunk / (int)n_query : 1;        // tiles of 64 nodes per item
    const long long n_items = n_chunks * ((n_node + kTile * sub - 1) / (kTile * sub));
    const unsigned grid = (unsigned)(n_items < kMaxBlocks ? n_items : kMaxBlocks);
    const bool wide = dim % 4 == 0 && ((reinterpret_cast<uintptr_t>(query) | reinterpret_cast<uintptr_t>(boundary)) & 15u) == 0;
    if (wide)
        hipLaunchKernelGGL(set_boundary_kernel<4>, dim3(grid), dim3(kThreads), 0, s, member, (long long)n_query,
                           (long long)n_node, (long long)row_stride, floor, query, (long long)dim, boundary, count, n_chunks,
                           n_items, sub);
    else
        hipLaunchKernelGGL(set_boundary_kernel<1>, dim3(grid), dim3(kThreads), 0, s, member, (long long)n_query,
                           (long long)n_node, (long long)row_stride, floor, query, (long long)dim, boundary, count, n_chunks,
                           n_items, sub);
    HIP_TRY(hipGetLastError());
    return ULTRA_OK;
}

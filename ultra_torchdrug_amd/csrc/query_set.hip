// query_set.hip -- the boundary condition of a relation projection whose source is a fuzzy SET of entities instead of one
// anchor, and its backward (a translation unit of libultra_rspmm.so; C ABI: ultra_set_boundary_f32 and
// ultra_set_boundary_backward_f32 in include/ultra_rspmm.h; DESIGN.md sections 16 and 19).
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
// nodes (see ultra_rspmm_frontier_f32 in epilogue.hip)
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


// ---- backward (ultra_set_boundary_backward_f32) -------------------------------------------------------------------------------
//     d_member[q][v] = keep(q, v) ? sum_d d_boundary[v][q][d] * query[q][d] : +0.0
//     d_query[q][d]  = sum over the kept v of member[q][v] * d_boundary[v][q][d]
// The forward's items (a chunk of queries x `sub` tiles of 64 nodes), read instead of written: a group of L lanes (a power of
// two up to 64, at most kBwdPieces pieces of VEC floats a lane) owns one (node, query) row of d_boundary, the groups of a block lie side by side along
// the chunk's queries and then along nodes, so that a wave's loads cover one contiguous run of a node's chunk.  A row that is
// not kept is never loaded.  The dot of a row is summed over the group in a fixed xor tree and leaves through LDS, so that
// d_member is stored along v.  A thread keeps its pieces of d_query in registers over ALL items of its block (blockIdx.y is the
// chunk: they belong to one query throughout); at the end the block adds its side-by-side groups in order and writes ONE
// partial row set, which set_boundary_dquery_kernel adds over the blocks in order.  No atomics: the same bits on every call.
constexpr int kBwdPieces = 4;        // pieces of VEC floats a lane holds of its row

template <int VEC>
__global__ __launch_bounds__(kThreads) void set_boundary_backward_kernel(
    const float *__restrict__ d_boundary, const float *__restrict__ member, long long n_query, long long n_node,
    long long row_stride, const float *__restrict__ floor, const float *__restrict__ query, long long dim,
    float *__restrict__ d_member, float *__restrict__ partial, int chunk, int sub, int group) {
    __shared__ float kept[kChunk][kTile + 1];
    __shared__ float dots[kChunk][kTile + 1];
    __shared__ float fold[kThreads * kBwdPieces * VEC];
    const int t = (int)threadIdx.x;
    const int wave = t / kTile, lane = t % kTile;
    const long long q0 = (long long)blockIdx.y * chunk;
    const int n_q = (int)(n_query - q0 < chunk ? n_query - q0 : chunk);
    const int n_slot = n_q * sub;                                   // <= kChunk
    const int n_group = kThreads / group;                           // >= chunk >= n_q
    const int side = n_group / n_q;                                 // nodes side by side
    const int g = t / group, piece = t % group;
    const int ql = g % n_q, vg = g / n_q;
    const bool active = vg < side;
    const long long row_floats = n_query * dim;
    const int n_piece = (int)(dim / VEC);                           // pieces of a row
    float qv[kBwdPieces][VEC], acc[kBwdPieces][VEC];
#pragma unroll
    for (int k = 0; k < kBwdPieces; ++k) {
        const int pc = piece + k * group;
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
            acc[k][e] = 0.0f;
            qv[k][e] = (active && pc < n_piece) ? query[(q0 + ql) * dim + (long long)pc * VEC + e] : 0.0f;
        }
    }
    const long long n_tiles = (n_node + (long long)kTile * sub - 1) / ((long long)kTile * sub);
    for (long long tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const long long v0 = tile * (kTile * sub);
        const int n_v = (int)(n_node - v0 < kTile * sub ? n_node - v0 : kTile * sub);
        for (int slot = wave; slot < n_slot; slot += kWaves) {      // stage: the forward's rule
            const long long q = q0 + slot % n_q;
            const int vl = slot / n_q * kTile + lane;
            float m = 0.0f;
            if (vl < n_v) m = member[q * row_stride + v0 + vl];
            bool keep = m > 0.0f;
            if (floor != nullptr) keep = keep && m >= floor[q];
            kept[slot][lane] = keep ? m : 0.0f;
            dots[slot][lane] = 0.0f;
        }
        __syncthreads();
        if (active) {
            const float *src = d_boundary + v0 * row_floats + (q0 + ql) * dim;
            for (int vl = vg; vl < n_v; vl += side) {
                const int slot = vl / kTile * n_q + ql;
                const float m = kept[slot][vl % kTile];
                if (!(m > 0.0f)) continue;                          // (uniform over the group: one row, one membership)
                const float *row = src + (long long)vl * row_floats;
                float dot = 0.0f;
#pragma unroll
                for (int k = 0; k < kBwdPieces; ++k) {
                    const int pc = piece + k * group;
                    if (pc < n_piece) {
                        float d[VEC];
                        if constexpr (VEC == 4) {
                            const float4 x = *reinterpret_cast<const float4 *>(row + (long long)pc * 4);
                            d[0] = x.x; d[1] = x.y; d[2] = x.z; d[3] = x.w;
                        } else {
                            d[0] = row[pc];
                        }
#pragma unroll
                        for (int e = 0; e < VEC; ++e) {
                            dot = dot + d[e] * qv[k][e];
                            acc[k][e] = acc[k][e] + m * d[e];
                        }
                    }
                }
                for (int s = group >> 1; s > 0; s >>= 1) dot = dot + __shfl_xor(dot, s, 64);
                if (piece == 0) dots[slot][vl % kTile] = dot;
            }
        }
        __syncthreads();
        for (int slot = wave; slot < n_slot; slot += kWaves) {      // d_member along v; not kept: the +0.0 staged above
            const long long q = q0 + slot % n_q;
            const int vl = slot / n_q * kTile + lane;
            if (vl < n_v) d_member[q * n_node + v0 + vl] = dots[slot][lane];
        }
        __syncthreads();                                            // the next tile restages
    }
    if (partial == nullptr) return;
    // ---- the block's d_query rows: side-by-side groups added in order
#pragma unroll
    for (int k = 0; k < kBwdPieces; ++k)
#pragma unroll
        for (int e = 0; e < VEC; ++e) fold[(k * VEC + e) * kThreads + t] = acc[k][e];
    __syncthreads();
    if (active && vg == 0) {
        float *out = partial + ((long long)blockIdx.y * gridDim.x + blockIdx.x) * ((long long)chunk * dim) + (long long)ql * dim;
#pragma unroll
        for (int k = 0; k < kBwdPieces; ++k) {
            const int pc = piece + k * group;
            if (pc < n_piece) {
#pragma unroll
                for (int e = 0; e < VEC; ++e) {
                    float total = 0.0f;
                    for (int s = 0; s < side; ++s) total = total + fold[(k * VEC + e) * kThreads + (s * n_q + ql) * group + piece];
                    out[(long long)pc * VEC + e] = total;
                }
            }
        }
    }
}

// d_query[q][d] = the blocks' partial rows of the query's chunk, added in block order
__global__ __launch_bounds__(kThreads) void set_boundary_dquery_kernel(const float *__restrict__ partial, long long n_query,
                                                                       long long dim, int chunk, int blocks,
                                                                       float *__restrict__ d_query) {
    const long long at = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (at >= n_query * dim) return;
    const long long q = at / dim, d = at % dim;
    const float *src = partial + (q / chunk) * blocks * ((long long)chunk * dim) + (q % chunk) * dim + d;
    float total = 0.0f;
#pragma unroll 8
    for (int b = 0; b < blocks; ++b) total = total + src[(long long)b * chunk * dim];
    d_query[at] = total;
}

// the decomposition both the entry and its workspace query use
struct BwdShape {
    int vec, group, chunk, sub, blocks;
    long long n_chunks;
};
bool backward_shape(long long n_query, long long n_node, long long dim, bool aligned, BwdShape *out) {
    BwdShape s;
    s.vec = (dim % 4 == 0 && aligned) ? 4 : 1;
    const long long n_piece = dim / s.vec;
    if (n_piece > (long long)kTile * kBwdPieces) return false;
    s.group = 1;
    while (s.group < n_piece && s.group < kTile) s.group *= 2;               // <= 64: a group never leaves its wave
    const int n_group = kThreads / s.group;
    s.chunk = n_group < kChunk ? n_group : kChunk;
    s.n_chunks = (n_query + s.chunk - 1) / s.chunk;
    s.sub = s.n_chunks == 1 ? kChunk / (int)n_query : 1;
    const long long n_tiles = (n_node + (long long)kTile * s.sub - 1) / ((long long)kTile * s.sub);
    long long per_chunk = kMaxBlocks / s.n_chunks;
    if (per_chunk < 1) per_chunk = 1;
    s.blocks = (int)(n_tiles < per_chunk ? n_tiles : per_chunk);
    *out = s;
    return s.n_chunks <= 65535;
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

// the d_query partial rows of ultra_set_boundary_backward_f32: one row set per block (the larger of the two row widths)
extern "C" size_t ultra_set_boundary_backward_workspace(int64_t n_query, int64_t n_node, int64_t dim) {
    if (n_query < 1 || n_node < 1 || dim < 1 || n_query > (1ll << 40) / dim) return 0;
    size_t most = 0;
    for (int aligned = 0; aligned < 2; ++aligned) {
        BwdShape s;
        if (!backward_shape(n_query, n_node, dim, aligned != 0, &s)) continue;
        const size_t bytes = (size_t)s.n_chunks * s.blocks * s.chunk * (size_t)dim * sizeof(float);
        most = bytes > most ? bytes : most;
    }
    return most;
}

extern "C" int ultra_set_boundary_backward_f32(const float *d_boundary, const float *member, int64_t n_query, int64_t n_node,
                                               int64_t row_stride, const float *floor, const float *query, int64_t dim,
                                               float *d_member, float *d_query, void *workspace, size_t workspace_bytes,
                                               void *stream) {
    if (n_query < 1 || n_node < 1 || dim < 1 || row_stride < n_node) return ULTRA_ERR_BAD_SHAPE;
    if (d_boundary == nullptr || member == nullptr || query == nullptr || d_member == nullptr) return ULTRA_ERR_NULL_POINTER;
    if (n_query > (1ll << 40) / dim || n_node > (1ll << 60) / (n_query * dim) || row_stride > (1ll << 60) / n_query)
        return ULTRA_ERR_BAD_SHAPE;
    const bool aligned = ((reinterpret_cast<uintptr_t>(query) | reinterpret_cast<uintptr_t>(d_boundary)) & 15u) == 0;
    BwdShape s;
    if (!backward_shape(n_query, n_node, dim, aligned, &s)) return ULTRA_ERR_BAD_SHAPE;
    float *partial = nullptr;
    if (d_query != nullptr) {
        const size_t need = (size_t)s.n_chunks * s.blocks * s.chunk * (size_t)dim * sizeof(float);
        if (workspace == nullptr) return ULTRA_ERR_NULL_POINTER;
        if (workspace_bytes < need) return ULTRA_ERR_WORKSPACE;
        partial = static_cast<float *>(workspace);
    }
    hipStream_t st = static_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)s.blocks, (unsigned)s.n_chunks);
    if (s.vec == 4)
        hipLaunchKernelGGL(set_boundary_backward_kernel<4>, grid, dim3(kThreads), 0, st, d_boundary, member, (long long)n_query,
                           (long long)n_node, (long long)row_stride, floor, query, (long long)dim, d_member, partial, s.chunk,
                           s.sub, s.group);
    else
        hipLaunchKernelGGL(set_boundary_backward_kernel<1>, grid, dim3(kThreads), 0, st, d_boundary, member, (long long)n_query,
                           (long long)n_node, (long long)row_stride, floor, query, (long long)dim, d_member, partial, s.chunk,
                           s.sub, s.group);
    HIP_TRY(hipGetLastError());
    if (d_query != nullptr) {
        const long long n = n_query * dim;
        hipLaunchKernelGGL(set_boundary_dquery_kernel, dim3((unsigned)((n + kThreads - 1) / kThreads)), dim3(kThreads), 0, st,
                           partial, (long long)n_query, (long long)dim, s.chunk, s.blocks, d_query);
        HIP_TRY(hipGetLastError());
    }
    return ULTRA_OK;
}

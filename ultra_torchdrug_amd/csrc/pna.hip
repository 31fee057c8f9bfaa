// ultra_torchdrug_amd/csrc/pna.hip -- PNA aggregation in inference (DESIGN.md "Native PNA inference").
//
// Two entries of include/ultra_rspmm.h:
//  * ultra_rspmm_pna_forward_f32: the four statistics of aggregate_func = "pna" (sum, sum of squares, max, min) from ONE walk
//    of the forward plan.  The kernel is segment_kernel / ChunkWalker (plan_general.hip) with four accumulators per column:
//    one wave per chunk and 64-column tile, relation tile in LDS where it fits, the same ticket scheduling, pieces of split
//    rows into the workspace and a fix-up pass in piece order.  Every plane is updated with exactly the operations the
//    corresponding ultra_rspmm_forward_f32 call performs (-ffp-contract=off: no fused multiply-add), in the same order per row
//    and piece, so every plane carries that call's bits.
//  * ultra_pna_combine_forward_f32: the layer epilogue over the statistics -- `_pna` (mean, std, the degree scalers) and
//    Linear(832 -> 64) + LayerNorm + relu + shortcut -- without the (rows, 768) update tensor.  The product runs on the exact-f32
//    matrix cores (v_mfma_f32_32x32x2_f32: bit for bit a k-ordered fmaf chain); its summation order is stated in the header.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "device_common.h"
#include "host_common.h"

namespace {

using namespace ultra_detail;        // kTile, kXcd, kMaxLdsBytes, kLdsHeader, tile_geometry (plan_path.h) and the host helpers

constexpr int kPnaBlock = 1024;      // threads per workgroup: 16 waves, 4 per SIMD, 128 VGPRs each
constexpr int kPnaUnroll = 8;        // edges in flight per wave: 3 staged values per edge next to the 4 accumulators
constexpr int kPnaFixUnroll = 16;    // piece sums in flight per wave and plane

enum Plane { PL_SUM = 0, PL_SQ = 1, PL_MAX = 2, PL_MIN = 3 };

struct PnaParams {
    const int32_t *row;
    const int32_t *node_a;
    const int32_t *rel;
    const float *weight;
    const int4 *chunks;
    const float *relation;   // [n_rel, F]
    const float *input;      // [n_src, F]
    const float *add_rows;   // [n_rows, F] or NULL: the boundary, dense
    const int32_t *bnode;    // or sparse: row bnode[c / bdim] holds bvec[c] in column c, every other element is 0
    const float *bvec;
    int bdim;
    float *out[4];           // [n_rows, F] each: sum, sq_sum, max, min
    float *partial;          // [4][n_pieces, F]
    long long plane_stride;  // n_pieces * F
    long long F;
    int n_chunks;
    int n_rel;
    int split;
    int n_slots;
    int blocks_per_label;
};

struct PnaFixParams {
    const int32_t *long_rows;   // [n_long][3]
    const float *partial;
    long long plane_stride;
    const float *add_rows;
    const int32_t *bnode;
    const float *bvec;
    int bdim;
    float *out[4];
    long long F;
    int n_long;
    int n_tiles;
};

// min / max in the forms of device_common.h's identity<> and reduce<>, NaN behaviour included (binary<> and uniform are its own)
constexpr float kLowest = -3.402823466e+38f, kLargest = 3.402823466e+38f;   // torchdrug's NaryMax / NaryMin start values
__device__ __forceinline__ float red_max(float acc, float y) { return (y > acc) ? y : acc; }
__device__ __forceinline__ float red_min(float acc, float y) { return (y < acc) ? y : acc; }
// acc + y with the accumulator as the instruction's FIRST operand.  Where two different NaNs meet in one addition (an input NaN
// and the -NaN that inf - inf or inf * 0 generate) the hardware keeps the first operand's, and the compiler is free to commute
// `acc + y`: fixup_kernel's adds came out accumulator first, this file's the other way round, and a split row whose pieces hold
// NaNs of both signs then differed from ultra_rspmm_forward_f32 in the sign bit of its NaN.  Used by the fix-up pass and the
// boundary epilogue; inside a chunk's walk the library's own kernels take both orders, so nothing is pinned there.
__device__ __forceinline__ float add_acc_first(float acc, float y) {
    float d;
    asm("v_add_f32_e32 %0, %1, %2" : "=v"(d) : "v"(acc), "v"(y));
    return d;
}

struct Stats {
    float sum, sq, max, min;
    __device__ __forceinline__ void reset() { sum = 0.0f; sq = 0.0f; max = kLowest; min = kLargest; }
    // the boundary element b as one more contribution of each plane
    __device__ __forceinline__ void add_boundary(float b) {
        sum = add_acc_first(sum, b);
        sq = add_acc_first(sq, b * b);
        max = red_max(max, b);
        min = red_min(min, b);
    }
};

// One chunk of the forward plan, processed by one wave for one column tile (ChunkWalker<KIND_FWD> with four planes).
template <int MUL, bool UNIT_W, bool REL_LDS>
struct PnaWalker {
    const PnaParams &p;
    const long long F;
    const long long col;    // this lane's column
    const long long lcol;   // column used for loads: clamped into range so that loads never need a predicate
    const bool active;      // col < F (stores only)
    const float *lds_rel;
    const int lane;
    const int b_node;       // sparse boundary of this lane's column (-1: none)
    const float b_val;
    int cur;
    Stats acc;
    bool is_piece;

    __device__ __forceinline__ float load_rel(int r) const {
        if constexpr (REL_LDS) return lds_rel[r * kTile + lane];
        else return p.relation[(long long)r * F + lcol];
    }
    __device__ __forceinline__ void store_row(int r, Stats v) const {
        if (active) {
            const long long at = (long long)r * F + col;
            if (p.add_rows != nullptr) v.add_boundary(p.add_rows[at]);
            else if (p.bnode != nullptr) v.add_boundary((r == b_node) ? b_val : 0.0f);
            p.out[PL_SUM][at] = v.sum;
            p.out[PL_SQ][at] = v.sq;
            p.out[PL_MAX][at] = v.max;
            p.out[PL_MIN][at] = v.min;
        }
    }
    __device__ __forceinline__ void store_empty(int from, int to) const {
        Stats e;
        e.reset();
        for (int q = from; q < to; ++q) store_row(q, e);
    }

    // kPnaUnroll consecutive edges starting at e0; FULL: all of them exist, else only n.
    template <bool FULL>
    __device__ __forceinline__ void batch(const int e0, const int n) {
        int ia[kPnaUnroll], ir[kPnaUnroll], irow[kPnaUnroll];
        float wv[kPnaUnroll], xv[kPnaUnroll], rv[kPnaUnroll];
#pragma unroll
        for (int u = 0; u < kPnaUnroll; ++u) {
            const int e = FULL ? e0 + u : e0 + min(u, n - 1);   // tail slots re-load the last edge, never used
            ia[u] = p.node_a[e];
            irow[u] = p.row[e];
            ir[u] = p.rel[e];
            if constexpr (!UNIT_W) wv[u] = p.weight[e];
        }
#pragma unroll
        for (int u = 0; u < kPnaUnroll; ++u) xv[u] = p.input[(long long)ia[u] * F + lcol];
#pragma unroll
        for (int u = 0; u < kPnaUnroll; ++u) rv[u] = load_rel(ir[u]);
#pragma unroll
        for (int u = 0; u < kPnaUnroll; ++u) {
            if (FULL || u < n) {
                if (!is_piece && irow[u] != cur) {
                    store_row(cur, acc);
                    store_empty(cur + 1, irow[u]);
                    cur = irow[u];
                    acc.reset();
                }
                float y = binary<MUL>(rv[u], xv[u]);
                float y2 = binary<MUL>(rv[u] * rv[u], xv[u] * xv[u]);   // the squared OPERANDS (ultra/layer.py:367)
                if constexpr (!UNIT_W) {
                    y = wv[u] * y;
                    y2 = wv[u] * y2;
                }
                acc.sum = acc.sum + y;
                acc.sq = acc.sq + y2;
                acc.max = red_max(acc.max, y);
                acc.min = red_min(acc.min, y);
            }
        }
    }

    __device__ __forceinline__ void run(const int4 d) {
        is_piece = d.w < 0;
        cur = d.z;
        acc.reset();
        int e0 = d.x;
        for (; e0 + kPnaUnroll <= d.y; e0 += kPnaUnroll) batch<true>(e0, kPnaUnroll);
        if (e0 < d.y) batch<false>(e0, d.y - e0);
        if (is_piece) {
            if (active) {
                float *slot = p.partial + (long long)(-d.w - 1) * F + col;
                slot[PL_SUM * p.plane_stride] = acc.sum;
                slot[PL_SQ * p.plane_stride] = acc.sq;
                slot[PL_MAX * p.plane_stride] = acc.max;
                slot[PL_MIN * p.plane_stride] = acc.min;
            }
        } else {
            store_row(cur, acc);
            store_empty(cur + 1, d.w);
        }
    }
};

// segment_kernel's frame: label = blockIdx % 8 owns whole column tiles, chunks dealt in serpentine order across workgroups and
// drawn from an LDS ticket counter within one.  Which wave takes which chunk never affects the result.
template <int MUL, bool UNIT_W, bool REL_LDS>
__global__ __launch_bounds__(kPnaBlock) void pna_segment_kernel(const PnaParams p) {
    extern __shared__ __attribute__((aligned(16))) float pna_lds[];
    int *ticket = reinterpret_cast<int *>(pna_lds);                 // first kLdsHeader bytes
    float *lds_rel = pna_lds + kLdsHeader / sizeof(float);
    const int lane = threadIdx.x & 63;
    const int label = blockIdx.x % kXcd;
    const int bl = blockIdx.x / kXcd;
    const int nb = p.blocks_per_label;

    for (int s = label; s < p.n_slots; s += kXcd) {
        const int tile = s / p.split;
        const int part = s - tile * p.split;
        const long long col = (long long)tile * kTile + lane;
        const bool active = col < p.F;
        if constexpr (REL_LDS) {
            const int total = p.n_rel * kTile;
            for (int i = threadIdx.x; i < total; i += kPnaBlock) {
                const int r = i >> 6;
                const long long c = (long long)tile * kTile + (i & 63);
                lds_rel[i] = (c < p.F) ? p.relation[(long long)r * p.F + c] : 0.0f;
            }
        }
        if (threadIdx.x == 0) *ticket = 0;
        __syncthreads();
        int b_node = -1;
        float b_val = 0.0f;
        if (p.bnode != nullptr && active) {
            b_node = p.bnode[col / p.bdim];
            b_val = p.bvec[col];
        }
        for (;;) {
            int t = 0;
            if (lane == 0) t = __hip_atomic_fetch_add(ticket, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            t = uniform(t);
            const int k = part + p.split * (t * nb + ((t & 1) ? (nb - 1 - bl) : bl));
            if (k >= p.n_chunks) break;
            const int4 d = p.chunks[uniform(k)];
            PnaWalker<MUL, UNIT_W, REL_LDS> walker{p, p.F, col, active ? col : p.F - 1, active, lds_rel, lane, b_node, b_val,
                                                   0, Stats{}, false};
            walker.run(d);
        }
        __syncthreads();   // all tickets drawn and the table no longer read before the next slot rewrites them
    }
}

// out[plane][row] = epilogue( partial[first] (+) partial[first + 1] (+) ... ) in piece order, from the identity (fixup_kernel)
template <int PLANE>
__device__ __forceinline__ float pna_fix_plane(const float *partial, long long F, long long col, int first, int n) {
    float acc = PLANE == PL_MAX ? kLowest : (PLANE == PL_MIN ? kLargest : 0.0f);
    for (int k0 = 0; k0 < n; k0 += kPnaFixUnroll) {
        float v[kPnaFixUnroll];
#pragma unroll
        for (int u = 0; u < kPnaFixUnroll; ++u) {
            const int k = min(k0 + u, n - 1);
            v[u] = partial[(long long)(first + k) * F + col];
        }
#pragma unroll
        for (int u = 0; u < kPnaFixUnroll; ++u)
            if (k0 + u < n) acc = PLANE == PL_MAX ? red_max(acc, v[u]) : (PLANE == PL_MIN ? red_min(acc, v[u]) : add_acc_first(acc, v[u]));
    }
    return acc;
}

__global__ __launch_bounds__(256) void pna_fixup_kernel(const PnaFixParams p) {
    const int lane = threadIdx.x & 63;
    const int wave_global = uniform((int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6));
    const int total = p.n_long * p.n_tiles;
    if (wave_global >= total) return;
    const int lr = wave_global / p.n_tiles;
    const int tile = wave_global - lr * p.n_tiles;
    const long long col = (long long)tile * kTile + lane;
    if (col >= p.F) return;
    const int row = p.long_rows[lr * 3 + 0];
    const int first = p.long_rows[lr * 3 + 1];
    const int n = p.long_rows[lr * 3 + 2];
    Stats v;
    v.sum = pna_fix_plane<PL_SUM>(p.partial + PL_SUM * p.plane_stride, p.F, col, first, n);
    v.sq = pna_fix_plane<PL_SQ>(p.partial + PL_SQ * p.plane_stride, p.F, col, first, n);
    v.max = pna_fix_plane<PL_MAX>(p.partial + PL_MAX * p.plane_stride, p.F, col, first, n);
    v.min = pna_fix_plane<PL_MIN>(p.partial + PL_MIN * p.plane_stride, p.F, col, first, n);
    const long long at = (long long)row * p.F + col;
    if (p.add_rows != nullptr) v.add_boundary(p.add_rows[at]);
    else if (p.bnode != nullptr) v.add_boundary((row == p.bnode[col / p.bdim]) ? p.bvec[col] : 0.0f);
    p.out[PL_SUM][at] = v.sum;
    p.out[PL_SQ][at] = v.sq;
    p.out[PL_MAX][at] = v.max;
    p.out[PL_MIN][at] = v.min;
}

// ---------------------------------------------------------------------------------------------------------------
// The epilogue.  A workgroup of 8 waves takes 32-row tiles; wave w owns the columns d = 8 w .. 8 w + 7 of the five row tensors
// (input, sum, sq_sum, max, min), i.e. K-slice w of the 832-wide product: 8 input columns and 8 * 12 update columns.  Its
// share of the weight -- 64 outputs x 104 columns -- stays in registers for the life of the workgroup (lane (i, h): rows i and
// 32 + i of the weight, the columns of d = 8 w + 4 h .. + 3), and its B operands are made in registers from the lane's own
// row: lane (i, h) loads 16 bytes of each tensor of row i, computes mean / std and the three scalings, and feeds them to
// mfma(A = weight, B = feature).  Nothing of the (rows, 768) update tensor exists anywhere.  The eight partial products meet in
// LDS (two buffers: one barrier per tile) and thread (row = t >> 4, outputs 4 (t & 15) .. + 3) adds them in wave order from the
// bias, then LayerNorm (sums over the row's 16 lanes as an xor butterfly), relu and the shortcut.

constexpr int kPcWaves = 8;
constexpr int kPcRows = 32;
constexpr int kPcStride = 68;                                   // floats per row of a partial: 64 + 4 (16-byte writes, no conflicts)
constexpr int kPcPartial = kPcRows * kPcStride;                 // one wave's partial
constexpr int kPcLdsFloats = 2 * kPcWaves * kPcPartial;

struct PnaCombineParams {
    const float *input, *sum, *sq, *max, *min;    // [rows, 64]
    const float *node_table;                      // [ceil(rows / n_query)][3]
    const float *weight;                          // [64][832]
    const float *bias, *gamma, *beta;
    float *out;
    long long rows;
    long long n_query;
    float ln_eps, pna_eps;
    int relu, shortcut;
};

struct PnaRowSlice {
    f32x4 x, s, q, mx, mn;
    float deg, scale, inv;
};

__global__ __launch_bounds__(kPcWaves * 64, 2) void pna_combine_kernel(const PnaCombineParams p) {
    extern __shared__ __attribute__((aligned(16))) float pc_lds[];
    const int lane = threadIdx.x & 63;
    const int w = uniform(threadIdx.x >> 6);
    const int i = lane & 31, h = lane >> 5;
    const int d0 = 8 * w + 4 * h;                 // the lane's four columns of every row tensor
    const long long n_tiles = (p.rows + kPcRows - 1) / kPcRows;

    // A operands: rows i and 32 + i of the weight at the lane's columns -- 4 of the input block, 48 of the update block
    float w_in[2][4], w_up[2][48];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const float *wr = p.weight + (long long)(32 * t + i) * 832;
#pragma unroll
        for (int j = 0; j < 4; ++j) w_in[t][j] = wr[d0 + j];
#pragma unroll
        for (int j = 0; j < 48; ++j) w_up[t][j] = wr[64 + d0 * 12 + j];
    }
    // finishing role of this thread
    const int f_row = threadIdx.x >> 4, f_col = (threadIdx.x & 15) * 4;
    const f32x4 f_bias = *reinterpret_cast<const f32x4 *>(p.bias + f_col);
    f32x4 f_gamma = {1.0f, 1.0f, 1.0f, 1.0f}, f_beta = {0.0f, 0.0f, 0.0f, 0.0f};
    if (p.gamma != nullptr) {
        f_gamma = *reinterpret_cast<const f32x4 *>(p.gamma + f_col);
        f_beta = *reinterpret_cast<const f32x4 *>(p.beta + f_col);
    }

    auto fetch = [&](long long tile) {
        PnaRowSlice r;
        long long row = tile * kPcRows + i;
        if (row >= p.rows) row = p.rows - 1;          // rows past the end repeat the last one and are never stored
        const long long at = row * 64 + d0;
        r.x = *reinterpret_cast<const f32x4 *>(p.input + at);
        r.s = *reinterpret_cast<const f32x4 *>(p.sum + at);
        r.q = *reinterpret_cast<const f32x4 *>(p.sq + at);
        r.mx = *reinterpret_cast<const f32x4 *>(p.max + at);
        r.mn = *reinterpret_cast<const f32x4 *>(p.min + at);
        const float *nt = p.node_table + (row / p.n_query) * 3;
        r.deg = nt[0]; r.scale = nt[1]; r.inv = nt[2];
        return r;
    };

    long long tile = blockIdx.x;
    if (tile >= n_tiles) return;
    PnaRowSlice nxt = fetch(tile);
    for (int buf = 0; tile < n_tiles; tile += gridDim.x, buf ^= 1) {
        const PnaRowSlice cur = nxt;
        if (tile + gridDim.x < n_tiles) nxt = fetch(tile + gridDim.x);     // in flight during the product

        f32x16 acc0, acc1;
#pragma unroll
        for (int r = 0; r < 16; ++r) { acc0[r] = 0.0f; acc1[r] = 0.0f; }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(w_in[0][j], cur.x[j], acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(w_in[1][j], cur.x[j], acc1, 0, 0, 0);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            // layer._pna, step by step
            const float mean = cur.s[j] / cur.deg;
            const float sq_mean = cur.q[j] / cur.deg;
            const float std = sqrtf(fmaxf(sq_mean - mean * mean, p.pna_eps));
            const float feat[4] = {mean, cur.mx[j], cur.mn[j], std};
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const float b[3] = {feat[s], feat[s] * cur.scale, feat[s] * cur.inv};
#pragma unroll
                for (int a = 0; a < 3; ++a) {
                    acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(w_up[0][(j * 4 + s) * 3 + a], b[a], acc0, 0, 0, 0);
                    acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(w_up[1][(j * 4 + s) * 3 + a], b[a], acc1, 0, 0, 0);
                }
            }
        }

        // acc_t[r] of lane (i, h) is output 32 t + (r & 3) + 8 (r >> 2) + 4 h of row i
        float *mine = pc_lds + (buf * kPcWaves + w) * kPcPartial + i * kPcStride;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            f32x4 v0, v1;
            v0.x = acc0[4 * g + 0]; v0.y = acc0[4 * g + 1]; v0.z = acc0[4 * g + 2]; v0.w = acc0[4 * g + 3];
            v1.x = acc1[4 * g + 0]; v1.y = acc1[4 * g + 1]; v1.z = acc1[4 * g + 2]; v1.w = acc1[4 * g + 3];
            *reinterpret_cast<f32x4 *>(mine + 8 * g + 4 * h) = v0;
            *reinterpret_cast<f32x4 *>(mine + 32 + 8 * g + 4 * h) = v1;
        }
        __syncthreads();

        // z = ((bias + P_0) + P_1) + ... + P_7
        f32x4 z = f_bias;
#pragma unroll
        for (int k = 0; k < kPcWaves; ++k)
            z = z + *reinterpret_cast<const f32x4 *>(pc_lds + (buf * kPcWaves + k) * kPcPartial + f_row * kPcStride + f_col);
        if (p.gamma != nullptr) {
            float s = ((z.x + z.y) + z.z) + z.w;
#pragma unroll
            for (int m = 1; m < 16; m <<= 1) s = s + __shfl_xor(s, m, 16);
            const float mean = s * (1.0f / 64.0f);
            const f32x4 dlt = z - mean;
            float ss = ((dlt.x * dlt.x + dlt.y * dlt.y) + dlt.z * dlt.z) + dlt.w * dlt.w;
#pragma unroll
            for (int m = 1; m < 16; m <<= 1) ss = ss + __shfl_xor(ss, m, 16);
            const float inv = 1.0f / sqrtf(ss * (1.0f / 64.0f) + p.ln_eps);
            z = (dlt * inv) * f_gamma + f_beta;
        }
        if (p.relu) {
#pragma unroll
            for (int j = 0; j < 4; ++j) z[j] = !(z[j] <= 0.0f) ? z[j] : 0.0f;
        }
        const long long row = tile * kPcRows + f_row;
        if (row < p.rows) {
            if (p.shortcut) z = z + *reinterpret_cast<const f32x4 *>(p.input + row * 64 + f_col);
            *reinterpret_cast<f32x4 *>(p.out + row * 64 + f_col) = z;
        }
    }
}

inline bool aligned16(const void *ptr) { return (reinterpret_cast<uintptr_t>(ptr) & 15u) == 0; }

}  // namespace

extern "C" {

size_t ultra_rspmm_pna_workspace_bytes(const ultra_segments *fwd, int64_t F) { return 4 * ultra_rspmm_workspace_bytes(fwd, F); }

int ultra_rspmm_pna_forward_f32(const ultra_segments *fwd, const float *relation, const float *input, const float *add_rows,
                                const int32_t *boundary_node, const float *boundary_value, int64_t block, float *sum,
                                float *sq_sum, float *max, float *min, void *workspace, size_t workspace_bytes, int64_t n_src,
                                int64_t n_rel, int64_t F, int mul_op, void *stream) {
    int rc = check_segments(fwd);
    if (rc) return rc;
    if (F <= 0 || n_src < 0 || n_rel < 0 || n_rel > 0x7fffffffLL) return ULTRA_ERR_BAD_SHAPE;
    if (mul_op < 0 || mul_op > 1) return ULTRA_ERR_BAD_OP;
    if (fwd->dense != nullptr) return ULTRA_ERR_BAD_SHAPE;       // the dense form sums in another order: four calls there
    if (fwd->n_rows > 0 && (sum == nullptr || sq_sum == nullptr || max == nullptr || min == nullptr)) return ULTRA_ERR_NULL_POINTER;
    if (fwd->n_edges > 0 && (relation == nullptr || input == nullptr)) return ULTRA_ERR_NULL_POINTER;
    if ((boundary_node == nullptr) != (boundary_value == nullptr)) return ULTRA_ERR_NULL_POINTER;
    if (boundary_node != nullptr) {
        if (add_rows != nullptr) return ULTRA_ERR_BAD_SHAPE;     // the boundary either dense or sparse
        if (block <= 0 || block > 0x7fffffffLL || F % block != 0) return ULTRA_ERR_BAD_SHAPE;
    }
    const size_t need = ultra_rspmm_pna_workspace_bytes(fwd, F);
    if (need > 0 && (workspace == nullptr || workspace_bytes < need)) return ULTRA_ERR_WORKSPACE;
    if (fwd->n_rows == 0) return ULTRA_OK;

    DeviceInfo *di = nullptr;
    rc = current_device_info(&di);
    if (rc) return rc;
    const TileGeometry geo = tile_geometry(F, kTile, di->n_cu);
    const size_t rel_bytes = (size_t)n_rel * kTile * sizeof(float);
    const bool rel_lds = n_rel > 0 && kLdsHeader + rel_bytes <= (size_t)kMaxLdsBytes;
    const size_t lds = kLdsHeader + (rel_lds ? rel_bytes : 0);
    hipStream_t st = static_cast<hipStream_t>(stream);

    PnaParams p{};
    p.row = fwd->row; p.node_a = fwd->node_a; p.rel = fwd->rel; p.weight = fwd->weight;
    p.chunks = reinterpret_cast<const int4 *>(fwd->chunks);
    p.relation = relation; p.input = input; p.add_rows = add_rows;
    p.bnode = boundary_node; p.bvec = boundary_value; p.bdim = boundary_node != nullptr ? (int)block : 0;
    p.out[PL_SUM] = sum; p.out[PL_SQ] = sq_sum; p.out[PL_MAX] = max; p.out[PL_MIN] = min;
    p.partial = static_cast<float *>(workspace);
    p.plane_stride = (long long)fwd->n_pieces * F;
    p.F = F;
    p.n_chunks = (int)fwd->n_chunks; p.n_rel = (int)n_rel;
    p.split = geo.split; p.n_slots = geo.n_slots; p.blocks_per_label = geo.blocks_per_label;
    rc = with_mul(mul_op, [&](auto mul) {
        return with_bool(fwd->weight == nullptr, [&](auto uw) {
            return with_bool(rel_lds, [&](auto rl) {
                return launch_with_lds(pna_segment_kernel<decltype(mul)::value, decltype(uw)::value, decltype(rl)::value>, p,
                                       geo.grid, lds, st, kPnaBlock);
            });
        });
    });
    if (rc) return rc;
    if (fwd->n_long_rows > 0) {
        PnaFixParams fp{};
        fp.long_rows = fwd->long_rows; fp.partial = p.partial; fp.plane_stride = p.plane_stride;
        fp.add_rows = add_rows; fp.bnode = p.bnode; fp.bvec = p.bvec; fp.bdim = p.bdim;
        for (int k = 0; k < 4; ++k) fp.out[k] = p.out[k];
        fp.F = F; fp.n_long = (int)fwd->n_long_rows; fp.n_tiles = geo.n_tiles;
        if ((long long)fwd->n_long_rows * geo.n_tiles > 0x7fffffffLL) return ULTRA_ERR_BAD_SHAPE;
        const int grid = (int)(((long long)fwd->n_long_rows * geo.n_tiles + 3) / 4);
        hipLaunchKernelGGL(pna_fixup_kernel, dim3(grid), dim3(256), 0, st, fp);
        HIP_TRY(hipGetLastError());
    }
    return ULTRA_OK;
}

int ultra_pna_combine_forward_f32(const float *input, const float *sum, const float *sq_sum, const float *max, const float *min,
                                  const float *node_table, int64_t n_query, const float *weight, const float *bias,
                                  const float *ln_weight, const float *ln_bias, float ln_eps, float pna_eps, int relu,
                                  int shortcut, float *out, int64_t rows, int64_t dim, void *stream) {
    if (dim != 64 || rows < 0 || n_query <= 0) return ULTRA_ERR_BAD_SHAPE;
    if (rows == 0) return ULTRA_OK;
    if (input == nullptr || sum == nullptr || sq_sum == nullptr || max == nullptr || min == nullptr || node_table == nullptr ||
        weight == nullptr || bias == nullptr || out == nullptr)
        return ULTRA_ERR_NULL_POINTER;
    if (ln_weight != nullptr && ln_bias == nullptr) return ULTRA_ERR_NULL_POINTER;
    if (!(aligned16(input) && aligned16(sum) && aligned16(sq_sum) && aligned16(max) && aligned16(min) && aligned16(out) &&
          aligned16(bias) && aligned16(ln_weight) && aligned16(ln_bias)))
        return ULTRA_ERR_BAD_SHAPE;
    DeviceInfo *di = nullptr;
    int rc = current_device_info(&di);
    if (rc) return rc;
    PnaCombineParams p{};
    p.input = input; p.sum = sum; p.sq = sq_sum; p.max = max; p.min = min; p.node_table = node_table;
    p.weight = weight; p.bias = bias; p.gamma = ln_weight; p.beta = ln_bias; p.out = out;
    p.rows = rows; p.n_query = n_query; p.ln_eps = ln_eps; p.pna_eps = pna_eps; p.relu = relu; p.shortcut = shortcut;
    const long long n_tiles = (rows + kPcRows - 1) / kPcRows;
    const int grid = (int)(n_tiles < di->n_cu ? n_tiles : di->n_cu);
    return launch_with_lds(pna_combine_kernel, p, grid, kPcLdsFloats * sizeof(float), static_cast<hipStream_t>(stream),
                           kPcWaves * 64);
}

}  // extern "C"

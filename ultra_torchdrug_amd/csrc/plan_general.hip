// ultra_torchdrug_amd/csrc/plan_general.hip -- the general plan kernel: every kind, every operator pair (launch_general).
//
// Design (DESIGN.md has the numbers):
//  * one lane = one fp32 column, one wave = one 64-column tile of a row; F is cut into ceil(F/64) tiles.
//    A tile of one source row is a 256-B contiguous segment, so every gather is one fully coalesced
//    global_load_dword per wave and each lane accumulates ITS column strictly in sorted-edge order
//    (that is what makes unsplit rows bit-identical to the sequential CPU oracle).
//  * the relation table of the tile (n_rel x 64 fp32) is staged once per workgroup in LDS, so the
//    per-edge relation operand costs one conflict-free ds_read_b32 and no L2 traffic.
//  * persistent grid, XCD-aware: blocks b and b+8 share an XCD (round-robin dispatch, speed only, never
//    correctness), so label = blockIdx % 8 owns whole column tiles: the N x 256 B slice of `input` that a
//    tile touches (3.7 MB for FB15k237) then lives in ONE XCD's 4 MB L2 while that tile is processed.
//  * per-wavefront segmented reduction over a precomputed chunk schedule (ultra_segments): a chunk is a
//    run of whole rows or one piece of a long row; edge metadata is wave-uniform and comes in through
//    scalar loads; UNROLL gathers are in flight per wave.  Long-row pieces go to a workspace and are added
//    in piece order by fixup_kernel: deterministic, no atomics.
//  * compiled with -ffp-contract=off: message = w * (rel (*|+) x) is rounded before it is accumulated,
//    exactly as the oracle does.
#include <hip/hip_runtime.h>
#include <type_traits>

#include <cstdint>

#include "device_common.h"
#include "plan_kernels.h"

namespace {

using namespace ultra_detail;        // kTile, kXcd, kLdsHeader, Kind (plan_path.h), the parameter blocks and the host helpers

// One chunk of the schedule, processed by one wave for one column tile.
//   KIND_FWD : acc (SUM)= w * (relation[rel] MUL input[node_a])
//   KIND_DX  : acc += ((grad[node_a] * dmask) * w) * d(MUL)/d(input)      rows = source nodes
//   KIND_DREL: acc += ((grad[node_b] * dmask) * w) * d(MUL)/d(relation)   rows = relations
// dmask = 1 for sum=add, (output == y) for min/max with y the forward message of that edge.
template <int KIND, int SUM, int MUL, bool UNIT_W, bool REL_LDS>
struct ChunkWalker {
    static constexpr int RED = (KIND == KIND_FWD) ? SUM : ULTRA_SUM_ADD;
    static constexpr bool MASKED = (KIND != KIND_FWD) && (SUM != ULTRA_SUM_ADD);
    // the per-edge relation row is needed by the forward and by d_input (mask and/or d(mul)/d(input) = relation)
    static constexpr bool NEED_REL_ID = (KIND == KIND_FWD) || (KIND == KIND_DX && (MASKED || MUL == ULTRA_MUL_MUL));

    const KParams &p;
    const long long F;
    const long long col;    // this lane's column
    const long long lcol;   // column used for loads: clamped into range so that loads never need a predicate
    const bool active;      // col < F (stores only)
    const float *lds_rel;
    const int lane;
    int cur;
    float acc;
    bool is_piece;

    __device__ __forceinline__ float load_rel(int r) const {
        if constexpr (REL_LDS) return lds_rel[r * kTile + lane];
        else return p.relation[(long long)r * F + lcol];
    }
    __device__ __forceinline__ void store_row(int r, float v) const {
        if (active) {
            // add_rows: forward -- the fused boundary epilogue; d_input -- the gradient the same rows receive from the
            // layer's epilogue (ultra_rspmm_backward_accumulate_f32; may alias `out`: read before it is written)
            if constexpr (KIND != KIND_DREL) {
                if (p.add_rows != nullptr) v = reduce<RED>(v, p.add_rows[(long long)r * F + col]);
                else if (KIND == KIND_FWD && p.bnode != nullptr) v = reduce<RED>(v, (r == p.bnode[col / p.bdim]) ? p.bvec[col] : 0.0f);
            }
            p.out[(long long)r * F + col] = v;
        }
    }

    // kUnroll consecutive edges starting at e0; FULL: all kUnroll exist, else only n of them.
    template <bool FULL>
    __device__ __forceinline__ void batch(const int e0, const int n) {
        int ia[kUnroll], ib[kUnroll], ir[kUnroll], irow[kUnroll];
        float wv[kUnroll];
        float v0[kUnroll], v1[kUnroll], v2[kUnroll];
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
            const int e = FULL ? e0 + u : e0 + min(u, n - 1);   // tail slots re-load the last edge, never used
            ia[u] = p.node_a[e];
            irow[u] = p.row[e];
            if constexpr (NEED_REL_ID) ir[u] = p.rel[e];
            if constexpr (KIND == KIND_DREL) ib[u] = p.node_b[e];
            if constexpr (!UNIT_W) wv[u] = p.weight[e];
        }
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
            if constexpr (KIND == KIND_FWD) {
                v0[u] = p.input[(long long)ia[u] * F + lcol];
            } else if constexpr (KIND == KIND_DX) {
                v0[u] = p.grad[(long long)ia[u] * F + lcol];
                if constexpr (MASKED) {
                    v1[u] = p.output[(long long)ia[u] * F + lcol];
                    v2[u] = p.input[(long long)irow[u] * F + lcol];
                }
            } else {
                v0[u] = p.grad[(long long)ib[u] * F + lcol];
                if constexpr (MASKED || MUL == ULTRA_MUL_MUL) v2[u] = p.input[(long long)ia[u] * F + lcol];
                if constexpr (MASKED) v1[u] = p.output[(long long)ib[u] * F + lcol];
            }
        }
        // relation operands of the batch: issued together (LDS reads or, for tables too big for LDS, L2 loads)
        float rv[kUnroll];
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
            rv[u] = 0.0f;
            if constexpr (NEED_REL_ID) rv[u] = load_rel(ir[u]);
            if constexpr (KIND == KIND_DREL && MASKED) rv[u] = p.relation[(long long)irow[u] * F + lcol];
        }
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
            if (FULL || u < n) {
                if (!is_piece && irow[u] != cur) {
                    store_row(cur, acc);
                    for (int q = cur + 1; q < irow[u]; ++q) store_row(q, identity<RED>());
                    cur = irow[u];
                    acc = identity<RED>();
                }
                if constexpr (KIND == KIND_FWD) {
                    float y = binary<MUL>(rv[u], v0[u]);
                    if constexpr (!UNIT_W) y = wv[u] * y;
                    acc = reduce<RED>(acc, y);
                } else {
                    float c = v0[u];   // grad[dst]
                    if constexpr (MASKED) {
                        float y = binary<MUL>(rv[u], v2[u]);   // forward message of this edge
                        if constexpr (!UNIT_W) y = wv[u] * y;
                        c = c * ((v1[u] == y) ? 1.0f : 0.0f);
                    }
                    if constexpr (!UNIT_W) c = c * wv[u];
                    if constexpr (MUL == ULTRA_MUL_MUL) c = c * (KIND == KIND_DX ? rv[u] : v2[u]);
                    acc = acc + c;
                }
            }
        }
    }

    __device__ __forceinline__ void run(const int4 d) {
        is_piece = d.w < 0;
        cur = d.z;
        acc = identity<RED>();
        int e0 = d.x;
        for (; e0 + kUnroll <= d.y; e0 += kUnroll) batch<true>(e0, kUnroll);
        if (e0 < d.y) batch<false>(e0, d.y - e0);
        if (is_piece) {
            if (active) p.partial[(long long)(-d.w - 1) * F + col] = acc;
        } else {
            store_row(cur, acc);
            for (int q = cur + 1; q < d.w; ++q) store_row(q, identity<RED>());
        }
    }
};

template <int KIND, int SUM, int MUL, bool UNIT_W, bool REL_LDS>
__global__ __launch_bounds__(kBlock) void segment_kernel(const KParams p) {
    extern __shared__ __attribute__((aligned(16))) float lds_raw[];
    int *ticket = reinterpret_cast<int *>(lds_raw);                 // first kLdsHeader bytes
    float *lds_rel = lds_raw + kLdsHeader / sizeof(float);
    const int lane = threadIdx.x & 63;
    const int label = blockIdx.x % kXcd;          // blocks sharing an XCD (round-robin dispatch; speed only)
    const int bl = blockIdx.x / kXcd;
    const int nb = p.blocks_per_label;

    for (int s = label; s < p.n_slots; s += kXcd) {
        const int tile = s / p.split;
        const int part = s - tile * p.split;
        const long long col = (long long)tile * kTile + lane;
        const bool active = col < p.F;
        if constexpr (REL_LDS) {
            const int total = p.n_rel * kTile;
            for (int i = threadIdx.x; i < total; i += kBlock) {
                const int r = i >> 6;
                const long long c = (long long)tile * kTile + (i & 63);
                lds_rel[i] = (c < p.F) ? p.relation[(long long)r * p.F + c] : 0.0f;
            }
        }
        if (threadIdx.x == 0) *ticket = 0;
        __syncthreads();
        // Work distribution.  Chunks are sorted heaviest first.  ACROSS workgroups they are dealt statically in
        // serpentine order (round t: workgroup bl takes chunk t*nb + bl on even t, t*nb + nb-1-bl on odd t);
        // WITHIN a workgroup the 16 waves draw rounds t from a ticket counter in LDS, so a wave that finishes early
        // simply takes the next chunk (heavy ones first: LPT) and all waves reach the slot barrier together.
        // Which wave computes which chunk never affects the result.
        for (;;) {
            int t = 0;
            if (lane == 0) t = __hip_atomic_fetch_add(ticket, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            t = uniform(t);
            const int k = part + p.split * (t * nb + ((t & 1) ? (nb - 1 - bl) : bl));
            if (k >= p.n_chunks) break;
            const int4 d = p.chunks[uniform(k)];
            ChunkWalker<KIND, SUM, MUL, UNIT_W, REL_LDS> walker{p, p.F, col, active ? col : p.F - 1, active, lds_rel, lane,
                                                                0, 0.0f, false};
            walker.run(d);
        }
        __syncthreads();   // all tickets drawn and tables no longer read before the next slot rewrites them
    }
}

// The launcher takes the variant from plan_path()'s decision and instantiates exactly the kernels a call can reach.
template <int KIND, int SUM, int MUL>
int launch_general(const KParams &p, const PlanPath &path, hipStream_t stream) {
    return with_bool(path.unit_w, [&](auto uw) {
        return with_bool(path.rel_lds, [&](auto rl) {
            constexpr bool UW = decltype(uw)::value, RL = decltype(rl)::value;
            // no LDS table where no per-edge relation operand is read: d_relation (rows are relations), d_input of add / add
            if constexpr (RL && (KIND == KIND_DREL || (KIND == KIND_DX && SUM == ULTRA_SUM_ADD && MUL == ULTRA_MUL_ADD)))
                return (int)ULTRA_ERR_BAD_OP;
            else {
                LaunchRecord rec;
                rec.family = FAM_GENERAL; rec.kind = KIND; rec.sum = SUM; rec.mul = MUL; rec.unit_w = UW; rec.rel_lds = RL;
                return launch_recorded(rec, segment_kernel<KIND, SUM, MUL, UW, RL>, p, path.grid, path.lds, stream, kBlock);
            }
        });
    });
}

}  // namespace

int ultra_detail::launch_general(int kind, int sum_op, int mul_op, const KParams &p, const PlanPath &path, hipStream_t stream) {
    return with_kind(kind, [&](auto k) {
        return with_sum_mul(sum_op, mul_op, [&](auto sum, auto mul) {
            return ::launch_general<decltype(k)::value, decltype(sum)::value, decltype(mul)::value>(p, path, stream);
        });
    });
}

// ultra_torchdrug_amd/csrc/plan_packed.hip -- the packed plan kernel, one chunk per wave (launch_packed).
//
// Packed fast path (forward, and d_input for sum=add): segment_kernel's walk (plan_general.hip), leaner instruction stream.
// The general kernel spends ~10 scalar-ALU/branch instructions per edge (three metadata words, a 64-bit
// row address, a row-change test); the CU issues one scalar instruction per cycle, so that, not memory, bounds
// it.  Here one 32-bit word per edge carries everything:
//     bits [0,8)            row - chunk.row_begin   (chunks hold <= 256 rows; pieces: 0)
//     bits [8, 8+bitsR)     relation id  -> (word & rel_mask) is directly the LDS byte offset rel * 256
//     bits [src_shift, 32)  gathered node id
// the gather is a buffer_load_dword with a 32-bit scalar byte offset (node * row_bytes: one s_lshr + one
// s_mul_i32), and a batch of 8 edges whose last edge is still in the current row skips all row tests.
#include <hip/hip_runtime.h>
#include <type_traits>

#include <cstdint>

#include "device_common.h"
#include "plan_kernels.h"

namespace {

using namespace ultra_detail;

// VAR 0: node id inside the packed word, relation tile in LDS (KG-sized graphs).
// VAR 1: as 0, and the gathered matrix's tile staged in LDS too (rows * 256 B next to the relation tile in 156 KB:
//        the relation graphs, 2R nodes) -- every gather is then a conflict-free ds_read_b32.
// VAR 2: big graphs -- ids do not fit one word: word = row delta | relation << 8, the node id comes from the plan's
//        node_a array (second scalar load per batch); relation row through a buffer load (table too big for LDS).
// VAR 3: as 2 with the relation tile in LDS.
// VAR 4: as 0, plus a software-managed cache of HOT gathered rows in the LDS left over next to the relation tile: the
//        plan lists the n_hot most frequently gathered nodes (KGs are heavy-tailed: the 140 hottest sources of the
//        FB15k237-shaped graph feed 49 % of its edges); the word's node field holds the cache slot for those and
//        n_hot + node for the rest, so a hot edge costs a ds_read_b32 instead of a trip through TA / L2.
// UN: gathers in flight per wave (8; 16 measured slower for cache-resident and for DRAM-resident graphs alike).
template <int KIND, int SUM, int MUL, bool UNIT_W, int VAR, int UN = kUnroll>
__global__ __launch_bounds__(kBlock) void packed_kernel(const PParams p) {
    constexpr bool X_LDS = (VAR == 1);
    constexpr bool BIG = (VAR == 2 || VAR == 3);
    constexpr bool REL_GLOBAL = (VAR == 2);
    constexpr bool HOT = (VAR == 4);
    static_assert(VAR == 0 || KIND != KIND_DREL, "variants 1-4 are for the single-gather kinds");
    static_assert(KIND == KIND_FWD || SUM == ULTRA_SUM_ADD, "packed path: forward, or the backward of sum-aggregation");
    constexpr int RED = (KIND == KIND_FWD) ? SUM : ULTRA_SUM_ADD;
    // forward / d_input: second operand = relation row (LDS).  d_relation (rows = relations): second operand =
    // input[src] (a second gather, only for mul), first = output_grad[dst] addressed by the meta2 word.
    constexpr bool NEEDS_REL = (KIND == KIND_FWD) || (KIND == KIND_DX && MUL == ULTRA_MUL_MUL);
    constexpr bool TWO_GATHERS = (KIND == KIND_DREL);
    extern __shared__ __attribute__((aligned(16))) float lds_raw[];
    int *ticket = reinterpret_cast<int *>(lds_raw);                 // first kLdsHeader bytes
    float *lds_rel = lds_raw + kLdsHeader / sizeof(float);
    const int lane = threadIdx.x & 63;
    const int label = blockIdx.x % kXcd;
    const int bl = blockIdx.x / kXcd;
    const int nb = p.blocks_per_label;
    const long long F = p.F;
    const __amdgpu_buffer_rsrc_t rsrc =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(p.gather), 0, p.gather_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t rsrc2 =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(TWO_GATHERS ? p.gather2 : p.gather), 0,
                                          TWO_GATHERS ? p.gather2_bytes : p.gather_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t rsrc_rel =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(p.relation), 0, p.relation_bytes, 0x00020000);

    for (int s = label; s < p.n_slots; s += kXcd) {
        const int tile = s / p.split;
        const int part = s - tile * p.split;
        const long long col = (long long)tile * kTile + lane;
        const bool active = col < F;
        const uint32_t voff = (uint32_t)((active ? col : F - 1) * 4);
        float *lds_x = lds_rel + (NEEDS_REL ? p.n_rel * kTile : 0);
        if constexpr (NEEDS_REL && !REL_GLOBAL) {
            const int total = p.n_rel * kTile;
            for (int i = threadIdx.x; i < total; i += kBlock) {
                const int r = i >> 6;
                const long long c = (long long)tile * kTile + (i & 63);
                lds_rel[i] = (c < F) ? p.relation[(long long)r * F + c] : 0.0f;
            }
        }
        if constexpr (X_LDS) {
            const int total = p.n_gather_rows * kTile;
            for (int i = threadIdx.x; i < total; i += kBlock) {
                const int r = i >> 6;
                const long long c = (long long)tile * kTile + (i & 63);
                lds_x[i] = (c < F) ? p.gather[(long long)r * F + c] : 0.0f;
            }
        }
        if constexpr (HOT) {   // hot-row cache: the tile segments of the plan's hot nodes
            const int total = p.n_hot * kTile;
            for (int i = threadIdx.x; i < total; i += kBlock) {
                const long long r = p.hot_nodes[i >> 6];
                const long long c = (long long)tile * kTile + (i & 63);
                lds_x[i] = (c < F) ? p.gather[r * F + c] : 0.0f;
            }
        }
        if (threadIdx.x == 0) *ticket = 0;
        __syncthreads();
        const char *lds_lane = reinterpret_cast<const char *>(lds_rel) + lane * 4;
        const char *lds_x_lane = reinterpret_cast<const char *>(lds_x) + lane * 4;
        // one gather: a 256-B row segment of `gather`, from LDS (X_LDS) or through a buffer load with a scalar offset
        auto gather_one = [&](uint32_t word) -> float {
            if constexpr (X_LDS) {
                return *reinterpret_cast<const float *>(lds_x_lane + ((word >> p.src_shift) << 8));
            } else if constexpr (HOT) {
                const uint32_t g = word >> p.src_shift;       // wave-uniform: a scalar branch
                if (g < (uint32_t)p.n_hot) return *reinterpret_cast<const float *>(lds_x_lane + (g << 8));
                return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(
                                                     rsrc, voff, (g - (uint32_t)p.n_hot) * p.row_bytes, 0));
            } else {
                return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(
                                                     rsrc, voff, (word >> p.src_shift) * p.row_bytes, 0));
            }
        };

        int b_node = -1;          // sparse boundary of this lane's column
        float b_val = 0.0f;
        if (KIND == KIND_FWD && p.bnode != nullptr && active) {
            b_node = p.bnode[col / p.bdim];
            b_val = p.bvec[col];
        }
        auto store_row = [&](int r, float v) {
            if (active) {
                if constexpr (KIND != KIND_DREL) {
                    if (p.add_rows != nullptr) v = reduce<RED>(v, p.add_rows[(long long)r * F + col]);
                    else if (KIND == KIND_FWD && p.bnode != nullptr) v = reduce<RED>(v, (r == b_node) ? b_val : 0.0f);
                }
                __builtin_nontemporal_store(v, &p.out[(long long)r * F + col]);   // streaming: keep the gathered rows in L2
            }
        };
        auto contribute = [&](float acc, float rv, float gv, float w) -> float {
            if constexpr (KIND == KIND_FWD) {
                float y = binary<MUL>(rv, gv);
                if constexpr (!UNIT_W) y = w * y;
                return reduce<RED>(acc, y);
            } else {
                float c = gv;
                if constexpr (!UNIT_W) c = c * w;
                if constexpr (MUL == ULTRA_MUL_MUL) c = c * rv;
                return acc + c;
            }
        };

        for (;;) {   // static serpentine deal across workgroups, LDS ticket counter within one (see segment_kernel)
            int t = 0;
            if (lane == 0) t = __hip_atomic_fetch_add(ticket, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            t = uniform(t);
            const int k = part + p.split * (t * nb + ((t & 1) ? (nb - 1 - bl) : bl));
            if (k >= p.n_chunks) break;
            const int4 d = p.chunks[uniform(k)];
            const uint32_t *meta = p.meta + d.x;
            const uint32_t *meta2 = (TWO_GATHERS || BIG) ? p.meta2 + d.x : nullptr;
            const float *wts = UNIT_W ? nullptr : p.weight + d.x;
            const int n = d.y - d.x;
            const bool is_piece = d.w < 0;
            const int row_base = d.z;
            uint32_t cur = 0;
            float acc = identity<RED>();
            int e0 = 0;
            for (; e0 + UN <= n; e0 += UN) {
                uint32_t m[UN];
                float wv[UN], gv[UN], rv[UN];
                uint32_t m2[UN];
#pragma unroll
                for (int u = 0; u < UN; ++u) {
                    m[u] = meta[e0 + u];
                    m2[u] = 0;
                    if constexpr (TWO_GATHERS || BIG) m2[u] = meta2[e0 + u];
                    wv[u] = 1.0f;
                    if constexpr (!UNIT_W) wv[u] = wts[e0 + u];
                }
#pragma unroll
                for (int u = 0; u < UN; ++u) {
                    if constexpr (TWO_GATHERS) {
                        gv[u] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rsrc2, voff, m2[u] * p.row_bytes, 0));
                    } else if constexpr (BIG) {
                        gv[u] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rsrc, voff, m2[u] * p.row_bytes, ULTRA_BIG_GATHER_AUX));
                    } else {
                        gv[u] = gather_one(m[u]);
                    }
                }
#pragma unroll
                for (int u = 0; u < UN; ++u) {
                    rv[u] = 0.0f;
                    if constexpr (NEEDS_REL && REL_GLOBAL)
                        rv[u] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rsrc_rel, voff, (m[u] >> 8) * p.row_bytes, 0));
                    if constexpr (NEEDS_REL && !REL_GLOBAL) rv[u] = *reinterpret_cast<const float *>(lds_lane + (m[u] & p.rel_mask));
                    if constexpr (TWO_GATHERS && MUL == ULTRA_MUL_MUL)
                        rv[u] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(
                                                              rsrc, voff, (m[u] >> p.src_shift) * p.row_bytes, 0));
                }
                if ((m[UN - 1] & 0xffu) == cur) {   // whole batch in the current row (always true for pieces)
#pragma unroll
                    for (int u = 0; u < UN; ++u) acc = contribute(acc, rv[u], gv[u], wv[u]);
                } else {
#pragma unroll
                    for (int u = 0; u < UN; ++u) {
                        const uint32_t dl = m[u] & 0xffu;
                        if (dl != cur) {
                            store_row(row_base + (int)cur, acc);
                            for (uint32_t q = cur + 1; q < dl; ++q) store_row(row_base + (int)q, identity<RED>());
                            cur = dl;
                            acc = identity<RED>();
                        }
                        acc = contribute(acc, rv[u], gv[u], wv[u]);
                    }
                }
            }
            if (e0 < n) {   // tail: fewer than UN edges
                const int rem = n - e0;
                uint32_t m[UN];
                float wv[UN], gv[UN], rv[UN];
                uint32_t m2[UN];
#pragma unroll
                for (int u = 0; u < UN; ++u) {
                    const int e = e0 + min(u, rem - 1);
                    m[u] = meta[e];
                    m2[u] = 0;
                    if constexpr (TWO_GATHERS || BIG) m2[u] = meta2[e];
                    wv[u] = 1.0f;
                    if constexpr (!UNIT_W) wv[u] = wts[e];
                }
#pragma unroll
                for (int u = 0; u < UN; ++u) {
                    if constexpr (TWO_GATHERS) {
                        gv[u] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rsrc2, voff, m2[u] * p.row_bytes, 0));
                    } else if constexpr (BIG) {
                        gv[u] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rsrc, voff, m2[u] * p.row_bytes, ULTRA_BIG_GATHER_AUX));
                    } else {
                        gv[u] = gather_one(m[u]);
                    }
                }
#pragma unroll
                for (int u = 0; u < UN; ++u) {
                    rv[u] = 0.0f;
                    if constexpr (NEEDS_REL && REL_GLOBAL)
                        rv[u] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rsrc_rel, voff, (m[u] >> 8) * p.row_bytes, 0));
                    if constexpr (NEEDS_REL && !REL_GLOBAL) rv[u] = *reinterpret_cast<const float *>(lds_lane + (m[u] & p.rel_mask));
                    if constexpr (TWO_GATHERS && MUL == ULTRA_MUL_MUL)
                        rv[u] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(
                                                              rsrc, voff, (m[u] >> p.src_shift) * p.row_bytes, 0));
                }
#pragma unroll
                for (int u = 0; u < UN; ++u) {
                    if (u < rem) {
                        const uint32_t dl = m[u] & 0xffu;
                        if (dl != cur) {
                            store_row(row_base + (int)cur, acc);
                            for (uint32_t q = cur + 1; q < dl; ++q) store_row(row_base + (int)q, identity<RED>());
                            cur = dl;
                            acc = identity<RED>();
                        }
                        acc = contribute(acc, rv[u], gv[u], wv[u]);
                    }
                }
            }
            if (is_piece) {
                if (active) p.partial[(long long)(-d.w - 1) * F + col] = acc;
            } else {
                store_row(row_base + (int)cur, acc);
                for (int q = row_base + (int)cur + 1; q < d.w; ++q) store_row(q, identity<RED>());
            }
        }
        __syncthreads();   // all tickets drawn, tables no longer read
    }
}

template <int KIND, int SUM, int MUL>
int launch_packed(const PParams &p, const PlanPath &path, hipStream_t stream) {
    return with_bool(path.unit_w, [&](auto uw) {
        auto go = [&](auto var) {
            constexpr int V = decltype(var)::value;
            constexpr int UN = (V == 2 || V == 3) ? kUnrollBig : kUnroll;
            constexpr bool UW = decltype(uw)::value;
            // d_input of add / add reads no relation operand: a wide-id plan never takes the form without the LDS tile
            if constexpr (KIND == KIND_DX && MUL == ULTRA_MUL_ADD && V == 2) return (int)ULTRA_ERR_BAD_OP;
            else {
                LaunchRecord rec;
                rec.family = FAM_PACKED; rec.kind = KIND; rec.sum = SUM; rec.mul = MUL; rec.unit_w = UW; rec.var = V; rec.unroll = UN;
                return launch_recorded(rec, packed_kernel<KIND, SUM, MUL, UW, V, UN>, p, path.grid, path.lds, stream, kBlock);
            }
        };
        if constexpr (KIND == KIND_DREL) return go(std::integral_constant<int, 0>{});      // the plain form only
        else return with_int<0, 1, 2, 3, 4>(path.var, go);
    });
}

}  // namespace

int ultra_detail::launch_packed(int kind, int sum_op, int mul_op, const PParams &p, const PlanPath &path, hipStream_t stream) {
    return with_kind(kind, [&](auto k) {
        constexpr int K = decltype(k)::value;
        return with_fast_ops<K>(sum_op, mul_op, [&](auto sum, auto mul) {
            return ::launch_packed<K, decltype(sum)::value, decltype(mul)::value>(p, path, stream);
        });
    });
}

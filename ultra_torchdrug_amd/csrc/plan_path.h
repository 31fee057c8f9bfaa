// plan_path.h -- which kernel a reduction plan runs, as a pure function (internal to libultra_rspmm.so).
//
// Plain C++17: nothing from HIP, no globals, no getenv, no heap.  Pointers are seen only as "present" and "16-byte aligned"
// flags, so tests/plan_path_main.cpp compiles this header with the host compiler alone and tests/test_plan_path_cpu.py pins
// every branch without a GPU.  run_plan (rspmm_kernels.hip) fills a PlanInput, calls plan_path() and launches by a switch on
// the result; ultra_rspmm_fwd_f32, layer_launch (layer_fused.hip) and run_rotate_plan (rotate.inc) share the tiling helpers.
#ifndef ULTRA_PLAN_PATH_H
#define ULTRA_PLAN_PATH_H

#include <cstddef>
#include <cstdint>

#include "ultra_rspmm.h"

namespace ultra_detail {

constexpr int kTile = 64;                  // columns per tile == wave width
constexpr int kXcd = 8;
constexpr int kMaxLdsBytes = 156 * 1024;   // leave a little of the 160 KiB
constexpr int kLdsHeader = 16;             // bytes in front of the tables: the workgroup's chunk ticket counter
constexpr int kPlanBlock = 1024;           // threads per workgroup of the chunked kernels (plan_kernels.h kBlock)
constexpr int kPlanRgBlock = 512;          // ... of rowgroup_kernel (rowgroup.inc kRgBlock)

enum Kind { KIND_FWD = 0, KIND_DX = 1, KIND_DREL = 2 };
enum Family { FAM_DENSE = 0, FAM_ROWGROUP = 1, FAM_QUAD = 2, FAM_PACKED = 3, FAM_GENERAL = 4 };
enum RelMode { REL_L2 = 0, REL_LDS = 1, REL_PART = 2 };        // where a rowgroup tile's relation rows are read from
enum ActMode { ACT_NONE = 0, ACT_BITS = 2, ACT_NODE = 3 };     // quad.inc ACT (1, the d_input form, is not dispatched)
enum UnrollClass { UNROLL_U = 0, UNROLL_UW = 1, UNROLL_UX = 2 };   // kQuadU / kQuadUW / kQuadUX
enum Fixup { FIX_NONE = 0, FIX_PLAIN = 1, FIX_MANY = 2 };

// ultra_rspmm_force_general_path, decoded (bit meanings: include/ultra_rspmm.h)
struct Knobs {
    bool force_general = false;         // bit 0: general kernel instead of the packed one
    bool no_x_lds = false;              // bit 1: packed kernel without staging the gathered matrix in LDS
    bool no_quad = false;               // bit 2: one chunk per wave (packed_kernel) instead of four (quad_kernel)
    bool no_rowgroup = false;           // bit 3: chunked kernels where one row per group (rowgroup_kernel) would run
    bool wide_groups = false;           // bit 4: rowgroup_kernel with 32 / 64 lanes per row even for cache-sized inputs
    bool no_concurrent_tiles = false;   // bit 5: quad_kernel walks a label's column tiles one after the other
    bool no_dense = false;              // bit 6: the edge list of a plan that carries a dense form (relgraph_dense.hip)
    bool no_dead_words = false;         // bit 7: the weighted kernels even where a plan carries marked words (packed_dead)
    bool no_paired = false;             // bit 8: the layer epilogue never as combine_paired_kernel (one wave per SIMD instead)
    bool force_paired = false;          // bit 9: combine_paired_kernel at every size (it runs large inputs only)
    bool score_lds_rows = false;        // bit 10: score_kernel<false>, the column-per-lane product with its LDS row phase
    bool combine_lds_rows = false;      // bit 11: combine_paired_kernel_lds, the column-per-lane product with its LDS row phase
};

inline Knobs decode_knobs(int mask) {
    Knobs k;
    k.force_general = (mask & 1) != 0;
    k.no_x_lds = (mask & 2) != 0;
    k.no_quad = (mask & 4) != 0;
    k.no_rowgroup = (mask & 8) != 0;
    k.wide_groups = (mask & 16) != 0;
    k.no_concurrent_tiles = (mask & 32) != 0;
    k.no_dense = (mask & 64) != 0;
    k.no_dead_words = (mask & 128) != 0;
    k.no_paired = (mask & 256) != 0;
    k.force_paired = (mask & 512) != 0;
    k.score_lds_rows = (mask & 1024) != 0;
    k.combine_lds_rows = (mask & 2048) != 0;
    return k;
}

inline int gcd_int(int a, int b) {
    while (b) {
        const int t = a % b;
        a = b;
        b = t;
    }
    return a;
}

// Persistent, XCD-aware grid over column tiles: label = blockIdx % 8 owns whole tiles; `split` parts per tile so that every
// label has work whatever n_tiles is.
struct TileGeometry {
    int n_tiles = 0, split = 0, n_slots = 0, blocks_per_label = 0, grid = 0;
};

inline TileGeometry tile_geometry(long long columns, int width, int n_cu) {
    TileGeometry g;
    g.n_tiles = (int)((columns + width - 1) / width);
    g.split = kXcd / gcd_int(g.n_tiles, kXcd);
    g.n_slots = g.n_tiles * g.split;
    g.blocks_per_label = (n_cu + kXcd - 1) / kXcd;
    g.grid = g.blocks_per_label * kXcd;
    return g;
}

// The tiling of rowgroup_kernel and of rowgroup_layer_kernel (one row per 16 / 32 / 64-lane group, column tiles of 64 / 128 /
// 256).  lds_base: bytes in front of the relation rows; lds_room: bytes the relation rows may take.
struct RowGroupTiling {
    int group = 16;
    int rel_mode = REL_L2;
    int n_rel_lds = 0;
    TileGeometry geo;
    size_t lds = 0;
};

inline RowGroupTiling rowgroup_tiling(long long F, long long gather_rows, long long n_rows, long long n_rel, int n_cu,
                                      bool wide_groups, size_t lds_base, size_t lds_room) {
    RowGroupTiling t;
    // Wide groups only where the gathered matrix cannot be cache-resident (beyond the 256 MB Infinity Cache): there one
    // contiguous fetch per edge beats L2 locality of 64-column tiles.
    const bool dram = wide_groups || (double)gather_rows * (double)F * 4.0 > 256.0 * 1024 * 1024;
    t.group = (dram && F % 256 == 0) ? 64 : ((dram && F % 128 == 0) ? 32 : 16);
    const int width = 4 * t.group;
    t.geo = tile_geometry(F, width, n_cu);
    // a part's rows are stored through one buffer descriptor with 32-bit offsets: keep rows_per_part * row bytes < 4 GiB
    while ((n_rows + t.geo.split - 1) / t.geo.split * F * 4 >= (1LL << 32) - 65536 && t.geo.split < (1 << 20)) t.geo.split *= 2;
    t.geo.n_slots = t.geo.n_tiles * t.geo.split;
    // Relation rows: from LDS when the tile's table fits; else the first rows of the table from LDS and the rest through
    // L2, when that is at least a quarter of the rows (every row served from LDS is one gather less through the
    // texture path the input rows need; measured on S-stress, 1 000 relations: 624 rows of a 64-column tile in LDS
    // 5.96 -> 5.67 ms, 312 rows of a 128-column tile 11.9 -> 11.1 ms, 156 rows of a 256-column tile 23.8 -> 24.1 ms).
    const size_t row_bytes = (size_t)width * sizeof(float);
    const size_t lds_need = (size_t)n_rel * row_bytes;
    const int part_rows = (int)(lds_room / row_bytes);
    t.lds = lds_base;
    if (n_rel > 0 && lds_need <= lds_room) {
        t.rel_mode = REL_LDS;
        t.n_rel_lds = (int)n_rel;
        t.lds += lds_need;
    } else if (n_rel > 0 && (long long)part_rows * 4 >= n_rel) {
        t.rel_mode = REL_PART;
        t.n_rel_lds = part_rows;
        t.lds += (size_t)part_rows * row_bytes;
    }
    return t;
}

// 16-byte alignment of the call's pointers, one bit each (a NULL pointer counts as aligned)
enum Aligned {
    AL_INPUT = 1, AL_GRAD = 2, AL_OUT = 4, AL_RELATION = 8, AL_ADD_ROWS = 16, AL_PARTIAL = 32, AL_BVEC = 64, AL_ALL = 127
};

// What run_plan knows about one call before it launches anything.
struct PlanInput {
    int kind = KIND_FWD, sum_op = ULTRA_SUM_ADD, mul_op = ULTRA_MUL_MUL;
    long long F = 0, n_rel = 0, gather_rows = 0, gather2_rows = 0;
    // the plan (ultra_segments): optional arrays as flags
    bool has_weight = false, has_node_b = false, has_row_ptr = false, has_packed = false, has_packed_dead = false,
         has_dense = false;
    long long packed_src_shift = 0, n_rows = 0, n_edges = 0, n_long_rows = 0, n_pieces = 0, n_hot = 0, dense_rows = 0,
              dense_cols = 0;
    // the call
    bool has_add_rows = false, has_bnode = false;
    int bdim = 0;
    bool has_act_bits = false, has_act_node = false;
    int act_words = 0;
    bool has_workspace = false;
    size_t workspace_bytes = 0;
    unsigned aligned = AL_ALL;
    // the process and the device
    Knobs knobs;
    int n_cu = 0;
    bool gfx950 = false;
};

// Everything a launch needs that is not a pointer.
struct PlanPath {
    int status = ULTRA_OK;
    int family = FAM_GENERAL;
    bool unit_w = false;            // the kernel's UNIT_W form (no weights, or the marked words of `dead`)
    int var = 0;                    // packed / quad: 0 plain, 1 gathered matrix in LDS, 2 / 3 wide ids without / with the
                                    //   relation tile in LDS, 4 hot-row cache
    bool x_lds = false, dead = false;   // quad
    int act = ACT_NONE;
    int unroll = UNROLL_U;
    int concurrent = 1;
    bool rel_lds = false;           // general: the relation tile in LDS
    int group = 0, rel_mode = REL_L2, n_rel_lds = 0;   // rowgroup
    TileGeometry geo;
    int grid = 0, block = 0;
    size_t lds = 0;
    int fixup = FIX_NONE, fixup_grid = 0;
};

inline void set_rowgroup(PlanPath &r, const RowGroupTiling &t) {
    r.family = FAM_ROWGROUP;
    r.group = t.group; r.rel_mode = t.rel_mode; r.n_rel_lds = t.n_rel_lds;
    r.geo = t.geo; r.grid = t.geo.grid; r.block = kPlanRgBlock; r.lds = t.lds;
}

// Is the plan's dense form usable for this call?  (what include/ultra_rspmm.h lists as preconditions, knobs aside)
inline bool dense_applies(const PlanInput &c) {
    if (!c.has_dense || c.has_weight || c.sum_op != ULTRA_SUM_ADD || c.n_rel != 4) return false;
    if (c.F % 16 != 0 || c.F * 4 >= (1LL << 24)) return false;
    if (c.dense_cols != c.gather_rows || c.gather_rows * c.F * 4 >= (1LL << 31)) return false;
    if (c.kind == KIND_DREL) {
        if (c.mul_op != ULTRA_MUL_MUL || c.n_rows != 4 || c.dense_rows != c.gather2_rows) return false;
        const long long n_vt = (c.dense_rows + 15) / 16;
        if (!c.has_workspace || c.workspace_bytes < (size_t)(n_vt * 4 * c.F) * sizeof(float)) return false;
    } else {
        if (c.dense_rows != c.n_rows) return false;
        if (c.kind == KIND_FWD && !c.has_add_rows && c.has_bnode && c.bdim <= 0) return false;
    }
    return true;
}

// ULTRA_CONC / ULTRA_CONC_MIN_ROWS (experiments, tools/conc_ab.sh): force the number of concurrent tiles of a quad launch;
// min_rows: only for gathered matrices of at least that many rows, i.e. not the relation graphs.  The caller reads the
// environment, and only for a quad path, as it always did.
inline void force_concurrent(PlanPath &path, int want, bool has_min_rows, long long min_rows, long long gather_rows) {
    if (path.family == FAM_QUAD && want >= 1 && path.geo.blocks_per_label % want == 0 && (!has_min_rows || gather_rows >= min_rows))
        path.concurrent = want;
}

// Precondition: the arguments passed run_plan's validation and the plan has rows.
inline PlanPath plan_path(const PlanInput &in) {
    PlanPath r;
    const int kind = in.kind;
    const long long F = in.F, n_rel = in.n_rel;
    const Knobs &k = in.knobs;
    auto aligned = [&](unsigned bits) { return (in.aligned & bits) == bits; };
    const unsigned al_gather = (kind == KIND_DX) ? AL_GRAD : AL_INPUT;
    const bool sum_add = in.sum_op == ULTRA_SUM_ADD, mul_mul = in.mul_op == ULTRA_MUL_MUL;
    const bool boundary_ok = !in.has_bnode || in.bdim % 4 == 0;

    r.geo = tile_geometry(F, kTile, in.n_cu);
    r.grid = r.geo.grid;
    r.block = kPlanBlock;
    r.unit_w = !in.has_weight;
    const size_t lds_need = (size_t)n_rel * kTile * sizeof(float);
    const bool rel_fits = n_rel > 0 && lds_need <= (size_t)kMaxLdsBytes;

    // dense relation graphs: the sum as a product with the plan's 0/1 matrix on the exact-f32 matrix cores -- the reference
    // order for every row, no pieces, no fix-up pass (relgraph_dense.hip)
    // (only on the architecture the instruction's summation order was probed on -- tools/ubench/mfma_order.hip, MI355X: a build
    // with ARCH=gfx942 walks the edge list -- and for finite operands only: fmaf(0, y, acc) == acc needs a finite y, so ONE
    // non-finite activation turns every row of a dense launch into NaN where the edge walk and the reference touch that node's
    // neighbours only; the eager callers test their relation tables as the frontier path does)
    if (in.has_dense && !k.no_dense && !k.force_general && !k.no_quad && !k.no_x_lds && in.gfx950 && dense_applies(in)) {
        r.family = FAM_DENSE;        // (grid and block are dense_launch's own)
        return r;
    }

    // big graphs of short rows (node ids outside the packed word, no split rows, row pointers present): one row per
    // 16-lane group (rowgroup.inc); same sequential order per row as every other kernel, so the same bits
    const bool big = in.packed_src_shift >= 32;          // node ids live in node_a, not in the packed word
    if (kind != KIND_DREL && !k.force_general && !k.no_rowgroup && in.has_row_ptr && big && in.n_long_rows == 0 && F % 4 == 0 &&
        (kind == KIND_FWD || sum_add) && aligned(al_gather | AL_OUT | AL_RELATION | AL_ADD_ROWS | AL_BVEC) && boundary_ok) {
        r.family = FAM_ROWGROUP;
        if (F >= (1LL << 30)) { r.status = ULTRA_ERR_BAD_SHAPE; return r; }   // row bytes are a 32-bit factor of the address arithmetic
        // d_input of sum-aggregation: the relation operand exists only for mul = mul
        const bool needs_rel = kind == KIND_FWD || mul_mul;
        const RowGroupTiling t = rowgroup_tiling(F, in.gather_rows, in.n_rows, needs_rel ? n_rel : 0, in.n_cu, k.wide_groups,
                                                 kLdsHeader, kMaxLdsBytes);
        set_rowgroup(r, t);
        return r;
    }

    if (in.n_long_rows > 0) {
        const bool red_add = kind != KIND_FWD || sum_add;
        const bool many_pieces = in.n_pieces >= 128 * in.n_long_rows;       // on average >= 128 pieces per split row
        r.fixup = (red_add && many_pieces) ? FIX_MANY : FIX_PLAIN;
        r.fixup_grid = (int)((in.n_long_rows * r.geo.n_tiles + 3) / 4);
    }

    // packed fast path: forward and sum-backward d_input, when the plan carries packed words, the relation
    // tile fits LDS and the gathered matrix is addressable with a 32-bit byte offset
    // (forward gathers `input`; d_input gathers `output_grad`; d_relation gathers both: grad by node_b, input by node_a)
    const unsigned long long gather_bytes = (unsigned long long)in.gather_rows * (unsigned long long)F * 4ull;
    const unsigned long long gather2_bytes = (unsigned long long)in.gather2_rows * (unsigned long long)F * 4ull;
    const unsigned long long relation_bytes = (unsigned long long)n_rel * (unsigned long long)F * 4ull;
    const bool lds_ok = kind == KIND_DREL || rel_fits || (big && relation_bytes < 0xffff0000ull && n_rel > 0);
    const bool use_packed = !k.force_general && in.has_packed && (kind == KIND_FWD || sum_add) && lds_ok &&
                            gather_bytes < 0xffff0000ull && gather2_bytes < 0xffff0000ull &&
                            (unsigned long long)F * 4ull < 0x7fffffffull && (kind != KIND_DREL || (in.has_node_b && !big));
    if (!use_packed) {
        r.family = FAM_GENERAL;
        // (d_relation: rows are relations -- no per-edge relation operand, no LDS table)
        const bool wants_rel_lds = kind == KIND_FWD || (kind == KIND_DX && (mul_mul || !sum_add));
        r.rel_lds = wants_rel_lds && rel_fits;
        r.lds = kLdsHeader + (r.rel_lds ? lds_need : 0);
        return r;
    }

    const bool needs_rel = kind == KIND_FWD || (kind == KIND_DX && mul_mul);
    // small gathered matrix (relation graphs: 2R nodes): stage its tile in LDS next to the relation tile
    const size_t lds_x_bytes = (size_t)in.gather_rows * kTile * sizeof(float);
    size_t lds_bytes = needs_rel ? lds_need : 0;
    if (big) {
        r.var = (needs_rel && !rel_fits) ? 2 : 3;
        if (r.var == 2) lds_bytes = 0;
    } else if (in.n_hot > 0) {
        // the plan's words address a hot-row cache: its rows must fit next to the relation tile
        const size_t hot_bytes = (size_t)in.n_hot * kTile * sizeof(float);
        if (lds_bytes + hot_bytes > (size_t)kMaxLdsBytes) { r.family = FAM_PACKED; r.status = ULTRA_ERR_BAD_SHAPE; return r; }
        r.var = 4;
        lds_bytes += hot_bytes;
    } else if ((kind != KIND_DREL || mul_mul) && !k.no_x_lds && in.gather_rows > 0 && lds_bytes + lds_x_bytes <= (size_t)kMaxLdsBytes) {
        r.var = 1;       // d_relation: the `input` rows (picked by source node) from LDS, output_grad stays a gather
        lds_bytes += lds_x_bytes;
    }
    // four chunks per wave, four columns per lane (quad.inc): needs 16-byte rows and pointers, and descriptors (words with
    // their PACK_SLACK of 16, output) below 4 GiB
    const bool meta_ok = ((unsigned long long)in.n_edges + 16ull) * 4ull < 0xffff0000ull;
    const bool out_ok = (unsigned long long)in.n_rows * (unsigned long long)F * 4ull < 0xffff0000ull;
    const bool quad = !k.no_quad && (r.var == 0 || r.var == 1) && F % 4 == 0 && out_ok && meta_ok &&
                      (unsigned long long)F * 4ull < (1ull << 24) && (kind != KIND_DREL || in.gather2_rows < (1ll << 24)) &&
                      aligned(al_gather | AL_GRAD | AL_OUT | AL_ADD_ROWS | AL_PARTIAL | AL_BVEC) && boundary_ok;
    if (!quad) {
        r.family = FAM_PACKED;
        if (kind == KIND_DREL) { r.var = 0; lds_bytes = 0; }     // packed_kernel's d_relation has the plain form only
        r.lds = kLdsHeader + lds_bytes;
        return r;
    }

    r.family = FAM_QUAD;
    // tiles of one label side by side (quad.inc): as many as the label has, while every team keeps >= 4
    // workgroups.  Measured on every shape tried (rocprofv3, F = 1 024 / 2 048): S-codexs 28.8 -> 19.7 us,
    // S-wn18rr 64.5 -> 60.6 / 172 -> 154 us, S-codexm 84.4 -> 80.8 us, S-fb15k237 246 -> 219 us -- also where
    // ONE tile's slice of the gathered matrix about fits the XCD's 4 MiB L2 and four do not (S-fb15k237: 4 x 3.7 MB).
    // There the walk one tile after the other fetches a third less beyond L2 (604 vs 930 MB, profiles/r04_l2_conc_ab.json)
    // and is still 40 us slower, 13 us per extra tile pass.  What that is NOT (profiles/quad_tile_order_ab.json, HIP
    // events, 226 us side by side): long pieces holding a pass up -- 263 us with piece_len = 128 and 32-edge chunks,
    // 266 / 270 / 263 us with 128 / 64 / 32-edge chunks at piece_len = 512, and no faster with the piece waves at raised
    // priority; the restaging of the relation tile per pass -- 16-byte loads took 2 us off each.  Unexplained and left as
    // measured; the slice shares L2 with 2.2 MB of edge words per pass, which was not separated.
    const int bpl = r.geo.blocks_per_label;
    const int slots_per_label = (r.geo.n_slots + kXcd - 1) / kXcd;
    while (!k.no_concurrent_tiles && r.concurrent * 2 <= slots_per_label && bpl % (r.concurrent * 2) == 0 && bpl / (r.concurrent * 2) >= 4)
        r.concurrent *= 2;
    // activity masks of the backward (quad.inc ACT), d_relation only: where the gathered matrix is not staged in LDS, the
    // bitmap fits behind the tables and a column tile is a query block.  The d_input form (ACT = 1) was built and measured:
    // that kernel is bound by its per-row epilogue (read-modify-write of the gradient it accumulates into) and per-edge issue,
    // not by its gathers -- 137 vs 138 us on the FB15k237-shaped graph, 156 vs 148 us on the WN18RR-shaped one with the mask --
    // so it is not dispatched; d_relation (two gathers per edge) gains 30-45 %.
    size_t act_bytes = 0;
    if (kind == KIND_DREL && r.var == 0 && F % kTile == 0) {
        if (in.has_act_bits && in.act_words > 0 && lds_bytes + (size_t)in.act_words * 4 <= (size_t)kMaxLdsBytes) {
            r.act = ACT_BITS;
            act_bytes = (size_t)in.act_words * 4;
        } else if (in.has_act_node && mul_mul) {
            r.act = ACT_NODE;      // (mul = add: d_relation does not depend on the input rows)
        }
    }
    // removed edges marked in a copy of the words (ultra_segments.packed_dead, quad.inc DEAD: removed edges by bit 31, every
    // other weight 1): the unit-weight kernel on those words
    r.dead = in.has_packed_dead && !k.no_dead_words && r.var == 0 && r.act != ACT_NODE && sum_add && mul_mul;
    if (r.dead) r.unit_w = true;
    r.x_lds = r.var == 1;
    // edges per group in flight: 8 would spill with per-edge weights (128 VGPRs at 16 waves per CU)
    r.unroll = !r.unit_w ? UNROLL_UW : (r.x_lds ? UNROLL_UX : UNROLL_U);
    r.lds = kLdsHeader + lds_bytes + act_bytes;
    return r;
}

}  // namespace ultra_detail

#endif

// plan_kernels.h -- what the translation units of the plan-kernel families share (internal): the kernels' parameter blocks,
// the constants a variant build can override with -D, the launch record's leaf, and the one launcher each family unit exports.
// run_plan (rspmm_kernels.hip) decides (plan_path.h), fills a parameter block and calls a launcher; the launcher's unit owns the
// family's kernels and instantiates exactly those a call can reach.
//
//     launch_general   plan_general.hip     segment_kernel
//     launch_packed    plan_packed.hip      packed_kernel
//     launch_quad      plan_quad.hip        quad_kernel (quad.inc)
//     launch_rowgroup  plan_rowgroup.hip    rowgroup_kernel (rowgroup.inc)
//     launch_fixup     epilogue.hip         fixup_kernel
// (plan_rotate.hip -- rotate.inc and its C entries -- dispatches outside plan_path() and exports no launcher.)
#ifndef ULTRA_PLAN_KERNELS_H
#define ULTRA_PLAN_KERNELS_H

#include "host_common.h"
#include "launch_record.h"

// Every macro below can be set through HIPFLAGS (variant builds: tools/kbench.py); each is defined here and nowhere else.
#ifndef ULTRA_BLOCK
#define ULTRA_BLOCK 1024
#endif
#ifndef ULTRA_UNROLL
#define ULTRA_UNROLL 8
#endif
#ifndef ULTRA_UNROLL_BIG
#define ULTRA_UNROLL_BIG 8
#endif
// cache policy of the big-graph gathers (aux of raw_buffer_load: 0 default, 2 nt): every row is touched ~10 times but far apart
#ifndef ULTRA_BIG_GATHER_AUX
#define ULTRA_BIG_GATHER_AUX 0
#endif

namespace ultra_detail {

constexpr int kBlock = ULTRA_BLOCK;            // threads per workgroup (1024: 16 waves, 4 per SIMD, 128 VGPRs each)
constexpr int kUnroll = ULTRA_UNROLL;          // gathers in flight per wave
constexpr int kUnrollBig = ULTRA_UNROLL_BIG;   // ... for the big-graph variants of packed_kernel (DRAM gathers; 16 measured 3 % slower); <= PACK_SLACK
static_assert(kBlock == kPlanBlock, "plan_path.h states the workgroup size of the chunked families");

struct KParams {
    const int32_t *row;
    const int32_t *node_a;
    const int32_t *node_b;
    const int32_t *rel;
    const float *weight;
    const int4 *chunks;
    const float *relation;   // [n_rel, F]
    const float *input;      // [n_src, F]
    const float *output;     // [n_dst, F]   (min/max backward only)
    const float *grad;       // [n_dst, F]   (backward only)
    const float *add_rows;   // [n_rows, F]  (forward only, optional fused epilogue)
    const int32_t *bnode;    // forward only: sparse form of add_rows -- row bnode[c / bdim] holds bvec[c] in column c,
    const float *bvec;       //   every other element is 0 (the Bellman-Ford boundary: ultra/model.py:106-107)
    int bdim;
    float *out;              // [n_rows, F]
    float *partial;          // [n_pieces, F]
    long long F;
    int n_chunks;
    int n_rel;
    int n_tiles;
    int split;
    int n_slots;
    int blocks_per_label;
    // backward, optional (see quad.inc ACT): which gradient / input rows are non-zero per 64-column tile
    const uint32_t *act_bits;   // [n_tiles][act_words] bitmap over destination nodes, or NULL
    int act_words;
    const int32_t *act_node;    // [n_tiles] the one source node whose input row is non-zero, or NULL
};

struct FixParams {
    const int32_t *long_rows;   // [n_long][3]
    const float *partial;
    const float *add_rows;
    const int32_t *bnode;
    const float *bvec;
    int bdim;
    float *out;
    long long F;
    int n_long;
    int n_tiles;
};

// packed_kernel / quad_kernel: one 32-bit word per edge carries everything (see plan_packed.hip)
struct PParams {
    const uint32_t *meta;
    const uint32_t *meta2;   // d_relation only: destination node of each edge (ultra_segments.node_b)
    const float *weight;
    const int4 *chunks;
    const float *relation;
    const float *gather;     // forward: input [n_src, F]; d_input: output_grad [n_dst, F]; d_relation: input
    const float *gather2;    // d_relation: output_grad [n_dst, F]
    const float *add_rows;
    const int32_t *bnode;    // sparse form of add_rows (see KParams)
    const float *bvec;
    int bdim;
    float *out;
    float *partial;
    long long F;
    uint32_t gather_bytes;
    uint32_t meta_bytes;     // quad_kernel: bytes of `meta` (and of `weight`): (n_edges + slack) * 4
    uint32_t meta2_bytes;    // quad_kernel: bytes of `meta2`: n_edges * 4
    uint32_t out_bytes;      // quad_kernel: bytes of `out` (and of `add_rows`): n_rows * F * 4
    uint32_t gather2_bytes;
    uint32_t relation_bytes;
    int n_gather_rows;
    const int32_t *hot_nodes;   // VAR 4: [n_hot] node ids whose rows are cached in LDS
    int n_hot;
    uint32_t row_bytes;
    uint32_t src_shift;
    uint32_t rel_mask;       // ((1 << bitsR) - 1) << 8
    int n_chunks;
    int n_rel;
    int n_tiles;
    int split;
    int n_slots;
    int blocks_per_label;
    int concurrent;          // quad_kernel: teams per label working on different column tiles at once (0 / 1: none)
    const uint32_t *act_bits;   // quad_kernel ACT = 1 / 2: [n_tiles][act_words]
    int act_words;
    const int32_t *act_node;    // quad_kernel ACT = 3: [n_tiles]
};

// rowgroup_kernel (rowgroup.inc)
struct RowGroupParams {
    const int32_t *row_ptr;     // [n_rows + 1]
    const int32_t *col;         // [E] gathered row of every edge
    const int32_t *rel;         // [E]
    const float *weight;        // [E] or NULL
    const float *relation;      // [n_rel, F]
    const float *gather;        // [n_cols, F]
    const float *add_rows;      // [n_rows, F] or NULL (fused epilogue, as in the plan kernels)
    const int32_t *bnode;       // sparse boundary (see KParams) or NULL
    const float *bvec;
    int bdim;
    float *out;                 // [n_rows, F]
    long long F;
    int n_rows;
    int n_rel;
    int n_rel_lds;              // relation rows held in LDS (all of them, or the first ones of a table too big for it)
    int n_tiles;                // column tiles of 4 G columns
    int split;                  // row parts per column tile, so that n_tiles * split is a multiple of the 8 XCD labels
    int n_slots;
    int blocks_per_label;
};

// What the plan runs of this thread launched (launch_record.h; ultra_rspmm_launch_records).  Host side only; runtime.hip.
extern thread_local LaunchRing g_launches;

// A launcher's leaf: `rec` names the template arguments of `kern` as the leaf instantiates it; the launch geometry is what
// goes to launch_with_lds and the tiling what the kernel's parameters hold.
template <typename Kern, typename Params>
int launch_recorded(LaunchRecord rec, Kern kern, const Params &p, int grid, size_t lds, hipStream_t stream, int block) {
    rec.grid = grid; rec.block = block; rec.lds = (int32_t)lds;
    rec.n_tiles = p.n_tiles; rec.split = p.split; rec.n_slots = p.n_slots; rec.blocks_per_label = p.blocks_per_label;
    LaunchRecord &slot = g_launches.push(rec);
    return slot.status = launch_with_lds(kern, p, grid, lds, stream, block);
}

// the kernels behind the rowgroup, quad and packed families: every operator pair forward, sum-aggregation backward
template <int KIND, typename Fn>
int with_fast_ops(int sum_op, int mul_op, Fn &&fn) {
    if constexpr (KIND == KIND_FWD) return with_sum_mul(sum_op, mul_op, fn);
    else return with_mul(mul_op, [&](auto mul) { return fn(std::integral_constant<int, ULTRA_SUM_ADD>{}, mul); });
}
template <typename Fn>
int with_kind(int kind, Fn &&fn) {
    return with_int<KIND_FWD, KIND_DX, KIND_DREL>(kind, fn);
}

// The launchers: the variant comes from plan_path()'s decision; kind / sum_op / mul_op are the run-time values of the kernels'
// leading template arguments (packed, quad and rowgroup backwards are sum-aggregation's whatever sum_op says, as with_fast_ops).
int launch_general(int kind, int sum_op, int mul_op, const KParams &p, const PlanPath &path, hipStream_t stream);
int launch_packed(int kind, int sum_op, int mul_op, const PParams &p, const PlanPath &path, hipStream_t stream);
int launch_quad(int kind, int sum_op, int mul_op, const PParams &p, const PlanPath &path, hipStream_t stream);
// backward: the d_input contribution order (sum-aggregation only); there is no d_relation form
int launch_rowgroup(int sum_op, int mul_op, bool backward, const RowGroupParams &p, const PlanPath &path, hipStream_t stream);
// fixup_kernel over the split rows, pieces added in piece order; noted in the record of the plan run launched just before
int launch_fixup(const FixParams &fp, int red, bool many_pieces, int grid, hipStream_t stream);

}  // namespace ultra_detail

#endif

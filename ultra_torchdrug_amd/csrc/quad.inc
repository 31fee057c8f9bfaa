// quad_kernel: the packed forward / d_input reduction with FOUR chunks per wave.  (included by plan_quad.hip, inside its anonymous namespace)
//
// packed_kernel gives a wave one chunk and a lane one column: every edge costs the wave ~9 instructions (3 scalar
// decode, 1 buffer_load_dword, 1 address add + 1 ds_read_b32, 1 mul, 1 add, wait/branch share) for 256 B of gather, and
// at 4 waves per SIMD the kernel is bound by instruction issue, not by L2 (profiles/r01_*: adding 7 instructions per
// edge made it 1.8x slower).  Here a wave is four 16-lane groups; a group owns a chunk of its own and a lane owns FOUR
// columns of the 64-column tile, so ONE buffer_load_dwordx4 / ds_read_b128 / v_pk_mul / v_pk_add serves four edges (one
// per group): ~3.5 instructions per edge.  Edge words are read per lane (the 16 lanes of a group read the same dword),
// addresses are per-lane VALU.  The four chunks of a wave are neighbours in the heaviest-first order (similar length);
// a group whose chunk ends early idles for the last batches.
//
// Summation order per output element is unchanged (edges of a row in plan order, pieces through the workspace), so the
// results are bit-identical to packed_kernel / segment_kernel and to the oracle with `piece = piece_len`.
// cache policy of the `out` stores (aux of raw_buffer_store): 0 = default, 2 = nt (streaming)
// ... and of the edge-word loads (read once per column tile, 4 B per edge)
#ifndef ULTRA_QUAD_WORD_AUX
#define ULTRA_QUAD_WORD_AUX 0
#endif
#ifndef ULTRA_QUAD_STORE_AUX
#define ULTRA_QUAD_STORE_AUX 2
#endif
// Experiment (VERDICT r4 item 2; default off, see DESIGN.md): gather each run of parallel edges once.  Consecutive edges of the
// (dst, src, rel)-sorted forward plan (and of the (src, dst, rel)-sorted d_input plan) that share the gathered node differ in
// their relation only; such an edge issues its gather past the end of the descriptor (returns 0, touches nothing) and takes the
// previous edge's row instead ((prev & kill) | loaded: one v_and_or_b32 per dword).  Same sums, same bits.
#ifndef ULTRA_QUAD_DEDUP
#define ULTRA_QUAD_DEDUP 0
#endif
// (qf4 / qu4, lds_read4 / lds_read1, reduce4 and identity4 -- the 16-lane groups' helpers, rowgroup.inc's too -- are
// device_common.h's.)

// ACT (backward of sum-aggregation only; round 4): the caller KNOWS that most gathered gradient rows are zero for this column
// tile, and says which are not -- 1: bitmap over the word's node (d_input: the destination whose output_grad row is gathered);
// 2: bitmap over the second gather's node (d_relation: the destination); 3: the word's node equals act_node[tile] (d_relation of
// the FIRST layer: the source whose input row is non-zero).  An inactive edge's gathers are issued past the end of their buffer
// descriptors -- they return 0.0 without touching memory -- and its contribution is the same (+-0) the full computation adds:
// identical bits, a fraction of the traffic.  One bitmap word read from LDS, a shift, a select and an OR per edge.  (ACT = 1 is
// kept as a template value but not dispatched: d_input is not bound by its gathers, see plan_path.h.)
// DEAD (round 5; sum aggregation with mul = mul, unit weights): the words are the plan's `packed_dead` copy -- bit 31 marks an edge the
// training step removed (weight 0 among weights of 1, ultra_edge_removal_marks).  A marked edge issues its gathers past the buffer
// descriptors: they return 0.0, the message is relation * 0 (forward), 0 * relation (d_input), 0 * 0 (d_relation) = (+-0), which is
// what the zero weight of the weighted form contributes (0 * message = +-0; adding either sign of zero to an accumulator that starts
// at +0 gives the same bits) -- without the weight loads, their hand-round and multiplies, and with 8 edges in flight instead of 6.
template <int KIND, int SUM, int MUL, bool UNIT_W, bool X_LDS, int U, int ACT = 0, bool DEAD = false>
__global__ __launch_bounds__(kBlock) void quad_kernel(const PParams p) {
    static_assert(KIND == KIND_FWD || SUM == ULTRA_SUM_ADD, "quad path: forward, or the backward of sum-aggregation");
    static_assert(!DEAD || (UNIT_W && !X_LDS && SUM == ULTRA_SUM_ADD && MUL == ULTRA_MUL_MUL && ACT != 1),
                  "marked words: unit weights, gathers through descriptors, summed DistMult messages");
    static_assert(ACT == 0 || (!X_LDS && ((KIND == KIND_DX && ACT == 1) || (KIND == KIND_DREL && (ACT == 2 || ACT == 3)))),
                  "activity masks: d_input by destination, d_relation by destination or by the tile's source node");
    constexpr int RED = (KIND == KIND_FWD) ? SUM : ULTRA_SUM_ADD;
    // forward / d_input: second operand = relation row (LDS).  d_relation (rows = relations): first operand =
    // output_grad[node_b] (meta2 word), second = input[node_a] (a second gather, only for mul)
    // X_LDS there (relation graphs: 2R nodes): the `input` rows, picked at random by source node, come from LDS; the
    // output_grad rows stay a gather (the plan is sorted by (rel, dst, src): consecutive edges share the row)
    constexpr bool TWO_GATHERS = (KIND == KIND_DREL);
    constexpr bool DIRECT_WORDS = X_LDS && !TWO_GATHERS;     // no gather instruction at all: plain per-lane word loads
    constexpr bool NEEDS_REL = (KIND == KIND_FWD) || (KIND == KIND_DX && MUL == ULTRA_MUL_MUL);
    extern __shared__ __attribute__((aligned(16))) float lds_raw[];
    int *ticket = reinterpret_cast<int *>(lds_raw);
    float *lds_rel = lds_raw + kLdsHeader / sizeof(float);
    const int lane = threadIdx.x & 63;
    const int grp = lane >> 4;
    const uint32_t lane_bytes = (uint32_t)(lane & 15) * 16u;     // this lane's 4 columns inside a 256-B tile row
    const int label = blockIdx.x % kXcd;
    // Small graphs: the workgroups of a label (an XCD) split into `conc` teams that work on `conc` of the label's column
    // tiles AT THE SAME TIME instead of all of them walking the tiles one after the other -- each team stages its tables
    // once and meets one slot barrier, where a tile holds only a chunk or two per 16-lane group (S-codexs: 4 tiles per
    // label, 1.6 chunks per group and tile).  Faster on every shape measured, also where the tiles' slices of the
    // gathered matrix no longer share the XCD's L2 (run_plan has the numbers).  Which team computes a tile never
    // enters a result.
    const int conc = p.concurrent > 1 ? p.concurrent : 1;
    const int team = (int)(blockIdx.x / kXcd) % conc;
    const int bl = (int)(blockIdx.x / kXcd) / conc;
    const int nb = p.blocks_per_label / conc;
    const long long F = p.F;
    const __amdgpu_buffer_rsrc_t rsrc =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(p.gather), 0, p.gather_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t rsrc_meta =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<uint32_t *>(p.meta), 0, p.meta_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t rsrc2 =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(TWO_GATHERS ? p.gather2 : p.gather), 0,
                                          TWO_GATHERS ? p.gather2_bytes : 0u, 0x00020000);
    const __amdgpu_buffer_rsrc_t rsrc_meta2 =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<uint32_t *>(TWO_GATHERS ? p.meta2 : p.meta), 0,
                                          TWO_GATHERS ? p.meta2_bytes : 0u, 0x00020000);
    const __amdgpu_buffer_rsrc_t rsrc_out = __builtin_amdgcn_make_buffer_rsrc(p.out, 0, p.out_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t rsrc_add =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(p.add_rows != nullptr ? p.add_rows : p.out), 0,
                                          p.add_rows != nullptr ? p.out_bytes : 0u, 0x00020000);
    const __amdgpu_buffer_rsrc_t rsrc_wt =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(UNIT_W ? p.gather : p.weight), 0, UNIT_W ? 0u : p.meta_bytes, 0x00020000);
    if ((uint32_t)(uintptr_t)(lds_char_ptr)lds_raw != 0u) __builtin_trap();
    // The relation tile is staged with 16-byte loads where the table is aligned (the one pointer the dispatch does not require
    // to be): the loop compiles to one load, a wait for it and one LDS write per round, so 474 relations (121 KB) were 30
    // round trips to L2 as dwords and are 8 now -- S-fb15k237 evaluation step 1.995 -> 1.956 ms over its five launches.  Eight
    // such loads in flight before the first write measured SLOWER (HISTORY, profiles/quad_tile_order_ab.json).
    const bool rel_vec = (reinterpret_cast<uintptr_t>(p.relation) & 15u) == 0;

    for (int s = label + kXcd * team; s < p.n_slots; s += kXcd * conc) {
        const int tile = s / p.split;
        const int part = s - tile * p.split;
        const long long col = (long long)tile * kTile + (lane & 15) * 4;
        const bool active = col < F;                               // F % 4 == 0 (dispatch condition)
        const uint32_t voff = (uint32_t)((active ? col : 0) * 4);
        float *lds_x = lds_rel + (NEEDS_REL ? p.n_rel * kTile : 0);
        if constexpr (NEEDS_REL) {
            if (rel_vec) {       // 16 bytes per lane: a lane's four columns are inside F or outside (F % 4 == 0)
                const int total = p.n_rel * (kTile / 4);
                for (int i = threadIdx.x; i < total; i += kBlock) {
                    const int r = i >> 4;
                    const long long c = (long long)tile * kTile + (i & 15) * 4;
                    qf4 v = {0.0f, 0.0f, 0.0f, 0.0f};
                    if (c < F) v = *reinterpret_cast<const qf4 *>(p.relation + (long long)r * F + c);
                    *reinterpret_cast<qf4 *>(lds_rel + 4 * i) = v;
                }
            } else {
                const int total = p.n_rel * kTile;
                for (int i = threadIdx.x; i < total; i += kBlock) {
                    const int r = i >> 6;
                    const long long c = (long long)tile * kTile + (i & 63);
                    lds_rel[i] = (c < F) ? p.relation[(long long)r * F + c] : 0.0f;
                }
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
        int b_node = -1;               // sparse boundary of this lane's four columns (one query block: bdim % 4 == 0)
        qf4 b_val = {0.0f, 0.0f, 0.0f, 0.0f};
        if (KIND == KIND_FWD && p.bnode != nullptr && active) {
            b_node = p.bnode[col / p.bdim];
            b_val = *reinterpret_cast<const qf4 *>(p.bvec + col);
        }
        int act_node = -1;
        if constexpr (ACT == 1 || ACT == 2) {      // this tile's bitmap behind the tables (X_LDS is off: lds_x is free)
            uint32_t *lds_act = reinterpret_cast<uint32_t *>(lds_x);
            const uint32_t *bits = p.act_bits + (long long)tile * p.act_words;
            for (int i = threadIdx.x; i < p.act_words; i += kBlock) lds_act[i] = bits[i];
        }
        if constexpr (ACT == 3) act_node = p.act_node[tile];
        if (threadIdx.x == 0) *ticket = 0;
        __syncthreads();
        const uint32_t rel_base = (uint32_t)kLdsHeader;                                  // byte addresses in LDS
        const uint32_t x_base = rel_base + (NEEDS_REL ? (uint32_t)p.n_rel * 256u : 0u);
        auto dead = [&](uint32_t key) -> uint32_t {      // all ones for an inactive row: OR-ed into a gather's byte offset
            if constexpr (ACT == 1 || ACT == 2) return ((lds_read1(x_base + (key >> 5) * 4u) >> (key & 31u)) & 1u) ? 0u : 0xffffffffu;
            if constexpr (ACT == 3) return (int)key == act_node ? 0u : 0xffffffffu;
            return 0u;
        };

        for (;;) {
            int t = 0;
            if (lane == 0) t = __hip_atomic_fetch_add(ticket, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            t = uniform(t);
            // the workgroup's chunk sequence (see packed_kernel): position q -> chunk part + split * (q * nb + serpentine(bl));
            // this wave takes positions 4t .. 4t+3, one per group
            const int k_first = part + p.split * (4 * t * nb + bl);
            if (k_first >= p.n_chunks) break;
            const int q = 4 * t + grp;
            const int k = part + p.split * (q * nb + ((q & 1) ? (nb - 1 - bl) : bl));
            const bool has = k < p.n_chunks;
            int4 d = {0, 0, 0, 0};
            if (has) d = p.chunks[k];
            const int n = d.y - d.x;
            const uint32_t e_begin = (uint32_t)d.x;
            const bool is_piece = d.w < 0;
            const int row_base = d.z;
            const int n01 = max(__builtin_amdgcn_readlane(n, 0), __builtin_amdgcn_readlane(n, 16));
            const int n23 = max(__builtin_amdgcn_readlane(n, 32), __builtin_amdgcn_readlane(n, 48));
            const int m01 = min(__builtin_amdgcn_readlane(n, 0), __builtin_amdgcn_readlane(n, 16));
            const int m23 = min(__builtin_amdgcn_readlane(n, 32), __builtin_amdgcn_readlane(n, 48));
            const int n_max = uniform(max(n01, n23)), n_min = uniform(min(m01, m23));
            const uint32_t e_bytes = e_begin * 4u;

            uint32_t cur = 0;
            qf4 acc = identity4<RED>();
            const bool adds = (KIND != KIND_DREL) && p.add_rows != nullptr;      // d_input: the epilogue's gradient (may alias out)
            const bool sparse_b = (KIND == KIND_FWD) && p.add_rows == nullptr && p.bnode != nullptr;
            // rows of `out` / `add_rows` are addressed with 32-bit byte offsets (out_bytes < 4 GiB: dispatch condition)
            const uint32_t base_off = (uint32_t)row_base * p.row_bytes + voff;
            auto load_add = [&](uint32_t off) -> qf4 {
                return __builtin_bit_cast(qf4, __builtin_amdgcn_raw_buffer_load_b128(rsrc_add, off, 0, 0));
            };

            auto store_row = [&](uint32_t dl, qf4 v) {       // row = row_base + dl
                if (active) {
                    // dense boundary (training forward, rspmm_sum_plus): read at the row's end; inference passes the
                    // sparse form, which costs no load at all
                    if (adds) v = reduce4<RED>(v, load_add(base_off + __umul24(dl, p.row_bytes)));
                    if (sparse_b) v = reduce4<RED>(v, (row_base + (int)dl == b_node) ? b_val : qf4{0.0f, 0.0f, 0.0f, 0.0f});
                    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(qu4, v), rsrc_out, base_off + __umul24(dl, p.row_bytes), 0, ULTRA_QUAD_STORE_AUX);
                }
            };
            auto store_empty = [&](uint32_t dl) {
                if (active) {
                    const uint32_t off = base_off + dl * p.row_bytes;
                    qf4 v = identity4<RED>();
                    if (adds) v = reduce4<RED>(v, load_add(off));
                    if (sparse_b) v = reduce4<RED>(v, (row_base + (int)dl == b_node) ? b_val : qf4{0.0f, 0.0f, 0.0f, 0.0f});
                    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(qu4, v), rsrc_out, off, 0, ULTRA_QUAD_STORE_AUX);
                }
            };
            auto contribute = [&](qf4 a, qf4 rv, qf4 gv, float w) -> qf4 {
                if constexpr (KIND == KIND_FWD) {
                    qf4 y;
                    if constexpr (MUL == ULTRA_MUL_MUL) y = rv * gv; else y = rv + gv;
                    if constexpr (!UNIT_W) y = w * y;
                    return reduce4<RED>(a, y);
                } else {
                    qf4 c = gv;
                    if constexpr (!UNIT_W) c = c * w;
                    if constexpr (MUL == ULTRA_MUL_MUL) c = c * rv;
                    return a + c;
                }
            };
            // rows between the one being reduced and the row of the next edge: close the former, fill the empty ones
            // In-place updates through tied asm operands: written as plain assignments the compiler keeps the old and
            // the new accumulator in different registers across the branch and copies 5 registers on EVERY edge of
            // the per-edge path, taken or not.
            const float ident = identity<RED>();
            auto next_row = [&](uint32_t dl) {
                store_row(cur, acc);
                for (uint32_t r = cur + 1; r < dl; ++r) store_empty(r);
                asm volatile("v_mov_b32 %0, %1" : "+v"(cur) : "v"(dl));
                asm volatile("v_mov_b32 %0, %1" : "+v"(acc.x) : "v"(ident));
                asm volatile("v_mov_b32 %0, %1" : "+v"(acc.y) : "v"(ident));
                asm volatile("v_mov_b32 %0, %1" : "+v"(acc.z) : "v"(ident));
                asm volatile("v_mov_b32 %0, %1" : "+v"(acc.w) : "v"(ident));
            };

            // Edge words (and node_b words) of the batch starting at edge i of every group's chunk.  A load in which all
            // 16 lanes of a group fetch the same dwords costs the L1 pipeline as much as a gather (it is paid per lane,
            // not per byte), so lane j of a group fetches word i + j ONCE (one dword per lane: a quarter of the cost
            // of a dwordx4) and the words are handed round the group with ds_bpermute.  Two batches ahead for the load,
            // one for the distribution.  No clamping at the end of a chunk: the loads are bounds-checked buffer loads,
            // what they return past the chunk is the next chunk's words or zeros -- valid ids either way -- and such
            // lanes are never reduced.
            const uint32_t lane_word = (uint32_t)min(lane & 15, U - 1) * 4u;
            const int bp_base = (lane & 48) * 4;                         // byte address of this group's lane 0
            auto load_compact = [&](int i, uint32_t &m, uint32_t &m2) {
                const uint32_t off = e_bytes + (uint32_t)i * 4u + lane_word;
                m = __builtin_amdgcn_raw_buffer_load_b32(rsrc_meta, off, 0, ULTRA_QUAD_WORD_AUX);
                m2 = 0;
                if constexpr (TWO_GATHERS) m2 = __builtin_amdgcn_raw_buffer_load_b32(rsrc_meta2, off, 0, 0);
            };
            auto distribute = [&](uint32_t m, uint32_t m2, uint32_t (&w)[U], uint32_t (&w2)[U]) {
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    w[u] = (uint32_t)__builtin_amdgcn_ds_bpermute(bp_base + 4 * u, (int)m);
                    w2[u] = 0;
                    if constexpr (TWO_GATHERS) w2[u] = (uint32_t)__builtin_amdgcn_ds_bpermute(bp_base + 4 * u, (int)m2);
                }
            };
            // X_LDS (every gather an LDS read already: the LDS pipe is the busy one there): plain per-lane loads of
            // all U words, one batch ahead
            auto load_words = [&](int i, uint32_t (&w)[U], uint32_t (&w2)[U]) {
                const uint32_t w_off = e_bytes + (uint32_t)i * 4u;      // one add, then immediate offsets
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    w[u] = __builtin_amdgcn_raw_buffer_load_b32(rsrc_meta, w_off + 4u * u, 0, ULTRA_QUAD_WORD_AUX);
                    w2[u] = 0;
                }
            };
            uint32_t wn[U], w2n[U];      // the NEXT batch's words
            uint32_t mw = 0, mw2 = 0;    // the words of the batch after that, one per lane
            // (never with marked words: the DEDUP compare reads node fields that carry the bit-31 mark and its kill mask would
            // replace the removed edges' -- ADVICE r5)
            constexpr bool DEDUP = ULTRA_QUAD_DEDUP && !TWO_GATHERS && !X_LDS && ACT == 0 && !DEAD;
            uint32_t prev_node = 0xffffffffu;       // DEDUP: the gathered node and row of the last edge of the previous batch
            qu4 prev_x = {0u, 0u, 0u, 0u};
            if constexpr (DIRECT_WORDS) {
                load_words(0, wn, w2n);
            } else {
                load_compact(0, mw, mw2);
                distribute(mw, mw2, wn, w2n);
                load_compact(U, mw, mw2);
            }

            auto batch = [&](auto tail_tag, int i) {
                constexpr bool TAIL = decltype(tail_tag)::value;
                uint32_t w[U], w2[U];
                float wt[U];
                qf4 xv[U], rv[U];
                uint32_t killm[U];
#pragma unroll
                for (int u = 0; u < U; ++u) { w[u] = wn[u]; w2[u] = w2n[u]; killm[u] = 0u; }
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const uint32_t node = w[u] >> p.src_shift;
                    if constexpr (TWO_GATHERS) {    // node ids < 2^24, row_bytes < 2^24 (dispatch conditions)
                        uint32_t kill = 0u;
                        if constexpr (ACT == 2) kill = dead(w2[u]);
                        if constexpr (ACT == 3) kill = dead(node);
                        if constexpr (DEAD) kill |= (uint32_t)((int32_t)w[u] >> 31);
                        xv[u] = __builtin_bit_cast(qf4, __builtin_amdgcn_raw_buffer_load_b128(
                                                            rsrc2, (__umul24(w2[u], p.row_bytes) + voff) | kill, 0, 0));
                        rv[u] = qf4{0.0f, 0.0f, 0.0f, 0.0f};
                        if constexpr (MUL == ULTRA_MUL_MUL) {
                            if constexpr (X_LDS)
                                rv[u] = lds_read4(((node << 8) | lane_bytes) + x_base);
                            else
                                rv[u] = __builtin_bit_cast(qf4, __builtin_amdgcn_raw_buffer_load_b128(
                                                                    rsrc, (__umul24(node, p.row_bytes) + voff) | kill, 0, 0));
                        }
                        continue;
                    }
                    if constexpr (X_LDS) {
                        xv[u] = lds_read4(((node << 8) | lane_bytes) + x_base);
                    } else {     // node < 2^24 (packed into the word), row_bytes < 2^24 (dispatch condition)
                        uint32_t kill = 0u;
                        if constexpr (ACT == 1) kill = dead(node);
                        if constexpr (DEAD) kill = (uint32_t)((int32_t)w[u] >> 31);
                        if constexpr (DEDUP) {
                            const uint32_t before = (u == 0) ? prev_node : (w[u > 0 ? u - 1 : 0] >> p.src_shift);
                            kill = (node == before) ? 0xffffffffu : 0u;
                            killm[u] = kill;
                        }
                        xv[u] = __builtin_bit_cast(qf4, __builtin_amdgcn_raw_buffer_load_b128(
                                                            rsrc, (__umul24(node, p.row_bytes) + voff) | kill, 0, 0));
                    }
                    if constexpr (NEEDS_REL)
                        rv[u] = lds_read4(((w[u] & p.rel_mask) | lane_bytes) + rel_base);
                    else
                        rv[u] = qf4{0.0f, 0.0f, 0.0f, 0.0f};
                }
                // per-edge weights: no address depends on them -- they travel with the gathers, not with the words
                if constexpr (!UNIT_W && !DIRECT_WORDS) {       // one weight per lane, handed round the group like the words
                    const int mine = (int)__builtin_amdgcn_raw_buffer_load_b32(rsrc_wt, e_bytes + (uint32_t)i * 4u + lane_word, 0, 0);
#pragma unroll
                    for (int u = 0; u < U; ++u) wt[u] = __builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute(bp_base + 4 * u, mine));
                } else {
#pragma unroll
                    for (int u = 0; u < U; ++u) {
                        wt[u] = 1.0f;
                        if constexpr (!UNIT_W)
                            wt[u] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(
                                                                  rsrc_wt, e_bytes + (uint32_t)i * 4u + 4u * u, 0, 0));
                    }
                }
                if constexpr (DIRECT_WORDS) {
                    if (i + U < n_max) load_words(i + U, wn, w2n);
                } else {
                    const uint32_t m = mw, m2 = mw2;
                    load_compact(i + 2 * U, mw, mw2);
                    distribute(m, m2, wn, w2n);
                }
                if constexpr (DEDUP) {       // a repeated node takes the row its predecessor holds (in edge order: runs chain)
#pragma unroll
                    for (int u = 0; u < U; ++u) {
                        const qu4 before = (u == 0) ? prev_x : __builtin_bit_cast(qu4, xv[u > 0 ? u - 1 : 0]);
                        const qu4 got = __builtin_bit_cast(qu4, xv[u]);
                        qu4 v;
                        v.x = (before.x & killm[u]) | got.x; v.y = (before.y & killm[u]) | got.y;
                        v.z = (before.z & killm[u]) | got.z; v.w = (before.w & killm[u]) | got.w;
                        xv[u] = __builtin_bit_cast(qf4, v);
                    }
                    prev_x = __builtin_bit_cast(qu4, xv[U - 1]);
                    prev_node = w[U - 1] >> p.src_shift;
                }
                bool same_row = false;
                if constexpr (!TAIL) same_row = __builtin_amdgcn_ballot_w64((w[U - 1] & 0xffu) != cur) == 0ull;
                if (same_row) {      // no group leaves its row inside this batch (always the case for pieces)
#pragma unroll
                    for (int u = 0; u < U; ++u) acc = contribute(acc, rv[u], xv[u], wt[u]);
                } else {
#pragma unroll
                    for (int u = 0; u < U; ++u) {
                        const bool valid = !TAIL || (i + u < n);
                        const uint32_t dl = w[u] & 0xffu;
                        if (valid) {
                            if (dl != cur) next_row(dl);
                            acc = contribute(acc, rv[u], xv[u], wt[u]);
                        }
                    }
                }
            };

            int i = 0;
            for (; i + U <= n_min; i += U) batch(std::false_type{}, i);
            for (; i < n_max; i += U) batch(std::true_type{}, i);

            if (has) {
                if (is_piece) {
                    if (active) *reinterpret_cast<qf4 *>(p.partial + (long long)(-d.w - 1) * F + col) = acc;
                } else {
                    store_row(cur, acc);
                    for (uint32_t r = cur + 1; r < (uint32_t)(d.w - row_base); ++r) store_empty(r);
                }
            }
        }
        __syncthreads();   // all tickets drawn, tables no longer read
    }
}

// rowgroup.inc -- rspmm straight from a CSR (row_ptr, col, rel[, w]): one destination row per 16-lane group.
// (included by plan_rowgroup.hip, inside its anonymous namespace)
//
// Two uses:
//  * the raw-CSR entry of the C ABI, ultra_rspmm_fwd_f32(row_ptr, src, rel, w, relation, x, out, ...) -- SURVEY.md 8b's
//    torch-free entry: no plan, no workspace, the summation order of every row is the strictly sequential (src, rel)
//    order of the coalesced CSR, i.e. the reference order (oracle `piece = 0`) for EVERY row;
//  * big graphs of short rows (config 5, S-stress: 10 M nodes / 100 M edges, ~10 edges per row, node ids too wide for the
//    packed edge word): run_plan() takes this kernel when the plan has no split rows.  The chunked kernels walk runs of
//    edges and test for a row boundary at every edge there (a batch of 8 edges crosses a boundary almost always);
//    here a row is a group's private loop and the gathers of four rows are in flight per wave-instruction.
//
// A wave = four groups of 16 lanes; a lane owns 4 adjacent columns of the 64-column tile, so one dwordx4 load fetches
// the 256-B row segments of four different rows' edges (1 KiB per wave-instruction); a row's whole window of up to 16
// edges is in flight at once (S-stress rows hold ~10 edges: one memory round trip per row), 8 waves per CU (the window's
// 64 + 64 value registers do not leave room for more: 768- / 1024-thread builds spill, 12.6 / 20 ms against 5.8).
// Edge ids: lane j of a group loads edge j of the row's current 16-edge window once (one dword each for col / rel / w) and
// ds_bpermute hands them round -- no 16-fold redundant loads.
//
// What shaped the loop (round 2, each step measured on S-stress, 10 M rows / 100 M edges / 1 000 relations):
//  * memory operations retire in order (vmcnt), so every iteration has exactly ONE exposed round trip, the gathers: the
//    row pointers of row i+2 and the edge window of row i+1 are requested before the gathers of row i are issued, and
//    the result of row i is stored at the top of iteration i+1 (a store at the bottom made the register rotation of the
//    loop wait for its own store);
//  * address arithmetic is one v_mad_u64_u32 per gather (id x row bytes + the lane's base) and slots past the row's end
//    are neither zero-filled nor read -- 12 VALU instructions per edge and wave before, 5 now -- and all crossbar
//    reads of a window are issued before the first gather (5.85 -> 5.42 ms on the same box);
//  * relation rows from LDS when the tile's table fits (n_rel x 4 G x 4 B <= 156 KiB); else the first rows of the table
//    from LDS and the rest through L2: a gather that misses L1 costs the texture path twice (fill + read: ~30 B/clk/CU,
//    tools/ubench/gather.hip), and input rows and relation rows are the same number of bytes there, so every relation row
//    served from LDS frees a quarter of that path (5.96 -> 5.67 ms).  The LDS rows are read AFTER the gathers have
//    returned: a register with a memory load pending for some lanes cannot take an LDS read for the others before the
//    load is back, and the compiler then waits for ALL gathers at every slot (the 9.5-10.8 ms of the first attempts).
//  * measured and not kept: cache-policy bits on the gathers (sc0 / sc1 no change, nt 2.2x slower on L2 hits), plain
//    instead of streaming stores (6.00 -> 6.07 ms), relation rows fetched after the input rows have arrived to free
//    their registers for a third wave per SIMD (5.69 -> 5.86 ms at 512 threads, 8.3 ms at 768: spills).
// Where the rest goes (same box, 5.85 ms): without the output stores 4.69 ms, with relation rows always L1-resident
// 5.40 ms, with the input rows L2-resident 3.04 ms; the bare gather of the same rows runs 6.2-6.6 TB/s.

// (RowGroupParams, which run_plan and the raw-CSR entry fill, is declared in plan_kernels.h.)

// BACKWARD: the d_input contribution ((grad * w) * relation) of the plan kernels instead of the forward message
// w * (relation (*|+) x) -- same factors, but fp32 products are rounded in that order.
#ifndef ULTRA_RG_BLOCK
#define ULTRA_RG_BLOCK 512
#endif
constexpr int kRelL2 = 0, kRelLds = 1, kRelPart = 2;     // where a tile's relation rows are read from (see the header)
constexpr int kRgBlock = ULTRA_RG_BLOCK;     // 8 waves per CU, up to 256 VGPRs: a whole 16-edge window of gathers + relation rows in flight

// G: lanes per row (16, 32 or 64): the group covers a column tile of 4 G columns.  G = 16 (64-column tiles, one query
// each) keeps a tile's slice of a cache-resident gathered matrix inside one XCD's L2; for matrices that live in DRAM wider
// groups fetch F = 128 / 256 columns of a row in ONE contiguous piece per edge instead of in 256-B pieces on separate passes
// over the edge list (S-stress at B = 4: 1 KiB per gather, the indices read once instead of four times).
template <int SUM, int MUL, bool UNIT_W, int REL, bool NEEDS_REL, bool BACKWARD, int G>
__global__ __launch_bounds__(kRgBlock) void rowgroup_kernel(const RowGroupParams p) {
    constexpr int U = 16;                                   // gathers in flight per group: the whole window
    constexpr bool REL_LDS = REL == kRelLds, REL_PART = REL == kRelPart && NEEDS_REL;
    constexpr int W = 4 * G;                                // columns per tile
    static_assert(G == 16 || G == 32 || G == 64, "a group is 16, 32 or 64 lanes");
    static_assert(!BACKWARD || SUM == ULTRA_SUM_ADD, "backward of sum-aggregation only");
    extern __shared__ __attribute__((aligned(16))) float lds_raw[];
    float *lds_rel = lds_raw + kLdsHeader / sizeof(float);
    const int lane = threadIdx.x & 63;
    const int sub = lane & (G - 1);
    const int bp_base = (lane & (64 - G)) * 4;            // byte address (ds_bpermute) of the group's lane 0
    const int label = blockIdx.x % kXcd;
    const int bl = blockIdx.x / kXcd;
    const int nb = p.blocks_per_label;
    const long long F = p.F;
    const int groups_per_block = kRgBlock / G;
    const int group_in_block = threadIdx.x / G;
    const qf4 zero4 = {0.0f, 0.0f, 0.0f, 0.0f};
    if ((uint32_t)(uintptr_t)(lds_char_ptr)lds_raw != 0u) __builtin_trap();      // lds_read4 takes absolute LDS addresses

    for (int s = label; s < p.n_slots; s += kXcd) {
        const int tile = s / p.split;
        const int part = s - tile * p.split;
        const long long col0 = (long long)tile * W + sub * 4;
        const bool active = col0 < F;                       // F % 4 == 0 (dispatch condition)
        const long long lcol = active ? col0 : 0;
        const uint32_t row_bytes = (uint32_t)F * 4u;                                  // F < 2^30 (host check)
        const char *gather_lane = reinterpret_cast<const char *>(p.gather + lcol);
        const char *relation_lane = reinterpret_cast<const char *>(p.relation + lcol);
        const uint32_t lds_lane = (uint32_t)kLdsHeader + (uint32_t)sub * 16u;
        if constexpr ((REL_LDS || REL_PART) && NEEDS_REL) {
            __syncthreads();                                // the previous slot's readers are done
            const int total = p.n_rel_lds * W;
            for (int i = threadIdx.x; i < total; i += kRgBlock) {
                const int r = i / W;
                const long long c = (long long)tile * W + (i % W);
                lds_rel[i] = (c < F) ? p.relation[(long long)r * F + c] : 0.0f;
            }
            __syncthreads();
        }
        int b_node = -1;
        qf4 b_val = zero4;
        if (p.bnode != nullptr && active) {
            b_node = p.bnode[col0 / p.bdim];
            b_val = *reinterpret_cast<const qf4 *>(p.bvec + col0);
        }
        // rows of this part, dealt to the groups of the label's workgroups round-robin
        const long long rows_per_part = ((long long)p.n_rows + p.split - 1) / p.split;
        const long long row_begin = (long long)part * rows_per_part;
        const long long row_end = min(row_begin + rows_per_part, (long long)p.n_rows);
        const long long stride = (long long)nb * groups_per_block;
        long long row = row_begin + (long long)bl * groups_per_block + group_in_block;

        // software pipeline over rows, two deep: while row i is reduced the first window of edge ids of row i+1 is
        // fetched (its row pointers arrived an iteration ago) and the row pointers of row i+2 are requested -- one
        // exposed memory round trip per row (the gathers), not two
        int beg, end, beg1, end1, n_col = 0, n_rel_id = 0;
        float n_w = 1.0f;
        auto load_ptrs = [&](long long r_, int &b_, int &e_) {
            b_ = 0; e_ = 0;
            if (r_ < row_end) {
                b_ = p.row_ptr[r_];
                e_ = p.row_ptr[r_ + 1];
            }
        };
        auto load_window = [&](int first, int last, int &c, int &r, float &w) {
            const int e = first + sub;                      // the first 16 lanes of a group hold the window
            c = 0; r = 0; w = 1.0f;
            if (sub < 16 && e < last) {
                c = p.col[e];
                if constexpr (NEEDS_REL) r = p.rel[e];
                if constexpr (!UNIT_W) w = p.weight[e];
            }
        };
        load_ptrs(row, beg, end);
        load_ptrs(row + stride, beg1, end1);
        load_window(beg, end, n_col, n_rel_id, n_w);
        // Memory operations retire in order (vmcnt), and a store is acknowledged later than a load returns.  The result of
        // row i therefore leaves as ONE UNCONDITIONAL buffer store issued right AFTER the gathers of row i+1's first window:
        // younger than those gathers, it does not have to be acknowledged before they count as returned (the compiler's
        // wait becomes vmcnt(1)), and it has the whole next round trip to retire.  (Stored at the top of the iteration -- older
        // than the gathers, and behind an `if` -- every row's round trip was max(gathers, acknowledgement of the previous
        // row's store): S-stress 5.85 ms with the stores, 4.69 without.)  Rows without a previous result, and lanes past
        // F, store to an offset outside the descriptor: dropped by the range check.  The descriptor covers this part's
        // rows only (the host keeps a part below 4 GiB), offsets are 32-bit.
        const unsigned long long part_bytes = (unsigned long long)(row_end - row_begin) * row_bytes;
        const __amdgpu_buffer_rsrc_t rsrc_out = __builtin_amdgcn_make_buffer_rsrc(
            reinterpret_cast<char *>(p.out) + (unsigned long long)row_begin * row_bytes, 0, (int)(uint32_t)part_bytes, 0x00020000);
        const uint32_t lane_off = (uint32_t)(col0 * 4);
        __builtin_amdgcn_s_waitcnt(0x0F70);                 // vmcnt(0): the loop is entered with no load pending
        qf4 st_v = zero4;
        uint32_t st_off = 0xffffffffu;
        qf4 xv[U], rv[U];
        float wv[U];
        uint32_t cid[U], rid[U];
        auto issue = [&](int n_here, int w_col, int w_rel, float w_w) {
#pragma unroll
            for (int u = 0; u < U; ++u) {          // all the crossbar reads first: they pipeline
                cid[u] = (uint32_t)__builtin_amdgcn_ds_bpermute(bp_base + 4 * u, w_col);
                rid[u] = 0;
                if constexpr (NEEDS_REL) rid[u] = (uint32_t)__builtin_amdgcn_ds_bpermute(bp_base + 4 * u, w_rel);
                wv[u] = 1.0f;
                if constexpr (!UNIT_W)
                    wv[u] = __builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute(bp_base + 4 * u, __builtin_bit_cast(int, w_w)));
            }
            // xv / rv of the slots past the row's end stay unwritten and unread (same predicate in `reduce`): no zero
            // fill, and ONE v_mad_u64_u32 per address (id x row bytes + the lane's base)
#pragma unroll
            for (int u = 0; u < U; ++u) {
                if (u < n_here) {
                    xv[u] = *reinterpret_cast<const qf4 *>(gather_lane + (unsigned long long)cid[u] * row_bytes);
                    if constexpr (NEEDS_REL) {
                        if constexpr (REL_LDS) rv[u] = lds_read4(lds_lane + rid[u] * (uint32_t)(W * 4));
                        else if constexpr (REL_PART) {      // the LDS-resident rows are read at reduce time
                            if (rid[u] >= (uint32_t)p.n_rel_lds)
                                rv[u] = *reinterpret_cast<const qf4 *>(relation_lane + (unsigned long long)rid[u] * row_bytes);
                        } else rv[u] = *reinterpret_cast<const qf4 *>(relation_lane + (unsigned long long)rid[u] * row_bytes);
                    }
                }
            }
        };
        auto reduce = [&](int n_here, qf4 &acc) {
            if constexpr (REL_PART) {
                // A register with a memory load pending cannot take an LDS read for other lanes before that load
                // returns (the compiler would wait for ALL gathers at every slot): LDS rows after the wait
#pragma unroll
                for (int u = 0; u < U; ++u)
                    if (u < n_here && rid[u] < (uint32_t)p.n_rel_lds) rv[u] = lds_read4(lds_lane + rid[u] * (uint32_t)(W * 4));
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                if (u < n_here) {
                    qf4 y;
                    if constexpr (BACKWARD) {
                        y = xv[u];
                        if constexpr (!UNIT_W) y = y * wv[u];
                        if constexpr (NEEDS_REL) y = y * rv[u];
                    } else {
                        if constexpr (MUL == ULTRA_MUL_MUL) y = rv[u] * xv[u];
                        else y = rv[u] + xv[u];
                        if constexpr (!UNIT_W) y = wv[u] * y;
                    }
                    acc = reduce4<SUM>(acc, y);
                }
            }
        };
        while (row < row_end) {
            const int cur_beg = beg, cur_end = end;
            int w_col = n_col, w_rel = n_rel_id;
            float w_w = n_w;
            const long long cur_row = row;
            row += stride;
            int beg2, end2;
            load_ptrs(row + stride, beg2, end2);            // row i+2 (zeros past the end)
            load_window(beg1, end1, n_col, n_rel_id, n_w);  // row i+1 (nothing past the end: beg1 == end1 == 0)
            beg = beg1; end = end1;
            beg1 = beg2; end1 = end2;
            qf4 addv = zero4;                               // the fused epilogue's operand travels with the gathers
            if (p.add_rows != nullptr && active) addv = *reinterpret_cast<const qf4 *>(reinterpret_cast<const char *>(p.add_rows + col0) + (unsigned long long)(uint32_t)cur_row * row_bytes);
            qf4 acc = identity4<SUM>();
            // first window (empty for a row without edges), the previous row's store behind its gathers
            {
                const int n_here = min(16, cur_end - cur_beg);
                issue(n_here, w_col, w_rel, w_w);
                __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(qu4, st_v), rsrc_out, st_off, 0, 2 /* nt */);
                reduce(n_here, acc);
            }
            for (int e0 = cur_beg + 16; e0 < cur_end; e0 += 16) {
                load_window(e0, cur_end, w_col, w_rel, w_w);
                const int n_here = min(16, cur_end - e0);
                issue(n_here, w_col, w_rel, w_w);
                reduce(n_here, acc);
            }
            st_v = acc;
            if (p.add_rows != nullptr) st_v = reduce4<SUM>(st_v, addv);
            else if (p.bnode != nullptr) st_v = reduce4<SUM>(st_v, ((int)cur_row == b_node) ? b_val : zero4);
            st_off = active ? (uint32_t)((unsigned long long)(cur_row - row_begin) * row_bytes) + lane_off : 0xffffffffu;
#ifdef ULTRA_RG_STORE_WINDOW      // diagnostic build (wrong results): every store lands in one L2-resident 256-KiB window
            if (active) st_off = (st_off & 0x3ffffu);
#endif
        }
        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(qu4, st_v), rsrc_out, st_off, 0, 2 /* nt */);
    }
}

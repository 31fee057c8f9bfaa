// frontier.inc -- the FIRST Bellman-Ford layer's rspmm, from the boundary in its sparse form.  (included by epilogue.hip, inside its anonymous namespace)
//
// The first layer of every Bellman-Ford reads `input = boundary` (ultra/model.py:116-120, ultra/rel_model.py:365-369),
// a tensor that is zero outside ONE row per query (model.py:106-107: row h_index[b] of query block b holds query[b]).
// With the DistMult message (mul) and sum aggregation (the shipped configuration, config/transductive/inference.yaml:13-14)
// an edge whose source row is zero contributes w * (rel * 0) = +-0, and `acc + (+-0)` leaves `acc` unchanged (acc
// starts at +0 and +0 + -0 = +0).  So
//     out[v, block b] = SUM over the edges (h_b -> v, r), in forward-plan order, of  w * (relation[r, block b] * query[b])
// and every other element is +0 (+ the boundary epilogue at row h_b): deg_out(h_b) edges per query instead of E.
//
// Bit-compatibility with the full kernels: the edges (h_b -> v, *) are consecutive in v's forward row (sorted by
// (src, rel)); a row longer than piece_len is summed there in pieces of piece_len consecutive contributions, each from
// +0, and the piece sums are added in piece order.  `fwd_rank[e]` (the position of edge e inside its destination row,
// forward order) gives the piece of every edge, and the same association is used here:
//     result = P_j1 + P_j2 + ...   with   P_j = ((0 + t_1) + t_2) + ...  over the terms that fall into piece j.
// tests/test_frontier_gpu.py requires equality with ultra_rspmm_forward_boundary_f32 on the dense boundary.
//
// Layout: edges in the d_input plan's order (src, dst, rel): the out-edges of a node are one contiguous range, sorted by
// (dst, rel).  A workgroup serves one query; its 16-lane groups (a lane owns 4 of the query block's 64 columns) cut
// that range into slices aligned to destination runs.  The relation rows come straight from L2 (a few hundred rows).

struct FrontierParams {
    const int32_t *src_ptr;     // [n_src + 1] first out-edge of every source node (d_input plan order)
    const int32_t *dst;         // [E] destination node           (by_src.node_a)
    const int32_t *rel;         // [E] relation id                (by_src.rel)
    const float *weight;        // [E] or NULL (unit weights)     (by_src.weight)
    const int32_t *fwd_rank;    // [E] position of the edge inside its destination row in forward-plan order
    const float *relation;      // [n_rel, F]
    const int32_t *bnode;       // [F / 64] boundary node of every query block
    const float *bvec;          // [F] boundary value
    float *out;                 // [n_rows, F], zero-filled before this kernel runs
    long long F;
    int piece_len;
    int slices;                 // workgroups per query
    int n_rel;                  // rows of `relation` (frontier_lds_kernel stages one message row per relation)
    int piece_shift;            // log2(piece_len) when it is a power of two, else -1
    // sparse first layer (ultra_first_layer_sparse_f32; NULL otherwise): the rows this kernel
    // writes are also LISTED, so that the layer's epilogue can run on them alone (every other row of the layer's output is
    // one constant vector).  No atomics and no counter: the slot of a row is a function of the plan --
    //   run_prefix[e] = number of (source, destination) runs that start at or before edge e in by_src order,
    // so the run of destination v among the out-edges [lo, hi) of h_b has ordinal run_prefix[first edge of the run] -
    // run_prefix[lo], and query b owns the slots [list_offset[b], list_offset[b + 1]): one per run + one for the row (h_b, b)
    // itself (holds -1 when a self loop's run already lists that row).  Every slot is written on every launch.
    const int32_t *run_prefix;  // [E]
    int32_t *row_list;          // [list_offset[n_query]] row ids  dest * n_query + b,  or -1
    const int32_t *list_offset; // [n_query + 1]
    int list_len;               // entries of row_list: a slot at or beyond it is not written (the caller sized the list too small)
};

constexpr int kFrontierThreads = 256;
constexpr int kFrontierU = 4;

template <bool UNIT_W>
__global__ __launch_bounds__(kFrontierThreads) void frontier_kernel(const FrontierParams p) {
    const int lane = threadIdx.x & 63;
    const int b = blockIdx.x;                                      // query block
    const long long col = (long long)b * 64 + (lane & 15) * 4;
    const int groups_per_block = kFrontierThreads / 16;
    const int g = blockIdx.y * groups_per_block + (threadIdx.x >> 4);
    const int n_groups = p.slices * groups_per_block;
    const int h = p.bnode[b];
    const qf4 q = *reinterpret_cast<const qf4 *>(p.bvec + col);
    const int lo = p.src_ptr[h], hi = p.src_ptr[h + 1];

    if (g == 0) {
        // row h of this block carries the boundary value even when no edge h -> h exists: 0 + value, as the full
        // kernel's epilogue computes it (the run of a self loop, if there is one, writes acc + value itself)
        bool self_loop = false;
        int a = lo, z = hi;                                        // first edge of the range with dst >= h
        while (a < z) {
            const int m = (a + z) >> 1;
            if (p.dst[m] < h) a = m + 1; else z = m;
        }
        self_loop = a < hi && p.dst[a] == h;
        if (!self_loop) {
            const qf4 zero = {0.0f, 0.0f, 0.0f, 0.0f};
            *reinterpret_cast<qf4 *>(p.out + (long long)h * p.F + col) = zero + q;
        }
        // listing (see FrontierParams): the query's last slot is its own row, unless a self loop's run lists it
        if (p.row_list != nullptr && (lane & 15) == 0 && p.list_offset[b + 1] - 1 < p.list_len)
            p.row_list[p.list_offset[b + 1] - 1] = self_loop ? -1 : h * (int)(p.F / 64) + b;
    }

    const int n = hi - lo;
    if (n <= 0) return;
    const int list_base = p.row_list != nullptr ? p.list_offset[b] : 0;
    const int prefix_lo = p.row_list != nullptr ? p.run_prefix[lo] : 0;
    const int per = (n + n_groups - 1) / n_groups;
    int e = lo + g * per;
    const int end = min(e + per, hi);
    if (e >= end) return;
    // A slice starts at the first destination run that BEGINS inside it.  Two hubs share up to R parallel edges (464 in
    // S-fb15k237's largest run), and every step of an edge-by-edge walk to the end of such a run is a dependent load:
    // the end is found by galloping + bisection (1 load when the run ends at once, ~2 log2(length) otherwise).  Hub
    // heads of real evaluation batches: 225 -> 160-215 us; what remains is the ONE group that sums the longest run of
    // the batch in order (windows of 16 edges per round trip, or requesting only the rows a group will sum, were
    // measured slower: 300 / 340 us).
    if (e > lo) {
        const int prev = p.dst[e - 1];
        int a = e, step = 1;                                // every edge in [e, a) has dst == prev
        while (a < hi && p.dst[a] == prev) { a += step; step <<= 1; }
        if (a > e) {                                        // the run ends in (a - step / 2, min(a, hi)]
            int z = min(a, hi);
            a = a - (step >> 1) + 1;
            while (a < z) {
                const int m = (a + z) >> 1;
                if (p.dst[m] == prev) a = m + 1; else z = m;
            }
        }
        e = a;
    }
    if (e >= end) return;

    int cur = p.dst[e];             // destination of the run being summed
    int run_first = e;              // its first edge (the run's slot in the row list)
    int cur_piece = -1;
    int piece_end_rank = 0;         // first forward rank beyond the open piece
    qf4 total = {0.0f, 0.0f, 0.0f, 0.0f};      // sum of the finished pieces of the run, in piece order
    qf4 piece = {0.0f, 0.0f, 0.0f, 0.0f};      // the piece being summed
    bool have_total = false;
    auto close_piece = [&]() {
        if (cur_piece >= 0) {
            total = have_total ? total + piece : (qf4{0.0f, 0.0f, 0.0f, 0.0f} + piece);
            have_total = true;
        }
    };
    auto close_run = [&]() {
        close_piece();
        qf4 v = total;
        // boundary epilogue of the forward kernels: + value at the query's own row, + 0.0f elsewhere
        v = v + ((cur == h) ? q : qf4{0.0f, 0.0f, 0.0f, 0.0f});
        *reinterpret_cast<qf4 *>(p.out + (long long)cur * p.F + col) = v;
        if (p.row_list != nullptr && (lane & 15) == 0) {
            const int slot = list_base + p.run_prefix[run_first] - prefix_lo;
            if (slot < p.list_len) p.row_list[slot] = cur * (int)(p.F / 64) + b;
        }
    };

    bool done = false;
    while (!done) {
        int d[kFrontierU], r[kFrontierU], k[kFrontierU];
        float w[kFrontierU];
        qf4 rv[kFrontierU];
#pragma unroll
        for (int u = 0; u < kFrontierU; ++u) {
            const int eu = min(e + u, hi - 1);
            d[u] = p.dst[eu];
            r[u] = p.rel[eu];
            k[u] = p.fwd_rank[eu];                          // rank in the destination's forward row; its piece: / piece_len
            w[u] = 1.0f;
            if constexpr (!UNIT_W) w[u] = p.weight[eu];
        }
#pragma unroll
        for (int u = 0; u < kFrontierU; ++u)
            rv[u] = *reinterpret_cast<const qf4 *>(p.relation + (long long)r[u] * p.F + col);
        // Fast path: the whole batch continues the open run inside the open piece (destinations and ranks ascend, so
        // the last edge decides).  The per-edge path below costs ~100 instructions an edge in one group's serial stream
        // -- and ONE group sums a run in order: the 464 parallel edges two hubs share took ~0.4 us each.
        if (e + kFrontierU <= hi && cur_piece >= 0 && d[kFrontierU - 1] == cur &&
            k[kFrontierU - 1] < piece_end_rank) {
#pragma unroll
            for (int u = 0; u < kFrontierU; ++u) {
                qf4 y = rv[u] * q;
                if constexpr (!UNIT_W) y = w[u] * y;
                piece = piece + y;
            }
            e += kFrontierU;
            continue;
        }
#pragma unroll
        for (int u = 0; u < kFrontierU; ++u) {
            if (done) break;
            const int eu = e + u;
            if (eu >= hi) { done = true; break; }
            if (d[u] != cur) {
                if (eu >= end) { done = true; break; }            // the next run belongs to the next slice
                close_run();
                cur = d[u];
                run_first = eu;
                cur_piece = -1;
                have_total = false;
            }
            const int piece_of_edge = k[u] / p.piece_len;
            if (piece_of_edge != cur_piece) {
                close_piece();
                cur_piece = piece_of_edge;
                piece_end_rank = (cur_piece + 1) * p.piece_len;
                piece = qf4{0.0f, 0.0f, 0.0f, 0.0f};
            }
            qf4 y = rv[u] * q;
            if constexpr (!UNIT_W) y = w[u] * y;
            piece = piece + y;
        }
        e += kFrontierU;
    }
    close_run();
}

// frontier_lds_kernel (round 3): the same sum with the query's MESSAGES in LDS.
//
// What sets frontier_kernel's time on real batches is one group walking a long destination run in order (two hubs share up
// to R parallel edges, 464 in S-fb15k237's largest): per batch of 4 edges it pays two DEPENDENT L2 round trips, the edge's
// ids and then the relation rows those ids name (~0.7 us a batch, 83-115 us for the run).  But the message of an edge
// (h_b -> v, r) does not depend on v:  w * (relation[r, block b] * query[b])  -- there are only R distinct products per
// query.  A workgroup (1 024 threads, one query, 1 / kFrontierLdsSlices of the out-edges) therefore stages all R products of
// its query in LDS once (R x 256 B: 121 KB for 474 relations; the same rounded product the per-edge multiply gives), and
// the walk needs the ids only: lane j of a 16-lane group fetches edge e + j's ids -- 16 edges per round trip, the next
// batch requested before the current one is summed -- and the ids travel round the group with ds_bpermute; every term is
// then one ds_read_b128.  Order of the additions, pieces, boundary epilogue: exactly frontier_kernel's.
// Used when R x 256 B fits the LDS budget; frontier_kernel stays for larger vocabularies.
constexpr int kFrontierLdsThreads = 1024;
constexpr int kFrontierLdsSlices = 8;

template <bool UNIT_W>
__global__ __launch_bounds__(kFrontierLdsThreads) void frontier_lds_kernel(const FrontierParams p) {
    extern __shared__ __attribute__((aligned(16))) float fl_msg[];         // [n_rel][64]: relation[r, block b] * query[b]
    const int lane = threadIdx.x & 63;
    const int sub = lane & 15;
    const int n_query = (int)(p.F / 64);
    const int b = blockIdx.x % n_query;                                    // query block
    const int slice = blockIdx.x / n_query;
    const long long col = (long long)b * 64 + sub * 4;
    const int h = p.bnode[b];
    const qf4 q = *reinterpret_cast<const qf4 *>(p.bvec + col);
    {
        const float *rel_b = p.relation + (long long)b * 64;
        const float *q_b = p.bvec + (long long)b * 64;
        for (int i = threadIdx.x; i < p.n_rel * 16; i += kFrontierLdsThreads) {
            const int r = i >> 4, c4 = (i & 15) * 4;
            const qf4 rv = *reinterpret_cast<const qf4 *>(rel_b + (long long)r * p.F + c4);
            const qf4 qq = *reinterpret_cast<const qf4 *>(q_b + c4);
            reinterpret_cast<qf4 *>(fl_msg)[i] = rv * qq;
        }
    }
    __syncthreads();
    const qf4 *msg = reinterpret_cast<const qf4 *>(fl_msg) + sub;           // this lane's 4 columns of row r: msg[r * 16]

    const int groups_per_block = kFrontierLdsThreads / 16;
    const int g = slice * groups_per_block + (threadIdx.x >> 4);
    const int n_groups = p.slices * groups_per_block;
    const int lo = p.src_ptr[h], hi = p.src_ptr[h + 1];

    const int list_base = p.row_list != nullptr ? p.list_offset[b] : 0;
    if (g == 0) {     // the boundary value at row h when no edge h -> h exists (see frontier_kernel)
        int a = lo, z = hi;
        while (a < z) {
            const int m = (a + z) >> 1;
            if (p.dst[m] < h) a = m + 1; else z = m;
        }
        const bool self_loop = a < hi && p.dst[a] == h;
        if (!self_loop) {
            const qf4 zero = {0.0f, 0.0f, 0.0f, 0.0f};
            *reinterpret_cast<qf4 *>(p.out + (long long)h * p.F + col) = zero + q;
        }
        if (p.row_list != nullptr && sub == 0 && p.list_offset[b + 1] - 1 < p.list_len)        // the query's last slot: its own row, unless a run lists it
            p.row_list[p.list_offset[b + 1] - 1] = self_loop ? -1 : h * n_query + b;
    }

    const int n = hi - lo;
    if (n <= 0) return;
    const int per = (n + n_groups - 1) / n_groups;
    int e = lo + g * per;
    const int end = min(e + per, hi);
    if (e >= end) return;
    if (e > lo) {     // a slice starts at the first destination run that BEGINS inside it: galloping + bisection
        const int prev = p.dst[e - 1];
        int a = e, step = 1;
        while (a < hi && p.dst[a] == prev) { a += step; step <<= 1; }
        if (a > e) {
            int z = min(a, hi);
            a = a - (step >> 1) + 1;
            while (a < z) {
                const int m = (a + z) >> 1;
                if (p.dst[m] == prev) a = m + 1; else z = m;
            }
        }
        e = a;
    }
    if (e >= end) return;

    // ordinal of the first run of this slice among the runs of h's out-edges (e is a run start); the walk closes its runs
    // in order, one slot each
    int slot = 0;
    if (p.row_list != nullptr) slot = list_base + p.run_prefix[e] - p.run_prefix[lo];
    // State of the walk: `cur` = destination of the open run, `cur_piece` = forward piece of the last summed edge (-1:
    // none yet), `open` = a piece is being summed, `total` = sum of the run's finished pieces (valid when have_total).
    int cur = p.dst[e];
    int cur_piece = -1;
    bool open = false, have_total = false;
    qf4 total = {0.0f, 0.0f, 0.0f, 0.0f};
    qf4 piece = {0.0f, 0.0f, 0.0f, 0.0f};
    auto close_piece = [&]() {
        if (open) {
            total = have_total ? total + piece : (qf4{0.0f, 0.0f, 0.0f, 0.0f} + piece);
            have_total = true;
        }
    };
    auto close_run = [&](int dest) {
        close_piece();
        qf4 v = total;
        v = v + ((dest == h) ? q : qf4{0.0f, 0.0f, 0.0f, 0.0f});       // boundary epilogue of the forward kernels
        *reinterpret_cast<qf4 *>(p.out + (long long)dest * p.F + col) = v;
        if (p.row_list != nullptr) {
            if (sub == 0 && slot < p.list_len) p.row_list[slot] = dest * n_query + b;
            ++slot;
        }
    };
    // ids of 16 consecutive edges, one per lane of the group (clamped at the range's end: never used beyond it)
    auto load_ids = [&](int e0, int &d, int &r, int &k, float &w) {
        const int eu = min(e0 + sub, hi - 1);
        d = p.dst[eu];
        r = p.rel[eu];
        k = p.fwd_rank[eu];
        w = 1.0f;
        if constexpr (!UNIT_W) w = p.weight[eu];
    };
    const int bp = (lane & 48) * 4;                                        // ds_bpermute byte address of this group's lane 0
    const int grp_shift = (lane >> 4) * 16;
    auto from = [&](int u, int v) -> int { return __builtin_amdgcn_ds_bpermute(bp + 4 * u, v); };

    int nd, nr, nk;
    float nw;
    load_ids(e, nd, nr, nk, nw);
    bool done = false;
    while (!done) {
        const int md = nd, mr = nr, mk = nk;
        const float mw = nw;
        load_ids(e + 16, nd, nr, nk, nw);                                  // the next batch's ids: in flight while this one is summed
        // Where runs and pieces begin inside the batch, for all 16 edges at once: lane j compares its edge with lane
        // j - 1's (DPP row shift; lane 0 with the walk's state), and a ballot hands every lane its group's 16 flags.
        // The per-edge path of frontier_kernel -- ~100 instructions an edge, on 16 waves per CU whose four groups
        // each branch their own way -- is what hub batches spent their time in, not memory.
        const int mp = p.piece_shift >= 0 ? (mk >> p.piece_shift) : (mk / p.piece_len);
        const int prev_d = __builtin_amdgcn_update_dpp(cur, md, 0x111, 0xf, 0xf, false);          // row_shr:1
        const int prev_p = __builtin_amdgcn_update_dpp(cur_piece, mp, 0x111, 0xf, 0xf, false);
        const int n_valid = min(16, hi - e);
        const bool starts_run = (md != prev_d) && sub < n_valid;
        const bool starts_piece = (starts_run || mp != prev_p) && sub < n_valid;
        const uint32_t run_bits = (uint32_t)(__builtin_amdgcn_ballot_w64(starts_run) >> grp_shift) & 0xffffu;
        const uint32_t piece_bits = (uint32_t)(__builtin_amdgcn_ballot_w64(starts_piece) >> grp_shift) & 0xffffu;
        // a run that begins at or beyond the slice's end belongs to the next group: the walk stops in front of it
        const int room = end - e;                                          // runs may begin at positions < room
        const uint32_t beyond = room >= 16 ? 0u : (room <= 0 ? 0xffffu : (0xffffu << room) & 0xffffu);
        const uint32_t stop_bits = run_bits & beyond;
        const int n_sum = min(n_valid, stop_bits ? __builtin_ctz(stop_bits) : 16);
        done = n_sum < 16;
#pragma unroll
        for (int half = 0; half < 2; ++half) {
            qf4 y[8];
#pragma unroll
            for (int v = 0; v < 8; ++v) {
                const int u = 8 * half + v;
                y[v] = msg[from(u, mr) * 16];
                if constexpr (!UNIT_W) y[v] = __builtin_bit_cast(float, from(u, __builtin_bit_cast(int, mw))) * y[v];
            }
            const uint32_t any = (run_bits | piece_bits) >> (8 * half) & 0xffu;
            if (any == 0u && n_sum >= 8 * half + 8) {                      // eight more terms of the open piece
#pragma unroll
                for (int v = 0; v < 8; ++v) piece = piece + y[v];
                continue;
            }
#pragma unroll
            for (int v = 0; v < 8; ++v) {
                const int u = 8 * half + v;
                if (u < n_sum) {
                    if ((run_bits >> u) & 1u) {
                        close_run(u == 0 ? cur : from(u - 1, md));
                        have_total = false;
                        open = false;
                    }
                    if ((piece_bits >> u) & 1u) {
                        close_piece();
                        open = true;
                        piece = qf4{0.0f, 0.0f, 0.0f, 0.0f};
                    }
                    piece = piece + y[v];
                }
            }
        }
        if (n_sum > 0) {                                                   // the walk's state: the last edge summed
            cur = from(n_sum - 1, md);
            cur_piece = from(n_sum - 1, mp);
        }
        e += 16;
    }
    close_run(cur);
}

// Sparse first layer: every row of the layer's output that the frontier does not touch is ONE vector -- the epilogue of a
// zero input row and a zero update row.  Every workgroup derives it here from the layer's parameters IN THE EPILOGUE KERNEL'S
// ORDER (combine_kernel): the exact-f32 matrix chain  acc = bias; acc = fma(0, w, acc) ...  leaves the bias (finite weights),
// LayerNorm sums its 64 columns as two sequential 32-column halves added once, squares likewise, then
// ((z - mean) * inv) * gamma + beta, relu, + the (zero) shortcut row -- same expressions, same translation unit, -ffp-contract=off,
// so the bits are the epilogue kernel's (tests: equality of the whole layer with the dense form).  Block 0 also lays out the
// row list: slot ranges per query from the plan's run counts (see FrontierParams).
constexpr int kSparseMaxQueries = 128;         // = kCbLdsQueries (the list epilogue keeps the queries' boundary in LDS)
struct ConstFillParams {
    qf4 *out;
    long long n4;
    const float *bias, *gamma, *beta;          // [64]; gamma == NULL: no LayerNorm
    float eps;
    int relu, shortcut;
    const int32_t *src_ptr, *run_prefix, *bnode;
    int n_query;
    int list_len;
    int32_t *list_offset;
};

__global__ __launch_bounds__(256) void const_fill_kernel(const ConstFillParams p) {
    __shared__ __attribute__((aligned(16))) float c[64];
    __shared__ int slots[kSparseMaxQueries];
    if (threadIdx.x < 64) {
        const int j = threadIdx.x;
        float v = p.bias[j];
        if (p.gamma != nullptr) {
            float s0 = 0.0f, s1 = 0.0f;
            for (int k = 0; k < 32; ++k) { s0 = s0 + p.bias[k]; s1 = s1 + p.bias[32 + k]; }
            const float mean = (s0 + s1) * (1.0f / 64.0f);
            float q0 = 0.0f, q1 = 0.0f;
            for (int k = 0; k < 32; ++k) {
                const float d0 = p.bias[k] - mean, d1 = p.bias[32 + k] - mean;
                q0 = q0 + d0 * d0;
                q1 = q1 + d1 * d1;
            }
            const float var = (q0 + q1) * (1.0f / 64.0f);
            const float inv = 1.0f / sqrtf(var + p.eps);
            v = ((v - mean) * inv) * p.gamma[j] + p.beta[j];
        }
        if (p.relu) v = !(v <= 0.0f) ? v : 0.0f;
        c[j] = p.shortcut ? v + 0.0f : v;        // the shortcut adds the (zero) input row
    }
    if (blockIdx.x == 0) {                      // (uniform per block: the barriers below are reached by all its threads)
        // every query's slot count in parallel (three dependent loads each), then one short serial prefix
        if ((int)threadIdx.x < p.n_query) {
            const int h = p.bnode[threadIdx.x];
            const int lo = p.src_ptr[h], hi = p.src_ptr[h + 1];
            slots[threadIdx.x] = (hi > lo ? p.run_prefix[hi - 1] - p.run_prefix[lo] + 1 : 0) + 1;
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            int total = 0;
            for (int b = 0; b < p.n_query; ++b) {
                p.list_offset[b] = total;
                total += slots[b];
            }
            p.list_offset[p.n_query] = total;        // (the epilogue reads min(total, list_len) entries)
        }
    }
    __syncthreads();
    const qf4 *c4 = reinterpret_cast<const qf4 *>(c);
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < p.n4; i += (long long)gridDim.x * 256) p.out[i] = c4[i & 15];
}

// `out` rows the frontier never touches are zero: filled by a kernel (see ultra_rspmm_frontier_f32 for why not a memset)
__global__ __launch_bounds__(256) void zero_fill_kernel(qf4 *out, long long n4) {
    const qf4 zero = {0.0f, 0.0f, 0.0f, 0.0f};
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long long)gridDim.x * 256) out[i] = zero;
}

// ---------------------------------------------------------------------------------------- first layer, backward
// boundary_rows_*: d_input of the FIRST layer of a Bellman-Ford in training.  That layer's input is the boundary
// (ultra/model.py:106-107,116-120): its gradient is consumed at ONE row per query only -- scatter_add_'s backward gathers
// row (anchor_q, q) -- so of the rspmm backward's d_input
//     d_input[u, q-block] = sum over out-edges (u -> v, r):  (grad[v, q-block] * w) * relation[r, q-block]     (mul = mul)
// only the rows u = anchor_q are needed: the out-edges of one node per query instead of all E edges for all queries
// (quad_kernel<DX>: 137-148 us per fine-tuning step on the FB15k237- / WN18RR-shaped graphs).  A hub anchor has tens of
// thousands of out-edges (Zipf heads), so a query's edge list is cut into kBRowsWaves contiguous pieces, one per wave of a
// (slices x queries) grid: a wave sums its piece in edge order -- the indices of the next eight edges are fetched while the
// rows of the current eight are in flight -- and writes a 64-float partial; boundary_rows_reduce_kernel adds a query's
// partials in piece order (deterministic) INTO d_input[anchor_q, q-block], which already holds the epilogue's share
// (rows (anchor_q, q) are distinct for distinct q).
struct BoundaryRowsParams {
    const int32_t *src_ptr;     // [n_src + 1]  (by_src plan order)
    const int32_t *dst;         // [E]          by_src.node_a
    const int32_t *rel;         // [E]
    const float *weight;        // [E] or NULL
    const float *relation;      // [n_rel, F] or NULL (mul = add: no relation factor)
    const float *grad;          // [n_dst, F]   the layer's d_update
    const int32_t *bnode;       // [F / 64]
    float *partial;             // [F / 64, kBRowsWaves, 64]
    float *d_input;             // [n_src, F]
    long long F;
};

constexpr int kBRowsSlices = 64;                        // workgroups per query
constexpr int kBRowsWaves = kBRowsSlices * 4;           // pieces per query

template <bool UNIT_W, bool HAS_REL>
__global__ __launch_bounds__(256) void boundary_rows_partial_kernel(const BoundaryRowsParams p) {
    const int lane = threadIdx.x & 63;
    const int g = blockIdx.x * 4 + uniform(threadIdx.x >> 6);        // piece of the query's edge list
    const int q = blockIdx.y;
    const int u = uniform(p.bnode[q]);
    const int lo = uniform(p.src_ptr[u]), hi = uniform(p.src_ptr[u + 1]);
    const int per = (hi - lo + kBRowsWaves - 1) / kBRowsWaves;
    const int a = lo + g * per;
    const int z = a + per < hi ? a + per : hi;
    const long long col = (long long)q * 64 + lane;
    float acc = 0.0f;
    // lanes 0..7 hold the ids of the batch's eight edges (clamped to the piece's last edge: unused slots re-read it)
    auto ids = [&](int e0, int &v, int &r, float &wt) {
        int e = e0 + (lane & 7);
        e = e < z ? e : z - 1;
        v = p.dst[e];
        r = 0;
        if constexpr (HAS_REL) r = p.rel[e];
        wt = 1.0f;
        if constexpr (!UNIT_W) wt = p.weight[e];
    };
    int v = 0, r = 0;
    float wt = 1.0f;
    if (a < z) ids(a, v, r, wt);
    for (int e0 = a; e0 < z; e0 += 8) {
        int v_next = 0, r_next = 0;
        float wt_next = 1.0f;
        if (e0 + 8 < z) ids(e0 + 8, v_next, r_next, wt_next);       // in flight under this batch's rows
        float gr[8], rr[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const long long vk = __builtin_amdgcn_readlane(v, k);
            gr[k] = p.grad[vk * p.F + col];
            rr[k] = 1.0f;
            if constexpr (HAS_REL) rr[k] = p.relation[(long long)__builtin_amdgcn_readlane(r, k) * p.F + col];
        }
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            if (e0 + k < z) {
                float y = gr[k];
                if constexpr (!UNIT_W) y = y * __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, wt), k));
                if constexpr (HAS_REL) y = y * rr[k];
                acc = acc + y;
            }
        }
        v = v_next; r = r_next; wt = wt_next;
    }
    p.partial[((long long)q * kBRowsWaves + g) * 64 + lane] = acc;
}

__global__ __launch_bounds__(64) void boundary_rows_reduce_kernel(const BoundaryRowsParams p) {
    const int lane = threadIdx.x;
    const int q = blockIdx.x;
    const float *part = p.partial + (long long)q * kBRowsWaves * 64 + lane;
    float total = 0.0f;
#pragma unroll 16
    for (int g = 0; g < kBRowsWaves; ++g) total = total + part[g * 64];
    float *dst = p.d_input + (long long)p.bnode[q] * p.F + (long long)q * 64 + lane;
    *dst = *dst + total;
}

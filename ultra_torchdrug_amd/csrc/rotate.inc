// rotate.inc -- rspmm with RotatE messages on the plan kernels' chunk schedule (included by plan_rotate.hip, inside its
// anonymous namespace).
//
// The message of an edge (u -> v, r, w) for query block b of width D = block (even; column c = b * D + d):
//     pair (b, d), d < H = D / 2:  re = input[u, c] * rel[r, c] - input[u, c + H] * rel[r, c + H]
//                                  im = input[u, c] * rel[r, c + H] + input[u, c + H] * rel[r, c]
//     message = w * (re, im), reduced with (+ | min | max) over the edges of row v
// = layer.message for message_func = "rotate" (ultra/layer.py:69-75, :256-262) with edge_weight applied as in aggregate.
//
// Order of operations (fp32, -ffp-contract=off; torch_ext.cpp's CPU twin evaluates exactly these expressions):
//   forward     y_re = (x_re * r_re) - (x_im * r_im);   y_im = (x_re * r_im) + (x_im * r_re);   [y = w * y];   acc (op)= y
//   d_input     g = output_grad[dst], masked per component by (output == y) for min / max (every tied edge is fed):
//               d_re = (g_re * r_re) + (g_im * r_im);   d_im = (g_im * r_re) - (g_re * r_im);   [d = w * d];   acc += d
//   d_relation  the same with x for r:  d_re = (g_re * x_re) + (g_im * x_im);   d_im = (g_im * x_re) - (g_re * x_im)
//   d_weight    y unweighted, g masked by (output == w * y):  acc += (g_re * y_re) + (g_im * y_im)   (rotate_weight_grad_kernel)
//
// Layout: one lane = one complex pair, one wave = 64 consecutive pairs (a pair tile: 128 columns, the re and im halves
// each contiguous inside a query block).  Each gather is two fully used dword loads per wave.  The rows, chunks, pieces
// and the fix-up pass over split rows are the general kernel's (segment_kernel / fixup_kernel): fixup_kernel reduces
// per column, so it does not care about the pairing, and results do not depend on which wave takes which chunk.
// The relation rows of a pair tile (n_rel x 128 floats) come from LDS where they fit, otherwise from L2.

struct RotParams {
    const int32_t *row;
    const int32_t *node_a;
    const int32_t *node_b;
    const int32_t *rel;
    const float *weight;
    const int4 *chunks;
    const float *relation;   // [n_rel, F]
    const float *input;      // [n_src, F]
    const float *output;     // [n_dst, F]  (min / max backward only)
    const float *grad;       // [n_dst, F]  (backward only)
    const float *add_rows;   // [n_rows, F] (forward only, optional)
    const int32_t *bnode;    // forward only: sparse boundary, row bnode[c / half / 2] holds bvec[c] in column c
    const float *bvec;
    float *out;
    float *partial;          // [n_pieces, F]
    long long F;
    int half;                // block / 2
    int n_pairs;             // F / 2
    int n_chunks;
    int n_rel;
    int n_tiles;             // pair tiles: ceil(n_pairs / 64)
    int split;
    int n_slots;
    int blocks_per_label;
};

__device__ __forceinline__ void rotate_message(float xr, float xi, float rr, float ri, float &yr, float &yi) {
    const float a = xr * rr, b = xi * ri, c = xr * ri, d = xi * rr;
    yr = a - b;
    yi = c + d;
}

template <int KIND, int SUM, bool UNIT_W, bool REL_LDS>
struct RotateWalker {
    static constexpr int RED = (KIND == KIND_FWD) ? SUM : ULTRA_SUM_ADD;
    static constexpr bool MASKED = (KIND != KIND_FWD) && (SUM != ULTRA_SUM_ADD);
    // the per-edge relation pair: forward, d_input; d_relation reads its row's pair only for the mask
    static constexpr bool NEED_REL_ID = (KIND != KIND_DREL);

    const RotParams &p;
    const long long cre;    // this lane's real column (clamped into range for loads)
    const long long cim;
    const bool active;      // pair < n_pairs (stores only)
    const int bq;           // query block of the pair (sparse boundary)
    const float *lds_rel;
    const int lane;
    int cur;
    float acc_re, acc_im;
    bool is_piece;

    __device__ __forceinline__ void load_rel(int r, float &re, float &im) const {
        if constexpr (REL_LDS) {
            re = lds_rel[r * (2 * kTile) + lane];
            im = lds_rel[r * (2 * kTile) + kTile + lane];
        } else {
            re = p.relation[(long long)r * p.F + cre];
            im = p.relation[(long long)r * p.F + cim];
        }
    }
    __device__ __forceinline__ void store_row(int r, float vre, float vim) const {
        if (active) {
            const long long o = (long long)r * p.F;
            if constexpr (KIND == KIND_FWD) {
                if (p.add_rows != nullptr) {
                    vre = reduce<RED>(vre, p.add_rows[o + cre]);
                    vim = reduce<RED>(vim, p.add_rows[o + cim]);
                } else if (p.bnode != nullptr) {
                    const bool hit = r == p.bnode[bq];
                    vre = reduce<RED>(vre, hit ? p.bvec[cre] : 0.0f);
                    vim = reduce<RED>(vim, hit ? p.bvec[cim] : 0.0f);
                }
            }
            p.out[o + cre] = vre;
            p.out[o + cim] = vim;
        }
    }
    __device__ __forceinline__ void close_rows(int upto) {
        store_row(cur, acc_re, acc_im);
        for (int q = cur + 1; q < upto; ++q) store_row(q, identity<RED>(), identity<RED>());
    }

    template <bool FULL>
    __device__ __forceinline__ void batch(const int e0, const int n) {
        int ia[kUnroll], ib[kUnroll], ir[kUnroll], irow[kUnroll];
        float wv[kUnroll];
        float g_re[kUnroll], g_im[kUnroll], x_re[kUnroll], x_im[kUnroll], o_re[kUnroll], o_im[kUnroll];
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
                x_re[u] = p.input[(long long)ia[u] * p.F + cre];
                x_im[u] = p.input[(long long)ia[u] * p.F + cim];
            } else {
                // d_input: rows = source nodes, node_a = destination; d_relation: node_a = source, node_b = destination
                const long long g_row = (KIND == KIND_DX) ? (long long)ia[u] : (long long)ib[u];
                const long long x_row = (KIND == KIND_DX) ? (long long)irow[u] : (long long)ia[u];
                g_re[u] = p.grad[g_row * p.F + cre];
                g_im[u] = p.grad[g_row * p.F + cim];
                if constexpr (MASKED || KIND == KIND_DREL) {
                    x_re[u] = p.input[x_row * p.F + cre];
                    x_im[u] = p.input[x_row * p.F + cim];
                }
                if constexpr (MASKED) {
                    o_re[u] = p.output[g_row * p.F + cre];
                    o_im[u] = p.output[g_row * p.F + cim];
                }
            }
        }
        float r_re[kUnroll], r_im[kUnroll];
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
            r_re[u] = r_im[u] = 0.0f;
            if constexpr (NEED_REL_ID) load_rel(ir[u], r_re[u], r_im[u]);
            if constexpr (KIND == KIND_DREL && MASKED) {
                r_re[u] = p.relation[(long long)irow[u] * p.F + cre];
                r_im[u] = p.relation[(long long)irow[u] * p.F + cim];
            }
        }
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
            if (FULL || u < n) {
                if (!is_piece && irow[u] != cur) {
                    close_rows(irow[u]);
                    cur = irow[u];
                    acc_re = acc_im = identity<RED>();
                }
                if constexpr (KIND == KIND_FWD) {
                    float yr, yi;
                    rotate_message(x_re[u], x_im[u], r_re[u], r_im[u], yr, yi);
                    if constexpr (!UNIT_W) { yr = wv[u] * yr; yi = wv[u] * yi; }
                    acc_re = reduce<RED>(acc_re, yr);
                    acc_im = reduce<RED>(acc_im, yi);
                } else {
                    float gr = g_re[u], gi = g_im[u];
                    if constexpr (MASKED) {
                        float yr, yi;
                        rotate_message(x_re[u], x_im[u], r_re[u], r_im[u], yr, yi);
                        if constexpr (!UNIT_W) { yr = wv[u] * yr; yi = wv[u] * yi; }
                        gr = gr * ((o_re[u] == yr) ? 1.0f : 0.0f);
                        gi = gi * ((o_im[u] == yi) ? 1.0f : 0.0f);
                    }
                    // the factor: relation for d_input, input for d_relation
                    const float fr = (KIND == KIND_DX) ? r_re[u] : x_re[u];
                    const float fi = (KIND == KIND_DX) ? r_im[u] : x_im[u];
                    const float a = gr * fr, b = gi * fi, c = gi * fr, d = gr * fi;
                    float dr = a + b, di = c - d;
                    if constexpr (!UNIT_W) { dr = wv[u] * dr; di = wv[u] * di; }
                    acc_re = acc_re + dr;
                    acc_im = acc_im + di;
                }
            }
        }
    }

    __device__ __forceinline__ void run(const int4 d) {
        is_piece = d.w < 0;
        cur = d.z;
        acc_re = acc_im = identity<RED>();
        int e0 = d.x;
        for (; e0 + kUnroll <= d.y; e0 += kUnroll) batch<true>(e0, kUnroll);
        if (e0 < d.y) batch<false>(e0, d.y - e0);
        if (is_piece) {
            if (active) {
                const long long o = (long long)(-d.w - 1) * p.F;
                p.partial[o + cre] = acc_re;
                p.partial[o + cim] = acc_im;
            }
        } else {
            close_rows(d.w);
        }
    }
};

// Same persistent grid, XCD labels, serpentine deal and LDS ticket counter as segment_kernel; a slot is one pair tile.
template <int KIND, int SUM, bool UNIT_W, bool REL_LDS>
__global__ __launch_bounds__(kBlock) void rotate_segment_kernel(const RotParams p) {
    extern __shared__ __attribute__((aligned(16))) float lds_raw[];
    int *ticket = reinterpret_cast<int *>(lds_raw);
    float *lds_rel = lds_raw + kLdsHeader / sizeof(float);
    const int lane = threadIdx.x & 63;
    const int label = blockIdx.x % kXcd;
    const int bl = blockIdx.x / kXcd;
    const int nb = p.blocks_per_label;

    for (int s = label; s < p.n_slots; s += kXcd) {
        const int tile = s / p.split;
        const int part = s - tile * p.split;
        const int pair = tile * kTile + lane;
        const bool active = pair < p.n_pairs;
        const int lp = active ? pair : p.n_pairs - 1;
        const int bq = lp / p.half;
        const long long cre = (long long)bq * (2 * p.half) + (lp - bq * p.half);
        if constexpr (REL_LDS) {
            // [r][0..63] real halves, [r][64..127] imaginary halves of the tile's 64 pairs
            const int total = p.n_rel * 2 * kTile;
            for (int i = threadIdx.x; i < total; i += kBlock) {
                const int r = i >> 7, j = i & 127;
                const int q = tile * kTile + (j & 63);
                float v = 0.0f;
                if (q < p.n_pairs) {
                    const int b = q / p.half;
                    const long long c = (long long)b * (2 * p.half) + (q - b * p.half) + ((j & 64) ? p.half : 0);
                    v = p.relation[(long long)r * p.F + c];
                }
                lds_rel[i] = v;
            }
        }
        if (threadIdx.x == 0) *ticket = 0;
        __syncthreads();
        for (;;) {
            int t = 0;
            if (lane == 0) t = __hip_atomic_fetch_add(ticket, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            t = uniform(t);
            const int k = part + p.split * (t * nb + ((t & 1) ? (nb - 1 - bl) : bl));
            if (k >= p.n_chunks) break;
            const int4 d = p.chunks[uniform(k)];
            RotateWalker<KIND, SUM, UNIT_W, REL_LDS> walker{p, cre, cre + p.half, active, bq, lds_rel, lane, 0, 0.0f, 0.0f, false};
            walker.run(d);
        }
        __syncthreads();
    }
}

template <int KIND, int SUM>
int launch_rotate_w(const RotParams &p, bool unit_w, bool rel_lds, int grid, size_t lds, hipStream_t stream) {
    return with_bool(unit_w, [&](auto uw) {
        return with_bool(rel_lds, [&](auto rl) {
            constexpr bool UW = decltype(uw)::value, RL = decltype(rl)::value;
            if constexpr (RL && KIND == KIND_DREL) return (int)ULTRA_ERR_BAD_OP;      // rows are relations: no LDS table
            else {
                LaunchRecord rec;
                rec.family = kFamRotate; rec.kind = KIND; rec.sum = SUM; rec.unit_w = UW; rec.rel_lds = RL;
                return launch_recorded(rec, rotate_segment_kernel<KIND, SUM, UW, RL>, p, grid, lds, stream, kBlock);
            }
        });
    });
}

// One plan with rotate messages: the checks of run_plan, rotate_segment_kernel over the chunk schedule, then fixup_kernel
// over the split rows (with the forward's boundary epilogue).  No dense / rowgroup / packed / quad family takes rotate.
template <int KIND>
int run_rotate_plan(const ultra_segments *seg, RotParams p, int64_t n_rel, int64_t F, int64_t block, int sum_op,
                    void *workspace, size_t workspace_bytes, hipStream_t stream) {
    int rc = check_segments(seg);
    if (rc) return rc;
    if (F <= 0 || F > 0x7ffffffeLL || n_rel < 0 || n_rel > 0x7fffffffLL) return ULTRA_ERR_BAD_SHAPE;
    if (block <= 0 || block % 2 != 0 || F % block != 0) return ULTRA_ERR_BAD_SHAPE;
    if (sum_op < 0 || sum_op > 2) return ULTRA_ERR_BAD_OP;
    const size_t need = ultra_rspmm_workspace_bytes(seg, F);
    if (need > 0 && (workspace == nullptr || workspace_bytes < need)) return ULTRA_ERR_WORKSPACE;
    if (seg->n_rows == 0) return ULTRA_OK;

    DeviceInfo *di = nullptr;
    rc = current_device_info(&di);
    if (rc) return rc;

    const int n_pairs = (int)(F / 2);
    const TileGeometry geo = tile_geometry(n_pairs, kTile, di->n_cu);      // a lane is a (re, im) pair
    const size_t lds_need = (size_t)n_rel * 2 * kTile * sizeof(float);
    const bool rel_lds = KIND != KIND_DREL && n_rel > 0 && lds_need <= (size_t)kMaxLdsBytes;

    p.row = seg->row;
    p.node_a = seg->node_a;
    p.node_b = seg->node_b;
    p.rel = seg->rel;
    p.weight = seg->weight;
    p.chunks = reinterpret_cast<const int4 *>(seg->chunks);
    p.partial = static_cast<float *>(workspace);
    p.F = F;
    p.half = (int)(block / 2);
    p.n_pairs = n_pairs;
    p.n_chunks = (int)seg->n_chunks;
    p.n_rel = (int)n_rel;
    p.n_tiles = geo.n_tiles;
    p.split = geo.split;
    p.n_slots = geo.n_slots;
    p.blocks_per_label = geo.blocks_per_label;
    const size_t lds = kLdsHeader + (rel_lds ? lds_need : 0);
    rc = with_sum(sum_op, [&](auto sum) {
        return launch_rotate_w<KIND, decltype(sum)::value>(p, seg->weight == nullptr, rel_lds, geo.grid, lds, stream);
    });
    if (rc) return rc;

    if (seg->n_long_rows > 0) {
        FixParams fp;
        fp.long_rows = seg->long_rows;
        fp.partial = p.partial;
        fp.add_rows = p.add_rows;
        fp.bnode = p.bnode;
        fp.bvec = p.bvec;
        fp.bdim = (int)block;
        fp.out = p.out;
        fp.F = F;
        fp.n_long = (int)seg->n_long_rows;
        fp.n_tiles = (int)((F + kTile - 1) / kTile);        // the fix-up walks plain 64-column tiles
        const long long waves = (long long)fp.n_long * fp.n_tiles;
        const int fgrid = (int)((waves + 3) / 4);
        return launch_fixup(fp, (KIND == KIND_FWD) ? sum_op : ULTRA_SUM_ADD, false, fgrid, stream);
    }
    return ULTRA_OK;
}

// d_weight of the rotate forward, edges in forward-plan order (ultra_rspmm_rotate_backward_weight_f32):
//     d_weight[e] = sum over the pairs of every query block of (g_re * y_re) + (g_im * y_im)
// with y the UNWEIGHTED message of edge e = (u -> v, r, w) and g = output_grad[v], masked per component for min / max by
// (output[v] == w * y) -- every tied edge is fed, as in the d_input / d_relation kernels above.
// One lane = one pair, a wave walks an edge's pair tiles (two fully used dword loads per gathered row and tile), each lane
// sums its tiles in tile order, then the __shfl_down tree.  TWO (n_pairs <= 32: the explain shape B = 1, D = 64 has 32 pairs):
// a wave takes two consecutive edges, one per 32-lane half, so that no lane idles and a wave-instruction still moves two
// whole 128-byte half rows; the tree then stops at offset 16.  Every d_weight entry is written.
template <int SUM, bool UNIT_W, bool TWO>
__global__ __launch_bounds__(256) void rotate_weight_grad_kernel(const int32_t *row, const int32_t *src, const int32_t *rel,
                                                                 const float *weight, const float *relation,
                                                                 const float *input, const float *output, const float *grad,
                                                                 float *d_weight, long long F, int half, int n_pairs,
                                                                 long long n_edges) {
    constexpr int G = TWO ? 32 : 64;                 // lanes per edge
    const int lane = threadIdx.x & 63;
    const int sub = TWO ? (lane >> 5) : 0;
    const int l = lane & (G - 1);
    const long long waves_total = ((long long)gridDim.x * blockDim.x) >> 6;
    const long long n_slots = TWO ? (n_edges + 1) / 2 : n_edges;
    long long slot = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    for (; slot < n_slots; slot += waves_total) {
        const long long e = TWO ? slot * 2 + sub : slot;
        const bool live = e < n_edges;               // the odd last edge leaves the upper half of its wave without one
        const long long ec = live ? e : n_edges - 1;
        const long long v = row[ec], u = src[ec], r = rel[ec];
        float wk = 1.0f;
        if constexpr (!UNIT_W) wk = weight[ec];
        float acc = 0.0f;
        for (int pair = l; pair < n_pairs; pair += G) {
            const int bq = pair / half;
            const long long cre = (long long)bq * (2 * half) + (pair - bq * half);
            const long long cim = cre + half;
            float yr, yi;
            rotate_message(input[u * F + cre], input[u * F + cim], relation[r * F + cre], relation[r * F + cim], yr, yi);
            float gr = grad[v * F + cre], gi = grad[v * F + cim];
            if constexpr (SUM != ULTRA_SUM_ADD) {
                float mr = yr, mi = yi;
                if constexpr (!UNIT_W) { mr = wk * yr; mi = wk * yi; }
                gr = gr * ((output[v * F + cre] == mr) ? 1.0f : 0.0f);
                gi = gi * ((output[v * F + cim] == mi) ? 1.0f : 0.0f);
            }
            const float a = gr * yr, b = gi * yi;
            acc = acc + (a + b);
        }
#pragma unroll
        for (int off = G / 2; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
        if (l == 0 && live) d_weight[e] = acc;
    }
}

template <int SUM>
int launch_rotate_weight_grad(const ultra_segments *fwd, const float *relation, const float *input, const float *output,
                              const float *grad, float *d_weight, long long F, int half, hipStream_t s) {
    const int n_pairs = (int)(F / 2);
    const bool two = n_pairs <= 32, unit = fwd->weight == nullptr;
    const long long n_slots = two ? (fwd->n_edges + 1) / 2 : fwd->n_edges;
    long long blocks = (n_slots + 3) / 4;
    if (blocks > 8192) blocks = 8192;
    return with_bool(unit, [&](auto uw) {
        return with_bool(two, [&](auto tw) -> int {
            hipLaunchKernelGGL((rotate_weight_grad_kernel<SUM, decltype(uw)::value, decltype(tw)::value>), dim3((int)blocks), dim3(256),
                               0, s, fwd->row, fwd->node_a, fwd->rel, fwd->weight, relation, input, output, grad, d_weight, F, half,
                               n_pairs, (long long)fwd->n_edges);
            HIP_TRY(hipGetLastError());
            return ULTRA_OK;
        });
    });
}

// rotate_weight_grad_kernel per query block (ultra_rspmm_rotate_backward_weight_blocks_f32): d_weight[b][e] = the sum above
// over the `half` pairs of query block b alone, query-major, every entry written.  One wave per edge -- ids and weight are read
// once -- walking the blocks in the order rotate_weight_grad_kernel takes on that block's columns alone, so that slice [b]
// carries its bits: lane l sums pairs l, l + 64, ... of the block, then the __shfl_down tree from 32.  TWO (half <= 32, as
// there): one block per 32-lane half of the wave -- blocks 2 i and 2 i + 1 together, a 128-byte half row per load and half
// -- and the tree stops at offset 16.  (The trip count is the wave's: an odd last block leaves the upper half idle, not out.)
template <int SUM, bool UNIT_W, bool TWO>
__global__ __launch_bounds__(256) void rotate_weight_grad_blocks_kernel(const int32_t *row, const int32_t *src, const int32_t *rel,
                                                                        const float *weight, const float *relation,
                                                                        const float *input, const float *output,
                                                                        const float *grad, float *d_weight, long long F,
                                                                        int half, long long n_blocks, long long n_edges) {
    constexpr int G = TWO ? 32 : 64;                 // lanes per block
    constexpr int STEP = TWO ? 2 : 1;                // blocks per wave and trip
    const int lane = threadIdx.x & 63;
    const int sub = TWO ? (lane >> 5) : 0;
    const int l = lane & (G - 1);
    const long long waves_total = ((long long)gridDim.x * blockDim.x) >> 6;
    long long e = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    for (; e < n_edges; e += waves_total) {
        const long long v = row[e], u = src[e], r = rel[e];
        float wk = 1.0f;
        if constexpr (!UNIT_W) wk = weight[e];
        for (long long b0 = 0; b0 < n_blocks; b0 += STEP) {
            const long long bq = b0 + sub;
            const bool live = bq < n_blocks;
            float acc = 0.0f;
            if (live) {
                for (int pair = l; pair < half; pair += G) {
                    const long long cre = bq * (2 * half) + pair;
                    const long long cim = cre + half;
                    float yr, yi;
                    rotate_message(input[u * F + cre], input[u * F + cim], relation[r * F + cre], relation[r * F + cim], yr, yi);
                    float gr = grad[v * F + cre], gi = grad[v * F + cim];
                    if constexpr (SUM != ULTRA_SUM_ADD) {
                        float mr = yr, mi = yi;
                        if constexpr (!UNIT_W) { mr = wk * yr; mi = wk * yi; }
                        gr = gr * ((output[v * F + cre] == mr) ? 1.0f : 0.0f);
                        gi = gi * ((output[v * F + cim] == mi) ? 1.0f : 0.0f);
                    }
                    const float a = gr * yr, b = gi * yi;
                    acc = acc + (a + b);
                }
            }
#pragma unroll
            for (int off = G / 2; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
            if (l == 0 && live) d_weight[bq * n_edges + e] = acc;
        }
    }
}

template <int SUM>
int launch_rotate_weight_grad_blocks(const ultra_segments *fwd, const float *relation, const float *input, const float *output,
                                     const float *grad, float *d_weight, long long F, int half, hipStream_t s) {
    const bool two = half <= 32, unit = fwd->weight == nullptr;
    long long blocks = (fwd->n_edges + 3) / 4;
    if (blocks > 8192) blocks = 8192;
    return with_bool(unit, [&](auto uw) {
        return with_bool(two, [&](auto tw) -> int {
            hipLaunchKernelGGL((rotate_weight_grad_blocks_kernel<SUM, decltype(uw)::value, decltype(tw)::value>), dim3((int)blocks),
                               dim3(256), 0, s, fwd->row, fwd->node_a, fwd->rel, fwd->weight, relation, input, output, grad, d_weight,
                               F, half, F / (2 * half), (long long)fwd->n_edges);
            HIP_TRY(hipGetLastError());
            return ULTRA_OK;
        });
    });
}

// combine_fused_bwd.inc -- the whole backward of the fused layer epilogue in ONE pass over the rows.
// (included by epilogue.hip, after combine_train.inc)
//
//     out = [input +] relu( LayerNorm( Linear_{128->64}( cat[input, update] ) ) )      (ultra/layer.py:386-392, model.py:126-127)
//
// combine_train.inc computes this backward with three kernels -- combine_backward_kernel (recompute z, LayerNorm /
// ReLU backward -> d_z), linear_wgrad_kernel (d_weight) and dxdu_kernel (d_input | d_update) -- which read the same
// rows three times (11 row-sized streams: 8 reads + 3 writes).  On a WN18RR-shaped fine-tuning step (655 k rows per
// layer) those three were 41 % of the step (profiles/r02_train_wn18rr_kernel_stats.csv).  Here a wave keeps a 32-row
// tile in LDS through all three GEMMs: 3 row-sized reads (input, update, grad_out) + 2 writes (d_input, d_update).
//
// Per 32-row tile (one wave, exact-f32 matrix cores, v_mfma_f32_32x32x2_f32):
//   B  z = cat[input, update] . W^T + b            128 MFMAs   same k order as the forward kernel: bit-identical z
//   C  LayerNorm statistics, ReLU mask, LayerNorm backward per row (two lanes per row) -> d_z, kept in LDS;
//      per-lane partial sums of d_gamma, d_beta, d_bias
//   E  d_weight += d_z^T . cat[input, update]       128 MFMAs   64 x 128 accumulator held in 128 VGPRs for the whole run
//   D  [d_input | d_update] = d_z . W               128 MFMAs   same k order as dxdu_kernel: bit-identical results
// W lives once in LDS in its natural [64][128] layout: row reads (b128) feed B, column reads (b32) feed D.
// The next tile's input / update rows are fetched into registers under phase D, grad_out under phase B (one wave per SIMD).
// At 3 x 128 MFMAs of 64 cycles per 32 rows the kernel is bound by the f32 matrix rate (157 TFLOP/s: 49 kFLOP per row),
// with the 1 280 B per row of HBM traffic just below it.
// Outputs per workgroup: a partial d_weight slab and partial d_bias / d_gamma / d_beta rows (its four waves' sums added
// in LDS); combine_reduce_kernel adds the partials in a fixed tree (deterministic, no atomics).

namespace {

constexpr int kFbZStride = 68;                         // z / d_z tile: 64 floats + 4 pad
constexpr int kFbWStride = 132;                        // W in LDS: 128 floats + 4 pad (as the activation tile)
constexpr int kFbTileFloats = kCbRows * kCbStride + kCbRows * kFbZStride;       // per wave: A tile + Z tile

// One level of the recursive-halving column sum: the lane keeps M of its 2 M partial sums (the upper half when `upper`),
// hands the other M to the lane `lane ^ mask` and adds what that lane hands back.
template <int M>
__device__ __forceinline__ void fb_halve(float (&a)[32], bool upper, int mask) {
#pragma unroll
    for (int j = 0; j < M; ++j) {
        const float send = upper ? a[j] : a[j + M];
        const float keep = upper ? a[j + M] : a[j];
        a[j] = keep + __shfl_xor(send, mask, 64);
    }
}

struct FusedBwdParams {
    const float *input;      // [rows, 64]
    const float *update;     // [rows, 64]
    const float *weight;     // [64, 128]
    const float *bias;       // [64]
    const float *gamma;      // [64] or NULL
    const float *beta;       // [64]
    const float *grad_out;   // [rows, 64]
    const float *z;          // HAVE_Z: [rows, 64] the Linear's output kept by the training forward (combine_kernel<.., ZOUT>)
    const int32_t *tile_list;   // LIST: the 32-row tiles to process, in this order; < 0 = padding (d_input / d_update are
    long long n_list;           //       zero-filled before the launch: every other tile's grad_out is zero by the caller's word)
    float *d_input;          // [rows, 64]   d_z . W[:, :64] (+ grad_out when shortcut)
    float *d_update;         // [rows, 64]   d_z . W[:, 64:]
    float *dw_partial;       // [n_workgroups, 64 * 128]
    float *small_partial;    // [n_workgroups, 3, 64]: d_bias | d_gamma | d_beta
    long long rows;
    float eps;
    int relu;
    int shortcut;
    const int32_t *rows_dev;    // optional: the number of rows that hold data, on the device (<= rows; the tiles beyond it are skipped,
                                // the rest of its last tile must be zero rows): compacted row lists whose length the host does not know
};

// HAVE_Z: phase B (the recomputation of z, a third of the matrix work) is replaced by loading the z the forward kept; this
// lane's half rows of z and grad_out for the NEXT tile travel to registers under phases E and D.
// LIST: only the tiles of p.tile_list (the last layer of a Bellman-Ford in training: grad_out is zero outside the rows of the
// candidate entities, ultra/model.py:177-183 -- a tenth of the tiles on a WN18RR-shaped batch).
template <bool HAVE_Z, bool LIST = false>
__global__ __launch_bounds__(kCbWaves * 64, 1) void combine_fused_backward_kernel(const FusedBwdParams p) {
    extern __shared__ __attribute__((aligned(16))) float fb_lds[];
    const int lane = threadIdx.x & 63;
    const int wl = uniform(threadIdx.x >> 6);
    float *w_lds = fb_lds;                                             // [64][kFbWStride]
    float *gb = fb_lds + 64 * kFbWStride;                              // gamma | beta (128 floats)
    float *tile = fb_lds + 64 * kFbWStride + 128 + wl * kFbTileFloats; // [32][kCbStride]: input | update
    float *zt = tile + kCbRows * kCbStride;                            // [32][kFbZStride]: z, then d_z
    const int i = lane & 31, h = lane >> 5;
    long long rows_live = p.rows;
    if (p.rows_dev != nullptr) rows_live = min(rows_live, (long long)uniform(p.rows_dev[0]));
    const long long n_tiles = LIST ? p.n_list : (rows_live + kCbRows - 1) / kCbRows;   // positions of the work list
    const long long wave_global = (long long)blockIdx.x * kCbWaves + wl;
    const long long wave_total = (long long)gridDim.x * kCbWaves;
    const bool has_ln = p.gamma != nullptr;

    for (int idx = threadIdx.x; idx < 64 * 128; idx += kCbWaves * 64) w_lds[(idx >> 7) * kFbWStride + (idx & 127)] = p.weight[idx];
    if (threadIdx.x < 128) gb[threadIdx.x] = has_ln ? (threadIdx.x < 64 ? p.gamma[threadIdx.x] : p.beta[threadIdx.x - 64]) : 0.0f;
    __syncthreads();
    const float bias0 = p.bias[i], bias1 = p.bias[i + 32];
    const int ln_row = lane >> 1, ln_half = lane & 1;

    f32x16 accw[2][4];                                   // d_weight[o = .. + 32 t][k = .. + 32 c], this wave's rows
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int c = 0; c < 4; ++c)
#pragma unroll
            for (int r = 0; r < 16; ++r) accw[t][c][r] = 0.0f;
    // d_bias / d_gamma / d_beta: column sums over the rows.  In phase C a lane holds 32 columns of ONE row, so a tile's
    // column sums are spread over the 32 row slots; a recursive-halving exchange (5 levels, 31 shuffles per array) leaves
    // every lane with the tile's sum of ONE column -- column `sum_col` of its half -- which it adds to a single register.
    // (Keeping 3 x 32 running sums per lane instead would not fit beside the matrix-core operands in 256 VGPRs.)
    float dgam = 0.0f, dbet = 0.0f, dbia = 0.0f;
    auto column_sum = [&](float (&a)[32]) -> float {
        fb_halve<16>(a, ((lane >> 1) & 1) != 0, 2);
        fb_halve<8>(a, ((lane >> 2) & 1) != 0, 4);
        fb_halve<4>(a, ((lane >> 3) & 1) != 0, 8);
        fb_halve<2>(a, ((lane >> 4) & 1) != 0, 16);
        fb_halve<1>(a, ((lane >> 5) & 1) != 0, 32);
        return a[0];
    };
    // the column whose sum ends up in this lane: bit k of the row slot selects the upper half at level k
    const int sum_col = 32 * (lane & 1) + (((lane >> 1) & 1) << 4 | ((lane >> 2) & 1) << 3 | ((lane >> 3) & 1) << 2 |
                                           ((lane >> 4) & 1) << 1 | ((lane >> 5) & 1));

    // Global memory goes through buffer resources: the tile's byte offset is a SCALAR (soffset), the lane's part ONE VGPR,
    // so no per-row 64-bit address lives in a register (the first version kept ~80 of them and spilled: every scratch
    // reload inside a matrix phase then waited, in order, for the HBM prefetch issued before it).  Rows past the end need
    // no clamping and no store guard: the range check returns 0 for them and drops their stores (rows * 256 B < 4 GiB is
    // the host's dispatch condition).
    const uint32_t row_bytes_total = (uint32_t)(p.rows * 256);
    // first row of the tile at position `i` of the work list (wave-uniform); p.rows for padding and past the end: every load
    // of such a tile returns 0 and every store is dropped, its gradients are zero
    auto tile_row = [&](long long i) -> long long {
        if (i >= n_tiles) return p.rows;
        if constexpr (LIST) {
            const long long t = p.tile_list[i];
            return t < 0 ? p.rows : t * kCbRows;
        }
        return i * kCbRows;
    };
    const __amdgpu_buffer_rsrc_t r_in = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(p.input), 0, row_bytes_total, 0x00020000);
    const __amdgpu_buffer_rsrc_t r_up = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(p.update), 0, row_bytes_total, 0x00020000);
    const __amdgpu_buffer_rsrc_t r_go = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(p.grad_out), 0, row_bytes_total, 0x00020000);
    const __amdgpu_buffer_rsrc_t r_z = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(HAVE_Z ? p.z : p.grad_out), 0, row_bytes_total, 0x00020000);
    const __amdgpu_buffer_rsrc_t r_dx = __builtin_amdgcn_make_buffer_rsrc(p.d_input, 0, row_bytes_total, 0x00020000);
    const __amdgpu_buffer_rsrc_t r_du = __builtin_amdgcn_make_buffer_rsrc(p.d_update, 0, row_bytes_total, 0x00020000);
    const uint32_t v_tile = (uint32_t)(lane >> 4) * 256u + (uint32_t)(lane & 15) * 16u;   // row (lane >> 4) of a 4-row, 1-KiB slab
    const uint32_t v_half = (uint32_t)ln_row * 256u + (uint32_t)ln_half * 128u;           // this lane's half row
    auto load4 = [&](__amdgpu_buffer_rsrc_t rs, uint32_t voff, uint32_t soff) -> f32x4 {
        return __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, voff, soff, 0));
    };
    // Register budget: everything that is not an MFMA accumulator must fit the 256 architectural VGPRs.  The next tile's
    // rows (64 VGPRs) are only in flight during phase D, whose 8 k cycles of matrix work hide the fetch; grad_out is
    // fetched under phase B.
    if (wave_global < n_tiles) {                         // first tile only: rows -> registers -> LDS, latency exposed
        const uint32_t s0 = (uint32_t)tile_row(wave_global) * 256u;
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const int r = 4 * q + (lane >> 4), c = (lane & 15) * 4;
            *reinterpret_cast<f32x4 *>(tile + r * kCbStride + c) = load4(r_in, v_tile, s0 + 1024u * q);
            *reinterpret_cast<f32x4 *>(tile + r * kCbStride + 64 + c) = load4(r_up, v_tile, s0 + 1024u * q);
        }
    }

    f32x4 gq[8], zq[8];
    if constexpr (HAVE_Z) {                              // first tile: latency exposed, like the rows above
        if (wave_global < n_tiles) {
            const uint32_t s0 = (uint32_t)tile_row(wave_global) * 256u;
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                gq[q] = load4(r_go, v_half + 16u * q, s0);
                zq[q] = load4(r_z, v_half + 16u * q, s0);
            }
        }
    }
    for (long long t = wave_global; t < n_tiles; t += wave_total) {
        const long long row0 = tile_row(t);
        // LIST: the list is ascending and -1 padded at its END, and a wave's positions ascend: the first padding entry ends its
        // work (round 5: a first-layer list sized for the worst case -- queries x (max runs + 1) slots -- made the kernel walk
        // 100 k+ empty positions at a full tile's cost each: 1.5 ms)
        if constexpr (LIST) {
            if (row0 >= p.rows) break;
        }
        const uint32_t s_row0 = (uint32_t)row0 * 256u;
        // ---- this lane's half row of grad_out: in flight during phase B, consumed in phase C
        if constexpr (!HAVE_Z) {
#pragma unroll
            for (int q = 0; q < 8; ++q) gq[q] = load4(r_go, v_half + 16u * q, s_row0);
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");          // the activation tile is in LDS

        if constexpr (!HAVE_Z) {
        // ---- B: recompute z (k order in[0], up[0], in[1], up[1], ... from the bias: the forward kernel's chain)
        f32x16 acc0, acc1;
#pragma unroll
        for (int r = 0; r < 16; ++r) { acc0[r] = bias0; acc1[r] = bias1; }
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const f32x4 av = *reinterpret_cast<const f32x4 *>(tile + i * kCbStride + 64 * h + 4 * q);
            const f32x4 w0 = *reinterpret_cast<const f32x4 *>(w_lds + i * kFbWStride + 64 * h + 4 * q);
            const f32x4 w1 = *reinterpret_cast<const f32x4 *>(w_lds + (i + 32) * kFbWStride + 64 * h + 4 * q);
            acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(av.x, w0.x, acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(av.x, w1.x, acc1, 0, 0, 0);
            acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(av.y, w0.y, acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(av.y, w1.y, acc1, 0, 0, 0);
            acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(av.z, w0.z, acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(av.z, w1.z, acc1, 0, 0, 0);
            acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(av.w, w0.w, acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(av.w, w1.w, acc1, 0, 0, 0);
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = (r & 3) + 8 * (r >> 2) + 4 * h;
            zt[row * kFbZStride + i] = acc0[r];
            zt[row * kFbZStride + 32 + i] = acc1[r];
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        }

        // ---- C: per row (two lanes, 32 columns each): LayerNorm statistics, ReLU mask, LayerNorm backward
        float v[32], g[32];
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            f32x4 d;
            if constexpr (HAVE_Z) d = zq[q];
            else d = *reinterpret_cast<const f32x4 *>(zt + ln_row * kFbZStride + 32 * ln_half + 4 * q);
            v[4 * q + 0] = d.x; v[4 * q + 1] = d.y; v[4 * q + 2] = d.z; v[4 * q + 3] = d.w;
            g[4 * q + 0] = gq[q].x; g[4 * q + 1] = gq[q].y; g[4 * q + 2] = gq[q].z; g[4 * q + 3] = gq[q].w;
        }
        if constexpr (HAVE_Z) {          // the NEXT tile's half rows: in flight under phases E and D
            const long long t_nx = t + wave_total;
            const uint32_t s_nx = (uint32_t)tile_row(t_nx) * 256u;
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                gq[q] = load4(r_go, v_half + 16u * q, s_nx);
                zq[q] = load4(r_z, v_half + 16u * q, s_nx);
            }
        }
        const float valid = (row0 + ln_row < p.rows) ? 1.0f : 0.0f;   // rows past the end are clamped copies
        if (has_ln) {
            float s = 0.0f;
#pragma unroll
            for (int c = 0; c < 32; ++c) s = s + v[c];
            const float so = __shfl_xor(s, 1, 64);
            const float mean = (ln_half == 0 ? s + so : so + s) * (1.0f / 64.0f);
            float ss = 0.0f;
#pragma unroll
            for (int c = 0; c < 32; ++c) { const float dlt = v[c] - mean; ss = ss + dlt * dlt; }
            const float sso = __shfl_xor(ss, 1, 64);
            const float var = (ln_half == 0 ? ss + sso : sso + ss) * (1.0f / 64.0f);
            const float rstd = 1.0f / sqrtf(var + p.eps);
            float s1 = 0.0f, s2 = 0.0f;
            float gcs[32], gxs[32];                      // gc and gc * xhat of this row half: summed over the rows below
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const f32x4 gm = *reinterpret_cast<const f32x4 *>(gb + 32 * ln_half + 4 * q);
                const f32x4 bt = *reinterpret_cast<const f32x4 *>(gb + 64 + 32 * ln_half + 4 * q);
                const float gam4[4] = {gm.x, gm.y, gm.z, gm.w};
                const float bet4[4] = {bt.x, bt.y, bt.z, bt.w};
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int c = 4 * q + j;
                    const float xh = (v[c] - mean) * rstd;
                    const float y = xh * gam4[j] + bet4[j];
                    float gc = g[c] * valid;
                    if (p.relu) gc = y > 0.0f ? gc : 0.0f;
                    gcs[c] = gc;
                    gxs[c] = gc * xh;
                    const float a = gc * gam4[j];
                    s1 = s1 + a;
                    s2 = s2 + a * xh;
                    v[c] = xh;
                    g[c] = a;
                }
            }
            dbet = dbet + column_sum(gcs);
            dgam = dgam + column_sum(gxs);
            const float s1o = __shfl_xor(s1, 1, 64), s2o = __shfl_xor(s2, 1, 64);
            const float m1 = (ln_half == 0 ? s1 + s1o : s1o + s1) * (1.0f / 64.0f);
            const float m2 = (ln_half == 0 ? s2 + s2o : s2o + s2) * (1.0f / 64.0f);
#pragma unroll
            for (int c = 0; c < 32; ++c) g[c] = rstd * ((g[c] - m1) - v[c] * m2);
        } else {
#pragma unroll
            for (int c = 0; c < 32; ++c) {
                float gc = g[c] * valid;
                if (p.relu) gc = v[c] > 0.0f ? gc : 0.0f;
                g[c] = gc;
            }
        }
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            f32x4 d;
            d.x = g[4 * q + 0]; d.y = g[4 * q + 1]; d.z = g[4 * q + 2]; d.w = g[4 * q + 3];
            *reinterpret_cast<f32x4 *>(zt + ln_row * kFbZStride + 32 * ln_half + 4 * q) = d;
        }
        dbia = dbia + column_sum(g);                                   // d_bias = column sums of d_z
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");

        // ---- E: d_weight += d_z^T . cat[input, update]; per pair of rows: A = d_z[row + h][i + 32 t], B = act[row + h][i + 32 c]
#pragma unroll 4
        for (int s = 0; s < 16; ++s) {
            const int row = 2 * s + h;
            const float a0 = zt[row * kFbZStride + i], a1 = zt[row * kFbZStride + 32 + i];
            const float b0 = tile[row * kCbStride + i], b1 = tile[row * kCbStride + 32 + i];
            const float b2 = tile[row * kCbStride + 64 + i], b3 = tile[row * kCbStride + 96 + i];
            accw[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, accw[0][0], 0, 0, 0);
            accw[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, accw[0][1], 0, 0, 0);
            accw[0][2] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b2, accw[0][2], 0, 0, 0);
            accw[0][3] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b3, accw[0][3], 0, 0, 0);
            accw[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, accw[1][0], 0, 0, 0);
            accw[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, accw[1][1], 0, 0, 0);
            accw[1][2] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b2, accw[1][2], 0, 0, 0);
            accw[1][3] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b3, accw[1][3], 0, 0, 0);
        }

        // ---- D: [d_input | d_update] = d_z . W   (k order o = 0, 32, 1, 33, ...: dxdu_kernel's chain)
        // the next tile's rows travel to registers meanwhile (phase E was the last reader of the activation tile)
        const long long t_next = t + wave_total;           // (past the last tile the range check returns zeros: never used)
        f32x4 pa[8], pb[8];
        {
            const uint32_t s_next = (uint32_t)tile_row(t_next) * 256u;
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                pa[q] = load4(r_in, v_tile, s_next + 1024u * q);
                pb[q] = load4(r_up, v_tile, s_next + 1024u * q);
            }
        }
        // the shortcut's pass-through gradient for the d_input half, fetched in the accumulators' own layout
        // (lane (i, h), register r <-> row (r & 3) + 8 (r >> 2) + 4 h, column i + 32 tt)
        const uint32_t v_acc = (uint32_t)h * 1024u + (uint32_t)i * 4u;
        float go[2][16];
        if (p.shortcut) {
#pragma unroll
            for (int tt = 0; tt < 2; ++tt)
#pragma unroll
                for (int r = 0; r < 16; ++r)
                    go[tt][r] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(
                                                              r_go, v_acc, s_row0 + (uint32_t)(((r & 3) + 8 * (r >> 2)) * 256 + 128 * tt), 0));
        }
        f32x16 acc[4];
#pragma unroll
        for (int tt = 0; tt < 4; ++tt)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[tt][r] = 0.0f;
#pragma unroll 2
        for (int q = 0; q < 8; ++q) {
            const f32x4 av = *reinterpret_cast<const f32x4 *>(zt + i * kFbZStride + 32 * h + 4 * q);
            const float *wcol = w_lds + (32 * h + 4 * q) * kFbWStride + i;
#pragma unroll
            for (int tt = 0; tt < 4; ++tt) {
                acc[tt] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.x, wcol[0 * kFbWStride + 32 * tt], acc[tt], 0, 0, 0);
                acc[tt] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.y, wcol[1 * kFbWStride + 32 * tt], acc[tt], 0, 0, 0);
                acc[tt] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.z, wcol[2 * kFbWStride + 32 * tt], acc[tt], 0, 0, 0);
                acc[tt] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.w, wcol[3 * kFbWStride + 32 * tt], acc[tt], 0, 0, 0);
            }
        }
        // The activation tile has been free since phase E: the next tile's rows go in now.  Their loads were issued
        // before the matrix phase and the stores below are issued after this point, so the wait covers only them
        // (staging the results through this tile first made every iteration wait for its own stores to retire).
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const int r = 4 * q + (lane >> 4), c = (lane & 15) * 4;
            *reinterpret_cast<f32x4 *>(tile + r * kCbStride + c) = pa[q];
            *reinterpret_cast<f32x4 *>(tile + r * kCbStride + 64 + c) = pb[q];
        }
        // results leave straight from the accumulator layout: one store = two rows x 128 contiguous bytes (whole lines)
#pragma unroll
        for (int tt = 0; tt < 4; ++tt)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                float v = acc[tt][r];
                if (tt < 2 && p.shortcut) v = v + go[tt & 1][r];
                const uint32_t soff = s_row0 + (uint32_t)(((r & 3) + 8 * (r >> 2)) * 256 + 128 * (tt & 1));
                __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(uint32_t, v), tt < 2 ? r_dx : r_du, v_acc, soff, 0);
            }
    }

    // ---- partial results: the four waves of the workgroup add theirs in LDS (wave order), one slab per workgroup
    __syncthreads();                                     // every wave is done with the tiles and with W: LDS is free
    {
        float *slab = fb_lds + wl * (64 * 128);          // 4 x 32 KB <= the 134 KB this kernel holds
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int c = 0; c < 4; ++c)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int o = (r & 3) + 8 * (r >> 2) + 4 * h + 32 * t;
                    slab[o * 128 + 32 * c + i] = accw[t][c][r];
                }
    }
    __syncthreads();
    float *out = p.dw_partial + (long long)blockIdx.x * (64 * 128);
    for (int idx = threadIdx.x; idx < 64 * 128; idx += kCbWaves * 64)
        out[idx] = ((fb_lds[idx] + fb_lds[64 * 128 + idx]) + fb_lds[2 * 64 * 128 + idx]) + fb_lds[3 * 64 * 128 + idx];
    __syncthreads();
    float *small = fb_lds;                               // [4 waves][3][64]
    small[wl * 192 + sum_col] = dbia;
    small[wl * 192 + 64 + sum_col] = dgam;
    small[wl * 192 + 128 + sum_col] = dbet;
    __syncthreads();
    if (threadIdx.x < 192)
        p.small_partial[(long long)blockIdx.x * 192 + threadIdx.x] =
            ((small[threadIdx.x] + small[192 + threadIdx.x]) + small[384 + threadIdx.x]) + small[576 + threadIdx.x];
}

// d_weight / d_bias / d_gamma / d_beta = the workgroups' partials added in a fixed tree: a block owns 64 outputs, its 16
// waves each add every 16th slab in order, then the 16 sums are added in wave order.
__global__ __launch_bounds__(1024) void combine_reduce_kernel(const float *dw_partial, const float *small_partial, int n_slabs,
                                                              float *d_weight, float *d_bias, float *d_gamma, float *d_beta) {
    __shared__ float part[16][64];
    const int lane = threadIdx.x & 63, wq = threadIdx.x >> 6;
    const int idx = blockIdx.x * 64 + lane;              // 128 blocks: d_weight; 3 more: the small vectors
    const bool is_w = idx < 64 * 128;
    const float *src = is_w ? dw_partial + idx : small_partial + (idx - 64 * 128);
    const long long stride = is_w ? 64 * 128 : 192;
    float s = 0.0f;
    for (int w = wq; w < n_slabs; w += 16) s = s + src[(long long)w * stride];
    part[wq][lane] = s;
    __syncthreads();
    if (wq == 0) {
        float total = part[0][lane];
#pragma unroll
        for (int k = 1; k < 16; ++k) total = total + part[k][lane];
        if (is_w) {
            d_weight[idx] = total;
        } else {
            const int k = idx - 64 * 128, which = k >> 6, col = k & 63;
            float *dst = which == 0 ? d_bias : (which == 1 ? d_gamma : d_beta);
            if (dst != nullptr) dst[col] = total;
        }
    }
}

}  // namespace

extern "C" {

int ultra_combine_backward_fused_waves(int device, int64_t rows, int *n_waves) {
    DeviceInfo *di = nullptr;
    int rc = device_info(device, &di);
    if (rc) return rc;
    const long long n_tiles = (rows + kCbRows - 1) / kCbRows;
    long long blocks = (n_tiles + kCbWaves - 1) / kCbWaves;
    if (blocks > di->n_cu) blocks = di->n_cu;
    if (blocks < 1) blocks = 1;
    if (n_waves) *n_waves = (int)(blocks * kCbWaves);
    return ULTRA_OK;
}

// fill: bit 0 -- zero d_input outside the listed tiles, bit 1 -- zero d_update (tile_list given only)
static int combine_backward_fused_impl(const float *input, const float *update, const float *weight, const float *bias,
                                       const float *ln_weight, const float *ln_bias, float ln_eps, int relu, int shortcut,
                                       const float *grad_out, const float *z, float *d_input, float *d_update, float *d_weight,
                                       float *d_bias, float *d_ln_weight, float *d_ln_bias, float *partial_workspace,
                                       size_t workspace_bytes, const int32_t *tile_list, int64_t n_list, int64_t rows, int64_t dim,
                                       int fill, const int32_t *rows_dev, void *stream) {
    if (dim != 64 || rows < 0 || rows > (1LL << 24) - 64 || n_list < 0) return ULTRA_ERR_BAD_SHAPE;     // 32-bit buffer offsets: (rows + a tile) * 256 B < 4 GiB
    if (rows == 0) return ULTRA_OK;
    if (input == nullptr || update == nullptr || weight == nullptr || bias == nullptr || grad_out == nullptr ||
        d_input == nullptr || d_update == nullptr || d_weight == nullptr || partial_workspace == nullptr)
        return ULTRA_ERR_NULL_POINTER;
    if (ln_weight != nullptr && ln_bias == nullptr) return ULTRA_ERR_NULL_POINTER;
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    int n_waves = 0;
    int rc = ultra_combine_backward_fused_waves(dev, rows, &n_waves);
    if (rc) return rc;
    if (workspace_bytes < (size_t)n_waves * (64 * 128 + 192) * sizeof(float)) return ULTRA_ERR_WORKSPACE;
    hipStream_t s = static_cast<hipStream_t>(stream);
    FusedBwdParams p;
    p.input = input; p.update = update; p.weight = weight; p.bias = bias; p.gamma = ln_weight; p.beta = ln_bias;
    p.grad_out = grad_out; p.z = z; p.d_input = d_input; p.d_update = d_update;
    p.dw_partial = partial_workspace;
    p.small_partial = partial_workspace + (size_t)(n_waves / kCbWaves) * (64 * 128);
    p.rows = rows; p.eps = ln_eps; p.relu = relu; p.shortcut = shortcut; p.rows_dev = rows_dev;
    const size_t lds = (size_t)(64 * kFbWStride + 128 + kCbWaves * kFbTileFloats) * sizeof(float);
    p.tile_list = tile_list; p.n_list = n_list;
    if (tile_list != nullptr) {
        // only the listed tiles are computed: everything else of d_input / d_update is zero (fill kernels, not memset nodes:
        // see ultra_rspmm_frontier_f32)
        const long long n4 = rows * 16;
        const unsigned fb = (unsigned)((n4 + 256 * 8 - 1) / (256 * 8) < 4096 ? (n4 + 256 * 8 - 1) / (256 * 8) : 4096);
        if (fill & 1) hipLaunchKernelGGL(zero_fill_kernel, dim3(fb ? fb : 1), dim3(256), 0, s, reinterpret_cast<qf4 *>(d_input), n4);
        if (fill & 2) hipLaunchKernelGGL(zero_fill_kernel, dim3(fb ? fb : 1), dim3(256), 0, s, reinterpret_cast<qf4 *>(d_update), n4);
        HIP_TRY(hipGetLastError());
        rc = ensure_lds_attribute(reinterpret_cast<const void *>(combine_fused_backward_kernel<false, true>), lds);
        if (rc) return rc;
        hipLaunchKernelGGL((combine_fused_backward_kernel<false, true>), dim3(n_waves / kCbWaves), dim3(kCbWaves * 64), lds, s, p);
    } else if (z != nullptr) {
        rc = ensure_lds_attribute(reinterpret_cast<const void *>(combine_fused_backward_kernel<true>), lds);      // (< kMaxLdsBytes)
        if (rc) return rc;
        hipLaunchKernelGGL(combine_fused_backward_kernel<true>, dim3(n_waves / kCbWaves), dim3(kCbWaves * 64), lds, s, p);
    } else {
        rc = ensure_lds_attribute(reinterpret_cast<const void *>(combine_fused_backward_kernel<false>), lds);
        if (rc) return rc;
        hipLaunchKernelGGL(combine_fused_backward_kernel<false>, dim3(n_waves / kCbWaves), dim3(kCbWaves * 64), lds, s, p);
    }
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(combine_reduce_kernel, dim3(128 + 3), dim3(1024), 0, s, p.dw_partial, p.small_partial,
                       n_waves / kCbWaves, d_weight, d_bias, ln_weight != nullptr ? d_ln_weight : nullptr,
                       ln_weight != nullptr ? d_ln_bias : nullptr);
    HIP_TRY(hipGetLastError());
    return ULTRA_OK;
}

int ultra_combine_backward_fused_f32(const float *input, const float *update, const float *weight, const float *bias,
                                     const float *ln_weight, const float *ln_bias, float ln_eps, int relu, int shortcut,
                                     const float *grad_out, const float *z, float *d_input, float *d_update, float *d_weight,
                                     float *d_bias, float *d_ln_weight, float *d_ln_bias, float *partial_workspace,
                                     size_t workspace_bytes, const int32_t *tile_list, int64_t n_list, int64_t rows, int64_t dim,
                                     void *stream) {
    return combine_backward_fused_impl(input, update, weight, bias, ln_weight, ln_bias, ln_eps, relu, shortcut, grad_out, z, d_input,
                                       d_update, d_weight, d_bias, d_ln_weight, d_ln_bias, partial_workspace, workspace_bytes,
                                       tile_list, n_list, rows, dim, 3, nullptr, stream);
}

}  // extern "C"

// combine_train.inc -- backward of the fused layer epilogue (included by epilogue.hip, after its kernels).
//
// Training counterpart of combine_kernel.  The reference runs the epilogue as ATen ops
//     output = self.linear(torch.cat([input, update], dim=-1)); layer_norm; relu        (ultra/layer.py:386-392)
//     hidden = hidden + layer_input                                                     (ultra/model.py:126-127)
// and autograd differentiates them one by one: on a WN18RR-shaped fine-tuning step (655 k rows) those launches are
// 90 % of the GPU time, the weight-gradient GEMM alone (64 x 655k x 128 through rocBLAS) 25 %.  Here:
//   combine_backward_kernel : recomputes z = Linear(cat[input, update]) on the f32 matrix cores (nothing but the
//       layer's inputs is kept from the forward), then LayerNorm-backward and the ReLU mask per row, and writes
//       d_z = dL/dz [rows, 64] plus per-wave partial sums of d_gamma / d_beta;
//   linear_wgrad_kernel     : d_weight = d_z^T . cat[input, update] as a row-split MFMA reduction with per-wave
//       partial slabs (no atomics; the slabs are summed in wave order afterwards).
//   dxdu_kernel             : d_input = [grad_out +] d_z . W[:, :64] and d_update = d_z . W[:, 64:] in one pass over
//       d_z on the matrix cores (ultra_combine_dxdu_f32; the shortcut's pass-through fused).

namespace {

struct CombineBwdParams {
    const float *input;      // [rows, 64]
    const float *update;     // [rows, 64]
    const float *weight;     // [64, 128]
    const float *bias;       // [64]
    const float *gamma;      // [64] or NULL
    const float *beta;       // [64]
    const float *grad_out;   // [rows, 64]  dL/d(out)
    float *d_z;              // [rows, 64]
    float *d_gamma_partial;  // [n_waves, 64]
    float *d_beta_partial;   // [n_waves, 64]
    long long rows;
    float eps;
    int relu;
};

__global__ __launch_bounds__(kCbWaves * 64, 1) void combine_backward_kernel(const CombineBwdParams p) {
    extern __shared__ __attribute__((aligned(16))) float cb_lds[];
    const int lane = threadIdx.x & 63;
    const int wl = uniform(threadIdx.x >> 6);
    float *tile = cb_lds + wl * kCbTileFloats;
    const int i = lane & 31, h = lane >> 5;
    const long long n_tiles = (p.rows + kCbRows - 1) / kCbRows;
    const long long wave_global = (long long)blockIdx.x * kCbWaves + wl;
    const long long wave_total = (long long)gridDim.x * kCbWaves;

    float w0[64], w1[64];
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        const f32x4 a = *reinterpret_cast<const f32x4 *>(p.weight + (long long)i * 128 + 64 * h + 4 * q);
        const f32x4 b = *reinterpret_cast<const f32x4 *>(p.weight + (long long)(i + 32) * 128 + 64 * h + 4 * q);
        w0[4 * q + 0] = a.x; w0[4 * q + 1] = a.y; w0[4 * q + 2] = a.z; w0[4 * q + 3] = a.w;
        w1[4 * q + 0] = b.x; w1[4 * q + 1] = b.y; w1[4 * q + 2] = b.z; w1[4 * q + 3] = b.w;
    }
    const float bias0 = p.bias[i], bias1 = p.bias[i + 32];
    const int ln_row = lane >> 1, ln_half = lane & 1;
    const bool has_ln = p.gamma != nullptr;
    float *gb = cb_lds + kCbWaves * kCbTileFloats;           // gamma | beta, shared by the workgroup
    if (has_ln && threadIdx.x < 128) gb[threadIdx.x] = threadIdx.x < 64 ? p.gamma[threadIdx.x] : p.beta[threadIdx.x - 64];
    __syncthreads();
    float dgam[32], dbet[32];
#pragma unroll
    for (int c = 0; c < 32; ++c) {
        dgam[c] = 0.0f;
        dbet[c] = 0.0f;
    }

    for (long long t = wave_global; t < n_tiles; t += wave_total) {
        const long long row0 = t * kCbRows;
        const long long last = p.rows - 1;
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const int r = 4 * q + (lane >> 4), c = (lane & 15) * 4;
            long long gr = row0 + r;
            gr = gr < last ? gr : last;
            const f32x4 a = *reinterpret_cast<const f32x4 *>(p.input + gr * 64 + c);
            const f32x4 b = *reinterpret_cast<const f32x4 *>(p.update + gr * 64 + c);
            *reinterpret_cast<f32x4 *>(tile + r * kCbStride + c) = a;
            *reinterpret_cast<f32x4 *>(tile + r * kCbStride + 64 + c) = b;
        }
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");

        // ---- recompute z (same k order as the forward kernel)
        f32x16 acc0, acc1;
#pragma unroll
        for (int r = 0; r < 16; ++r) { acc0[r] = bias0; acc1[r] = bias1; }
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const f32x4 av = *reinterpret_cast<const f32x4 *>(tile + i * kCbStride + 64 * h + 4 * q);
            acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(av.x, w0[4 * q + 0], acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(av.x, w1[4 * q + 0], acc1, 0, 0, 0);
            acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(av.y, w0[4 * q + 1], acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(av.y, w1[4 * q + 1], acc1, 0, 0, 0);
            acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(av.z, w0[4 * q + 2], acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(av.z, w1[4 * q + 2], acc1, 0, 0, 0);
            acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(av.w, w0[4 * q + 3], acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(av.w, w1[4 * q + 3], acc1, 0, 0, 0);
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");

        // ---- z -> LDS (update half), dL/d(out) tile -> LDS (input half; the activations are consumed)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = (r & 3) + 8 * (r >> 2) + 4 * h;
            tile[row * kCbStride + 64 + i] = acc0[r];
            tile[row * kCbStride + 96 + i] = acc1[r];
        }
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const int r = 4 * q + (lane >> 4), c = (lane & 15) * 4;
            long long gr = row0 + r;
            gr = gr < last ? gr : last;
            const f32x4 gq = *reinterpret_cast<const f32x4 *>(p.grad_out + gr * 64 + c);
            *reinterpret_cast<f32x4 *>(tile + r * kCbStride + c) = gq;
        }
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");

        // ---- per row (two lanes, 32 columns each): LayerNorm statistics, ReLU mask, LayerNorm backward
        float v[32], g[32];
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const f32x4 d = *reinterpret_cast<const f32x4 *>(tile + ln_row * kCbStride + 64 + 32 * ln_half + 4 * q);
            const f32x4 e = *reinterpret_cast<const f32x4 *>(tile + ln_row * kCbStride + 32 * ln_half + 4 * q);
            v[4 * q + 0] = d.x; v[4 * q + 1] = d.y; v[4 * q + 2] = d.z; v[4 * q + 3] = d.w;
            g[4 * q + 0] = e.x; g[4 * q + 1] = e.y; g[4 * q + 2] = e.z; g[4 * q + 3] = e.w;
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
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const f32x4 gq = *reinterpret_cast<const f32x4 *>(gb + 32 * ln_half + 4 * q);
                const f32x4 bq = *reinterpret_cast<const f32x4 *>(gb + 64 + 32 * ln_half + 4 * q);
                const float gam4[4] = {gq.x, gq.y, gq.z, gq.w};
                const float bet4[4] = {bq.x, bq.y, bq.z, bq.w};
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int c = 4 * q + j;
                    const float xh = (v[c] - mean) * rstd;
                    const float y = xh * gam4[j] + bet4[j];
                    float gc = g[c] * valid;
                    if (p.relu) gc = y > 0.0f ? gc : 0.0f;
                    dbet[c] = dbet[c] + gc;
                    dgam[c] = dgam[c] + gc * xh;
                    const float a = gc * gam4[j];
                    s1 = s1 + a;
                    s2 = s2 + a * xh;
                    v[c] = xh;
                    g[c] = a;
                }
            }
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
            *reinterpret_cast<f32x4 *>(tile + ln_row * kCbStride + 64 + 32 * ln_half + 4 * q) = d;
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const int r = 4 * q + (lane >> 4), c = (lane & 15) * 4;
            const f32x4 d = *reinterpret_cast<const f32x4 *>(tile + r * kCbStride + 64 + c);
            if (row0 + r < p.rows) *reinterpret_cast<f32x4 *>(p.d_z + (row0 + r) * 64 + c) = d;
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    }

    // ---- per-wave partial d_gamma / d_beta: lane (row, half) holds 32 column sums; add the 32 rows in row order
    if (has_ln && wave_global < wave_total) {
#pragma unroll
        for (int c = 0; c < 32; ++c) {
            tile[lane * 64 + c] = dgam[c];
            tile[lane * 64 + 32 + c] = dbet[c];
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        const int half = lane >> 5, k = lane & 31;      // this lane reduces output column `lane`
        float sg = 0.0f, sb = 0.0f;
        for (int r = 0; r < 32; ++r) {
            sg = sg + tile[(2 * r + half) * 64 + k];
            sb = sb + tile[(2 * r + half) * 64 + 32 + k];
        }
        p.d_gamma_partial[wave_global * 64 + lane] = sg;
        p.d_beta_partial[wave_global * 64 + lane] = sb;
    }
}

struct WGradParams {
    const float *d_z;      // [rows, 64]
    const float *input;    // [rows, 64]
    const float *update;   // [rows, 64]
    float *partial;        // [n_waves, 64 * 128]
    float *bias_partial;   // [n_waves, 64] column sums of d_z (= d_bias partials) or NULL
    long long rows;
    long long rows_per_wave;   // even
};

// d_weight[o][k] = sum_rows d_z[row][o] * cat[input, update][row][k]:  D[64 x 128] += A[64 x 2] . B[2 x 128] per pair of
// rows; lane (i, h): A = d_z[row + h][i + 32 t], B = act[row + h][i + 32 c] -- both plain coalesced dword loads.
__global__ __launch_bounds__(kCbWaves * 64, 2) void linear_wgrad_kernel(const WGradParams p) {
    const int lane = threadIdx.x & 63;
    const int i = lane & 31, h = lane >> 5;
    const long long wave_global = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const long long r_begin = wave_global * p.rows_per_wave;
    long long r_end = r_begin + p.rows_per_wave;
    if (r_end > p.rows) r_end = p.rows;
    f32x16 acc[2][4];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int c = 0; c < 4; ++c)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[t][c][r] = 0.0f;
    float bsum0 = 0.0f, bsum1 = 0.0f;      // d_bias: column sums of the d_z values this lane loads anyway
    constexpr int kSteps = 4;
    for (long long r0 = r_begin; r0 < r_end; r0 += 2 * kSteps) {
        float a[kSteps][2], b[kSteps][4];
#pragma unroll
        for (int s = 0; s < kSteps; ++s) {
            const long long r = r0 + 2 * s + h;
            const bool ok = r < r_end;
            const long long rr = ok ? r : (p.rows - 1);
            a[s][0] = p.d_z[rr * 64 + i];
            a[s][1] = p.d_z[rr * 64 + 32 + i];
            b[s][0] = p.input[rr * 64 + i];
            b[s][1] = p.input[rr * 64 + 32 + i];
            b[s][2] = p.update[rr * 64 + i];
            b[s][3] = p.update[rr * 64 + 32 + i];
            if (!ok) { a[s][0] = 0.0f; a[s][1] = 0.0f; }
            bsum0 = bsum0 + a[s][0];
            bsum1 = bsum1 + a[s][1];
        }
#pragma unroll
        for (int s = 0; s < kSteps; ++s)
#pragma unroll
            for (int t = 0; t < 2; ++t)
#pragma unroll
                for (int c = 0; c < 4; ++c)
                    acc[t][c] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[s][t], b[s][c], acc[t][c], 0, 0, 0);
    }
    if (p.bias_partial != nullptr) {       // even rows (h = 0) + odd rows (h = 1) of this wave's range
        const float o0 = __shfl_xor(bsum0, 32, 64), o1 = __shfl_xor(bsum1, 32, 64);
        if (h == 0) {
            p.bias_partial[wave_global * 64 + i] = bsum0 + o0;
            p.bias_partial[wave_global * 64 + 32 + i] = bsum1 + o1;
        }
    }
    float *out = p.partial + wave_global * (64 * 128);
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int c = 0; c < 4; ++c)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int o = (r & 3) + 8 * (r >> 2) + 4 * h + 32 * t;
                out[o * 128 + 32 * c + i] = acc[t][c][r];
            }
}

// d_input | d_update of the fused epilogue:  [d_x | d_u] = d_z [rows, 64] . W [64, 128]   (+ grad_out on the d_x half when
// the layer has a shortcut), one pass over d_z instead of two BLAS GEMMs.  Same tile scheme as linear_kernel: W
// (transposed) in LDS, a wave-private 32-row tile; k order of the fmaf chain: o = 0, 32, 1, 33, ...
struct DxDuParams {
    const float *d_z;        // [rows, 64]
    const float *weight;     // [64, 128] (nn.Linear.weight)
    const float *grad_out;   // [rows, 64] or NULL
    float *d_input;          // [rows, 64]
    float *d_update;         // [rows, 64]
    long long rows;
};

__global__ __launch_bounds__(kCbWaves * 64, 1) void dxdu_kernel(const DxDuParams p) {
    constexpr int K = 64, N = 128, kWStride = K + 4, kTStride = N + 4;
    extern __shared__ __attribute__((aligned(16))) float dx_lds[];
    float *w_lds = dx_lds;                                          // [N][kWStride]: w_lds[c][o] = W[o][c]
    const int lane = threadIdx.x & 63;
    const int wl = uniform(threadIdx.x >> 6);
    float *tile = dx_lds + N * kWStride + wl * (32 * kTStride);     // [32][kTStride], wave private
    const int i = lane & 31, h = lane >> 5;
    for (int idx = threadIdx.x; idx < K * N; idx += kCbWaves * 64) {
        const int o = idx / N, c = idx % N;                         // coalesced read of W, transposed write
        w_lds[c * kWStride + o] = p.weight[idx];
    }
    __syncthreads();
    const long long n_tiles = (p.rows + 31) / 32;
    const long long wave_global = (long long)blockIdx.x * kCbWaves + wl;
    const long long wave_total = (long long)gridDim.x * kCbWaves;
    for (long long t = wave_global; t < n_tiles; t += wave_total) {
        const long long row0 = t * 32;
        const long long last = p.rows - 1;
#pragma unroll
        for (int q = 0; q < 8; ++q) {                               // 32 rows x 64 floats, 4 rows per 1-KiB load
            const int r = 4 * q + (lane >> 4), c = (lane & 15) * 4;
            long long gr = row0 + r;
            gr = gr < last ? gr : last;
            *reinterpret_cast<f32x4 *>(tile + r * kTStride + c) = *reinterpret_cast<const f32x4 *>(p.d_z + gr * 64 + c);
        }
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
        f32x16 acc[4];
#pragma unroll
        for (int tt = 0; tt < 4; ++tt)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[tt][r] = 0.0f;
#pragma unroll
        for (int q = 0; q < K / 8; ++q) {
            const f32x4 av = *reinterpret_cast<const f32x4 *>(tile + i * kTStride + (K / 2) * h + 4 * q);
#pragma unroll
            for (int tt = 0; tt < 4; ++tt) {
                const f32x4 wv = *reinterpret_cast<const f32x4 *>(w_lds + (i + 32 * tt) * kWStride + (K / 2) * h + 4 * q);
                acc[tt] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.x, wv.x, acc[tt], 0, 0, 0);
                acc[tt] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.y, wv.y, acc[tt], 0, 0, 0);
                acc[tt] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.z, wv.z, acc[tt], 0, 0, 0);
                acc[tt] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.w, wv.w, acc[tt], 0, 0, 0);
            }
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");          // all reads of d_z done before the tile is rewritten
#pragma unroll
        for (int tt = 0; tt < 4; ++tt)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = (r & 3) + 8 * (r >> 2) + 4 * h;
                tile[row * kTStride + 32 * tt + i] = acc[tt][r];
            }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const int r = 4 * q + (lane >> 4), c = (lane & 15) * 4;
            if (row0 + r < p.rows) {
                f32x4 dx = *reinterpret_cast<const f32x4 *>(tile + r * kTStride + c);
                const f32x4 du = *reinterpret_cast<const f32x4 *>(tile + r * kTStride + 64 + c);
                if (p.grad_out != nullptr) dx = dx + *reinterpret_cast<const f32x4 *>(p.grad_out + (row0 + r) * 64 + c);
                *reinterpret_cast<f32x4 *>(p.d_input + (row0 + r) * 64 + c) = dx;
                *reinterpret_cast<f32x4 *>(p.d_update + (row0 + r) * 64 + c) = du;
            }
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    }
}

}  // namespace

extern "C" {

int ultra_combine_backward_waves(int device, int64_t rows, int *n_ln_waves, int *n_wgrad_waves) {
    DeviceInfo *di = nullptr;
    int rc = device_info(device, &di);
    if (rc) return rc;
    const long long n_tiles = (rows + kCbRows - 1) / kCbRows;
    long long blocks = (n_tiles + kCbWaves - 1) / kCbWaves;
    if (blocks > di->n_cu) blocks = di->n_cu;
    if (blocks < 1) blocks = 1;
    if (n_ln_waves) *n_ln_waves = (int)(blocks * kCbWaves);
    long long wblocks = (long long)di->n_cu * 2;
    const long long max_useful = (rows + 63) / 64;            // at least 64 rows per wave
    if (wblocks * kCbWaves > max_useful) wblocks = (max_useful + kCbWaves - 1) / kCbWaves;
    if (wblocks < 1) wblocks = 1;
    if (n_wgrad_waves) *n_wgrad_waves = (int)(wblocks * kCbWaves);
    return ULTRA_OK;
}

int ultra_combine_backward_f32(const float *input, const float *update, const float *weight, const float *bias,
                               const float *ln_weight, const float *ln_bias, float ln_eps, int relu,
                               const float *grad_out, float *d_z, float *d_ln_weight_partial,
                               float *d_ln_bias_partial, float *d_weight_partial, float *d_bias_partial, int64_t rows,
                               int64_t dim, void *stream) {
    if (dim != 64 || rows < 0) return ULTRA_ERR_BAD_SHAPE;
    if (rows == 0) return ULTRA_OK;
    if (input == nullptr || update == nullptr || weight == nullptr || bias == nullptr || grad_out == nullptr ||
        d_z == nullptr || d_weight_partial == nullptr)
        return ULTRA_ERR_NULL_POINTER;
    if (ln_weight != nullptr && (ln_bias == nullptr || d_ln_weight_partial == nullptr || d_ln_bias_partial == nullptr))
        return ULTRA_ERR_NULL_POINTER;
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    int ln_waves = 0, wg_waves = 0;
    int rc = ultra_combine_backward_waves(dev, rows, &ln_waves, &wg_waves);
    if (rc) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);

    CombineBwdParams p;
    p.input = input; p.update = update; p.weight = weight; p.bias = bias; p.gamma = ln_weight; p.beta = ln_bias;
    p.grad_out = grad_out; p.d_z = d_z; p.d_gamma_partial = d_ln_weight_partial; p.d_beta_partial = d_ln_bias_partial;
    p.rows = rows; p.eps = ln_eps; p.relu = relu;
    const size_t lds = (size_t)(kCbWaves * kCbTileFloats + 128) * sizeof(float);
    rc = launch_with_lds(combine_backward_kernel, p, ln_waves / kCbWaves, lds, s, kCbWaves * 64, (int)lds);
    if (rc) return rc;

    WGradParams w;
    w.d_z = d_z; w.input = input; w.update = update; w.partial = d_weight_partial; w.bias_partial = d_bias_partial;
    w.rows = rows;
    long long per = (rows + wg_waves - 1) / wg_waves;
    per = (per + 1) & ~1LL;
    w.rows_per_wave = per;
    hipLaunchKernelGGL(linear_wgrad_kernel, dim3(wg_waves / kCbWaves), dim3(kCbWaves * 64), 0, s, w);
    HIP_TRY(hipGetLastError());
    return ULTRA_OK;
}

int ultra_combine_dxdu_f32(const float *d_z, const float *weight, const float *grad_out, float *d_input, float *d_update,
                           int64_t rows, int64_t dim, void *stream) {
    if (dim != 64 || rows < 0) return ULTRA_ERR_BAD_SHAPE;
    if (rows == 0) return ULTRA_OK;
    if (d_z == nullptr || weight == nullptr || d_input == nullptr || d_update == nullptr) return ULTRA_ERR_NULL_POINTER;
    DeviceInfo *di = nullptr;
    int rc = current_device_info(&di);
    if (rc) return rc;
    DxDuParams p;
    p.d_z = d_z; p.weight = weight; p.grad_out = grad_out; p.d_input = d_input; p.d_update = d_update; p.rows = rows;
    const size_t lds = (size_t)(128 * 68 + kCbWaves * 32 * 132) * sizeof(float);
    const long long n_tiles = (rows + 31) / 32;
    long long blocks = (n_tiles + kCbWaves - 1) / kCbWaves;
    if (blocks > di->n_cu) blocks = di->n_cu;
    return launch_with_lds(dxdu_kernel, p, (int)blocks, lds, static_cast<hipStream_t>(stream), kCbWaves * 64, (int)lds);
}

}  // extern "C"

// project_bwd.inc -- backward of the grouped relation projections (project_kernel), all layers in one launch.
// (included by dense_layers.hip, after dense.inc)
//
//     out_l[r, b, :] = W2_l . relu( W1_l . x[b, r, :] + b1_l ) + b2_l          l = 0 .. L-1      (project_kernel)
//
// = the `relation_projection` MLPs of the entity layers (ultra/layer.py:228,318-319) with the (B, R, D) -> (R, B*D)
// transpose of :325-326.  In training the reference (and round 1 here) ran them as 12 Linear layers through autograd:
// per fine-tuning step 36 small GEMMs, 12 bias reductions, 12 relu passes and the transposes -- ~100 launches of 3-10 us
// on B * R rows (352 for a WN18RR-sized vocabulary at B = 16, 7 584 for FB15k237's).  Here, per 32-row tile and layer:
//     recompute  h = relu(W1 x + b1)                       (the forward kernel's chain: same bits)
//     d_h  = (g W2) * (h > 0)          d_W2 += g^T h       d_b2 += colsum g
//     d_x_l = d_h W1                   d_W1 += d_h^T x     d_b1 += colsum d_h
// five 32 x 64 x 64 products on the exact-f32 matrix cores (v_mfma_f32_32x32x2_f32), tiles in LDS, the two 64 x 64
// weight-gradient accumulators of a layer in registers for the life of the wave.  d_x of the layers lands in one
// [L, rows, 64] buffer (the caller sums over L: x feeds every layer).  Parameter gradients: per-workgroup partial slabs,
// then project_bwd_reduce_kernel.  Results are held to fp64 autograd of the reference chain at 2e-5 of each gradient's
// scale (tests/test_frontier_sampler_gpu.py); the sums over rows run in tile order (round-robin over waves), i.e. they
// depend on the grid size like every split reduction here, never on timing.

namespace {

constexpr int kPbWaves = 4;                   // one wave per SIMD (round 5; two before: half the matrix cores idle, 396 us at B = 64);
                                              // three 32 x 68 tiles per wave (d_h overwrites h) + the two weight matrices: 137 KiB of LDS
constexpr int kPbSlab = 2 * 64 * 64 + 128;    // d_W1 | d_W2 | d_b1 | d_b2 of one workgroup

struct ProjectBwdParams {
    const float *relation;                     // [rows = B * R, 64]
    const float *w1[kProjMaxLayers], *b1[kProjMaxLayers], *w2[kProjMaxLayers];
    const float *grad[kProjMaxLayers];         // each [R, B, 64]; NULL: no gradient reached this layer's table
    float *d_relation;                         // [n_layers, rows, 64]
    float *partial;                            // [n_layers * blocks_per_layer, kPbSlab]
    long long rows;
    int batch, n_rel, n_layers, blocks_per_layer;
};

__global__ __launch_bounds__(kPbWaves * 64, 1) void project_bwd_kernel(const ProjectBwdParams p) {
    constexpr int K = 64, kStride = K + 4, kTileF = 32 * kStride;
    extern __shared__ __attribute__((aligned(16))) float pb_lds[];
    float *w1_lds = pb_lds, *w2_lds = pb_lds + K * kStride;          // [64][kStride] each, nn.Linear layout [out][in]
    const int lane = threadIdx.x & 63;
    const int wl = uniform(threadIdx.x >> 6);
    float *xt = pb_lds + 2 * K * kStride + wl * (3 * kTileF);       // x | g | h tiles of this wave; d_h takes h's place
    float *gt = xt + kTileF, *ht = gt + kTileF, *dt = ht;
    const int i = lane & 31, h = lane >> 5;
    const int l = blockIdx.x / p.blocks_per_layer, bl = blockIdx.x % p.blocks_per_layer;
    for (int idx = threadIdx.x; idx < K * (K / 4); idx += kPbWaves * 64) {
        const int r = idx / (K / 4), c = (idx % (K / 4)) * 4;
        *reinterpret_cast<f32x4 *>(w1_lds + r * kStride + c) = *reinterpret_cast<const f32x4 *>(p.w1[l] + r * K + c);
        *reinterpret_cast<f32x4 *>(w2_lds + r * kStride + c) = *reinterpret_cast<const f32x4 *>(p.w2[l] + r * K + c);
    }
    __syncthreads();
    const float bias1[2] = {p.b1[l][i], p.b1[l][i + 32]};
    const float *grad = p.grad[l];
    float *d_x = p.d_relation + (long long)l * p.rows * K;
    const long long n_tiles = (p.rows + 31) / 32;
    const long long wave_global = (long long)bl * kPbWaves + wl;
    const long long wave_total = (long long)p.blocks_per_layer * kPbWaves;

    f32x16 aw1[2][2], aw2[2][2];               // d_W1[j][k], d_W2[o][k]: blocks [tm][tn] of 32 x 32
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) { aw1[a][b][r] = 0.0f; aw2[a][b][r] = 0.0f; }
    float db1 = 0.0f, db2 = 0.0f;              // column `lane` of d_b1 / d_b2

    // D[row][col] = sum_k A[row][k] * Wt[k][col] with A a 32 x 64 tile (row per lane) and the weight read as
    //   ROWS_ARE_OUT: W[col][k]   (x W^T: the forward's chain, k = 0, 32, 1, 33, ...)
    //   else:         W[k][col]   (g W:   k = 0, 32, 1, 33, ... over the output index)
    auto gemm = [&](const float *a_tile, const float *w_lds, auto rows_are_out_tag, const float (&init)[2], f32x16 (&acc)[2]) {
        constexpr bool rows_are_out = decltype(rows_are_out_tag)::value;
#pragma unroll
        for (int tt = 0; tt < 2; ++tt)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[tt][r] = init[tt];
#pragma unroll
        for (int q = 0; q < K / 8; ++q) {
            const f32x4 av = *reinterpret_cast<const f32x4 *>(a_tile + i * kStride + (K / 2) * h + 4 * q);
            const float a4[4] = {av.x, av.y, av.z, av.w};
#pragma unroll
            for (int tt = 0; tt < 2; ++tt) {
                float w4[4];
                if constexpr (rows_are_out) {
                    const f32x4 wv = *reinterpret_cast<const f32x4 *>(w_lds + (i + 32 * tt) * kStride + (K / 2) * h + 4 * q);
                    w4[0] = wv.x; w4[1] = wv.y; w4[2] = wv.z; w4[3] = wv.w;
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e) w4[e] = w_lds[((K / 2) * h + 4 * q + e) * kStride + i + 32 * tt];
                }
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[tt] = __builtin_amdgcn_mfma_f32_32x32x2f32(a4[e], w4[e], acc[tt], 0, 0, 0);
            }
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    };
    // acc[m][n] += sum_row L[row][m] * R[row][n] over the 32 rows of two tiles (rows s and s + 16 per step)
    auto outer = [&](const float *left, const float *right, f32x16 (&acc)[2][2]) {
#pragma unroll 4
        for (int s = 0; s < 16; ++s) {
            const int row = s + 16 * h;
            const float a0 = left[row * kStride + i], a1 = left[row * kStride + 32 + i];
            const float b0 = right[row * kStride + i], b1 = right[row * kStride + 32 + i];
            acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[1][1], 0, 0, 0);
        }
    };
    const float zero2[2] = {0.0f, 0.0f};

    for (long long t = wave_global; t < n_tiles; t += wave_total) {
        const long long row0 = t * 32;
        const long long last = p.rows - 1;
        // ---- stage x rows (b, r) and the matching rows (r, b) of this layer's table gradient (zeros past the end)
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const int r = 4 * q + (lane >> 4), c = (lane & 15) * 4;
            const long long gr = row0 + r;
            const long long cr = gr < last ? gr : last;
            *reinterpret_cast<f32x4 *>(xt + r * kStride + c) = *reinterpret_cast<const f32x4 *>(p.relation + cr * K + c);
            f32x4 g = {0.0f, 0.0f, 0.0f, 0.0f};
            if (grad != nullptr && gr < p.rows) {
                const long long b = gr / p.n_rel, rel = gr % p.n_rel;
                g = *reinterpret_cast<const f32x4 *>(grad + (rel * p.batch + b) * K + c);
            }
            *reinterpret_cast<f32x4 *>(gt + r * kStride + c) = g;
        }
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");

        f32x16 acc[2];
        // ---- h = relu(W1 x + b1)
        gemm(xt, w1_lds, std::true_type{}, bias1, acc);
#pragma unroll
        for (int tt = 0; tt < 2; ++tt)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = (r & 3) + 8 * (r >> 2) + 4 * h;
                const float v = acc[tt][r];
                ht[row * kStride + 32 * tt + i] = !(v <= 0.0f) ? v : 0.0f;
            }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        // ---- d_W2 += g^T h   (before d_h overwrites h)
        outer(gt, ht, aw2);
        // ---- d_h = (g W2) * (h > 0), in h's tile: every lane reads and writes the same elements
        gemm(gt, w2_lds, std::false_type{}, zero2, acc);
#pragma unroll
        for (int tt = 0; tt < 2; ++tt)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = (r & 3) + 8 * (r >> 2) + 4 * h;
                const float on = ht[row * kStride + 32 * tt + i];
                dt[row * kStride + 32 * tt + i] = on > 0.0f ? acc[tt][r] : 0.0f;
            }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        // ---- d_W1 += d_h^T x,  column sums
        outer(dt, xt, aw1);
        {
            float s2 = 0.0f, s1 = 0.0f;
#pragma unroll 8
            for (int r = 0; r < 32; ++r) {
                s2 = s2 + gt[r * kStride + lane];
                s1 = s1 + dt[r * kStride + lane];
            }
            db2 = db2 + s2;
            db1 = db1 + s1;
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");          // g tile free: d_x goes there
        // ---- d_x = d_h W1
        gemm(dt, w1_lds, std::false_type{}, zero2, acc);
#pragma unroll
        for (int tt = 0; tt < 2; ++tt)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = (r & 3) + 8 * (r >> 2) + 4 * h;
                gt[row * kStride + 32 * tt + i] = acc[tt][r];
            }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const int r = 4 * q + (lane >> 4), c = (lane & 15) * 4;
            const long long gr = row0 + r;
            if (gr < p.rows) *reinterpret_cast<f32x4 *>(d_x + gr * K + c) = *reinterpret_cast<const f32x4 *>(gt + r * kStride + c);
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    }

    // ---- the workgroup's partial slab: wave 0 writes, waves 1 .. 3 add (wave order), then one coalesced copy out
    float *slab = pb_lds + 2 * K * kStride;                          // the waves' tiles are free now (kPbSlab <= 12 * kTileF)
    auto deposit = [&](bool add) {
#pragma unroll
        for (int tm = 0; tm < 2; ++tm)
#pragma unroll
            for (int tn = 0; tn < 2; ++tn)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int m = (r & 3) + 8 * (r >> 2) + 4 * h + 32 * tm, n = i + 32 * tn;
                    float *a = slab + m * 64 + n, *b = slab + 4096 + m * 64 + n;
                    *a = add ? *a + aw1[tm][tn][r] : aw1[tm][tn][r];
                    *b = add ? *b + aw2[tm][tn][r] : aw2[tm][tn][r];
                }
        float *c1 = slab + 8192 + lane, *c2 = slab + 8192 + 64 + lane;
        *c1 = add ? *c1 + db1 : db1;
        *c2 = add ? *c2 + db2 : db2;
    };
    __syncthreads();
    if (wl == 0) deposit(false);
    for (int w = 1; w < kPbWaves; ++w) {
        __syncthreads();
        if (wl == w) deposit(true);
    }
    __syncthreads();
    float *out = p.partial + (long long)blockIdx.x * kPbSlab;
    for (int e = threadIdx.x; e < kPbSlab; e += kPbWaves * 64) out[e] = slab[e];
}

struct ProjectReduceParams {
    const float *partial;
    float *d_w1[kProjMaxLayers], *d_b1[kProjMaxLayers], *d_w2[kProjMaxLayers], *d_b2[kProjMaxLayers];
    int blocks_per_layer;
};

// grid (ceil(kPbSlab / 256), n_layers): element e of layer l = sum over the layer's workgroups, in workgroup order
__global__ __launch_bounds__(256) void project_bwd_reduce_kernel(const ProjectReduceParams p) {
    const int e = blockIdx.x * 256 + threadIdx.x, l = blockIdx.y;
    if (e >= kPbSlab) return;
    const float *src = p.partial + (long long)l * p.blocks_per_layer * kPbSlab + e;
    float s = 0.0f;
    for (int b = 0; b < p.blocks_per_layer; ++b) s = s + src[(long long)b * kPbSlab];
    if (e < 4096) p.d_w1[l][e] = s;
    else if (e < 8192) p.d_w2[l][e - 4096] = s;
    else if (e < 8192 + 64) p.d_b1[l][e - 8192] = s;
    else p.d_b2[l][e - 8192 - 64] = s;
}

}  // namespace

extern "C" {

int ultra_relation_project_backward_blocks(int device, int64_t batch, int64_t n_rel, int64_t n_layers, int64_t *blocks) {
    if (blocks == nullptr) return ULTRA_ERR_NULL_POINTER;
    if (batch < 0 || n_rel < 0 || n_layers < 0) return ULTRA_ERR_BAD_SHAPE;
    DeviceInfo *di = nullptr;
    int rc = device_info(device, &di);
    if (rc) return rc;
    const long long count = n_layers < kProjMaxLayers ? n_layers : kProjMaxLayers;
    const long long n_tiles = (batch * n_rel + 31) / 32;
    long long per_layer = (n_tiles + kPbWaves - 1) / kPbWaves;
    const long long cap = count > 0 ? (di->n_cu + count - 1) / count : 1;       // one workgroup per CU over all layers
    if (per_layer > cap) per_layer = cap;
    if (per_layer < 1) per_layer = 1;
    *blocks = per_layer;
    return ULTRA_OK;
}

int ultra_relation_project_backward_f32(const float *relation, const float *const *w1, const float *const *b1,
                                        const float *const *w2, const float *const *grad, float *d_relation_layers,
                                        float *const *d_w1, float *const *d_b1, float *const *d_w2, float *const *d_b2,
                                        void *workspace, size_t workspace_bytes, int64_t n_layers, int64_t batch,
                                        int64_t n_rel, int64_t dim, void *stream) {
    if (dim != 64 || n_layers < 0 || n_layers > kProjMaxLayers || batch < 0 || n_rel < 0 || batch > 0x7fffffffLL ||
        n_rel > 0x7fffffffLL)
        return ULTRA_ERR_BAD_SHAPE;
    if (n_layers == 0) return ULTRA_OK;
    if (relation == nullptr && batch * n_rel > 0) return ULTRA_ERR_NULL_POINTER;
    if (w1 == nullptr || b1 == nullptr || w2 == nullptr || grad == nullptr || d_w1 == nullptr || d_b1 == nullptr ||
        d_w2 == nullptr || d_b2 == nullptr || (d_relation_layers == nullptr && batch * n_rel > 0))
        return ULTRA_ERR_NULL_POINTER;
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    int64_t per_layer = 0;
    int rc = ultra_relation_project_backward_blocks(dev, batch, n_rel, n_layers, &per_layer);
    if (rc) return rc;
    const size_t need = (size_t)n_layers * (size_t)per_layer * kPbSlab * sizeof(float);
    if (workspace == nullptr || workspace_bytes < need) return ULTRA_ERR_WORKSPACE;
    ProjectBwdParams p{};
    ProjectReduceParams q{};
    p.relation = relation;
    for (int64_t l = 0; l < n_layers; ++l) {
        if (w1[l] == nullptr || b1[l] == nullptr || w2[l] == nullptr || d_w1[l] == nullptr || d_b1[l] == nullptr ||
            d_w2[l] == nullptr || d_b2[l] == nullptr)
            return ULTRA_ERR_NULL_POINTER;
        p.w1[l] = w1[l]; p.b1[l] = b1[l]; p.w2[l] = w2[l]; p.grad[l] = grad[l];
        q.d_w1[l] = d_w1[l]; q.d_b1[l] = d_b1[l]; q.d_w2[l] = d_w2[l]; q.d_b2[l] = d_b2[l];
    }
    p.d_relation = d_relation_layers;
    p.partial = static_cast<float *>(workspace);
    p.rows = batch * n_rel; p.batch = (int)batch; p.n_rel = (int)n_rel; p.n_layers = (int)n_layers;
    p.blocks_per_layer = (int)per_layer;
    q.partial = p.partial;
    q.blocks_per_layer = (int)per_layer;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const size_t lds = (size_t)(2 * 64 * 68 + kPbWaves * 3 * 32 * 68) * sizeof(float);
    rc = launch_with_lds(project_bwd_kernel, p, (int)(per_layer * n_layers), lds, s, kPbWaves * 64, (int)lds);
    if (rc) return rc;
    hipLaunchKernelGGL(project_bwd_reduce_kernel, dim3((kPbSlab + 255) / 256, (unsigned)n_layers), dim3(256), 0, s, q);
    HIP_TRY(hipGetLastError());
    return ULTRA_OK;
}

}  // extern "C"

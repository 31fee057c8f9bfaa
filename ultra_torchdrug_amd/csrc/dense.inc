// dense.inc -- the small dense layers around the Bellman-Ford stacks, in a documented summation order
// (included by dense_layers.hip).
//
// The reference runs them as nn.Linear through torchdrug's MLP: the per-layer relation projection 64 -> 64 -> 64
// (/root/reference/ultra/layer.py:228,318-319) and the score head 128 -> 128 -> 1 (ultra/model.py:53,193).  BLAS
// libraries do not define their summation order, so scores computed by two correct implementations differ in the
// last bits and filtered RANKS -- integers -- can flip on near-ties.  These kernels fix the order (a k-ordered fmaf
// chain, which is exactly what v_mfma_f32_32x32x2_f32 computes), oracle_linear_forward / oracle_rowdot restate it
// on the CPU, and the whole inference path becomes bit-reproducible between the HIP library and the CPU oracle.
//
//   linear_kernel<K, N> : out[rows, N] = relu?( in[rows, K] . W[N, K]^T + b )       (K, N) in {(64, 64), (128, 128)}
//       k order: lane half h = 0 walks k = 0 .. K/2-1, h = 1 walks k = K/2 .. K-1, i.e. the chain visits
//       k = 0, K/2, 1, K/2+1, ... starting from the bias.  W lives in LDS (padded rows), the activations of a
//       32-row tile in a wave-private LDS tile (coalesced in, row-per-lane out).
//   rowdot_kernel       : out[row] = b + sum_k in[row, k] * w[k], k ascending, one lane per row (the 128 -> 1 head).

namespace {

struct LinearParams {
    const float *input;   // [rows, K]
    const float *weight;  // [N, K]
    const float *bias;    // [N]
    float *out;           // [rows, N]
    long long rows;
    int relu;
};

template <int K, int N>
__global__ __launch_bounds__(kCbWaves * 64, 1) void linear_kernel(const LinearParams p) {
    static_assert(K == N && (K == 64 || K == 128), "supported shapes: 64x64, 128x128");
    constexpr int kStride = K + 4;                 // padded row: conflict-free ds_read_b128 of row-per-lane fragments
    constexpr int kOutTiles = N / 32;
    extern __shared__ __attribute__((aligned(16))) float dl_lds[];
    float *w_lds = dl_lds;                                         // [N][kStride]
    const int lane = threadIdx.x & 63;
    const int wl = uniform(threadIdx.x >> 6);
    float *tile = dl_lds + N * kStride + wl * (32 * kStride);      // [32][kStride], wave private
    const int i = lane & 31, h = lane >> 5;
    for (int idx = threadIdx.x; idx < N * (K / 4); idx += kCbWaves * 64) {
        const int r = idx / (K / 4), c = (idx % (K / 4)) * 4;
        *reinterpret_cast<f32x4 *>(w_lds + r * kStride + c) = *reinterpret_cast<const f32x4 *>(p.weight + (long long)r * K + c);
    }
    __syncthreads();
    float bias[kOutTiles];
#pragma unroll
    for (int t = 0; t < kOutTiles; ++t) bias[t] = p.bias[i + 32 * t];

    const long long n_tiles = (p.rows + 31) / 32;
    const long long wave_global = (long long)blockIdx.x * kCbWaves + wl;
    const long long wave_total = (long long)gridDim.x * kCbWaves;
    constexpr int kLoadsPerTile = 32 * K / 256;     // 1-KiB wave loads (256 floats each)
    for (long long t = wave_global; t < n_tiles; t += wave_total) {
        const long long row0 = t * 32;
        const long long last = p.rows - 1;
#pragma unroll
        for (int q = 0; q < kLoadsPerTile; ++q) {
            const int flat = q * 256 + lane * 4;                    // float index inside the 32 x K tile
            const int r = flat / K, c = flat % K;
            long long gr = row0 + r;
            gr = gr < last ? gr : last;
            *reinterpret_cast<f32x4 *>(tile + r * kStride + c) = *reinterpret_cast<const f32x4 *>(p.input + gr * K + c);
        }
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");

        f32x16 acc[kOutTiles];
#pragma unroll
        for (int tt = 0; tt < kOutTiles; ++tt)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[tt][r] = bias[tt];
#pragma unroll
        for (int q = 0; q < K / 8; ++q) {                           // 4 k-steps per iteration
            const f32x4 av = *reinterpret_cast<const f32x4 *>(tile + i * kStride + (K / 2) * h + 4 * q);
#pragma unroll
            for (int tt = 0; tt < kOutTiles; ++tt) {
                const f32x4 wv = *reinterpret_cast<const f32x4 *>(w_lds + (i + 32 * tt) * kStride + (K / 2) * h + 4 * q);
                acc[tt] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.x, wv.x, acc[tt], 0, 0, 0);
                acc[tt] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.y, wv.y, acc[tt], 0, 0, 0);
                acc[tt] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.z, wv.z, acc[tt], 0, 0, 0);
                acc[tt] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.w, wv.w, acc[tt], 0, 0, 0);
            }
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
        for (int tt = 0; tt < kOutTiles; ++tt)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = (r & 3) + 8 * (r >> 2) + 4 * h;
                float v = acc[tt][r];
                if (p.relu) v = !(v <= 0.0f) ? v : 0.0f;
                tile[row * kStride + 32 * tt + i] = v;
            }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
        for (int q = 0; q < kLoadsPerTile; ++q) {
            const int flat = q * 256 + lane * 4;
            const int r = flat / N, c = flat % N;
            const f32x4 d = *reinterpret_cast<const f32x4 *>(tile + r * kStride + c);
            if (row0 + r < p.rows) *reinterpret_cast<f32x4 *>(p.out + (row0 + r) * N + c) = d;
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    }
}

// out[row] = bias + sum_{k ascending} in[row, k] * w[k]   (fmaf chain), one lane per row
__global__ __launch_bounds__(256) void rowdot_kernel(const float *input, const float *weight, const float *bias, float *out,
                                                     long long rows, int K) {
    const long long row = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (row >= rows) return;
    float acc = bias[0];
    const float *in = input + row * K;
    for (int k = 0; k < K; k += 4) {
        const f32x4 v = *reinterpret_cast<const f32x4 *>(in + k);
        const f32x4 w = *reinterpret_cast<const f32x4 *>(weight + k);
        acc = __builtin_fmaf(v.x, w.x, acc);
        acc = __builtin_fmaf(v.y, w.y, acc);
        acc = __builtin_fmaf(v.z, w.z, acc);
        acc = __builtin_fmaf(v.w, w.w, acc);
    }
    out[row] = acc;
}


// score_kernel: the score head of full-batch evaluation.
//     score[b, n] = w2 . relu( W1 . cat[ hidden[n, b, :], query[b, :] ] + b1 ) + b2
// = ultra/model.py:134-138 (node_feature = cat[hidden, query]), :177-183 (transpose + gather of the candidate
// tails -- the identity permutation when every entity is a candidate, ultra/task.py:249-253) and :193 (mlp), which
// the reference runs as cat + gather + 2 GEMMs + relu over N * B rows of 128 inputs.  The query half of every row is one
// of B vectors, so its share of the first layer is computed once per query (score_query_bias_kernel):
//     c[b, o] = b1[o] + W1[o, 64:] . query[b]          (fmaf chain k = 64, 96, 65, 97, ... from the bias)
//     h[n, b, o] = relu( c[b, o] + W1[o, :64] . hidden[n, b] )   (chain k = 0, 32, 1, 33, ... from c: the matrix cores' order)
//     score = b2 + sum_{o ascending} h[o] w2[o]       (fmaf chain, one lane per row)
// -- half the matrix work of the 128-wide product (the kernel ran at 1.5 x its exact-f32 matrix time: 145-166 us for
// 465 k rows).  oracle/rspmm_oracle.c restates this order (oracle_linear_forward with grouped bias rows).
struct ScoreParams {
    const float *hidden;   // [n_node, batch, 64]
    const float *query;    // [batch, 64]
    const float *w1;       // [128, 128]
    const float *b1;       // [128]
    const float *w2;       // [128]
    const float *b2;       // [1]
    float *qbias;          // [batch, 128]  scratch: c above
    float *out;            // [batch, n_node]
    long long n_node;
    int batch;
};

constexpr int kScoreLdsBatch = 64;      // up to this many queries keep c in LDS (stride 136: the two row halves of a D
constexpr int kScoreCStride = 136;      // fragment, 4 queries apart, land 32 banks apart)

__global__ __launch_bounds__(128) void score_query_bias_kernel(const ScoreParams p) {
    const int b = blockIdx.x, o = threadIdx.x;
    const float *w = p.w1 + o * 128 + 64;
    const float *q = p.query + (long long)b * 64;
    float acc = p.b1[o];
    for (int s = 0; s < 32; ++s) {
        acc = __builtin_fmaf(q[s], w[s], acc);
        acc = __builtin_fmaf(q[32 + s], w[32 + s], acc);
    }
    p.qbias[(long long)b * 128 + o] = acc;
}

// score_kernel_lds (knob bit 10): the column-per-lane product, whose result crosses LDS before the per-row w2 dot
__global__ __launch_bounds__(kCbWaves * 64, 1) void score_kernel_lds(const ScoreParams p) {
    constexpr int K = 64, N = 128, kWStride = K + 4, kTStride = N + 4;
    extern __shared__ __attribute__((aligned(16))) float dl_lds[];
    float *w_lds = dl_lds;                                         // [128][kWStride]: W1[:, :64]
    float *w2_lds = w_lds + N * kWStride;                          // [128]
    float *c_lds = w2_lds + N;                                     // [kScoreLdsBatch][kScoreCStride]
    const int lane = threadIdx.x & 63;
    const int wl = uniform(threadIdx.x >> 6);
    float *tile = c_lds + kScoreLdsBatch * kScoreCStride + wl * (32 * kTStride);
    const int i = lane & 31, h = lane >> 5;
    for (int idx = threadIdx.x; idx < N * (K / 4); idx += kCbWaves * 64) {
        const int r = idx / (K / 4), c = (idx % (K / 4)) * 4;
        *reinterpret_cast<f32x4 *>(w_lds + r * kWStride + c) = *reinterpret_cast<const f32x4 *>(p.w1 + (long long)r * 128 + c);
    }
    if (threadIdx.x < N) w2_lds[threadIdx.x] = p.w2[threadIdx.x];
    const bool c_in_lds = p.batch <= kScoreLdsBatch;
    if (c_in_lds)
        for (int idx = threadIdx.x; idx < p.batch * N; idx += kCbWaves * 64) c_lds[(idx >> 7) * kScoreCStride + (idx & 127)] = p.qbias[idx];
    __syncthreads();
    const float b2 = p.b2[0];
    // `out` as a buffer (host side: batch * n_node * 4 B < 4 GiB)
    const __amdgpu_buffer_rsrc_t rsrc_out = __builtin_amdgcn_make_buffer_rsrc(p.out, 0, (int)(unsigned)(p.n_node * p.batch * 4), 0x00020000);

    const long long rows = p.n_node * p.batch;
    const long long n_tiles = (rows + 31) / 32;
    const long long wave_global = (long long)blockIdx.x * kCbWaves + wl;
    const long long wave_total = (long long)gridDim.x * kCbWaves;
    // one wave per SIMD: the NEXT tile's rows travel to registers while the matrix cores work on the current tile (as in
    // combine_kernel<true>)
    const long long last = rows - 1;
    f32x4 ph[8];
    auto fetch = [&](long long t) {
#pragma unroll
        for (int q = 0; q < 8; ++q) {                               // 32 rows x 64 floats of hidden, 4 rows per load
            const int r = 4 * q + (lane >> 4), c = (lane & 15) * 4;
            long long gr = t * 32 + r;
            gr = gr < last ? gr : last;
            ph[q] = *reinterpret_cast<const f32x4 *>(p.hidden + gr * 64 + c);
        }
    };
    if (wave_global < n_tiles) fetch(wave_global);
    for (long long t = wave_global; t < n_tiles; t += wave_total) {
        const long long row0 = t * 32;
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const int r = 4 * q + (lane >> 4), c = (lane & 15) * 4;
            *reinterpret_cast<f32x4 *>(tile + r * kTStride + c) = ph[q];
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        if (t + wave_total < n_tiles) fetch(t + wave_total);

        // accumulators start from the query's share: row (r&3) + 8 (r>>2) + 4 h of the tile is query (row0 + row) % batch
        const long long node0 = row0 / p.batch;                    // wave-uniform: the tile's first row is (node0, q0)
        const unsigned q0 = (unsigned)(row0 - node0 * p.batch);
        f32x16 acc[4];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const unsigned qq = q0 + (unsigned)((r & 3) + 8 * (r >> 2) + 4 * h);          // < batch + 32
            const unsigned b = p.batch >= 32 ? (qq >= (unsigned)p.batch ? qq - (unsigned)p.batch : qq) : qq % (unsigned)p.batch;
#pragma unroll
            for (int tt = 0; tt < 4; ++tt)
                acc[tt][r] = c_in_lds ? c_lds[b * kScoreCStride + i + 32 * tt] : p.qbias[(long long)b * 128 + i + 32 * tt];
        }
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
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
        for (int tt = 0; tt < 4; ++tt)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = (r & 3) + 8 * (r >> 2) + 4 * h;
                const float v = acc[tt][r];
                tile[row * kTStride + 32 * tt + i] = !(v <= 0.0f) ? v : 0.0f;
            }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        // second layer: one lane per row, k ascending fmaf chain (the order of rowdot_kernel); lanes 32..63 repeat rows 0..31
        float s = b2;
        for (int k = 0; k < N; k += 4) {
            const f32x4 v = *reinterpret_cast<const f32x4 *>(tile + i * kTStride + k);
            const f32x4 w = *reinterpret_cast<const f32x4 *>(w2_lds + k);
            s = __builtin_fmaf(v.x, w.x, s);
            s = __builtin_fmaf(v.y, w.y, s);
            s = __builtin_fmaf(v.z, w.z, s);
            s = __builtin_fmaf(v.w, w.w, s);
        }
        // one UNCONDITIONAL buffer store per tile (lanes 32..63 and rows past the end get an out-of-range offset, which the
        // bounds check drops): behind a branch the compiler waits with vmcnt(0) for the prefetched rows at the top of the
        // loop, i.e. for this store's acknowledgement (combine_kernel's note)
        {
            const long long gr = row0 + i;
            const unsigned qq = q0 + (unsigned)i;
            const unsigned step = p.batch >= 32 ? (qq >= (unsigned)p.batch ? 1u : 0u) : qq / (unsigned)p.batch;
            const unsigned b = qq - step * (unsigned)p.batch;
            const long long off = ((long long)b * p.n_node + node0 + step) * 4;
            const bool live = lane < 32 && gr < rows;
            __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(uint32_t, s), rsrc_out, live ? (unsigned)off : 0xffffffffu, 0, 0);
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    }
}

// score_kernel (the default form), row per lane: the product is issued as mfma(A = W1, B = rows), so lane (i, h) holds outputs
// 32 tt + (r&3) + 8 (r>>2) + 4 h of ROW i in acc[tt][r] -- the same products in the same k order as mfma(A = rows, B = W1)
// above, whose result is column per lane and crosses LDS before the per-row w2 dot (64 ds_write_b32, 64 ds_read_b128 and three
// more full LDS waits per tile).  Here relu runs on the accumulators, 32 v_permlane32_swap on the pairs (acc[2p][r], acc[2p+1][r])
// give lane i outputs [64p, 64p+32) and lane i+32 outputs [64p+32, 64p+64) of row i in a compile-time register order, and the
// w2 chain (o ascending from b2) runs in four phases of 32 with the running sum handed across lane ^ 32 three times; the half
// that does not hold the sum runs the same instructions on values that are discarded.
// W1[:, :64] (128 registers, combine_kernel's way) and the lane's halves of w2 (64) live in registers; LDS holds c and the staged
// 32 x 64 tiles only: 8 writes, 8 fragment reads and 16 seed reads of 16 bytes per tile and lane.
// CMEM: c read from memory (batch > kScoreLdsBatch) -- a template parameter, not a branch: loads that MAY be in flight make the
// compiler wait for the prefetch where the paths join (combine_kernel's note).
//   Registers (the build's resource remark): 256 VGPRs + 84 AGPRs (CMEM: + 86), no scratch; one wave per SIMD.
//   Measured (profiles/row_per_lane_ab.json): 132 -> 102 us event-timed at 465 k rows against score_kernel_lds.
template <bool CMEM>
__global__ __launch_bounds__(kCbWaves * 64, 1) void score_kernel(const ScoreParams p) {
    constexpr int K = 64, kTStride = K + 4;
    extern __shared__ __attribute__((aligned(16))) float dl_lds[];
    float *c_lds = dl_lds;                                         // [kScoreLdsBatch][kScoreCStride]
    const int lane = threadIdx.x & 63;
    const int wl = uniform(threadIdx.x >> 6);
    float *tile = c_lds + kScoreLdsBatch * kScoreCStride + wl * (32 * kTStride);     // [32][kTStride], wave private
    const int i = lane & 31, h = lane >> 5;
    // A operand fragments, lane (i, h): W1[i + 32 tt][32 h + s], s = 0..31;  w2r[pp][c] = w2[64 pp + 32 h + c]
    float wr[4][32], w2r[2][32];
#pragma unroll
    for (int tt = 0; tt < 4; ++tt)
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const f32x4 a = *reinterpret_cast<const f32x4 *>(p.w1 + (long long)(i + 32 * tt) * 128 + 32 * h + 4 * q);
            wr[tt][4 * q + 0] = a.x; wr[tt][4 * q + 1] = a.y; wr[tt][4 * q + 2] = a.z; wr[tt][4 * q + 3] = a.w;
        }
#pragma unroll
    for (int pp = 0; pp < 2; ++pp)
#pragma unroll
        for (int c = 0; c < 32; ++c) w2r[pp][c] = p.w2[64 * pp + 32 * h + c];
    if constexpr (!CMEM)
        for (int idx = threadIdx.x; idx < p.batch * 128; idx += kCbWaves * 64) c_lds[(idx >> 7) * kScoreCStride + (idx & 127)] = p.qbias[idx];
    __syncthreads();
    const float b2 = p.b2[0];
    // `out` as a buffer (host side: batch * n_node * 4 B < 4 GiB)
    const __amdgpu_buffer_rsrc_t rsrc_out = __builtin_amdgcn_make_buffer_rsrc(p.out, 0, (int)(unsigned)(p.n_node * p.batch * 4), 0x00020000);

    const long long rows = p.n_node * p.batch;
    const long long n_tiles = (rows + 31) / 32;
    const long long wave_global = (long long)blockIdx.x * kCbWaves + wl;
    const long long wave_total = (long long)gridDim.x * kCbWaves;
    if (wave_global >= n_tiles) return;
    // one wave per SIMD: the NEXT tile's rows travel to registers while the matrix cores work on the current tile
    const long long last = rows - 1;
    f32x4 ph[8];
    auto fetch = [&](long long t) {
#pragma unroll
        for (int q = 0; q < 8; ++q) {                               // 32 rows x 64 floats of hidden, 4 rows per load
            const int r = 4 * q + (lane >> 4), c = (lane & 15) * 4;
            long long gr = t * 32 + r;
            gr = gr < last ? gr : last;
            ph[q] = *reinterpret_cast<const f32x4 *>(p.hidden + gr * 64 + c);
        }
    };
    fetch(wave_global);
    // One store that stores nothing (its offset is out of the descriptor's range), so that the loop is ENTERED as its back edge
    // re-enters it, 8 loads in flight with one store behind them (combine_paired_kernel's note): vmcnt is in order, and
    // without it every tile waits with vmcnt(0), i.e. for the acknowledgement of the previous tile's store.
    __builtin_amdgcn_raw_buffer_store_b32(0u, rsrc_out, 0xffffffffu, 0, 0);
    // (node0, q0) of a tile's first row, carried from tile to tile: a 64-bit division per tile on the scalar unit otherwise,
    // and with one wave per SIMD nothing runs under it
    const long long stride_rows = wave_total * 32;
    const long long stride_nodes = stride_rows / p.batch;
    const unsigned stride_q = (unsigned)(stride_rows - stride_nodes * p.batch);
    long long node0 = wave_global * 32 / p.batch;
    unsigned q0 = (unsigned)(wave_global * 32 - node0 * p.batch);
    for (long long t = wave_global; t < n_tiles; t += wave_total) {
        const long long row0 = t * 32;
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const int r = 4 * q + (lane >> 4), c = (lane & 15) * 4;
            *reinterpret_cast<f32x4 *>(tile + r * kTStride + c) = ph[q];
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        // accumulators start from the query's share: the lane's row i is query b = (q0 + i) % batch, its 64 seeds are 16 groups
        // of four consecutive c[b][32 tt + 8 g + 4 h ..] (kScoreCStride keeps them 16-byte aligned).  CMEM: loaded BEFORE the
        // prefetch is issued, so that the product waits for them and not for the prefetch behind them
        const unsigned qq = q0 + (unsigned)i;                                              // < batch + 32
        const unsigned b = p.batch >= 32 ? (qq >= (unsigned)p.batch ? qq - (unsigned)p.batch : qq) : qq % (unsigned)p.batch;
        const float *c_row = CMEM ? p.qbias + (long long)b * 128 : c_lds + b * kScoreCStride;
        f32x16 acc[4];
#pragma unroll
        for (int tt = 0; tt < 4; ++tt)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const f32x4 cv = *reinterpret_cast<const f32x4 *>(c_row + 32 * tt + 8 * g + 4 * h);
                acc[tt][4 * g + 0] = cv.x; acc[tt][4 * g + 1] = cv.y; acc[tt][4 * g + 2] = cv.z; acc[tt][4 * g + 3] = cv.w;
            }
        // the next tile, UNCONDITIONALLY (past the end: the last row, eight times): behind a branch the compiler waits for every
        // load that may be in flight where the paths join, and the prefetch becomes synchronous
        fetch(t + wave_total);
#pragma unroll
        for (int q = 0; q < K / 8; ++q) {
            const f32x4 bv = *reinterpret_cast<const f32x4 *>(tile + i * kTStride + (K / 2) * h + 4 * q);
#pragma unroll
            for (int tt = 0; tt < 4; ++tt) {
                acc[tt] = __builtin_amdgcn_mfma_f32_32x32x2f32(wr[tt][4 * q + 0], bv.x, acc[tt], 0, 0, 0);
                acc[tt] = __builtin_amdgcn_mfma_f32_32x32x2f32(wr[tt][4 * q + 1], bv.y, acc[tt], 0, 0, 0);
                acc[tt] = __builtin_amdgcn_mfma_f32_32x32x2f32(wr[tt][4 * q + 2], bv.z, acc[tt], 0, 0, 0);
                acc[tt] = __builtin_amdgcn_mfma_f32_32x32x2f32(wr[tt][4 * q + 3], bv.w, acc[tt], 0, 0, 0);
            }
        }
        // relu on the accumulators, then the half swaps: afterwards x[pp][4 g + j] is output 64 pp + 32 h + 8 g + j of row i and
        // y[pp][4 g + j] is output 64 pp + 32 h + 8 g + 4 + j
        float x[2][16], y[2][16];
#pragma unroll
        for (int pp = 0; pp < 2; ++pp)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float lo = acc[2 * pp][r], hi = acc[2 * pp + 1][r];
                x[pp][r] = !(lo <= 0.0f) ? lo : 0.0f;
                y[pp][r] = !(hi <= 0.0f) ? hi : 0.0f;
                half_swap(x[pp][r], y[pp][r]);
            }
        // second layer: o ascending fmaf chain from b2 (rowdot_kernel's order).  Phase (pp, half): the lanes of that half add
        // outputs [64 pp + 32 half, + 32) of their row, then hand the sum to lane ^ 32; it ends in lanes 32..63
        float s = b2;
#pragma unroll
        for (int ph2 = 0; ph2 < 4; ++ph2) {
            const int pp = ph2 >> 1;
#pragma unroll
            for (int g = 0; g < 4; ++g) {
#pragma unroll
                for (int j = 0; j < 4; ++j) s = __builtin_fmaf(x[pp][4 * g + j], w2r[pp][8 * g + j], s);
#pragma unroll
                for (int j = 0; j < 4; ++j) s = __builtin_fmaf(y[pp][4 * g + j], w2r[pp][8 * g + 4 + j], s);
            }
            if (ph2 < 3) {
                // lanes 32..63 of the first result hold the lower half's sum, lanes 0..31 of the second the upper half's
                float from_lower = s, from_upper = s;
                half_swap(from_lower, from_upper);
                s = (ph2 & 1) == 0 ? from_lower : from_upper;
            }
        }
        // one UNCONDITIONAL buffer store per tile, from the half that holds the sum (score_kernel_lds's note)
        {
            const unsigned step = p.batch >= 32 ? (qq >= (unsigned)p.batch ? 1u : 0u) : qq / (unsigned)p.batch;
            const long long off = ((long long)b * p.n_node + node0 + step) * 4;
            const bool live = lane >= 32 && row0 + i < rows;
            __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(uint32_t, s), rsrc_out, live ? (unsigned)off : 0xffffffffu, 0, 0);
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");          // the fragment reads are done before the tile is rewritten
        node0 += stride_nodes;
        q0 += stride_q;
        if (q0 >= (unsigned)p.batch) { q0 -= (unsigned)p.batch; ++node0; }
    }
}

template <int K>
int launch_linear(const LinearParams &p, int n_cu, hipStream_t stream) {
    constexpr int kStride = K + 4;
    const size_t lds = (size_t)(K * kStride + kCbWaves * 32 * kStride) * sizeof(float);
    const long long n_tiles = (p.rows + 31) / 32;
    long long blocks = (n_tiles + kCbWaves - 1) / kCbWaves;
    if (blocks > n_cu) blocks = n_cu;
    return launch_with_lds(linear_kernel<K, K>, p, (int)blocks, lds, stream, kCbWaves * 64, (int)lds);
}

}  // namespace

namespace {      // (kernels and their parameter blocks stay out of the exported symbol table)

// ---------------------------------------------------------------------------------------- relation projections, grouped
// project_kernel: the relation projections of ALL entity layers in one launch,
//     out_l[r, b, :] = W2_l . relu( W1_l . relation[b, r, :] + b1_l ) + b2_l          l = 0 .. L-1
// = GeneralizedRelationalConvNBFMod.relation_projection (a 2-layer MLP, ultra/layer.py:228,318-319) followed by the
// (B, R, D) -> (R, B*D) transpose of :325-326, which the reference (and the per-layer path here) issues per layer:
// 2 linear launches + 1 transposing copy, 6 times per Bellman-Ford.  Same fmaf chains as linear_kernel<64, 64>
// (k = 0, 32, 1, 33, ... from the bias), so the tables are bit-identical to the per-layer path.
constexpr int kProjMaxLayers = 8;
struct ProjectParams {
    const float *relation;                 // [B, R, 64]
    const float *w1[kProjMaxLayers], *b1[kProjMaxLayers], *w2[kProjMaxLayers], *b2[kProjMaxLayers];
    float *out[kProjMaxLayers];            // each [R, B * repeat, 64]
    long long rows;                        // B * R
    int batch, n_rel, n_layers, blocks_per_layer;
    int repeat;                            // every projected row (b, r) is written to the query blocks b, b + B, ... (b + (repeat-1) B)
    long long stride_b, stride_r;          // relation[b, r, :] starts stride_b * b + stride_r * r floats in (contiguous: R * 64, 64)
};

__global__ __launch_bounds__(kCbWaves * 64, 1) void project_kernel(const ProjectParams p) {
    constexpr int K = 64, kStride = K + 4;
    extern __shared__ __attribute__((aligned(16))) float pj_lds[];
    float *w1_lds = pj_lds, *w2_lds = pj_lds + K * kStride;         // [64][kStride] each
    const int lane = threadIdx.x & 63;
    const int wl = uniform(threadIdx.x >> 6);
    float *tile = pj_lds + 2 * K * kStride + wl * (32 * kStride);
    const int i = lane & 31, h = lane >> 5;
    const int l = blockIdx.x / p.blocks_per_layer, bl = blockIdx.x % p.blocks_per_layer;
    for (int idx = threadIdx.x; idx < K * (K / 4); idx += kCbWaves * 64) {
        const int r = idx / (K / 4), c = (idx % (K / 4)) * 4;
        *reinterpret_cast<f32x4 *>(w1_lds + r * kStride + c) = *reinterpret_cast<const f32x4 *>(p.w1[l] + r * K + c);
        *reinterpret_cast<f32x4 *>(w2_lds + r * kStride + c) = *reinterpret_cast<const f32x4 *>(p.w2[l] + r * K + c);
    }
    __syncthreads();
    const float bias1[2] = {p.b1[l][i], p.b1[l][i + 32]}, bias2[2] = {p.b2[l][i], p.b2[l][i + 32]};
    float *out = p.out[l];
    const long long n_tiles = (p.rows + 31) / 32;
    const long long wave_global = (long long)bl * kCbWaves + wl;
    const long long wave_total = (long long)p.blocks_per_layer * kCbWaves;
    auto gemm = [&](const float *w_lds, const float (&bias)[2], f32x16 (&acc)[2]) {
#pragma unroll
        for (int tt = 0; tt < 2; ++tt)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[tt][r] = bias[tt];
#pragma unroll
        for (int q = 0; q < K / 8; ++q) {
            const f32x4 av = *reinterpret_cast<const f32x4 *>(tile + i * kStride + (K / 2) * h + 4 * q);
#pragma unroll
            for (int tt = 0; tt < 2; ++tt) {
                const f32x4 wv = *reinterpret_cast<const f32x4 *>(w_lds + (i + 32 * tt) * kStride + (K / 2) * h + 4 * q);
                acc[tt] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.x, wv.x, acc[tt], 0, 0, 0);
                acc[tt] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.y, wv.y, acc[tt], 0, 0, 0);
                acc[tt] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.z, wv.z, acc[tt], 0, 0, 0);
                acc[tt] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.w, wv.w, acc[tt], 0, 0, 0);
            }
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");          // fragment reads done before the tile is rewritten
    };
    auto spill = [&](const f32x16 (&acc)[2], bool relu) {            // D -> tile, row-major
#pragma unroll
        for (int tt = 0; tt < 2; ++tt)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = (r & 3) + 8 * (r >> 2) + 4 * h;
                float v = acc[tt][r];
                if (relu) v = !(v <= 0.0f) ? v : 0.0f;
                tile[row * kStride + 32 * tt + i] = v;
            }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    };
    for (long long t = wave_global; t < n_tiles; t += wave_total) {
        const long long row0 = t * 32;
        const long long last = p.rows - 1;
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const int r = 4 * q + (lane >> 4), c = (lane & 15) * 4;
            long long gr = row0 + r;
            gr = gr < last ? gr : last;
            const long long b = gr / p.n_rel, rel = gr - b * p.n_rel;
            *reinterpret_cast<f32x4 *>(tile + r * kStride + c) = *reinterpret_cast<const f32x4 *>(p.relation + b * p.stride_b + rel * p.stride_r + c);
        }
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
        f32x16 acc[2];
        gemm(w1_lds, bias1, acc);
        spill(acc, true);
        gemm(w2_lds, bias2, acc);
        spill(acc, false);
#pragma unroll
        for (int q = 0; q < 8; ++q) {                               // input row (b, r) -> output row (r, b)
            const int r = 4 * q + (lane >> 4), c = (lane & 15) * 4;
            const long long gr = row0 + r;
            if (gr < p.rows) {
                const long long b = gr / p.n_rel, rel = gr % p.n_rel;
                const f32x4 v = *reinterpret_cast<const f32x4 *>(tile + r * kStride + c);
                for (int j = 0; j < p.repeat; ++j)
                    *reinterpret_cast<f32x4 *>(out + (rel * ((long long)p.batch * p.repeat) + b + (long long)j * p.batch) * K + c) = v;
            }
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    }
}

// ------------------------------------------------------------------------------------------------ filtered ranking
// rank[q] = 1 + #{c : pred[q, target[q]] <= pred[q, c]} - #{c in filter(q) : pred[q, target[q]] <= pred[q, c]}
// = sum((pos_pred <= pred) & mask, -1) + 1 of ultra/task.py:307-315 with mask = "every candidate except the known
// truths" (task.py:65-100) given as per-query lists of DISTINCT candidates instead of a dense (B, N) boolean.
// Integer result; one workgroup per query.
__global__ __launch_bounds__(256) void filtered_rank_kernel(const float *pred, long long row_stride, long long n_cand,
                                                            const int64_t *target, const int32_t *filt_ptr,
                                                            const int32_t *filt_node, int64_t *rank) {
    __shared__ long long part[4];
    const long long q = blockIdx.x;
    const float *row = pred + q * row_stride;
    const float pos = row[target[q]];
    long long count = 0;
    for (long long c = threadIdx.x; c < n_cand; c += blockDim.x) count += (pos <= row[c]) ? 1 : 0;
    if (filt_ptr != nullptr) {
        const int lo = filt_ptr[q], hi = filt_ptr[q + 1];
        for (int k = lo + (int)threadIdx.x; k < hi; k += (int)blockDim.x) count -= (pos <= row[filt_node[k]]) ? 1 : 0;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) count += __shfl_down(count, off, 64);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = count;
    __syncthreads();
    if (threadIdx.x == 0) rank[q] = part[0] + part[1] + part[2] + part[3] + 1;
}

}  // namespace

extern "C" {

int ultra_filtered_rank(const float *pred, int64_t n_query, int64_t n_cand, int64_t row_stride, const int64_t *target,
                        const int32_t *filt_ptr, const int32_t *filt_node, int64_t *rank, void *stream) {
    if (n_query < 0 || n_cand <= 0 || row_stride < n_cand || n_query > 0x7fffffffLL) return ULTRA_ERR_BAD_SHAPE;
    if (n_query == 0) return ULTRA_OK;
    if (pred == nullptr || target == nullptr || rank == nullptr) return ULTRA_ERR_NULL_POINTER;
    if (filt_ptr != nullptr && filt_node == nullptr) return ULTRA_ERR_NULL_POINTER;
    hipLaunchKernelGGL(filtered_rank_kernel, dim3((unsigned)n_query), dim3(256), 0, static_cast<hipStream_t>(stream), pred,
                       (long long)row_stride, (long long)n_cand, target, filt_ptr, filt_node, rank);
    HIP_TRY(hipGetLastError());
    return ULTRA_OK;
}

}  // extern "C"

extern "C" {

int ultra_linear_forward_f32(const float *input, const float *weight, const float *bias, float *out, int64_t rows,
                             int64_t in_dim, int64_t out_dim, int relu, void *stream) {
    if (rows < 0) return ULTRA_ERR_BAD_SHAPE;
    if (rows == 0) return ULTRA_OK;
    if (input == nullptr || weight == nullptr || bias == nullptr || out == nullptr) return ULTRA_ERR_NULL_POINTER;
    hipStream_t s = static_cast<hipStream_t>(stream);
    DeviceInfo *di = nullptr;
    int rc = current_device_info(&di);
    if (rc) return rc;
    if (out_dim == 1 && in_dim % 4 == 0) {          // the 128 -> 1 score head (no activation after the last layer)
        if (relu) return ULTRA_ERR_BAD_SHAPE;
        const long long blocks = (rows + 255) / 256;
        hipLaunchKernelGGL(rowdot_kernel, dim3((unsigned)blocks), dim3(256), 0, s, input, weight, bias, out,
                           (long long)rows, (int)in_dim);
        HIP_TRY(hipGetLastError());
        return ULTRA_OK;
    }
    LinearParams p;
    p.input = input; p.weight = weight; p.bias = bias; p.out = out; p.rows = rows; p.relu = relu;
    if (in_dim == 64 && out_dim == 64) return launch_linear<64>(p, di->n_cu, s);
    if (in_dim == 128 && out_dim == 128) return launch_linear<128>(p, di->n_cu, s);
    return ULTRA_ERR_BAD_SHAPE;
}


int ultra_score_forward_f32(const float *hidden, const float *query, const float *w1, const float *b1, const float *w2,
                            const float *b2, float *query_bias, float *out, int64_t n_node, int64_t batch, void *stream) {
    if (n_node < 0 || batch < 0 || batch > 0x7fffffffLL) return ULTRA_ERR_BAD_SHAPE;
    if (n_node == 0 || batch == 0) return ULTRA_OK;
    if (n_node > 0xfffffff0LL / 4 / batch) return ULTRA_ERR_BAD_SHAPE;      // `out` is addressed as one buffer: < 4 GiB
    if (hidden == nullptr || query == nullptr || w1 == nullptr || b1 == nullptr || w2 == nullptr || b2 == nullptr ||
        query_bias == nullptr || out == nullptr)
        return ULTRA_ERR_NULL_POINTER;
    DeviceInfo *di = nullptr;
    int rc = current_device_info(&di);
    if (rc) return rc;
    ScoreParams p;
    p.hidden = hidden; p.query = query; p.w1 = w1; p.b1 = b1; p.w2 = w2; p.b2 = b2; p.qbias = query_bias; p.out = out;
    p.n_node = n_node; p.batch = (int)batch;
    const bool rpl = !g_knobs.score_lds_rows;           // knob bit 10: the column-per-lane product with its LDS row phase
    const size_t lds = rpl ? (size_t)(kScoreLdsBatch * kScoreCStride + kCbWaves * 32 * 68) * sizeof(float)
                           : (size_t)(128 * 68 + 128 + kScoreLdsBatch * kScoreCStride + kCbWaves * 32 * 132) * sizeof(float);
    hipLaunchKernelGGL(score_query_bias_kernel, dim3((unsigned)batch), dim3(128), 0, static_cast<hipStream_t>(stream), p);
    const long long n_tiles = (n_node * batch + 31) / 32;
    long long blocks = (n_tiles + kCbWaves - 1) / kCbWaves;
    if (blocks > di->n_cu) blocks = di->n_cu;
    HIP_TRY(hipGetLastError());
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (!rpl) return launch_with_lds(score_kernel_lds, p, (int)blocks, lds, st, kCbWaves * 64, (int)lds);
    if (batch > kScoreLdsBatch) return launch_with_lds(score_kernel<true>, p, (int)blocks, lds, st, kCbWaves * 64, (int)lds);
    return launch_with_lds(score_kernel<false>, p, (int)blocks, lds, st, kCbWaves * 64, (int)lds);
}

int ultra_relation_project_f32(const float *relation, int64_t stride_b, int64_t stride_r, const float *const *w1,
                               const float *const *b1, const float *const *w2, const float *const *b2, float *const *out,
                               int64_t n_layers, int64_t batch, int64_t repeat, int64_t n_rel, int64_t dim, void *stream) {
    if (dim != 64 || n_layers < 0 || batch < 0 || n_rel < 0 || batch > 0x7fffffffLL || n_rel > 0x7fffffffLL || repeat < 1 ||
        repeat > 64 || stride_b < 0 || stride_r < 0 || ((stride_b | stride_r) & 3))          // rows stay 16-byte aligned
        return ULTRA_ERR_BAD_SHAPE;
    if (n_layers == 0 || batch == 0 || n_rel == 0) return ULTRA_OK;
    if (relation == nullptr || w1 == nullptr || b1 == nullptr || w2 == nullptr || b2 == nullptr || out == nullptr)
        return ULTRA_ERR_NULL_POINTER;
    DeviceInfo *di = nullptr;
    int rc = current_device_info(&di);
    if (rc) return rc;
    const size_t lds = (size_t)(2 * 64 * 68 + kCbWaves * 32 * 68) * sizeof(float);
    for (int64_t first = 0; first < n_layers; first += kProjMaxLayers) {
        const int count = (int)((n_layers - first) < kProjMaxLayers ? (n_layers - first) : kProjMaxLayers);
        ProjectParams p{};
        p.relation = relation;
        for (int l = 0; l < count; ++l) {
            if (w1[first + l] == nullptr || b1[first + l] == nullptr || w2[first + l] == nullptr || b2[first + l] == nullptr ||
                out[first + l] == nullptr)
                return ULTRA_ERR_NULL_POINTER;
            p.w1[l] = w1[first + l]; p.b1[l] = b1[first + l]; p.w2[l] = w2[first + l]; p.b2[l] = b2[first + l];
            p.out[l] = out[first + l];
        }
        p.rows = batch * n_rel; p.batch = (int)batch; p.n_rel = (int)n_rel; p.n_layers = count; p.repeat = (int)repeat;
        p.stride_b = stride_b; p.stride_r = stride_r;
        const long long n_tiles = (p.rows + 31) / 32;
        long long per_layer = (n_tiles + kCbWaves - 1) / kCbWaves;
        const long long cap = (2LL * di->n_cu + count - 1) / count;          // ~2 workgroups per CU over all layers
        if (per_layer > cap) per_layer = cap;
        if (per_layer < 1) per_layer = 1;
        p.blocks_per_layer = (int)per_layer;
        rc = launch_with_lds(project_kernel, p, (int)(per_layer * count), lds, static_cast<hipStream_t>(stream), kCbWaves * 64, (int)lds);
        if (rc) return rc;
    }
    return ULTRA_OK;
}

}  // extern "C"

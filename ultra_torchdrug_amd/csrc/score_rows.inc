// score_rows.inc -- the score head on the CANDIDATE rows of a training step, forward and backward.
// (included by epilogue.hip, last)
//
//     score[b, j] = w2 . relu( W1 . cat[ hidden[t[b, j], b, :], query[b, :] ] + b1 ) + b2
//
// = ultra/model.py:177-183,193 with the candidates picked before the concatenation (B * (K + 1) = 2 064 rows of 128 inputs on
// a fine-tuning batch).  As ATen ops that is an index, a cat, two BLAS products and their backward -- four more products,
// bias sums, an index_put with a sort, fills and copies: ~55 launches, 0.35 ms of a 6 ms step for 70 MFLOP.  Here:
//   forward   score_rows_forward_kernel     a wave per row, W1 transposed in LDS; keeps h = relu(.) for the backward
//   backward  score_rows_backward_kernel    a workgroup per query b: d_pre, d_in = d_pre . W1 per row (a wave each), d_query[b]
//                                           summed in row order, d_hidden rows written in place (zero-filled by the caller's
//                                           call; rows that repeat inside a query are added one after the other)
//             score_rows_wgrad_*            d_W1, d_b1, d_w2, d_b2: sums over the rows in 16 slices, slices added in order
// fp32 throughout, every sum in a fixed order (deterministic); gradients agree with autograd of the reference chain to fp32
// rounding (tests/test_model_gpu.py).

namespace {

struct ScoreRowsParams {
    const float *hidden;        // [n_node, B, 64]
    const float *query;         // [B, 64]
    const long long *t_index;   // [B, K1]
    const float *w1;            // [128, 128]
    const float *b1;            // [128]
    const float *w2;            // [128]
    const float *b2;            // [1]
    float *h;                   // [B * K1, 128]  relu(pre): kept by the forward, read by the backward
    float *in_rows;             // [B * K1, 128]  cat[hidden row, query]: kept by the forward for the weight gradient
    float *partial;             // [kSrSlices, 129, 129] weight-gradient partial sums (backward scratch)
    float *score;               // [B, K1]
    const float *grad;          // [B, K1]        backward: d loss / d score
    float *d_pre;               // [B * K1, 128]
    float *d_hidden;            // [n_node, B, 64] zero-filled before the backward kernel runs
    float *d_query;             // [B, 64]
    float *d_w1;                // [128, 128]
    float *d_b1;                // [128]
    float *d_w2;                // [128]
    float *d_b2;                // [1]
    int n_batch, per_row;       // B, K1
};

constexpr int kSrThreads = 1024;
constexpr int kSrSlices = 16;                                     // row slices of the weight-gradient sums
constexpr int kSrWStride = 129;                                   // W1^T rows in LDS: 128 + 1 (bank spread for the staging writes)

// sum over the 64 lanes in a fixed tree (xor 32, 16, .. 1): every lane ends with the same value
__device__ __forceinline__ float sr_wave_sum(float v) {
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) v = v + __shfl_xor(v, m, 64);
    return v;
}

__global__ __launch_bounds__(kSrThreads) void score_rows_forward_kernel(const ScoreRowsParams p) {
    extern __shared__ float sr_lds[];
    float *wt = sr_lds;                                           // [128 k][kSrWStride]: W1^T
    float *in_lds = sr_lds + 128 * kSrWStride;                    // [16 waves][128]
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    for (int i = threadIdx.x; i < 128 * 128; i += kSrThreads) wt[(i & 127) * kSrWStride + (i >> 7)] = p.w1[i];
    __syncthreads();
    const int n_rows = p.n_batch * p.per_row;
    const float bias0 = p.b1[lane], bias1 = p.b1[lane + 64];
    const float v0 = p.w2[lane], v1 = p.w2[lane + 64];
    float *mine = in_lds + w * 128;
    for (int r = blockIdx.x * 16 + w; r < n_rows; r += gridDim.x * 16) {
        const int b = r / p.per_row;
        const long long t = p.t_index[r];
        const float xin = p.hidden[(t * p.n_batch + b) * 64 + lane], qin = p.query[(long long)b * 64 + lane];
        mine[lane] = xin;
        mine[64 + lane] = qin;
        p.in_rows[(long long)r * 128 + lane] = xin;
        p.in_rows[(long long)r * 128 + 64 + lane] = qin;
        __builtin_amdgcn_s_waitcnt(0xc07f);                       // lgkmcnt(0): this wave's LDS writes (one wave owns `mine`)
        float a0 = bias0, a1 = bias1;
#pragma unroll 8
        for (int k = 0; k < 128; ++k) {
            const float x = mine[k];
            a0 = __builtin_fmaf(wt[k * kSrWStride + lane], x, a0);
            a1 = __builtin_fmaf(wt[k * kSrWStride + 64 + lane], x, a1);
        }
        a0 = !(a0 <= 0.0f) ? a0 : 0.0f;
        a1 = !(a1 <= 0.0f) ? a1 : 0.0f;
        p.h[(long long)r * 128 + lane] = a0;
        p.h[(long long)r * 128 + 64 + lane] = a1;
        const float s = sr_wave_sum(a0 * v0 + a1 * v1);
        if (lane == 0) p.score[r] = s + p.b2[0];
    }
}

// one workgroup per query b: its K1 rows are dealt to the 16 waves (row j to wave j % 16)
__global__ __launch_bounds__(kSrThreads) void score_rows_backward_kernel(const ScoreRowsParams p) {
    extern __shared__ float sr_lds[];
    float *wl = sr_lds;                                           // [128 o][128 k]: W1 as it lies (lane k reads a row of o's)
    float *dp_lds = sr_lds + 128 * 128;                           // [16 waves][128]
    float *dq_lds = dp_lds + 16 * 128;                            // [K1][64] d_in of the query half, per row
    float *dx_lds = dq_lds + (size_t)p.per_row * 64;              // [K1][64] d_in of the hidden half, per row
    int *dup = reinterpret_cast<int *>(dx_lds + (size_t)p.per_row * 64);      // [K1]: 1 = an earlier row of this query has the same node
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int b = blockIdx.x, K1 = p.per_row;
    for (int i = threadIdx.x; i < 128 * 128; i += kSrThreads) wl[i] = p.w1[i];
    int *node = dup + K1;                                         // [K1] this query's candidate nodes (ids < 2^31)
    for (int j = threadIdx.x; j < K1; j += kSrThreads) node[j] = (int)p.t_index[(long long)b * K1 + j];
    __syncthreads();
    for (int j = threadIdx.x; j < K1; j += kSrThreads) {
        const int t = node[j];
        int d = 0;
        for (int e = 0; e < j; ++e) d |= (node[e] == t) ? 1 : 0;
        dup[j] = d;
    }
    __syncthreads();
    const float v0 = p.w2[lane], v1 = p.w2[lane + 64];
    float *mine = dp_lds + w * 128;
    for (int j = w; j < K1; j += 16) {
        const long long r = (long long)b * K1 + j;
        const float g = p.grad[r];
        const float h0 = p.h[r * 128 + lane], h1 = p.h[r * 128 + 64 + lane];
        const float d0 = h0 > 0.0f ? g * v0 : 0.0f, d1 = h1 > 0.0f ? g * v1 : 0.0f;
        p.d_pre[r * 128 + lane] = d0;
        p.d_pre[r * 128 + 64 + lane] = d1;
        mine[lane] = d0;
        mine[64 + lane] = d1;
        __builtin_amdgcn_s_waitcnt(0xc07f);                       // lgkmcnt(0): this wave's own LDS writes
        float x0 = 0.0f, x1 = 0.0f;                               // d_in[lane] (hidden half), d_in[64 + lane] (query half)
#pragma unroll 8
        for (int o = 0; o < 128; ++o) {
            const float d = mine[o];
            x0 = __builtin_fmaf(d, wl[o * 128 + lane], x0);
            x1 = __builtin_fmaf(d, wl[o * 128 + 64 + lane], x1);
        }
        dq_lds[j * 64 + lane] = x1;
        dx_lds[j * 64 + lane] = x0;
        if (!dup[j]) {                                            // the first row of its node in this query: plain store
            const long long t = p.t_index[r];
            p.d_hidden[(t * p.n_batch + b) * 64 + lane] = x0;
        }
    }
    __syncthreads();                                              // (waits for this wave's stores, then the barrier)
    // d_query[b] = sum over the rows, in row order (one wave)
    if (w == 0) {
        float acc = 0.0f;
        for (int j = 0; j < K1; ++j) acc = acc + dq_lds[j * 64 + lane];
        p.d_query[(long long)b * 64 + lane] = acc;
    }
    // rows whose node repeats inside this query (duplicate negatives: rare): ADDED one after the other, in row order
    if (w == 1) {
        for (int j = 0; j < K1; ++j) {
            if (!dup[j]) continue;
            const long long t = p.t_index[(long long)b * K1 + j];
            float *dst = p.d_hidden + (t * p.n_batch + b) * 64 + lane;
            const float cur = __builtin_nontemporal_load(dst);
            *dst = cur + dx_lds[j * 64 + lane];
            __builtin_amdgcn_s_waitcnt(0x0f70);                   // vmcnt(0): before the next row's load of (possibly) this address
        }
    }
}

// Weight gradients: d_W1 = d_pre^T . in, d_b1 = d_pre^T . 1, d_w2 = grad^T . h, d_b2 = grad^T . 1 -- sums over the rows.
// score_rows_wgrad_partial_kernel: block (o, s): output row o (o = 128: the second layer's row) over the rows of slice s, thread
// k one column (sixteen rows' operands in flight); score_rows_wgrad_reduce_kernel adds the slices in order.
__global__ __launch_bounds__(128) void score_rows_wgrad_partial_kernel(const ScoreRowsParams p) {
    const int k = threadIdx.x, o = blockIdx.x, sl = blockIdx.y;
    const int n_rows = p.n_batch * p.per_row;
    const int per = (n_rows + kSrSlices - 1) / kSrSlices;
    const int lo = sl * per, hi = min(lo + per, n_rows);
    const float *a_col = o < 128 ? p.d_pre + o : p.grad;          // A[r] = a_col[r * a_stride]
    const int a_stride = o < 128 ? 128 : 1;
    const float *bmat = o < 128 ? p.in_rows : p.h;                // B[r][k]
    float acc = 0.0f, asum = 0.0f;
    for (int r0 = lo; r0 < hi; r0 += 16) {
        float a[16], x[16];
#pragma unroll
        for (int u = 0; u < 16; ++u) {
            const int r = r0 + u < hi ? r0 + u : hi - 1;
            a[u] = a_col[(long long)r * a_stride];
            x[u] = bmat[(long long)r * 128 + k];
        }
#pragma unroll
        for (int u = 0; u < 16; ++u)
            if (r0 + u < hi) {
                acc = __builtin_fmaf(a[u], x[u], acc);
                asum = asum + a[u];
            }
    }
    float *out = p.partial + ((long long)sl * 129 + o) * 129;
    out[k] = acc;
    if (k == 0) out[128] = asum;
}

__global__ __launch_bounds__(129) void score_rows_wgrad_reduce_kernel(const ScoreRowsParams p) {
    const int k = threadIdx.x, o = blockIdx.x;                    // k = 128: the bias column
    float total = 0.0f;
    for (int sl = 0; sl < kSrSlices; ++sl) total = total + p.partial[((long long)sl * 129 + o) * 129 + k];
    if (o < 128) {
        if (k < 128) p.d_w1[o * 128 + k] = total;
        else p.d_b1[o] = total;
    } else {
        if (k < 128) p.d_w2[k] = total;
        else p.d_b2[0] = total;
    }
}

}  // namespace

extern "C" {

int ultra_score_rows_forward_f32(const float *hidden, const float *query, const int64_t *t_index, const float *w1, const float *b1,
                                 const float *w2, const float *b2, float *h, float *in_rows, float *score, int64_t n_batch,
                                 int64_t per_row, void *stream) {
    if (n_batch < 0 || per_row < 0 || n_batch * per_row > 0x7fffffffLL) return ULTRA_ERR_BAD_SHAPE;
    if (n_batch * per_row == 0) return ULTRA_OK;
    if (hidden == nullptr || query == nullptr || t_index == nullptr || w1 == nullptr || b1 == nullptr || w2 == nullptr ||
        b2 == nullptr || h == nullptr || in_rows == nullptr || score == nullptr)
        return ULTRA_ERR_NULL_POINTER;
    ScoreRowsParams p{};
    p.hidden = hidden; p.query = query; p.t_index = reinterpret_cast<const long long *>(t_index); p.w1 = w1; p.b1 = b1; p.w2 = w2;
    p.b2 = b2; p.h = h; p.in_rows = in_rows; p.score = score; p.n_batch = (int)n_batch; p.per_row = (int)per_row;
    const size_t lds = (size_t)(128 * kSrWStride + 16 * 128) * sizeof(float);
    int rc = ensure_lds_attribute(reinterpret_cast<const void *>(score_rows_forward_kernel), lds);
    if (rc) return rc;
    long long blocks = (n_batch * per_row + 15) / 16;
    if (blocks > 256) blocks = 256;
    hipLaunchKernelGGL(score_rows_forward_kernel, dim3((unsigned)blocks), dim3(kSrThreads), lds, static_cast<hipStream_t>(stream), p);
    HIP_TRY(hipGetLastError());
    return ULTRA_OK;
}

// d_hidden [n_node, B, 64] is zero-filled here (a fill kernel), then the candidate rows are written.  Scratch: d_pre
// [B * K1, 128], partial [16 * 129 * 129].
int ultra_score_rows_backward_f32(const float *hidden, const float *query, const int64_t *t_index, const float *w1, const float *w2,
                                  const float *h, const float *in_rows, const float *grad, float *d_pre, float *partial,
                                  float *d_hidden, float *d_query, float *d_w1, float *d_b1, float *d_w2, float *d_b2,
                                  int64_t n_node, int64_t n_batch, int64_t per_row, void *stream) {
    if (n_node < 0 || n_batch < 0 || per_row < 0 || n_batch * per_row > 0x7fffffffLL || per_row > 160) return ULTRA_ERR_BAD_SHAPE;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const long long n4 = n_node * n_batch * 16;
    const auto fill_d_hidden = [&]() -> int {
        const unsigned fb = (unsigned)((n4 + 256 * 8 - 1) / (256 * 8) < 4096 ? (n4 + 256 * 8 - 1) / (256 * 8) : 4096);
        hipLaunchKernelGGL(zero_fill_kernel, dim3(fb ? fb : 1), dim3(256), 0, s, reinterpret_cast<qf4 *>(d_hidden), n4);
        HIP_TRY(hipGetLastError());
        return ULTRA_OK;
    };
    if (n_batch * per_row == 0) {       // no rows: EVERY gradient is zero, d_query's too (the row operands are empty and may be NULL)
        if (d_w1 == nullptr || d_b1 == nullptr || d_w2 == nullptr || d_b2 == nullptr || (n4 > 0 && d_hidden == nullptr) ||
            (n_batch > 0 && d_query == nullptr))
            return ULTRA_ERR_NULL_POINTER;
        if (n4 > 0) {
            const int rc = fill_d_hidden();
            if (rc) return rc;
        }
        if (n_batch > 0) HIP_TRY(hipMemsetAsync(d_query, 0, (size_t)n_batch * 64 * sizeof(float), s));
        HIP_TRY(hipMemsetAsync(d_w1, 0, 128 * 128 * sizeof(float), s));
        HIP_TRY(hipMemsetAsync(d_b1, 0, 128 * sizeof(float), s));
        HIP_TRY(hipMemsetAsync(d_w2, 0, 128 * sizeof(float), s));
        HIP_TRY(hipMemsetAsync(d_b2, 0, sizeof(float), s));
        return ULTRA_OK;
    }
    // (`hidden` is not read by the backward -- its candidate rows are in in_rows -- and may be NULL)
    if (query == nullptr || t_index == nullptr || w1 == nullptr || w2 == nullptr || h == nullptr ||
        in_rows == nullptr || partial == nullptr || grad == nullptr || d_pre == nullptr || d_hidden == nullptr || d_query == nullptr || d_w1 == nullptr || d_b1 == nullptr ||
        d_w2 == nullptr || d_b2 == nullptr)
        return ULTRA_ERR_NULL_POINTER;
    if (n4 > 0) {
        const int rc = fill_d_hidden();
        if (rc) return rc;
    }
    ScoreRowsParams p{};
    p.hidden = hidden; p.query = query; p.t_index = reinterpret_cast<const long long *>(t_index); p.w1 = w1; p.w2 = w2;
    p.h = const_cast<float *>(h); p.in_rows = const_cast<float *>(in_rows); p.partial = partial; p.grad = grad; p.d_pre = d_pre; p.d_hidden = d_hidden; p.d_query = d_query; p.d_w1 = d_w1;
    p.d_b1 = d_b1; p.d_w2 = d_w2; p.d_b2 = d_b2; p.n_batch = (int)n_batch; p.per_row = (int)per_row;
    const size_t lds = (size_t)(128 * 128 + 16 * 128 + 2 * per_row * 64 + 2 * per_row) * sizeof(float);
    if (lds > (size_t)kMaxLdsBytes) return ULTRA_ERR_BAD_SHAPE;
    int rc = ensure_lds_attribute(reinterpret_cast<const void *>(score_rows_backward_kernel), lds);
    if (rc) return rc;
    hipLaunchKernelGGL(score_rows_backward_kernel, dim3((unsigned)n_batch), dim3(kSrThreads), lds, s, p);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(score_rows_wgrad_partial_kernel, dim3(129, kSrSlices), dim3(128), 0, s, p);
    hipLaunchKernelGGL(score_rows_wgrad_reduce_kernel, dim3(129), dim3(129), 0, s, p);
    HIP_TRY(hipGetLastError());
    return ULTRA_OK;
}

}  // extern "C"

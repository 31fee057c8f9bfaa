// first_layer_train.inc -- the FIRST layer of an entity Bellman-Ford in TRAINING, sparse end to end (round 5; VERDICT r4 item 5 i).
// (included by epilogue.hip, after combine_fused_bwd.inc)
//
// The first layer's input is the boundary (/root/reference/ultra/model.py:106-107,116-120): zero outside one row per query.  A row
// (v, q) that no out-edge of the query's boundary node reaches (and v is not that node) has a zero input row and a zero update row:
// its output is ONE vector for the whole layer, c = [0 +] relu(LayerNorm(bias)).  Inference has used that since round 4
// (ultra_first_layer_sparse_f32).  In training the layer's backward on such a row is a FIXED linear map of its upstream gradient:
//     d_weight += d_z^T . [0; 0] = 0;    d_input, d_update of the row are never read (the boundary's gradient is consumed at the
//     boundary rows, the rspmm backward of this layer reads d_update at the destinations of the boundary nodes' out-edges: all listed);
//     d_beta += g * m,  d_gamma += (g * m) * n,  d_bias += J . ((g * m) * gamma)
// with m = [LayerNorm(bias) * gamma + beta > 0] (relu), n = the normalised bias row and J the LayerNorm Jacobian at z = bias -- the same
// for every such row, so the sums over the ~99.9 % untouched rows need only the COLUMN SUMS of the upstream gradient over them:
// (sum over all rows) - (sum over the listed rows).  The listed rows -- (node, query) rows of different queries rarely share a 32-row
// tile, so a tile list would carry ~32 rows per listed row (the first build: 166 us where the dense kernel took 335) -- are
// COMPACTED: gathered into dense buffers, run through the ordinary one-pass epilogue backward (which reads the row count from the
// device), and their d_input / d_update rows scattered back.
//   forward : ultra_first_layer_sparse_train_f32 -- constant fill of `out`, the frontier's rows into `update` (listed; every other
//             row of `update` stays unwritten and is never read), the epilogue on the listed rows update -> out
//   backward: ultra_first_layer_epilogue_backward_f32 -- zero fill of d_input, gather of the listed rows of input / update / grad_out,
//             the one-pass backward on them, scatter of d_input / d_update, column sums of grad_out over all rows and over the
//             listed rows, and the untouched rows' share added to d_bias / d_gamma / d_beta.
// Gradients equal the dense layer's up to the association of the sums (tests/test_model_gpu.py).

namespace {

// the listed rows of up to three (rows, 64) matrices, compacted: dst[k] = src[row_list[k]] for k < count; zero rows up to the next
// multiple of 32 (the backward's last tile); 16 lanes x 16 bytes per row
struct GatherRowsParams {
    const int32_t *row_list;
    const int32_t *count;       // device: entries of row_list in use (clamped to cap)
    int cap;                    // slots of row_list
    int cap32;                  // rows of the compact buffers: cap rounded up to whole 32-row tiles
    const float *src[3];
    float *dst[3];
    int n_arrays;
    long long rows;             // rows of the source matrices (row ids at or beyond it are treated as empty slots)
};

__global__ __launch_bounds__(256) void gather_rows_kernel(const GatherRowsParams p) {
    const int count = min(p.count[0], p.cap);
    const int padded = min((count + 31) / 32 * 32, p.cap32);       // (the buffers hold cap32 rows: the last tile is always whole)
    const int part = threadIdx.x & 15;
    for (long long k = ((long long)blockIdx.x * 256 + threadIdx.x) >> 4; k < padded; k += ((long long)gridDim.x * 256) >> 4) {
        const int row = k < count ? p.row_list[k] : -1;
        const bool live = row >= 0 && row < p.rows;
        for (int a = 0; a < p.n_arrays; ++a) {
            qf4 v = {0.0f, 0.0f, 0.0f, 0.0f};
            if (live) v = *reinterpret_cast<const qf4 *>(p.src[a] + (long long)row * 64 + 4 * part);
            *reinterpret_cast<qf4 *>(p.dst[a] + k * 64 + 4 * part) = v;
        }
    }
}

// ... and back: dst[row_list[k]] = src[k] (the listed rows are distinct: one slot per (source, destination) run)
__global__ __launch_bounds__(256) void scatter_rows_kernel(const GatherRowsParams p) {
    const int count = min(p.count[0], p.cap);
    const int part = threadIdx.x & 15;
    for (long long k = ((long long)blockIdx.x * 256 + threadIdx.x) >> 4; k < count; k += ((long long)gridDim.x * 256) >> 4) {
        const int row = p.row_list[k];
        if (row < 0 || row >= p.rows) continue;
        for (int a = 0; a < p.n_arrays; ++a)
            *reinterpret_cast<qf4 *>(p.dst[a] + (long long)row * 64 + 4 * part) = *reinterpret_cast<const qf4 *>(p.src[a] + k * 64 + 4 * part);
    }
}

// Column sums of a (rows, 64) matrix, deterministic: block b sums its rows in row order per (column, row slice) lane, the slices and
// then the blocks are added in a fixed order.  rows_dev (optional): the number of rows that count, on the device.
constexpr int kColSumBlocks = 512;

__global__ __launch_bounds__(256) void column_sum_partial_kernel(const float *x, long long rows, const int32_t *rows_dev, float *partial) {
    __shared__ float part[4][64];
    const int c = threadIdx.x & 63, slice = threadIdx.x >> 6;          // 4 row slices x 64 columns
    if (rows_dev != nullptr) rows = min(rows, (long long)rows_dev[0]);
    float acc = 0.0f;
    const long long per = (rows + gridDim.x - 1) / gridDim.x;
    const long long r0 = (long long)blockIdx.x * per, r1 = min(r0 + per, rows);
    for (long long r = r0 + slice; r < r1; r += 32) {                  // rows r0 + slice, + 4, ...: 8 loads in flight, added in order
        float v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = (r + 4 * j < r1) ? x[(r + 4 * j) * 64 + c] : 0.0f;
#pragma unroll
        for (int j = 0; j < 8; ++j)
            if (r + 4 * j < r1) acc = acc + v[j];
    }
    part[slice][c] = acc;
    __syncthreads();
    if (slice == 0) partial[(long long)blockIdx.x * 64 + c] = ((part[0][c] + part[1][c]) + part[2][c]) + part[3][c];
}

// the blocks' partials: 16 slices of blocks (b = slice, slice + 16, ...) summed in order each, then the slices in order
__global__ __launch_bounds__(1024) void column_sum_final_kernel(const float *partial, int n_blocks, float *out) {
    __shared__ float part[16][64];
    const int c = threadIdx.x & 63, slice = threadIdx.x >> 6;
    float acc = 0.0f;
    for (int b0 = slice; b0 < n_blocks; b0 += 16 * 8) {
        float v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = (b0 + 16 * j < n_blocks) ? partial[(long long)(b0 + 16 * j) * 64 + c] : 0.0f;
#pragma unroll
        for (int j = 0; j < 8; ++j)
            if (b0 + 16 * j < n_blocks) acc = acc + v[j];
    }
    part[slice][c] = acc;
    __syncthreads();
    if (slice == 0) {
        float total = part[0][c];
#pragma unroll
        for (int k = 1; k < 16; ++k) total = total + part[k][c];
        out[c] = total;
    }
}

// The untouched rows' share of the epilogue's parameter gradients (see the header of this file): one thread per column.
__global__ __launch_bounds__(64) void const_rows_backward_kernel(const float *sum_all, const float *sum_tiles, const float *bias,
                                                                 const float *gamma, const float *beta, float eps, int relu,
                                                                 float *d_bias, float *d_gamma, float *d_beta) {
    __shared__ float red[64];
    const int j = threadIdx.x;
    const float g = sum_all[j] - sum_tiles[j];                          // column sum of the upstream gradient over the untouched rows
    auto total = [&](float v) -> float {                                // sum over the 64 columns, every thread gets it
        __syncthreads();
        red[j] = v;
        __syncthreads();
        float s = 0.0f;
        for (int k = 0; k < 64; ++k) s = s + red[k];
        return s;
    };
    if (gamma == nullptr) {                                             // no LayerNorm: y = z = bias
        const float m = relu ? (bias[j] > 0.0f ? 1.0f : 0.0f) : 1.0f;
        d_bias[j] = d_bias[j] + g * m;
        return;
    }
    const float mean = total(bias[j]) * (1.0f / 64.0f);
    const float dlt = bias[j] - mean;
    const float var = total(dlt * dlt) * (1.0f / 64.0f);
    const float inv = 1.0f / sqrtf(var + eps);
    const float n = dlt * inv;
    const float y = n * gamma[j] + beta[j];
    const float m = relu ? (y > 0.0f ? 1.0f : 0.0f) : 1.0f;
    const float dy = g * m;
    d_beta[j] = d_beta[j] + dy;
    d_gamma[j] = d_gamma[j] + dy * n;
    const float dn = dy * gamma[j];
    const float s1 = total(dn) * (1.0f / 64.0f), s2 = total(dn * n) * (1.0f / 64.0f);
    d_bias[j] = d_bias[j] + inv * (dn - s1 - n * s2);
}


// d_relation of the FIRST layer from the boundary nodes' out-edges only.  The layer's input is zero outside row src_node[b] of column
// block b, so of the E edges the d_relation plan walks, only the out-edges of that one node contribute to block b: the masked full
// kernel (quad_kernel<KIND_DREL, ACT = 3>) still reads every edge word to find them.  Here one 16-lane group takes one ITEM of the
// plan -- a piece of a split relation row, or a whole unsplit row: a range [begin, end) of the plan's edge order -- and one column
// block, finds the boundary node's out-edges inside that range (src_relpos: per source node the plan positions of its out-edges,
// ascending) and sums them in plan order from 0; pieces go to the fix-up's slots.  Skipped edges would have added +0 to an
// accumulator that is never -0: the same bits as the masked kernel.
struct DrelBoundaryParams {
    const int32_t *items;        // [n_items][3] {begin, end, target}: target >= 0 a relation row, < 0 piece slot -(target + 1)
    const int32_t *dst;          // plan's node_b
    const float *weight;         // plan's weights or null
    const int32_t *src_ptr, *src_relpos, *src_node;
    const float *input, *grad;
    float *partial, *out;
    long long F;
    int n_items, n_tiles, n_src;
};

template <bool UNIT_W>
__global__ __launch_bounds__(256) void drel_boundary_kernel(const DrelBoundaryParams p) {
    const long long g = ((long long)blockIdx.x * 256 + threadIdx.x) >> 4;
    if (g >= (long long)p.n_items * p.n_tiles) return;
    const int item = (int)(g / p.n_tiles), tile = (int)(g - (long long)item * p.n_tiles);
    const int begin = p.items[item * 3 + 0], end = p.items[item * 3 + 1], target = p.items[item * 3 + 2];
    const long long col = (long long)tile * kTile + (threadIdx.x & 15) * 4;
    const int h = p.src_node[tile];
    qf4 acc = qf4{0.0f, 0.0f, 0.0f, 0.0f};
    if (h >= 0 && h < p.n_src && begin < end) {
        int lo = p.src_ptr[h];
        const int hi = p.src_ptr[h + 1];
        int top = hi;
        while (lo < top) {                                   // first out-edge at or behind `begin`
            const int mid = (lo + top) >> 1;
            if (p.src_relpos[mid] < begin) lo = mid + 1; else top = mid;
        }
        const qf4 x = *reinterpret_cast<const qf4 *>(p.input + (long long)h * p.F + col);
        constexpr int U = 8;
        for (int e = lo; e < hi; e += U) {
            int pos[U];
            qf4 gv[U];
            float w[U];
#pragma unroll
            for (int u = 0; u < U; ++u) pos[u] = p.src_relpos[min(e + u, hi - 1)];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const bool live = e + u < hi && pos[u] < end;
                const int at = live ? pos[u] : begin;
                gv[u] = *reinterpret_cast<const qf4 *>(p.grad + (long long)p.dst[at] * p.F + col);
                w[u] = UNIT_W ? 1.0f : p.weight[at];
            }
            bool done = false;
#pragma unroll
            for (int u = 0; u < U; ++u) {
                if (e + u >= hi || pos[u] >= end) { done = true; break; }
                qf4 c = gv[u];
                if constexpr (!UNIT_W) c = c * w[u];
                c = c * x;
                acc = acc + c;
            }
            if (done) break;
        }
    }
    float *to = target >= 0 ? p.out + (long long)target * p.F : p.partial + (long long)(-target - 1) * p.F;
    *reinterpret_cast<qf4 *>(to + col) = acc;
}

}  // namespace

extern "C" {

int ultra_column_sum_blocks(void) { return kColSumBlocks; }

int ultra_column_sum_f32(const float *x, int64_t rows, const int32_t *rows_dev, float *partial_workspace, float *out, void *stream) {
    if (rows < 0) return ULTRA_ERR_BAD_SHAPE;
    if (x == nullptr || partial_workspace == nullptr || out == nullptr) return ULTRA_ERR_NULL_POINTER;
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(column_sum_partial_kernel, dim3(kColSumBlocks), dim3(256), 0, s, x, (long long)rows, rows_dev, partial_workspace);
    hipLaunchKernelGGL(column_sum_final_kernel, dim3(1), dim3(1024), 0, s, partial_workspace, kColSumBlocks, out);
    HIP_TRY(hipGetLastError());
    return ULTRA_OK;
}

size_t ultra_first_layer_epilogue_backward_workspace(int device, int64_t list_cap) {
    if (list_cap <= 0) return 0;
    const int64_t cap32 = (list_cap + 31) / 32 * 32;
    int n_waves = 0;
    if (ultra_combine_backward_fused_waves(device, cap32, &n_waves)) return 0;
    return (size_t)(5 * cap32 * 64 + (int64_t)n_waves * (64 * 128 + 192) + (int64_t)kColSumBlocks * 64 + 128) * sizeof(float);
}

int ultra_first_layer_epilogue_backward_f32(const float *input, const float *update, const float *grad_out, const int32_t *row_list,
                                            const int32_t *list_count, int64_t list_cap, const float *weight, const float *bias,
                                            const float *ln_weight, const float *ln_bias, float ln_eps, int relu, int shortcut,
                                            float *d_input, float *d_update, float *d_weight, float *d_bias, float *d_ln_weight,
                                            float *d_ln_bias, float *workspace, size_t workspace_bytes, int64_t rows, void *stream) {
    if (rows <= 0 || list_cap <= 0 || list_cap > 0x7fffffffLL || rows > (1LL << 24) - 64) return ULTRA_ERR_BAD_SHAPE;
    if (input == nullptr || update == nullptr || grad_out == nullptr || row_list == nullptr || list_count == nullptr || weight == nullptr ||
        bias == nullptr || d_input == nullptr || d_update == nullptr || d_weight == nullptr || d_bias == nullptr || workspace == nullptr)
        return ULTRA_ERR_NULL_POINTER;
    if (ln_weight != nullptr && (ln_bias == nullptr || d_ln_weight == nullptr || d_ln_bias == nullptr)) return ULTRA_ERR_NULL_POINTER;
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    if (workspace_bytes < ultra_first_layer_epilogue_backward_workspace(dev, list_cap)) return ULTRA_ERR_WORKSPACE;
    const int64_t cap32 = (list_cap + 31) / 32 * 32;
    if (cap32 > (1LL << 24) - 64) return ULTRA_ERR_BAD_SHAPE;
    int n_waves = 0;
    int rc = ultra_combine_backward_fused_waves(dev, cap32, &n_waves);
    if (rc) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    float *c_in = workspace, *c_up = c_in + cap32 * 64, *c_go = c_up + cap32 * 64, *c_din = c_go + cap32 * 64, *c_dup = c_din + cap32 * 64;
    float *fused_ws = c_dup + cap32 * 64;
    float *sum_ws = fused_ws + (int64_t)n_waves * (64 * 128 + 192);
    float *s_all = sum_ws + (int64_t)kColSumBlocks * 64, *s_list = s_all + 64;
    // d_input leaves the autograd node: zero outside the listed rows (d_update is read at listed rows only: no fill)
    {
        const long long n4 = rows * 16;
        const unsigned fb = (unsigned)((n4 + 256 * 8 - 1) / (256 * 8) < 4096 ? (n4 + 256 * 8 - 1) / (256 * 8) : 4096);
        hipLaunchKernelGGL(zero_fill_kernel, dim3(fb ? fb : 1), dim3(256), 0, s, reinterpret_cast<qf4 *>(d_input), n4);
    }
    GatherRowsParams g{};
    g.row_list = row_list; g.count = list_count; g.cap = (int)list_cap; g.cap32 = (int)cap32; g.rows = rows; g.n_arrays = 3;
    g.src[0] = input; g.src[1] = update; g.src[2] = grad_out; g.dst[0] = c_in; g.dst[1] = c_up; g.dst[2] = c_go;
    hipLaunchKernelGGL(gather_rows_kernel, dim3(1024), dim3(256), 0, s, g);
    HIP_TRY(hipGetLastError());
    rc = combine_backward_fused_impl(c_in, c_up, weight, bias, ln_weight, ln_bias, ln_eps, relu, shortcut, c_go, nullptr, c_din, c_dup,
                                     d_weight, d_bias, d_ln_weight, d_ln_bias, fused_ws, (size_t)n_waves * (64 * 128 + 192) * sizeof(float),
                                     nullptr, 0, cap32, 64, 0, list_count, s);
    if (rc) return rc;
    GatherRowsParams sc{};
    sc.row_list = row_list; sc.count = list_count; sc.cap = (int)list_cap; sc.cap32 = (int)cap32; sc.rows = rows; sc.n_arrays = 2;
    sc.src[0] = c_din; sc.src[1] = c_dup; sc.dst[0] = d_input; sc.dst[1] = d_update;
    hipLaunchKernelGGL(scatter_rows_kernel, dim3(1024), dim3(256), 0, s, sc);
    HIP_TRY(hipGetLastError());
    // the untouched rows' share of d_bias / d_gamma / d_beta from the column sums of the upstream gradient over them (listed rows whose
    // slot is empty (-1) were gathered as zero rows: they add nothing to either sum)
    rc = ultra_column_sum_f32(grad_out, rows, nullptr, sum_ws, s_all, stream);
    if (rc) return rc;
    rc = ultra_column_sum_f32(c_go, cap32, list_count, sum_ws, s_list, stream);
    if (rc) return rc;
    hipLaunchKernelGGL(const_rows_backward_kernel, dim3(1), dim3(64), 0, s, s_all, s_list, bias, ln_weight, ln_bias, ln_eps, relu, d_bias,
                       d_ln_weight, d_ln_bias);
    HIP_TRY(hipGetLastError());
    return ULTRA_OK;
}

int ultra_rspmm_drelation_boundary_f32(const ultra_segments *by_rel, const int32_t *items, int64_t n_items, const int32_t *src_ptr,
                                       const int32_t *src_relpos, const int32_t *src_node, const float *input,
                                       const float *output_grad, float *d_relation, void *workspace, size_t workspace_bytes,
                                       int64_t n_src, int64_t n_rel, int64_t F, void *stream) {
    if (by_rel == nullptr || src_node == nullptr || input == nullptr || output_grad == nullptr || d_relation == nullptr)
        return ULTRA_ERR_NULL_POINTER;
    if (!segments_abi_ok(by_rel)) return ULTRA_ERR_ABI;
    if (F <= 0 || F % kTile != 0 || n_rel != by_rel->n_rows || n_items < n_rel || n_items > 0x7fffffffLL || n_src <= 0 ||
        n_items != by_rel->n_pieces + n_rel - by_rel->n_long_rows)
        return ULTRA_ERR_BAD_SHAPE;
    if (n_rel == 0) return ULTRA_OK;
    if (items == nullptr || src_ptr == nullptr || (by_rel->n_edges > 0 && (src_relpos == nullptr || by_rel->node_b == nullptr)))
        return ULTRA_ERR_NULL_POINTER;
    if (by_rel->n_pieces > 0 && (workspace == nullptr || workspace_bytes < (size_t)by_rel->n_pieces * (size_t)F * sizeof(float)))
        return ULTRA_ERR_WORKSPACE;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int n_tiles = (int)(F / kTile);
    DrelBoundaryParams p{};
    p.items = items; p.dst = by_rel->node_b; p.weight = by_rel->weight; p.src_ptr = src_ptr; p.src_relpos = src_relpos;
    p.src_node = src_node; p.input = input; p.grad = output_grad; p.partial = static_cast<float *>(workspace); p.out = d_relation;
    p.F = F; p.n_items = (int)n_items; p.n_tiles = n_tiles; p.n_src = (int)n_src;
    const long long groups = (long long)n_items * n_tiles;
    const long long blocks = (groups + 15) / 16;
    if (blocks > 0x7fffffffLL) return ULTRA_ERR_BAD_SHAPE;
    if (by_rel->weight == nullptr) hipLaunchKernelGGL(drel_boundary_kernel<true>, dim3((int)blocks), dim3(256), 0, s, p);
    else hipLaunchKernelGGL(drel_boundary_kernel<false>, dim3((int)blocks), dim3(256), 0, s, p);
    HIP_TRY(hipGetLastError());
    if (by_rel->n_long_rows > 0) {
        FixParams fp{};
        fp.long_rows = by_rel->long_rows; fp.partial = p.partial; fp.out = d_relation; fp.F = F;
        fp.n_long = (int)by_rel->n_long_rows; fp.n_tiles = n_tiles;
        const long long waves = (long long)fp.n_long * n_tiles;
        const int fgrid = (int)((waves + 3) / 4);
        if (by_rel->n_pieces >= 128 * by_rel->n_long_rows)
            hipLaunchKernelGGL((fixup_kernel<ULTRA_SUM_ADD, 64>), dim3(fgrid), dim3(256), 0, s, fp);
        else hipLaunchKernelGGL(fixup_kernel<ULTRA_SUM_ADD>, dim3(fgrid), dim3(256), 0, s, fp);
        HIP_TRY(hipGetLastError());
    }
    return ULTRA_OK;
}

}  // extern "C"

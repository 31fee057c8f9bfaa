// guard.inc -- the divergence guard of training steps: does any of a LIST of fp32 tensors hold an inf or a NaN?  (the contract
// is in include/ultra_rspmm.h; engine.FiniteGuard is the caller).  The reference trains under torch.autograd.set_detect_anomaly
// (script/run_full.py:127), which stops a run at the step that produces a NaN; a captured step can read nothing back, so it
// leaves its verdict in a small device record that the host polls outside the graph.
//
//   nonfinite_scan_kernel    one launch per kGuardTensors tensors: their addresses and sizes travel BY VALUE in the kernel
//                            arguments (a hipGraph kernel node stores them; no table in device memory, so no memcpy node and no
//                            memset node enters a captured step).  Block b scans one chunk of kGuardChunk elements of one tensor
//                            (a prefix table of chunk counts maps b to its tensor).  An element is non-finite iff its exponent
//                            bits are all ones.  The chunk is read as 16-byte words from the first 16-byte boundary on, the up to
//                            three elements before it and after the last whole word one by one: a view that starts at an odd
//                            element offset scans like any other.  A wave that met a non-finite element does ONE
//                            atomicMin(&record[pending], index of the tensor): the lowest index wins whatever order the blocks ran
//                            in (an ordinary global integer atomic from one lane).
//   nonfinite_commit_kernel  one thread, ordered behind the scans of a step on the stream: moves `pending` into the sticky
//                            `tripped_*` pair if nothing tripped before, resets `pending`, counts the step.  With advance = 0
//                            it only latches: a step scans its parameters BEFORE the forward and latches them, so a parameter
//                            that was bad when the step began is what the record names, not the loss it went on to ruin
//                            (index 0, which would win the atomicMin of a single commit).
namespace {
constexpr int kGuardTensors = 32;                    // tensors per launch
constexpr int kGuardChunk = 4096;                    // fp32 elements per block
constexpr int kGuardThreads = 256;
constexpr int kGuardClean = 0x7fffffff;              // record[pending] when nothing was found

struct GuardTable {
    const uint32_t *ptr[kGuardTensors];
    long long numel[kGuardTensors];
    int first_block[kGuardTensors + 1];              // first_block[t + 1] - first_block[t] = chunks of tensor t
    int n_tensors;
    int first_index;
};

__device__ inline uint32_t guard_bad(uint32_t bits) { return (bits & 0x7f800000u) == 0x7f800000u ? 1u : 0u; }

__global__ __launch_bounds__(kGuardThreads) void nonfinite_scan_kernel(const GuardTable table, int32_t *record) {
    const int block = (int)blockIdx.x;
    int t = 0;
    while (t + 1 < table.n_tensors && table.first_block[t + 1] <= block) ++t;     // (uniform: scalar loads of the arguments)
    const long long start = (long long)(block - table.first_block[t]) * kGuardChunk;
    const long long left = table.numel[t] - start;
    if (left <= 0) return;
    const int count = left < kGuardChunk ? (int)left : kGuardChunk;
    const uint32_t *base = table.ptr[t] + start;
    // [0, head): before the first 16-byte boundary; then n_wide whole words; then tail elements
    int head = (int)((16u - (unsigned)(reinterpret_cast<uintptr_t>(base) & 15u)) & 15u) >> 2;
    if (head > count) head = count;
    const int n_wide = (count - head) >> 2;
    const int tail_at = head + 4 * n_wide;
    uint32_t bad = 0;
    if ((int)threadIdx.x < head) bad = guard_bad(base[threadIdx.x]);
    const uint4 *wide = reinterpret_cast<const uint4 *>(base + head);
    for (int v = (int)threadIdx.x; v < n_wide; v += kGuardThreads) {
        const uint4 w = wide[v];
        bad |= guard_bad(w.x) | guard_bad(w.y) | guard_bad(w.z) | guard_bad(w.w);      // (no short circuit: one 16-byte load)
    }
    if ((int)threadIdx.x < count - tail_at) bad |= guard_bad(base[tail_at + threadIdx.x]);
    if (__any((int)bad) && (threadIdx.x & 63u) == 0) atomicMin(&record[ULTRA_GUARD_PENDING], table.first_index + t);
}

__global__ void nonfinite_commit_kernel(int32_t *record, int advance) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    const int32_t pending = record[ULTRA_GUARD_PENDING];
    const int32_t step = record[ULTRA_GUARD_STEP] + 1;                 // the step under way: steps are numbered from 1
    if (record[ULTRA_GUARD_TRIPPED_STEP] < 0 && pending != kGuardClean) {
        record[ULTRA_GUARD_TRIPPED_STEP] = step;
        record[ULTRA_GUARD_TRIPPED_TENSOR] = pending;
    }
    record[ULTRA_GUARD_PENDING] = kGuardClean;
    if (advance) record[ULTRA_GUARD_STEP] = step;
}
}  // namespace

extern "C" int ultra_nonfinite_scan_tensors(void) { return kGuardTensors; }
extern "C" int ultra_nonfinite_scan_chunk(void) { return kGuardChunk; }

extern "C" int ultra_nonfinite_scan_f32(const float *const *ptrs, const int64_t *numel, int64_t n_tensors, int64_t first_index,
                                        int32_t *record, void *stream) {
    if (n_tensors < 0 || first_index < 0 || first_index + n_tensors >= (int64_t)kGuardClean) return ULTRA_ERR_BAD_SHAPE;
    if (n_tensors == 0) return ULTRA_OK;
    if (ptrs == nullptr || numel == nullptr || record == nullptr) return ULTRA_ERR_NULL_POINTER;
    for (int64_t i = 0; i < n_tensors; ++i) {                          // nothing is launched for a list with a bad entry
        if (numel[i] < 0) return ULTRA_ERR_BAD_SHAPE;
        if (numel[i] > 0 && ptrs[i] == nullptr) return ULTRA_ERR_NULL_POINTER;
        if (reinterpret_cast<uintptr_t>(ptrs[i]) & 3u) return ULTRA_ERR_BAD_SHAPE;
        if ((numel[i] + kGuardChunk - 1) / kGuardChunk > 0x3fffffffLL) return ULTRA_ERR_BAD_SHAPE;
    }
    int64_t at = 0;
    while (at < n_tensors) {
        GuardTable table{};
        long long blocks = 0;
        int n = 0;
        // a launch takes up to kGuardTensors tensors and at most 2^30 blocks (a longer tensor starts a launch of its own)
        while (at + n < n_tensors && n < kGuardTensors) {
            const long long chunks = (numel[at + n] + kGuardChunk - 1) / kGuardChunk;
            if (n > 0 && blocks + chunks > 0x3fffffffLL) break;
            table.ptr[n] = reinterpret_cast<const uint32_t *>(ptrs[at + n]);
            table.numel[n] = numel[at + n];
            table.first_block[n] = (int)blocks;
            blocks += chunks;
            ++n;
        }
        for (int i = n; i <= kGuardTensors; ++i) table.first_block[i] = (int)blocks;
        table.n_tensors = n;
        table.first_index = (int)(first_index + at);
        if (blocks > 0) {
            hipLaunchKernelGGL(nonfinite_scan_kernel, dim3((unsigned)blocks), dim3(kGuardThreads), 0,
                               static_cast<hipStream_t>(stream), table, record);
            HIP_TRY(hipGetLastError());
        }
        at += n;
    }
    return ULTRA_OK;
}

extern "C" int ultra_nonfinite_commit(int32_t *record, int advance, void *stream) {
    if (record == nullptr) return ULTRA_ERR_NULL_POINTER;
    hipLaunchKernelGGL(nonfinite_commit_kernel, dim3(1), dim3(1), 0, static_cast<hipStream_t>(stream), record,
                       advance);
    HIP_TRY(hipGetLastError());
    return ULTRA_OK;
}

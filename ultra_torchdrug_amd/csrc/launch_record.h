// launch_record.h -- which kernel a plan run actually launched, as a small per-thread record (internal to libultra_rspmm.so).
//
// Plain C++17: nothing from HIP, no heap, no locks, no getenv, so tests/launch_record_main.cpp compiles this header with the
// host compiler alone.  The launchers of the plan_*.hip units (plan_kernels.h) write one record per plan run AT THEIR LEAVES, from the
// template arguments they instantiate (not from plan_path()'s decision: the mapping from decision to kernel is what the record
// lets a test see); launch_fixup adds the fix-up kernel to the record of the run it belongs to.  A record is a row of int32;
// a field a family does not have holds -1.  Writing one is a handful of integer stores.
#ifndef ULTRA_LAUNCH_RECORD_H
#define ULTRA_LAUNCH_RECORD_H

#include <cstdint>
#include <cstring>

namespace ultra_detail {

constexpr int kFamRotate = 5;      // `family` of run_rotate_plan, which dispatches outside plan_path(); 0 .. 4 are plan_path.h's Family

struct LaunchRecord {
    int32_t seq = 0;                // per-thread count of plan runs that reached a launch, this one included
    int32_t status = 0;             // what the launch returned (ultra_status)
    int32_t family = -1;            // Family, or kFamRotate
    int32_t kind = -1;              // KIND_FWD / KIND_DX / KIND_DREL (rowgroup: from BACKWARD)
    int32_t sum = -1, mul = -1;     // template SUM / MUL (rotate: mul -1)
    int32_t unit_w = -1;            // template UNIT_W
    int32_t var = -1;               // packed_kernel VAR
    int32_t x_lds = -1;             // quad_kernel X_LDS
    int32_t unroll = -1;            // quad_kernel U / packed_kernel UNROLL: edges in flight, as instantiated
    int32_t act = -1, dead = -1;    // quad_kernel ACT / DEAD
    int32_t rel_lds = -1;           // segment_kernel / rotate_segment_kernel REL_LDS
    int32_t rel_mode = -1, group = -1, needs_rel = -1, backward = -1;     // rowgroup_kernel REL / G / NEEDS_REL / BACKWARD
    int32_t concurrent = -1;        // quad: the value copied into the kernel's parameters
    int32_t grid = -1, block = -1, lds = -1;      // as passed to launch_with_lds
    int32_t n_tiles = -1, split = -1, n_slots = -1, blocks_per_label = -1;     // the kernel's parameters
    int32_t n_rel_lds = -1;         // rowgroup: the kernel's parameter
    int32_t fixup = 0;              // Fixup: 0 none, 1 plain, 2 many
    int32_t fixup_sum = -1;         // the reduction fixup_kernel was instantiated with
    int32_t fixup_grid = -1;
};

constexpr int kLaunchRecordFields = (int)(sizeof(LaunchRecord) / sizeof(int32_t));
static_assert(sizeof(LaunchRecord) == kLaunchRecordFields * sizeof(int32_t), "a record is a row of int32");

// the fields in the order of the struct, space-separated (ultra_rspmm_launch_record_fields)
constexpr const char *kLaunchRecordFieldNames =
    "seq status family kind sum mul unit_w var x_lds unroll act dead rel_lds rel_mode group needs_rel backward concurrent grid block "
    "lds n_tiles split n_slots blocks_per_label n_rel_lds fixup fixup_sum fixup_grid";

// The last kSlots records of one thread, and how many were written since the last clear (not capped: a reader sees an
// overflow).  `seq` goes on counting across clears, so a record left over from an earlier call never looks new.
struct LaunchRing {
    static constexpr int kSlots = 8;
    LaunchRecord slot[kSlots];
    int32_t seq = 0;
    int64_t written = 0;

    LaunchRecord &push(const LaunchRecord &r) {
        LaunchRecord &dst = slot[written % kSlots];
        dst = r;
        seq = (int32_t)(((uint32_t)seq + 1u) & 0x7fffffffu);       // (wraps to 0 after 2^31 runs instead of overflowing)
        dst.seq = seq;
        ++written;
        return dst;
    }
    LaunchRecord *last() { return written > 0 ? &slot[(written - 1) % kSlots] : nullptr; }
    void clear() { written = 0; }
    // Copies the newest min(written, kSlots, max_rows) records, oldest of them first, as rows of kLaunchRecordFields int32;
    // returns `written`.
    int64_t copy(int32_t *rows, int max_rows) const {
        int64_t n = written < kSlots ? written : kSlots;
        if (n > max_rows) n = max_rows < 0 ? 0 : max_rows;
        for (int64_t i = 0; i < n; ++i) {
            const LaunchRecord &src = slot[(written - n + i) % kSlots];
            std::memcpy(rows + i * kLaunchRecordFields, &src, sizeof(src));
        }
        return written;
    }
};

}  // namespace ultra_detail

#endif

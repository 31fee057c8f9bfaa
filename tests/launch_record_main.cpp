// tests/launch_record_main.cpp -- stand-alone host program over csrc/launch_record.h (tests/test_launch_record_cpu.py builds it
// with the host compiler and -fsanitize=address,undefined; it is never loaded into Python and needs no GPU).
//
// `--fields` prints the field names and the number of int32 in a row; without arguments the program drives a LaunchRing the
// way the launchers do and prints one line per step: `<step> <count> <rows copied> <seq of every copied row ...> | <family of
// every copied row ...>`.  Every check is made by the test from these lines; the program only fails (exit 1) where the ring
// itself would have to be misused to go on.
#include <cstdio>
#include <cstring>

#include "launch_record.h"

using namespace ultra_detail;

static void show(const char *step, const LaunchRing &ring, int max_rows) {
    int32_t rows[(LaunchRing::kSlots + 1) * kLaunchRecordFields];
    for (auto &v : rows) v = -777;
    const long long count = ring.copy(rows, max_rows);
    long long kept = count < LaunchRing::kSlots ? count : LaunchRing::kSlots;
    if (kept > max_rows) kept = max_rows;
    std::printf("%s %lld %lld", step, count, kept);
    for (long long i = 0; i < kept; ++i) std::printf(" %d", rows[i * kLaunchRecordFields + 0]);
    std::printf(" |");
    for (long long i = 0; i < kept; ++i) std::printf(" %d", rows[i * kLaunchRecordFields + 2]);
    // nothing behind the copied rows was touched
    std::printf(" | %d\n", rows[kept * kLaunchRecordFields]);
}

int main(int argc, char **argv) {
    if (argc > 1 && std::strcmp(argv[1], "--fields") == 0) {
        std::printf("%s\n%d\n", kLaunchRecordFieldNames, kLaunchRecordFields);
        return 0;
    }
    static LaunchRing ring;
    show("empty", ring, LaunchRing::kSlots);
    if (ring.last() != nullptr) return 1;
    for (int i = 0; i < 3; ++i) {
        LaunchRecord rec;
        rec.family = 100 + i;
        LaunchRecord &slot = ring.push(rec);
        slot.status = 0;
        if (ring.last() != &slot) return 1;
    }
    show("three", ring, LaunchRing::kSlots);
    ring.last()->fixup = 2;              // launch_fixup amends the newest record
    ring.last()->fixup_sum = 0;
    ring.last()->fixup_grid = 7;
    {
        int32_t rows[LaunchRing::kSlots * kLaunchRecordFields];
        ring.copy(rows, LaunchRing::kSlots);
        std::printf("fixup %d %d %d %d\n", rows[2 * kLaunchRecordFields + kLaunchRecordFields - 3],
                    rows[2 * kLaunchRecordFields + kLaunchRecordFields - 2], rows[2 * kLaunchRecordFields + kLaunchRecordFields - 1],
                    rows[1 * kLaunchRecordFields + kLaunchRecordFields - 3]);
    }
    for (int i = 3; i < 11; ++i) {       // 11 writes in all: the ring wraps
        LaunchRecord rec;
        rec.family = 100 + i;
        ring.push(rec);
    }
    show("wrapped", ring, LaunchRing::kSlots);
    show("two_rows", ring, 2);
    show("no_rows", ring, 0);
    ring.clear();
    show("cleared", ring, LaunchRing::kSlots);
    if (ring.last() != nullptr) return 1;
    LaunchRecord rec;
    rec.family = 200;
    ring.push(rec);
    show("after_clear", ring, LaunchRing::kSlots);
    // a default record: every optional field -1, no fix-up
    const LaunchRecord blank;
    int32_t row[kLaunchRecordFields];
    std::memcpy(row, &blank, sizeof(blank));
    std::printf("blank");
    for (int k = 0; k < kLaunchRecordFields; ++k) std::printf(" %d", row[k]);
    std::printf("\n");
    return 0;
}

// tests/plan_path_main.cpp -- stand-alone host program over csrc/plan_path.h (tests/test_plan_path_cpu.py builds it with the
// host compiler and -fsanitize=address,undefined; it is never loaded into Python and needs no GPU).
//
// stdin : one case per line, the integers of kInputFields in that order, then `forced_conc has_min_rows min_rows`
//         (forced_conc 0 = ULTRA_CONC not set)
// stdout: one line per case, the integers of kOutputFields (print them with `--fields`)
#include <cstdio>
#include <cstring>

#include "plan_path.h"

using namespace ultra_detail;

static const char *kInputFields =
    "kind sum_op mul_op F n_rel gather_rows gather2_rows has_weight has_node_b has_row_ptr has_packed has_packed_dead has_dense "
    "packed_src_shift n_rows n_edges n_long_rows n_pieces n_hot dense_rows dense_cols has_add_rows has_bnode bdim has_act_bits "
    "has_act_node act_words has_workspace workspace_bytes aligned knobs n_cu gfx950 forced_conc has_min_rows min_rows";
static const char *kOutputFields =
    "status family unit_w var x_lds dead act unroll concurrent rel_lds group rel_mode n_rel_lds n_tiles split n_slots "
    "blocks_per_label grid block lds fixup fixup_grid";

int main(int argc, char **argv) {
    if (argc > 1 && std::strcmp(argv[1], "--fields") == 0) {
        std::printf("%s\n%s\n", kInputFields, kOutputFields);
        return 0;
    }
    long long v[36];
    for (;;) {
        for (int i = 0; i < 36; ++i)
            if (std::scanf("%lld", &v[i]) != 1) return i == 0 ? 0 : 1;
        PlanInput in;
        int i = 0;
        in.kind = (int)v[i++]; in.sum_op = (int)v[i++]; in.mul_op = (int)v[i++];
        in.F = v[i++]; in.n_rel = v[i++]; in.gather_rows = v[i++]; in.gather2_rows = v[i++];
        in.has_weight = v[i++] != 0; in.has_node_b = v[i++] != 0; in.has_row_ptr = v[i++] != 0; in.has_packed = v[i++] != 0;
        in.has_packed_dead = v[i++] != 0; in.has_dense = v[i++] != 0;
        in.packed_src_shift = v[i++]; in.n_rows = v[i++]; in.n_edges = v[i++]; in.n_long_rows = v[i++]; in.n_pieces = v[i++];
        in.n_hot = v[i++]; in.dense_rows = v[i++]; in.dense_cols = v[i++];
        in.has_add_rows = v[i++] != 0; in.has_bnode = v[i++] != 0; in.bdim = (int)v[i++];
        in.has_act_bits = v[i++] != 0; in.has_act_node = v[i++] != 0; in.act_words = (int)v[i++];
        in.has_workspace = v[i++] != 0; in.workspace_bytes = (size_t)v[i++];
        in.aligned = (unsigned)v[i++];
        in.knobs = decode_knobs((int)v[i++]);
        in.n_cu = (int)v[i++]; in.gfx950 = v[i++] != 0;
        const int forced_conc = (int)v[i++];
        const bool has_min_rows = v[i++] != 0;
        const long long min_rows = v[i++];
        PlanPath r = plan_path(in);
        if (forced_conc != 0) force_concurrent(r, forced_conc, has_min_rows, min_rows, in.gather_rows);
        std::printf("%d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %zu %d %d\n", r.status, r.family, (int)r.unit_w, r.var,
                    (int)r.x_lds, (int)r.dead, r.act, r.unroll, r.concurrent, (int)r.rel_lds, r.group, r.rel_mode, r.n_rel_lds,
                    r.geo.n_tiles, r.geo.split, r.geo.n_slots, r.geo.blocks_per_label, r.grid, r.block, r.lds, r.fixup, r.fixup_grid);
    }
}

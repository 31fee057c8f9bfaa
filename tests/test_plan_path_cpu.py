"""Which kernel a plan runs: csrc/plan_path.h, the pure decision behind run_plan, pinned branch by branch without a GPU.

tests/plan_path_main.cpp is compiled with the host compiler under -fsanitize=address,undefined (a stand-alone program:
nothing is loaded into Python) and fed the table below.  Every case is the smallest plan that reaches its branch.  The
expected values were worked out by hand from run_plan as it stood BEFORE the decision was split out of it -- launch_rowgroup,
launch_quad_w and the packed / general launchers of that commit, rule by rule -- and not from the output of plan_path().

Numbers used below: a 64-column relation tile is 256 B per relation, kMaxLdsBytes = 159 744 B = 624 such rows, every
launch has a 16-byte LDS header; n_cu = 256 gives 32 workgroups per XCD label (grid 256), n_cu = 248 (after
ultra_rspmm_reserve_cus(8)) gives 31, which no power of two divides: concurrent tiles stay at 1 there.  The `*_cus` rows at the
end hold the geometry at 8, 24 and 240 compute units (the floor, an odd count per label, bench.py's reserved legs), which
tests/test_cu_count_gpu.py runs on the device.
"""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ultra_torchdrug_amd", "csrc")

FWD, DX, DREL = 0, 1, 2
ADD, MIN, MAX = 0, 1, 2
MUL_MUL, MUL_ADD = 0, 1
DENSE, ROWGROUP, QUAD, PACKED, GENERAL = 0, 1, 2, 3, 4
REL_L2, REL_LDS, REL_PART = 0, 1, 2
U, UW, UX = 0, 1, 2
AL_INPUT, AL_GRAD, AL_OUT, AL_RELATION, AL_ADD_ROWS, AL_PARTIAL, AL_BVEC, AL_ALL = 1, 2, 4, 8, 16, 32, 64, 127
BAD_SHAPE = 2
HDR = 16
TABLE = 12 * 256            # the relation tile of the base plan

# a knowledge-graph forward: 5 000 nodes, 12 relations, ids inside the packed word, unit weights, one 64-column tile
BASE = dict(kind=FWD, sum_op=ADD, mul_op=MUL_MUL, F=64, n_rel=12, gather_rows=5000, gather2_rows=0, has_weight=0, has_node_b=0,
            has_row_ptr=0, has_packed=1, has_packed_dead=0, has_dense=0, packed_src_shift=12, n_rows=5000, n_edges=40000,
            n_long_rows=0, n_pieces=0, n_hot=0, dense_rows=0, dense_cols=0, has_add_rows=0, has_bnode=0, bdim=0, has_act_bits=0,
            has_act_node=0, act_words=0, has_workspace=0, workspace_bytes=0, aligned=AL_ALL, knobs=0, n_cu=256, gfx950=1,
            forced_conc=0, has_min_rows=0, min_rows=0)
# d_relation of the same graph: rows are relations, the words hold the source node only, destination nodes in node_b
BY_REL = dict(kind=DREL, n_rows=12, has_node_b=1, packed_src_shift=8, gather2_rows=5000)
# the same graph with node ids outside the packed word: row pointers, no split rows
WIDE = dict(packed_src_shift=32, has_row_ptr=1)
# a relation graph in its dense form: 100 nodes, 4 relation types
DENSE_PLAN = dict(has_dense=1, n_rel=4, n_rows=100, gather_rows=100, dense_rows=100, dense_cols=100, n_edges=8000)
SPLIT = dict(n_long_rows=2, n_pieces=256, has_workspace=1, workspace_bytes=256 * 64 * 4)

GEO1 = dict(n_tiles=1, split=8, n_slots=8, blocks_per_label=32, grid=256)        # one 64-column tile on 256 CUs
QUAD0 = dict(status=0, family=QUAD, var=0, x_lds=0, dead=0, act=0, unit_w=1, unroll=U, concurrent=1, block=1024, lds=HDR + TABLE,
             fixup=0, **GEO1)


def case(name, *overrides, **expect):
    inp = dict(BASE)
    for o in overrides:
        inp.update(o)
    return pytest.param(inp, expect, id=name)


CASES = [
    # ---- dense: taken, and refused for each precondition (the plan then walks its edges: 100 gathered rows fit LDS, var 1)
    case("dense", DENSE_PLAN, status=0, family=DENSE, fixup=0),
    case("dense_d_input", DENSE_PLAN, dict(kind=DX), family=DENSE),
    case("dense_weights", DENSE_PLAN, dict(has_weight=1), family=QUAD, var=1, unit_w=0, unroll=UW, lds=HDR + 1024 + 25600),
    case("dense_sum_min", DENSE_PLAN, dict(sum_op=MIN), family=QUAD, var=1, unroll=UX, lds=HDR + 1024 + 25600),
    case("dense_n_rel_5", DENSE_PLAN, dict(n_rel=5), family=QUAD, var=1, lds=HDR + 1280 + 25600),
    case("dense_F_72", DENSE_PLAN, dict(F=72), family=QUAD, var=1, n_tiles=2, split=4, n_slots=8, lds=HDR + 1024 + 25600),
    case("dense_gfx942", DENSE_PLAN, dict(gfx950=0), family=QUAD, var=1),
    case("dense_knob0", DENSE_PLAN, dict(knobs=1), family=GENERAL, rel_lds=1, lds=HDR + 1024),
    case("dense_knob1", DENSE_PLAN, dict(knobs=2), family=QUAD, var=0, x_lds=0, lds=HDR + 1024),
    case("dense_knob2", DENSE_PLAN, dict(knobs=4), family=PACKED, var=1, lds=HDR + 1024 + 25600),
    case("dense_knob6", DENSE_PLAN, dict(knobs=64), family=QUAD, var=1, x_lds=1, lds=HDR + 1024 + 25600),
    # ---- rowgroup: wide ids + row pointers + no split rows
    case("rowgroup_16", WIDE, status=0, family=ROWGROUP, group=16, rel_mode=REL_LDS, n_rel_lds=12, block=512, lds=HDR + TABLE,
         unit_w=1, fixup=0, **GEO1),
    case("rowgroup_weights", WIDE, dict(has_weight=1), family=ROWGROUP, unit_w=0),
    case("rowgroup_d_input_mul", WIDE, dict(kind=DX), family=ROWGROUP, rel_mode=REL_LDS, lds=HDR + TABLE),
    case("rowgroup_d_input_add", WIDE, dict(kind=DX, mul_op=MUL_ADD), family=ROWGROUP, rel_mode=REL_L2, n_rel_lds=0, lds=HDR),
    case("rowgroup_knob4_F128", WIDE, dict(knobs=16, F=128), family=ROWGROUP, group=32, n_tiles=1, split=8, lds=HDR + 12 * 512),
    case("rowgroup_knob4_F256", WIDE, dict(knobs=16, F=256), family=ROWGROUP, group=64, n_tiles=1, split=8, lds=HDR + 12 * 1024),
    case("rowgroup_knob4_F384", WIDE, dict(knobs=16, F=384), family=ROWGROUP, group=32, n_tiles=3, split=8, n_slots=24),
    case("rowgroup_knob4_F64", WIDE, dict(knobs=16), family=ROWGROUP, group=16),
    case("rowgroup_256MB", WIDE, dict(F=128, gather_rows=524288), family=ROWGROUP, group=16, n_tiles=2, split=4),
    case("rowgroup_above_256MB", WIDE, dict(F=128, gather_rows=524289), family=ROWGROUP, group=32, n_tiles=1, split=8),
    case("rowgroup_above_256MB_F256", WIDE, dict(F=256, gather_rows=262145), family=ROWGROUP, group=64, n_tiles=1),
    case("rowgroup_rel_624", WIDE, dict(n_rel=624), family=ROWGROUP, rel_mode=REL_LDS, n_rel_lds=624, lds=HDR + 159744),
    case("rowgroup_rel_625", WIDE, dict(n_rel=625), family=ROWGROUP, rel_mode=REL_PART, n_rel_lds=624, lds=HDR + 159744),
    case("rowgroup_rel_2496", WIDE, dict(n_rel=2496), family=ROWGROUP, rel_mode=REL_PART, n_rel_lds=624, lds=HDR + 159744),
    case("rowgroup_rel_2497", WIDE, dict(n_rel=2497), family=ROWGROUP, rel_mode=REL_L2, n_rel_lds=0, lds=HDR),
    # rows_per_part * 256 B must stay below 4 GiB - 64 KiB = 16 776 960 rows: 8 parts hold 134 215 672 rows, not 134 215 680
    case("rowgroup_split_8", WIDE, dict(n_rows=134215672), family=ROWGROUP, split=8, n_slots=8),
    case("rowgroup_split_16", WIDE, dict(n_rows=134215680), family=ROWGROUP, split=16, n_slots=16, grid=256),
    case("rowgroup_F_2_30", WIDE, dict(F=1 << 30), status=BAD_SHAPE),
    case("rowgroup_248_cus", WIDE, dict(n_cu=248), family=ROWGROUP, blocks_per_label=31, grid=248),
    # ... refused: the chunked kernels over wide ids (var 3: relation tile in LDS)
    case("rowgroup_knob3", WIDE, dict(knobs=8), family=PACKED, var=3, block=1024, lds=HDR + TABLE),
    case("rowgroup_split_rows", WIDE, SPLIT, family=PACKED, var=3, fixup=2),
    case("rowgroup_no_row_ptr", WIDE, dict(has_row_ptr=0), family=PACKED, var=3),
    case("rowgroup_relation_unaligned", WIDE, dict(aligned=AL_ALL - AL_RELATION), family=PACKED, var=3),
    case("rowgroup_d_input_min", WIDE, dict(kind=DX, sum_op=MIN), family=GENERAL, rel_lds=1, lds=HDR + TABLE),
    # ---- quad
    case("quad_var0", **QUAD0),
    case("quad_var1", dict(gather_rows=100), family=QUAD, var=1, x_lds=1, unroll=UX, lds=HDR + TABLE + 25600),
    case("quad_var1_weights", dict(gather_rows=100, has_weight=1), family=QUAD, var=1, unit_w=0, unroll=UW),
    case("quad_var1_knob1", dict(gather_rows=100, knobs=2), family=QUAD, var=0, x_lds=0, unroll=U, lds=HDR + TABLE),
    case("quad_weights", dict(has_weight=1), family=QUAD, var=0, unit_w=0, unroll=UW, dead=0),
    case("quad_conc1_two_tiles", dict(F=128), family=QUAD, n_tiles=2, split=4, n_slots=8, concurrent=1),
    case("quad_conc2", dict(F=1024), family=QUAD, n_tiles=16, split=1, n_slots=16, concurrent=2, grid=256, lds=HDR + TABLE),
    case("quad_conc4", dict(F=2048), family=QUAD, n_tiles=32, split=1, n_slots=32, concurrent=4),
    case("quad_conc8", dict(F=4096), family=QUAD, n_tiles=64, n_slots=64, concurrent=8),
    case("quad_conc8_is_the_most", dict(F=8192), family=QUAD, n_tiles=128, concurrent=8),
    case("quad_conc_248_cus", dict(F=4096, n_cu=248), family=QUAD, blocks_per_label=31, grid=248, concurrent=1),
    case("quad_conc_knob5", dict(F=4096, knobs=32), family=QUAD, concurrent=1),
    case("quad_conc_forced", dict(forced_conc=2), family=QUAD, concurrent=2),
    case("quad_conc_forced_not_a_divisor", dict(forced_conc=3, F=4096), family=QUAD, concurrent=8),
    case("quad_conc_forced_min_rows_met", dict(forced_conc=2, has_min_rows=1, min_rows=4096), family=QUAD, concurrent=2),
    case("quad_conc_forced_min_rows_unmet", dict(forced_conc=2, has_min_rows=1, min_rows=4096, gather_rows=100), family=QUAD,
         var=1, concurrent=1),
    case("quad_dead_words", dict(has_weight=1, has_packed_dead=1), family=QUAD, dead=1, unit_w=1, unroll=U, lds=HDR + TABLE),
    case("quad_dead_words_knob7", dict(has_weight=1, has_packed_dead=1, knobs=128), family=QUAD, dead=0, unit_w=0, unroll=UW),
    case("quad_dead_words_sum_max", dict(has_weight=1, has_packed_dead=1, sum_op=MAX), family=QUAD, dead=0, unit_w=0),
    case("quad_dead_words_x_lds", dict(has_weight=1, has_packed_dead=1, gather_rows=100), family=QUAD, var=1, dead=0, unit_w=0),
    case("quad_d_input", dict(kind=DX), **QUAD0),
    case("quad_d_input_add", dict(kind=DX, mul_op=MUL_ADD), family=QUAD, var=0, lds=HDR),
    case("quad_d_relation", BY_REL, family=QUAD, var=0, act=0, lds=HDR, **GEO1),
    case("quad_d_relation_x_lds", BY_REL, dict(gather_rows=100), family=QUAD, var=1, x_lds=1, unroll=UX, lds=HDR + 25600),
    case("quad_d_relation_bitmap", BY_REL, dict(has_act_bits=1, act_words=157), family=QUAD, act=2, lds=HDR + 628),
    case("quad_d_relation_bitmap_weights", BY_REL, dict(has_act_bits=1, act_words=157, has_weight=1), family=QUAD, act=2, unroll=UW),
    case("quad_d_relation_bitmap_dead", BY_REL, dict(has_act_bits=1, act_words=157, has_weight=1, has_packed_dead=1), family=QUAD,
         act=2, dead=1, unit_w=1, unroll=U),
    case("quad_d_relation_node", BY_REL, dict(has_act_node=1), family=QUAD, act=3, lds=HDR),
    case("quad_d_relation_node_dead", BY_REL, dict(has_act_node=1, has_weight=1, has_packed_dead=1), family=QUAD, act=3, dead=0,
         unit_w=0, unroll=UW),
    case("quad_d_relation_bitmap_and_node", BY_REL, dict(has_act_bits=1, act_words=157, has_act_node=1), family=QUAD, act=2),
    # 39 936 words = 159 744 B is the most that fits (d_relation keeps no relation tile); one more falls back to the node
    case("quad_d_relation_bitmap_fits", BY_REL, dict(has_act_bits=1, act_words=39936, has_act_node=1), family=QUAD, act=2,
         lds=HDR + 159744),
    case("quad_d_relation_bitmap_too_big", BY_REL, dict(has_act_bits=1, act_words=39937, has_act_node=1), family=QUAD, act=3, lds=HDR),
    case("quad_d_relation_bitmap_too_big_no_node", BY_REL, dict(has_act_bits=1, act_words=39937), family=QUAD, act=0, lds=HDR),
    case("quad_d_relation_bitmap_x_lds", BY_REL, dict(has_act_bits=1, act_words=4, gather_rows=100), family=QUAD, var=1, act=0),
    case("quad_d_relation_bitmap_F_96", BY_REL, dict(has_act_bits=1, act_words=157, F=96), family=QUAD, act=0),
    case("quad_d_relation_add", BY_REL, dict(mul_op=MUL_ADD, gather_rows=100), family=QUAD, var=0, x_lds=0, act=0, lds=HDR),
    case("quad_d_relation_add_bitmap", BY_REL, dict(mul_op=MUL_ADD, has_act_bits=1, act_words=157), family=QUAD, act=2, lds=HDR + 628),
    case("quad_d_relation_add_node", BY_REL, dict(mul_op=MUL_ADD, has_act_node=1), family=QUAD, act=0, lds=HDR),
    # ---- packed: one chunk per wave
    case("packed_F_66", dict(F=66), status=0, family=PACKED, var=0, n_tiles=2, split=4, block=1024, grid=256, lds=HDR + TABLE),
    case("packed_input_unaligned", dict(aligned=AL_ALL - AL_INPUT), family=PACKED, var=0),
    case("packed_grad_unaligned", dict(kind=DX, aligned=AL_ALL - AL_GRAD), family=PACKED, var=0),
    case("packed_d_input_input_unaligned", dict(kind=DX, aligned=AL_ALL - AL_INPUT), family=QUAD),
    case("packed_out_unaligned", dict(aligned=AL_ALL - AL_OUT), family=PACKED),
    case("packed_add_rows_unaligned", dict(has_add_rows=1, aligned=AL_ALL - AL_ADD_ROWS), family=PACKED),
    case("packed_partial_unaligned", dict(aligned=AL_ALL - AL_PARTIAL), family=PACKED),
    case("packed_bvec_unaligned", dict(has_bnode=1, bdim=64, aligned=AL_ALL - AL_BVEC), family=PACKED),
    case("quad_relation_unaligned", dict(aligned=AL_ALL - AL_RELATION), family=QUAD),
    case("packed_bdim_6", dict(F=132, has_bnode=1, bdim=6), family=PACKED),
    case("packed_knob2", dict(knobs=4), family=PACKED, var=0, lds=HDR + TABLE),
    case("packed_knob2_x_lds", dict(knobs=4, gather_rows=100), family=PACKED, var=1, lds=HDR + TABLE + 25600),
    case("packed_d_relation", BY_REL, dict(knobs=4, gather_rows=100), family=PACKED, var=0, lds=HDR),
    case("packed_var3", dict(packed_src_shift=32), family=PACKED, var=3, lds=HDR + TABLE),
    case("packed_var2", dict(packed_src_shift=32, n_rel=700), family=PACKED, var=2, lds=HDR),
    case("packed_var3_d_input_add", dict(packed_src_shift=32, n_rel=700, kind=DX, mul_op=MUL_ADD), family=PACKED, var=3, lds=HDR),
    case("packed_var4", dict(n_hot=100), family=PACKED, var=4, lds=HDR + TABLE + 25600),
    case("packed_var4_fits", dict(n_hot=612), status=0, family=PACKED, var=4, lds=HDR + 159744),
    case("packed_var4_too_large", dict(n_hot=613), status=BAD_SHAPE),
    # ---- general
    case("general_knob0", dict(knobs=1), status=0, family=GENERAL, rel_lds=1, unit_w=1, block=1024, lds=HDR + TABLE, **GEO1),
    case("general_no_packed", dict(has_packed=0), family=GENERAL, rel_lds=1),
    case("general_table_beyond_lds", dict(n_rel=625), family=GENERAL, rel_lds=0, lds=HDR),
    case("general_d_input_min", dict(kind=DX, sum_op=MIN), family=GENERAL, rel_lds=1, lds=HDR + TABLE),
    case("general_d_input_max_add", dict(kind=DX, sum_op=MAX, mul_op=MUL_ADD), family=GENERAL, rel_lds=1),
    case("general_d_input_add_add", dict(kind=DX, mul_op=MUL_ADD, knobs=1), family=GENERAL, rel_lds=0, lds=HDR),
    case("general_d_relation_max", BY_REL, dict(sum_op=MAX), family=GENERAL, rel_lds=0, lds=HDR),
    case("general_d_relation_no_node_b", BY_REL, dict(has_node_b=0), family=GENERAL, rel_lds=0, lds=HDR),
    case("general_d_relation_wide", BY_REL, dict(packed_src_shift=32), family=GENERAL, lds=HDR),
    # ---- fix-up pass over the split rows
    case("fixup_none", fixup=0, fixup_grid=0),
    case("fixup_many_at_128_per_row", SPLIT, family=QUAD, fixup=2, fixup_grid=1),
    case("fixup_plain_below_128_per_row", SPLIT, dict(n_pieces=255), family=QUAD, fixup=1, fixup_grid=1),
    case("fixup_min_has_no_many_form", SPLIT, dict(sum_op=MIN), family=QUAD, fixup=1),
    case("fixup_d_input_min_adds", SPLIT, dict(kind=DX, sum_op=MIN), family=GENERAL, fixup=2),
    case("fixup_grid", SPLIT, dict(F=1024, n_long_rows=3, n_pieces=30), fixup=1, fixup_grid=12),
    case("fixup_general", SPLIT, dict(knobs=1), family=GENERAL, fixup=2),
]


# ---- the compute-unit count: the minimum (8), an odd number of workgroups per label (24) and what bench.py leaves its
# multi-GPU legs (240 = 256 - 16).  blocks_per_label = ceil(n_cu / 8) = 1, 3, 30; grid = 8 * that.  `concurrent`, by hand from
# the loop "c -> 2c while 2c <= slots_per_label and bpl % 2c == 0 and bpl / 2c >= 4" (slots_per_label = ceil(n_slots / 8)):
#   bpl = 1:  1 % 2 != 0                                                   -> 1 at every F
#   bpl = 3:  3 % 2 != 0                                                   -> 1 at every F
#   bpl = 30: F = 64:   1 tile x split 8 = 8 slots, 1 per label: 2 > 1     -> 1
#             F = 1024: 16 tiles x split 1, 2 per label: 2 <= 2, 30 % 2 == 0, 15 >= 4 -> 2; then 4 > 2 -> 2
#             F = 4096: 64 tiles, 8 per label: 2 as above; then 30 % 4 = 2 -> 2
CU_GEO = {8: (1, 8), 24: (3, 24), 240: (30, 240)}
QUAD_TILES = {64: (1, 8, 8), 1024: (16, 1, 16), 4096: (64, 1, 64)}          # F -> n_tiles, split, n_slots
QUAD_CONC = {(8, 64): 1, (8, 1024): 1, (8, 4096): 1, (24, 64): 1, (24, 1024): 1, (24, 4096): 1,
             (240, 64): 1, (240, 1024): 2, (240, 4096): 2}
for _n_cu, (_bpl, _grid) in CU_GEO.items():
    _geo = dict(blocks_per_label=_bpl, grid=_grid)
    for _F, (_tiles, _split, _slots) in QUAD_TILES.items():
        CASES.append(case("quad_F%d_%d_cus" % (_F, _n_cu), dict(F=_F, n_cu=_n_cu), status=0, family=QUAD, n_tiles=_tiles,
                          split=_split, n_slots=_slots, concurrent=QUAD_CONC[_n_cu, _F], **_geo))
    CASES.append(case("rowgroup_%d_cus" % _n_cu, WIDE, dict(n_cu=_n_cu), status=0, family=ROWGROUP, group=16, n_tiles=1, split=8,
                      n_slots=8, **_geo))
    CASES.append(case("packed_F66_%d_cus" % _n_cu, dict(F=66, n_cu=_n_cu), status=0, family=PACKED, n_tiles=2, split=4, n_slots=8,
                      **_geo))
    CASES.append(case("general_%d_cus" % _n_cu, dict(knobs=1, n_cu=_n_cu), status=0, family=GENERAL, n_tiles=1, split=8, n_slots=8,
                      **_geo))


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++") or shutil.which("clang++")
    assert cxx is not None, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("plan_path") / "plan_path_main")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", CSRC, "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "plan_path_main.cpp"), "-o", exe])
    fields = subprocess.run([exe, "--fields"], check=True, capture_output=True, text=True).stdout.splitlines()

    def decide(inputs):
        lines = "".join(" ".join(str(int(inp[f])) for f in fields[0].split()) + "\n" for inp in inputs)
        done = subprocess.run([exe], input=lines, check=True, capture_output=True, text=True)
        assert done.stderr == ""
        rows = [dict(zip(fields[1].split(), map(int, line.split()))) for line in done.stdout.splitlines()]
        assert len(rows) == len(inputs)
        return rows

    return decide


def test_input_fields_are_the_programs(program):
    """BASE names exactly the integers the program reads (a field added on one side only would shift every case)."""
    assert program([BASE])[0]["status"] == 0


@pytest.mark.parametrize("inp,expect", CASES)
def test_plan_path(program, inp, expect):
    got = program([inp])[0]
    assert {k: got[k] for k in expect} == expect, got


def test_header_is_plain_cxx():
    """The decision includes nothing from HIP and reads neither globals nor the environment."""
    text = open(os.path.join(CSRC, "plan_path.h")).read()
    for word in ("hip/", "getenv(", "malloc(", "new ", "std::vector", "std::string", "g_knobs"):
        assert word not in text, word

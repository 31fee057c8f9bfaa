"""What ``tests/test_address_width_gpu.py`` relies on, held without a GPU: the boundary-row chooser on hand-computed cases, the
kernel family (and rowgroup split) every case's shape gets from csrc/plan_path.h -- through the stand-alone program of
``tests/plan_path_main.cpp``, as ``tests/test_plan_path_cpu.py`` does --, the exactness of every case's subgraph on the worst
grid fill, every case's stated memory need, and the host guard constants DESIGN.md "Address width" quotes, each read out of
plan_path.h by probing the program on both sides of it.
"""
import numpy as np
import pytest

import address_width as AW

QUAD, PACKED, GENERAL, ROWGROUP, DENSE = AW.FAM_QUAD, AW.FAM_PACKED, AW.FAM_GENERAL, AW.FAM_ROWGROUP, AW.FAM_DENSE


@pytest.fixture(scope="module")
def decide(tmp_path_factory):
    return AW.build_plan_program(tmp_path_factory.mktemp("address_width"))


# ------------------------------------------------------------------------------------------------ boundary_rows
def test_boundary_rows_of_a_small_operand_are_its_ends():
    assert AW.boundary_rows(100, 4096).tolist() == [0, 1, 2, 3, 96, 97, 98, 99]
    assert AW.boundary_rows(5, 4096).tolist() == [0, 1, 2, 3, 4]
    assert AW.boundary_rows(100, 4096, k=2).tolist() == [0, 1, 98, 99]


def test_boundary_rows_past_4_gib_by_hand():
    """1 048 640 rows of 4096 B: 2^31 is the first byte of row 524 288, 0xffff0000 of row 1 048 560, 2^32 of row 1 048 576."""
    want = ([0, 1, 2, 3] + list(range(524284, 524292)) + list(range(1048556, 1048564)) + list(range(1048572, 1048580))
            + [1048636, 1048637, 1048638, 1048639])
    assert AW.boundary_rows(AW.PAST_4GIB, 4096).tolist() == want
    # the rows AFTER 2^32 are what a wrapped 32-bit offset sends to the start of the tensor
    assert {1048576, 1048577, 1048578, 1048579} <= set(AW.boundary_rows(AW.PAST_4GIB, 4096).tolist())


def test_boundary_rows_reach_a_limit_only_where_the_operand_does():
    last = AW.boundary_rows(AW.LAST_ADMITTED, 4096).tolist()                 # 0xfffef000 bytes: past 2^31 only
    assert last == [0, 1, 2, 3] + list(range(524284, 524292)) + list(range(1048555, 1048559))
    refused = AW.boundary_rows(AW.FIRST_REFUSED, 4096).tolist()              # exactly 0xffff0000 bytes: the rows below it
    assert refused == [0, 1, 2, 3] + list(range(524284, 524292)) + list(range(1048556, 1048560))


def test_boundary_rows_of_the_epilogues_by_hand():
    """Rows of 256 B: 2^31 is row 8 388 608, 0xffff0000 row 16 776 960, 2^32 row 16 777 216."""
    rows = AW.boundary_rows(1 << 24, 256).tolist()
    assert rows == [0, 1, 2, 3] + list(range(8388604, 8388612)) + list(range(16776956, 16776964)) + list(range(16777212, 16777216))
    rows = AW.boundary_rows((1 << 24) - 1, 256).tolist()
    assert rows[-4:] == [16777211, 16777212, 16777213, 16777214] and 16776960 in rows


def test_boundary_rows_on_both_sides_of_every_cut():
    rows = AW.boundary_rows(1000, 4096, k=2, cuts=[250, 500]).tolist()
    assert rows == [0, 1, 248, 249, 250, 251, 498, 499, 500, 501, 998, 999]
    assert AW.part_cuts(2097119, 2) == [1048560] and AW.part_cuts(10, 4) == [3, 6, 9] and AW.part_cuts(10, 1) == []


def test_banded_graph_touches_the_large_side_at_boundary_rows_only():
    for case in AW.FORWARD_CASES + AW.BACKWARD_CASES:
        g = AW.case_graph(case)
        big = g["dst"] if case["large"] == "dst" else g["src"]
        small = g["src"] if case["large"] == "dst" else g["dst"]
        assert set(big.tolist()) == set(g["live"].tolist()) and set(g["live"].tolist()) < set(g["rows"].tolist())
        assert 5 <= len(g["empty"]) <= 12 and not set(g["empty"].tolist()) & set(big.tolist())
        assert small.max() < AW.N_SMALL and g["rel"].max() < AW.N_REL <= 16 and 100 <= len(g["dst"]) <= 1000
        key = (g["dst"] * g["n_src"] + g["src"]) * g["n_rel"] + g["rel"]
        assert len(np.unique(key)) == len(key) and (np.diff(key) > 0).all()      # distinct, in forward-plan order
        if case.get("hub", True):
            assert np.bincount(g["dst"]).max() > AW.PIECE_LEN                     # one destination row is split


# ------------------------------------------------------------------------------------------------ families
@pytest.mark.parametrize("case", AW.FORWARD_CASES + AW.BACKWARD_CASES, ids=lambda c: c["name"])
def test_every_case_gets_the_family_the_gpu_test_asserts(case, decide):
    graph = AW.case_graph(case)
    for s, m in case.get("ops", [("add", "mul")]):
        got = decide([AW.case_plan_input(case, graph, s, m)])[0]
        assert got["status"] == 0 and got["family"] == case["family"], got


def test_case_tables_hold_what_the_limits_need():
    names = {c["name"]: c for c in AW.FORWARD_CASES + AW.BACKWARD_CASES}
    for operand in ("out", "input"):
        assert {names["%s_%s%s" % (operand, tag, "" if operand == "out" else "_unit")]["n"]
                for tag in ("last_admitted", "first_refused", "past_4gib")} == {AW.LAST_ADMITTED, AW.FIRST_REFUSED, AW.PAST_4GIB}
    assert AW.LAST_ADMITTED * 4096 < 0xffff0000 == AW.FIRST_REFUSED * 4096 and AW.PAST_4GIB * 4096 > 1 << 32
    assert names["out_last_admitted"]["family"] == QUAD and names["out_first_refused"]["family"] == PACKED
    assert names["input_first_refused_unit"]["family"] == GENERAL and names["input_last_admitted_knob4"]["family"] == PACKED
    assert names["input_past_4gib_wide_ids"]["family"] == ROWGROUP


def test_rowgroup_split_sizes_come_from_rowgroup_tiling(decide):
    """F = 1024, 128 gathered rows: 16 column tiles of 64, split 1.  A part stays below 2^32 - 65536 bytes = 1 048 560 rows, so
    the split doubles at 1 048 560 rows and again at 2 * 1 048 560 - 1 (ceil(n / 2) reaches 1 048 560)."""
    sizes = AW.rowgroup_split_sizes(decide)
    assert sizes == [(1048559, 1, 1048560, 2), (2097118, 2, 2097119, 4)]
    for last, split, first, doubled in sizes:
        for n, want in ((last, split), (first, doubled)):
            got = decide([AW.plan_input(AW.FWD, n, AW.N_SMALL, wide_ids=True)])[0]
            assert (got["family"], got["split"], got["n_tiles"], got["group"]) == (ROWGROUP, want, 16, 16)
            per = (n + want - 1) // want
            assert per * 4096 < (1 << 32) - 65536


# ------------------------------------------------------------------------------------------------ exactness, memory
@pytest.mark.parametrize("case", AW.FORWARD_CASES + AW.BACKWARD_CASES, ids=lambda c: c["name"])
def test_every_subgraph_is_exact_on_the_worst_grid_fill(case):
    graph = AW.case_graph(case)
    for message in {m for _, m in case.get("ops", [("add", "mul")])}:
        AW.worst_case_is_exact(graph, message)


def test_rowgroup_subgraphs_are_exact(decide):
    for last, split, first, doubled in AW.rowgroup_split_sizes(decide):
        for n, s in ((last, split), (first, doubled)):
            case = dict(name="rowgroup", kind=AW.FWD, large="dst", n=n, hub=False, weighted=True)
            AW.worst_case_is_exact(AW.case_graph(case, cuts=AW.part_cuts(n, s)))
            assert AW.case_bytes(case) < AW.CAP_BYTES


def test_every_stated_memory_need_is_below_the_cap():
    for case in AW.FORWARD_CASES + AW.BACKWARD_CASES:
        assert AW.case_bytes(case) >= case["n"] * 4096 and AW.case_bytes(case) < AW.CAP_BYTES, case["name"]
    for rows in AW.EPILOGUE_ROWS:
        assert AW.epilogue_bytes(rows, backward=True) < AW.CAP_BYTES
    assert AW.CAP_BYTES == 48 << 30 and AW.EPILOGUE_ROWS == (16777152, 16777153, 16777215, 16777216)


# ------------------------------------------------------------------------------------------------ the guards, read by probing
def _threshold(decide, make, lo, hi, key="family"):
    """The first value in (lo, hi] at which ``decide(make(value))[key]`` differs from what it is at ``lo``."""
    base = decide([make(lo)])[0][key]
    assert decide([make(hi)])[0][key] != base
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if decide([make(mid)])[0][key] == base else (lo, mid)
    return hi


def test_descriptor_guards_are_the_ones_design_md_quotes(decide):
    big = 1 << 34
    # out_ok: n_rows * F * 4 < 0xffff0000 (quad -> packed)
    assert _threshold(decide, lambda n: AW.plan_input(AW.FWD, n, AW.N_SMALL), 1, big) * 4096 == 0xffff0000
    # gather_bytes < 0xffff0000 (quad -> general), forward and d_input, and both gathers of d_relation
    assert _threshold(decide, lambda n: dict(AW.plan_input(AW.FWD, AW.N_SMALL, n), packed_src_shift=12, has_row_ptr=0), 1, big) \
        * 4096 == 0xffff0000
    assert _threshold(decide, lambda n: dict(AW.plan_input(AW.DX, n, AW.N_SMALL), packed_src_shift=12, has_row_ptr=0), 1, big) \
        * 4096 == 0xffff0000
    assert _threshold(decide, lambda n: AW.plan_input(AW.DREL, AW.N_SMALL, n), 1, big) * 4096 == 0xffff0000
    assert _threshold(decide, lambda n: AW.plan_input(AW.DREL, n, AW.N_SMALL), 1, big) * 4096 == 0xffff0000
    # d_relation's second gather multiplies a node id with __umul24: gather2_rows < 2^24 (F = 4: 16-byte rows, 256 MiB)
    assert _threshold(decide, lambda n: AW.plan_input(AW.DREL, n, AW.N_SMALL, F=4), 1, 1 << 27) == 1 << 24
    # row bytes are a __umul24 operand of quad_kernel: F * 4 < 2^24
    assert _threshold(decide, lambda f: AW.plan_input(AW.FWD, 8, 8, F=4 * f), 1, 1 << 24) * 16 == 1 << 24
    # meta_ok: (n_edges + 16) * 4 < 0xffff0000
    assert (_threshold(decide, lambda e: AW.plan_input(AW.FWD, AW.N_SMALL, AW.N_SMALL, n_edges=e), 1, big) + 16) * 4 == 0xffff0000
    # a rowgroup part: rows_per_part * F * 4 < 2^32 - 65536
    first = _threshold(decide, lambda n: AW.plan_input(AW.FWD, n, AW.N_SMALL, wide_ids=True), 1, big, key="split")
    assert first * 4096 == (1 << 32) - 65536
    # the dense relation-graph form: gather_rows * F * 4 < 2^31 and F * 4 < 2^24
    dense = lambda n, f: dict(AW.plan_input(AW.FWD, n, n, n_rel=4, F=f), has_dense=1, dense_rows=n, dense_cols=n)
    assert decide([dense(100, 64)])[0]["family"] == DENSE
    assert _threshold(decide, lambda n: dense(n, 1024), 100, big) * 4096 == 1 << 31
    assert _threshold(decide, lambda f: dense(16, 16 * f), 1, 1 << 24) * 64 == 1 << 24


def test_the_python_guards_agree_with_the_library():
    """functional.py sends the epilogue's backward to the three-kernel form where the one-pass entry refuses
    (csrc/combine_fused_bwd.inc: rows > 2^24 - 64), and first_layer_train_forward declines at the same size."""
    from ultra_torchdrug_amd import functional as UF
    assert UF.FUSED_BACKWARD_MAX_ROWS == (1 << 24) - 64 == AW.EPILOGUE_ROWS[0]
    assert (UF.FUSED_BACKWARD_MAX_ROWS + 64) * 256 == 1 << 32


# ------------------------------------------------------------------------------------------------ the other families' cases
@pytest.mark.parametrize("case", AW.OPERATOR_CASES, ids=lambda c: c["name"])
def test_operator_cases_are_exact_and_fit(case):
    """Weight gradients and rotate messages (pairs of 32 columns) on the worst grid fill; three large tensors at the most."""
    graph = AW.case_graph(case)
    AW.worst_case_is_exact(graph, "mul")
    AW.worst_case_is_exact(graph, "rotate", block=8)
    assert np.bincount(graph["dst"]).max() > AW.PIECE_LEN
    assert AW.case_bytes(dict(case, operator=True)) < AW.CAP_BYTES


@pytest.mark.parametrize("case", AW.GATHER2_CASES, ids=lambda c: c["name"])
def test_gather2_cases_sit_on_both_sides_of_2_24_rows(case, decide):
    graph = AW.case_graph(case)
    assert graph["n_dst"] in ((1 << 24) - 1, 1 << 24) and case["n"] * 16 < 1 << 31 and graph["n_dst"] - 1 in graph["rows"]
    got = decide([AW.case_plan_input(case, graph)])[0]
    assert got["status"] == 0 and got["family"] == case["family"], got
    AW.worst_case_is_exact(graph)
    assert AW.case_bytes(case) < AW.CAP_BYTES


def test_set_boundary_shape_is_past_4_gib():
    n, q, d = AW.SET_BOUNDARY_SHAPE
    assert n * q * d * 4 > 1 << 32 and 2 * n * q * d * 4 + AW.GIB < AW.CAP_BYTES
    assert AW.boundary_rows(n, q * d * 4).tolist() == AW.boundary_rows(AW.PAST_4GIB, 4096).tolist()


def test_pna_and_head_shapes():
    case = AW.PNA_CASE
    plane = case["n"] * 4096
    assert (1 << 31) < plane and 2 * plane > 1 << 32 and 3 * plane > 6 << 30 and 6 * plane + AW.GIB < AW.CAP_BYTES
    graph = AW.case_graph(case)
    AW.worst_case_is_exact(graph, "mul")
    assert (1 << 31) // 4096 in graph["rows"]
    n, b = AW.SCORE_SHAPE
    assert n * b * 256 > 1 << 32 and n * b * 4 < 0xfffffff0 and 2 * n * b * 256 < AW.CAP_BYTES
    n, q = AW.PNA_COMBINE_SHAPE
    assert n * q > 1 << 24 and 8 * n * q * 256 < AW.CAP_BYTES

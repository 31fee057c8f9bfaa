"""The launch record's ring (csrc/launch_record.h) without a GPU: tests/launch_record_main.cpp is compiled with the host compiler
under -fsanitize=address,undefined (a stand-alone program: nothing is loaded into Python) and drives a ring the way the
launchers do -- push at a leaf, amend the newest record for the fix-up pass, copy out, clear."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ultra_torchdrug_amd", "csrc")

FIELDS = ("seq status family kind sum mul unit_w var x_lds unroll act dead rel_lds rel_mode group needs_rel backward concurrent "
          "grid block lds n_tiles split n_slots blocks_per_label n_rel_lds fixup fixup_sum fixup_grid").split()


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++") or shutil.which("clang++")
    assert cxx is not None, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("launch_record") / "launch_record_main")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", CSRC, os.path.join(ROOT, "tests", "launch_record_main.cpp"), "-o", exe])
    return exe


@pytest.fixture(scope="module")
def steps(program):
    done = subprocess.run([program], check=True, capture_output=True, text=True)
    assert done.stderr == ""
    out = {}
    for line in done.stdout.splitlines():
        name, rest = line.split(" ", 1)
        out[name] = [[int(v) for v in part.split()] for part in rest.split("|")]
    return out


def test_field_names_cover_the_row(program):
    """One name per int32 of a row, no name twice, and the names a binding relies on are there."""
    names, count = subprocess.run([program, "--fields"], check=True, capture_output=True, text=True).stdout.splitlines()
    assert names.split() == FIELDS and int(count) == len(FIELDS) == len(set(FIELDS))
    assert "  " not in names and names == names.strip()


def test_ring_starts_empty(steps):
    assert steps["empty"] == [[0, 0], [], [-777]]


def test_seq_is_monotone_and_records_come_out_oldest_first(steps):
    (count, kept, *seqs), families, behind = steps["three"]
    assert (count, kept) == (3, 3) and seqs == [1, 2, 3] and families == [100, 101, 102] and behind == [-777]


def test_fixup_amends_the_newest_record_only(steps):
    assert steps["fixup"] == [[2, 0, 7, 0]]


def test_ring_wraps_and_keeps_the_newest_eight(steps):
    (count, kept, *seqs), families, behind = steps["wrapped"]
    assert count == 11 and count > 8, "the count is not capped: an overflow is visible"
    assert kept == 8 and seqs == list(range(4, 12)) and families == list(range(103, 111)) and behind == [-777]


def test_copy_honours_the_callers_row_limit(steps):
    (count, kept, *seqs), families, behind = steps["two_rows"]
    assert (count, kept) == (11, 2) and seqs == [10, 11] and families == [109, 110] and behind == [-777]
    assert steps["no_rows"] == [[11, 0], [], [-777]]


def test_clear_resets_the_count_but_not_seq(steps):
    assert steps["cleared"] == [[0, 0], [], [-777]]
    (count, kept, *seqs), families, _ = steps["after_clear"]
    assert (count, kept) == (1, 1) and families == [200]
    assert seqs == [12], "seq goes on counting, so a record from before the clear can never pass for a new one"


def test_blank_record_marks_absent_fields(steps):
    row = dict(zip(FIELDS, steps["blank"][0]))
    assert row["seq"] == 0 and row["status"] == 0 and row["fixup"] == 0
    assert all(v == -1 for k, v in row.items() if k not in ("seq", "status", "fixup"))


def test_header_is_plain_cxx():
    text = open(os.path.join(CSRC, "launch_record.h")).read()
    for word in ("hip/", "getenv(", "malloc(", "new ", "std::vector", "std::string", "mutex", "atomic", "thread"):
        assert word not in text.replace("per-thread", "").replace("one thread", "").replace("of the thread", ""), word

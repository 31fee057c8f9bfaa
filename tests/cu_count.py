"""The compute-unit count the library sizes its grids for, as a test axis.

``ultra_rspmm_reserve_cus(n)`` makes every later launch size its grid for ``max(8, total - n)`` compute units (csrc/runtime.hip).
``compute_units(n)`` runs a block at exactly ``n``; ``expected_geometry`` restates, from csrc/plan_path.h as written, what a
plan launch records at ``n``: ``tile_geometry`` (line 79) and the ``concurrent`` loop of ``plan_path`` (line 320).

The setting is one integer of the process, shared by the ctypes and the dispatcher binding (both call the same library), and
size queries (``ultra_combine_backward_waves``, ``ultra_score_backward_workspace`` ...) read it as the launches do: a caller
changes it between calls, never between a size query and its launch.  Tests therefore assert from the launch record that the
geometry they asked for is the one that ran.
"""
import contextlib
import math

XCD = 8                         # kXcd: labels of the persistent grids, and the floor of the compute-unit count
CU_COUNTS = (8, 24, 240)        # the minimum; three workgroups per label (odd: no team split); what bench.py reserves down to


def total_compute_units(device=0):
    from ultra_torchdrug_amd import _lib
    return _lib.device_info(device)["n_cu"]


@contextlib.contextmanager
def compute_units(n, device=0):
    """Every launch inside sizes its grid for exactly ``n`` compute units; the default is restored on the way out."""
    from ultra_torchdrug_amd import _lib
    lib = _lib.load()
    total = total_compute_units(device)
    assert n >= XCD and total >= n, "the device has %d compute units, the case needs %d" % (total, n)
    try:
        assert lib.ultra_rspmm_reserve_cus(total - n) == 0
        yield n
    finally:
        assert lib.ultra_rspmm_reserve_cus(0) == 0


def expected_geometry(n_cu, F, width=64, family_is_quad=False, knob=0, columns=None):
    """``n_tiles``, ``split``, ``n_slots``, ``blocks_per_label``, ``grid`` of a plan launch over ``columns`` (default ``F``) columns
    in tiles of ``width`` on ``n_cu`` compute units, and for quad_kernel its ``concurrent`` tiles (knob bit 5 switches them off).
    (rowgroup_tiling's doubling of ``split`` beyond 4 GiB per part is not restated: no test here has such a plan.)"""
    columns = F if columns is None else columns
    n_tiles = -(-columns // width)
    split = XCD // math.gcd(n_tiles, XCD)
    n_slots = n_tiles * split
    bpl = -(-n_cu // XCD)
    geo = dict(n_tiles=n_tiles, split=split, n_slots=n_slots, blocks_per_label=bpl, grid=bpl * XCD)
    if family_is_quad:
        per_label = -(-n_slots // XCD)
        conc = 1
        while not (knob & 32) and 2 * conc <= per_label and bpl % (2 * conc) == 0 and bpl // (2 * conc) >= 4:
            conc *= 2
        geo["concurrent"] = conc
    return geo

"""The edge-weight gradient of rotate messages without a GPU: ``ultra_rspmm_rotate_backward_weight_f32`` is in the binding's
signature table and exported by the built library, and its argument checks return the documented codes before any device work
(no device is touched here: every call returns from its checks)."""
import ctypes

import pytest
import torch

ENTRY = "ultra_rspmm_rotate_backward_weight_f32"
OK, BAD_OP, BAD_SHAPE, NULL_POINTER, ABI = 0, 1, 2, 3, 7


def test_entry_is_in_the_signature_table_and_exported():
    from ultra_torchdrug_amd import _lib
    assert ENTRY in _lib.SIGNATURES and ENTRY in _lib.EXPORTS
    restype, argtypes = _lib.SIGNATURES[ENTRY]
    # (fwd, relation, input, output, output_grad, d_weight, n_rel, F, block, sum_op, stream)
    assert restype is ctypes.c_int and len(argtypes) == 11 and argtypes[0] is _lib.seg
    assert argtypes[6:10] == [ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, ctypes.c_int]
    lib = _lib.load()
    entry = getattr(lib, ENTRY)
    assert entry.argtypes == argtypes and entry.restype is restype


def test_c_abi_checks_come_before_any_device_work():
    from ultra_torchdrug_amd import _lib
    lib = _lib.load()
    empty = _lib.UltraSegments()
    # addresses that are never dereferenced: every call below returns from the argument checks
    fake = ctypes.addressof(ctypes.create_string_buffer(64))

    def call(seg, F, block, sum_op, output=None, ptr=None):
        return getattr(lib, ENTRY)(ctypes.byref(seg), ptr, ptr, output, ptr, ptr, 3, F, block, sum_op, None)

    assert call(empty, 64, 64, 0) == OK                         # zero edges: nothing to do, NULL operands accepted
    assert call(empty, 64, 64, 2) == OK
    for F, block in ((64, 7), (64, 0), (64, -2), (96, 64), (0, 64), (-64, 64)):
        assert call(empty, F, block, 0) == BAD_SHAPE, (F, block)
    assert call(empty, 64, 64, 3) == BAD_OP and call(empty, 64, 64, -1) == BAD_OP
    assert call(empty, 64, 7, 3) == BAD_SHAPE                   # the shape is looked at first
    foreign = _lib.UltraSegments()
    foreign.abi_version = 7
    assert call(foreign, 64, 64, 0) == ABI
    assert call(foreign, 64, 7, 9) == ABI                       # ... and the plan before everything else
    short = _lib.UltraSegments()
    short.struct_bytes -= 8
    assert call(short, 64, 64, 0) == ABI

    one = _lib.UltraSegments()
    one.n_rows, one.n_edges = 1, 1
    one.row = one.node_a = one.rel = fake
    assert call(one, 64, 64, 0) == NULL_POINTER                 # operands missing
    assert call(one, 64, 64, 2, output=None, ptr=fake) == NULL_POINTER      # max reads the forward output
    assert call(one, 64, 64, 1, output=None, ptr=fake) == NULL_POINTER      # min too
    assert call(one, 64, 7, 2, output=None, ptr=fake) == BAD_SHAPE
    assert call(one, 64, 64, 5, output=None, ptr=fake) == BAD_OP
    no_index = _lib.UltraSegments()
    no_index.n_rows, no_index.n_edges = 1, 1
    assert call(no_index, 64, 64, 0, ptr=fake) == NULL_POINTER  # a plan with edges and no index arrays


def test_edge_weight_is_device_only_and_validated():
    """``rotate_rspmm(edge_weight=)`` on CPU tensors raises, as ``generalized_rspmm(edge_weight=)`` does; the shape is checked."""
    from ultra_torchdrug_amd import RelCSR, rotate_rspmm
    gen = torch.Generator().manual_seed(0)
    dst, src, rel = (torch.randint(0, m, (40,), generator=gen) for m in (10, 10, 3))
    csr = RelCSR(dst, src, rel, None, 10, 10, 3)
    relation, x = torch.randn(3, 8, generator=gen), torch.randn(10, 8, generator=gen)
    with pytest.raises(RuntimeError, match="MI355X"):
        rotate_rspmm(csr, relation, x, "add", 4, edge_weight=torch.ones(csr.n_edges))
    with pytest.raises(RuntimeError, match="one weight per coalesced edge"):
        rotate_rspmm(csr, relation, x, "add", 4, edge_weight=torch.ones(csr.n_edges + 1))
    assert torch.equal(rotate_rspmm(csr, relation, x, "add", 4), rotate_rspmm(csr, relation, x, "add", 4, edge_weight=None))


def test_native_edge_grad_conditions():
    """Which layers take a leaf per coalesced edge: the graph and dtype conditions of ``layer.native_edge_grad``."""
    from types import SimpleNamespace
    from ultra_torchdrug_amd.layer import GeneralizedRelationalConvNBFMod as Conv
    unit = SimpleNamespace(relcsr=SimpleNamespace(unit_weight=True))
    weighted = SimpleNamespace(relcsr=SimpleNamespace(unit_weight=False))
    x32, x64 = torch.zeros(1), torch.zeros(1, dtype=torch.float64)
    conv = lambda message, aggregate, dim=64: Conv(dim, dim, 4, dim, message_func=message, aggregate_func=aggregate)
    for message in ("distmult", "transe", "rotate"):
        for aggregate in ("sum", "max"):
            assert conv(message, aggregate).native_edge_grad(weighted, x32)
        assert conv(message, "mean").native_edge_grad(unit, x32)
        assert not conv(message, "mean").native_edge_grad(weighted, x32)
        assert not conv(message, "pna").native_edge_grad(unit, x32)
    assert not conv("rotate", "sum").native_edge_grad(unit, x64)
    assert not conv("rotate", "sum", dim=7).native_edge_grad(unit, x32)
    assert conv("distmult", "sum_nobound").native_edge_grad(unit, x32)          # as before
    assert not conv("rotate", "sum_nobound").native_edge_grad(unit, x32)

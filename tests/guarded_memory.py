"""Poisoned, guard-banded allocations: what a launch TOUCHES, next to what it returns.

The rest of the suite compares results.  This module makes two further classes of error visible without a sanitizer, a
debugger or an edit to the product:

* reads of memory nobody wrote -- every ``torch.empty`` / ``empty_like`` of the product modules is handed out filled with a
  recognisable poison, so a result that depends on an unwritten slab, slack word or unlisted row is a NaN (or differs from the
  unguarded run) instead of the zeros a fresh process usually finds there;
* writes (and result-bearing reads) past the end of an operand -- every allocation lies between two bands of a fixed byte
  pattern that :meth:`Guard.check` compares afterwards; inputs copied with :func:`banded` lie between NaN (floats) or zero
  (integers) bands, so rows read past their end reach a sum as NaN.

Layout of one carved buffer (``uint8``)::

    [ band | body | pad to 256 B | band ]

The body starts ``band`` bytes into the buffer; ``band`` is a multiple of 256, so the body is 256-byte aligned relative to the
buffer (misaligned bases are not tested here).  The pad belongs to the trailing band: it holds the pattern and is checked.

Band size.  By default the larger of 64 KiB and 32 rows of the case's widest row (``widest_row`` bytes, given by the test).  The
largest unit any kernel used by the cases of ``tests/test_memory_bounds_gpu.py`` stores at once is a 32-row tile of 64 fp32
columns -- the epilogues (``combine*.inc``, ``layer_fused.hip``, ``dense.inc``: 32 x 256 B = 8 KiB; the tail tile's stray rows are
at most 31 of them) and the score head's 32-row tile; quad_kernel, rowgroup and the fix-up pass store one row of F floats per
lane group (the cases pass their F as ``widest_row``, so a band is never less than 32 such rows; F <= 256 columns outside the
whole-step case, whose 32 queries make rows of 8 KiB and bands of 256 KiB), the integer kernels one element per lane and the plan
builders one 16-byte chunk record.  8 KiB is an eighth of the 64 KiB minimum, so no case has a tile larger than half its band:
a whole stray tile lands inside the band, where it is seen, and not beyond it.  This is a condition read from the kernels, not a
measurement.

Body poison.  fp32 / fp64 (and fp16 / bf16) bodies hold a quiet NaN with the payload ``0xDEAD`` (:data:`POISON_F32`,
:data:`POISON_F64`; :func:`has_poison` finds it in a result).  Integer and byte bodies hold all-ones bytes, i.e. ``-1``: an
uninitialised integer that a kernel uses as a row or element index then addresses the LEADING BAND of the tensor it indexes --
mapped memory, where a write is caught by ``check()`` and a read meets the band's pattern -- rather than a wild address that
would fault the device.  Blind spot: the project itself uses ``-1`` as list padding (``row_list`` slots, top-K indices, sample
slots), so a kernel that mistakes an unwritten ``-1`` for padding is not caught by the body poison alone; such lists are
compared with their reference exactly by the cases.  ``torch.zeros`` / ``zeros_like`` / ``full`` / ``ones`` get bands but keep
their values.

``guarded(*modules)`` replaces the name ``torch`` in the given product modules (default ``functional`` and ``relcsr``; on request
``graph``, ``layer``, ``model``, ``rel_model``, ``task``, ``engine``) by a proxy that forwards everything but those six allocation
functions.  Tensor caches of the product that could hand back an unguarded workspace are cleared on entry (and again on exit,
so that no carved tensor outlives its guard): ``functional._sparse_cache``.  That is the only module-level tensor cache; plans,
frontier indices and completion keys hang off ``RelCSR`` / ``Graph`` objects and ``task._relation_cache`` off the task, which the
cases build INSIDE the guard.  ``.new_empty`` / ``.new_zeros`` / ``.new_full`` are tensor methods the proxy cannot see
(``tests/test_guarded_memory_cpu.py`` lists every one the product has, with its reason).

Limit: the rspmm, rotate, beam-search and hop-distance operators of ``csrc/torch_ext.cpp`` allocate with ``at::empty`` in C++,
which no Python proxy sees.  With ``ULTRA_BINDING=ctypes`` (``_torch_ext.binding()`` reads the environment at each call, so
``monkeypatch.setenv`` is enough) the same operands are allocated in ``functional.py`` and are guarded.  The guard refuses to
start while a stream is capturing: its fills and checks are launches of their own.
"""
import contextlib
import importlib
import struct
import sys

import pytest
import torch as _torch

PRODUCT = "ultra_torchdrug_amd"
DEFAULT_MODULES = ("functional", "relcsr")
ALL_MODULES = ("functional", "relcsr", "graph", "layer", "model", "rel_model", "task", "engine")
INTERCEPTED = ("empty", "empty_like", "zeros", "zeros_like", "full", "ones")

BAND_BYTE = 0xA5
MIN_BAND = 64 * 1024
ALIGN = 256
POISON_F32 = 0x7FC0DEAD                 # quiet NaN, payload 0xDEAD
POISON_F64 = 0x7FF80000DEADDEAD
INPUT_NAN_F32 = 0x7FC0B0B0              # the NaN of banded() inputs' bands: another payload than the body poison
INPUT_NAN_F64 = 0x7FF80000B0B0B0B0
_THIS_FILE = __file__[:-1] if __file__.endswith((".pyc", ".pyo")) else __file__


def _round_up(n, to):
    return (int(n) + to - 1) // to * to


def _signed(bits, width):
    return bits - (1 << width) if bits >> (width - 1) else bits


def default_band(widest_row=0):
    """The larger of 64 KiB and 32 rows of ``widest_row`` bytes, as a multiple of 256."""
    return _round_up(max(MIN_BAND, 32 * int(widest_row)), ALIGN)


def _call_site():
    """File and line of the nearest caller outside this module."""
    frame = sys._getframe(1)
    while frame is not None and frame.f_code.co_filename == _THIS_FILE:
        frame = frame.f_back
    return (frame.f_code.co_filename, frame.f_lineno) if frame is not None else ("?", 0)


def _fill_bits(flat, dtype, bits32, bits64):
    """Fills the flat tensor ``flat`` of float ``dtype`` with the NaN whose bit pattern is given."""
    if dtype == _torch.float32:
        flat.view(_torch.int32).fill_(_signed(bits32, 32))
    elif dtype == _torch.float64:
        flat.view(_torch.int64).fill_(_signed(bits64, 64))
    else:
        flat.fill_(float("nan"))


class _Record:
    __slots__ = ("buffer", "band", "nbytes", "shape", "dtype", "site", "kind", "pattern")

    def describe(self):
        return "%s %s %s carved at %s:%d" % (self.kind, tuple(self.shape), self.dtype, self.site[0], self.site[1])


class BandDamage(AssertionError):
    """``Guard.check()``: some byte of a band no longer holds its pattern."""


class Guard:
    """Carves tensors out of banded buffers and remembers every one of them."""

    def __init__(self, band=None, widest_row=0):
        self.band = _round_up(band, ALIGN) if band is not None else default_band(widest_row)
        self.records = []

    # ------------------------------------------------------------------------------------------------ allocation
    def _carve(self, shape, dtype, device, kind, pattern):
        shape = tuple(int(s) for s in shape)
        dtype = dtype if dtype is not None else _torch.get_default_dtype()
        item = _torch.empty((), dtype=dtype).element_size()
        numel = 1
        for s in shape:
            if s < 0:
                raise RuntimeError("negative dimension in %s" % (shape,))
            numel *= s
        nbytes = numel * item
        buffer = _torch.empty(2 * self.band + _round_up(nbytes, ALIGN), dtype=_torch.uint8, device=device)
        rec = _Record()
        rec.buffer, rec.band, rec.nbytes, rec.shape, rec.dtype, rec.kind = buffer, self.band, nbytes, shape, dtype, kind
        rec.site = _call_site()
        rec.pattern = _torch.tensor(pattern, dtype=_torch.uint8, device=buffer.device)
        if len(pattern) == 1:
            buffer.fill_(pattern[0])
        else:
            buffer.view(-1, len(pattern)).copy_(rec.pattern)
        self.records.append(rec)
        body = buffer[self.band:self.band + nbytes]
        body = body.view(dtype) if nbytes else _torch.empty(0, dtype=dtype, device=buffer.device)
        return body.view(shape), rec

    def carve(self, shape, dtype=None, device=None, poison=True):
        """A contiguous tensor of ``shape`` / ``dtype`` between two bands; ``poison``: NaN with a payload (floats), -1 (the rest)."""
        body, _ = self._carve(shape, dtype, device, "allocation", (BAND_BYTE,))
        if poison and body.numel():
            flat = body.view(-1)
            if body.dtype.is_floating_point:
                _fill_bits(flat, body.dtype, POISON_F32, POISON_F64)
            elif body.dtype.is_complex:
                flat.fill_(complex(float("nan"), float("nan")))
            elif body.dtype == _torch.bool:
                flat.fill_(True)
            else:
                flat.view(_torch.uint8).fill_(0xFF)
        return body

    def banded(self, tensor, fill=None):
        """A contiguous copy of ``tensor`` whose bands hold ``fill``: by default NaN for floats -- rows read past the end reach a
        sum as NaN -- and 0 for integers -- in range, so an over-read of an index array never becomes a wild gather."""
        dtype = tensor.dtype
        item = tensor.element_size()
        if fill is None:
            if dtype == _torch.float32:
                pattern = struct.pack("<I", INPUT_NAN_F32)
            elif dtype == _torch.float64:
                pattern = struct.pack("<Q", INPUT_NAN_F64)
            elif dtype.is_floating_point:
                pattern = bytes(_torch.full((1,), float("nan"), dtype=dtype).view(_torch.uint8).tolist())
            else:
                pattern = bytes(item)
        else:
            pattern = bytes(_torch.full((1,), fill, dtype=dtype).view(_torch.uint8).tolist())
        body, _ = self._carve(tensor.shape, dtype, tensor.device, "input", tuple(pattern))
        body.copy_(tensor.detach())
        return body

    # ------------------------------------------------------------------------------------------------ the check
    def damage(self):
        """``[(record, first damaged byte offset relative to the body's start)]``; negative offsets lie in the leading band."""
        if any(r.buffer.is_cuda for r in self.records):
            _torch.cuda.synchronize()
        by_device = {}
        for r in self.records:
            by_device.setdefault(r.buffer.device, []).append(r)
        found = []
        for records in by_device.values():
            counts = []
            for r in records:
                p = r.pattern.numel()
                lead = r.buffer[:r.band].view(-1, p)
                trail_from = r.band + _round_up(r.nbytes, p)                 # (nbytes is a multiple of the item size = p)
                trail = r.buffer[trail_from:].view(-1, p)
                counts.append((lead != r.pattern).sum() + (trail != r.pattern).sum())
            for r, count in zip(records, _torch.stack(counts).tolist()):
                if count:
                    p = r.pattern.numel()
                    whole = r.buffer.clone()
                    whole[r.band:r.band + r.nbytes] = r.pattern.repeat(_round_up(r.nbytes, p) // p)[:r.nbytes]
                    bad = (whole.view(-1, p) != r.pattern).view(-1).nonzero()
                    found.append((r, int(bad[0]) - r.band))
        return found

    def check(self):
        """Synchronises, then asserts that every band of every carved buffer still holds its pattern."""
        found = self.damage()
        if found:
            raise BandDamage("; ".join(
                "%s band of %s damaged: first byte at offset %d from the body's start (body is %d bytes)"
                % ("leading" if off < 0 else "trailing", r.describe(), off, r.nbytes) for r, off in found))


def has_poison(tensor):
    """True where a float tensor still holds the body poison of :meth:`Guard.carve` (any element)."""
    if tensor is None or tensor.numel() == 0:
        return False
    t = tensor.detach().contiguous().view(-1)
    if t.dtype == _torch.float32:
        return bool((t.view(_torch.int32) == _signed(POISON_F32, 32)).any())
    if t.dtype == _torch.float64:
        return bool((t.view(_torch.int64) == _signed(POISON_F64, 64)).any())
    raise TypeError("has_poison: only fp32 / fp64 carry a recognisable payload, got %s" % t.dtype)


# ---------------------------------------------------------------------------------------------------- the proxy
def _sizes(args):
    if len(args) == 1 and not isinstance(args[0], int) and hasattr(args[0], "__iter__") and not isinstance(args[0], _torch.Tensor):
        return tuple(int(s) for s in args[0])
    return tuple(int(s) for s in args)


def _options(kwargs, allowed=("dtype", "device", "memory_format", "requires_grad")):
    unknown = set(kwargs) - set(allowed)
    if unknown:
        raise TypeError("guarded_memory: the allocation proxy does not know the keyword(s) %s" % sorted(unknown))
    fmt = kwargs.get("memory_format")
    if fmt is not None and fmt not in (_torch.contiguous_format, _torch.preserve_format):
        raise TypeError("guarded_memory: carved tensors are contiguous, got memory_format=%s" % fmt)
    return kwargs.get("dtype"), kwargs.get("device"), bool(kwargs.get("requires_grad", False))


class TorchProxy:
    """Stands for the module ``torch`` inside a product module: everything is forwarded but the six allocation functions."""

    def __init__(self, guard):
        self._guard = guard

    def __getattr__(self, name):
        return getattr(_torch, name)

    def _new(self, sizes, dtype, device, requires_grad, poison):
        out = self._guard.carve(sizes, dtype, device, poison)
        return out.requires_grad_() if requires_grad else out

    def empty(self, *size, **kwargs):
        dtype, device, grad = _options(kwargs)
        return self._new(_sizes(size), dtype, device, grad, True)

    def zeros(self, *size, **kwargs):
        dtype, device, grad = _options(kwargs)
        out = self._new(_sizes(size), dtype, device, False, False)
        out.zero_()
        return out.requires_grad_() if grad else out

    def ones(self, *size, **kwargs):
        dtype, device, grad = _options(kwargs)
        out = self._new(_sizes(size), dtype, device, False, False)
        out.fill_(1)
        return out.requires_grad_() if grad else out

    def full(self, size, fill_value, **kwargs):
        dtype, device, grad = _options(kwargs)
        if dtype is None:
            if isinstance(fill_value, _torch.Tensor):
                dtype = fill_value.dtype
            elif isinstance(fill_value, bool):
                dtype = _torch.bool
            elif isinstance(fill_value, int):
                dtype = _torch.int64
            elif isinstance(fill_value, complex):
                dtype = _torch.complex64
        out = self._new(_sizes((size,)), dtype, device, False, False)
        out.fill_(fill_value)
        return out.requires_grad_() if grad else out

    def empty_like(self, tensor, **kwargs):
        dtype, device, grad = _options(kwargs)
        return self._new(tuple(tensor.shape), dtype or tensor.dtype, device if device is not None else tensor.device, grad, True)

    def zeros_like(self, tensor, **kwargs):
        dtype, device, grad = _options(kwargs)
        out = self._new(tuple(tensor.shape), dtype or tensor.dtype, device if device is not None else tensor.device, False, False)
        out.zero_()
        return out.requires_grad_() if grad else out


def _product_module(name):
    return importlib.import_module("%s.%s" % (PRODUCT, name))


def _clear_caches():
    _product_module("functional")._sparse_cache.clear()


@contextlib.contextmanager
def guarded(*modules, band=None, widest_row=0):
    """``with guarded("functional", "relcsr") as guard:`` -- the product modules allocate through ``guard`` for the duration;
    on a clean exit the modules are restored and ``guard.check()`` runs."""
    if _torch.cuda.is_available() and _torch.cuda.is_initialized() and _torch.cuda.is_current_stream_capturing():
        raise RuntimeError("guarded_memory: a stream is capturing; the guard's fills and checks are launches of their own")
    names = modules or DEFAULT_MODULES
    unknown = set(names) - set(ALL_MODULES)
    if unknown:
        raise ValueError("guarded_memory: not a product module that can be proxied: %s" % sorted(unknown))
    mods = [_product_module(n) for n in names]
    guard = Guard(band=band, widest_row=widest_row)
    proxy = TorchProxy(guard)
    _clear_caches()
    saved = [m.torch for m in mods]
    for m in mods:
        m.torch = proxy
    try:
        yield guard
    finally:
        for m, real in zip(mods, saved):
            m.torch = real
        _clear_caches()
    guard.check()


@pytest.fixture(name="guarded")
def guarded_fixture(request):
    """The default guard (``functional`` and ``relcsr``) around one test; ``@pytest.mark.parametrize("guarded", [modules],
    indirect=True)`` names other modules.  ``check()`` runs when the test returns."""
    modules = tuple(getattr(request, "param", ()) or ())
    with guarded(*modules) as guard:
        yield guard

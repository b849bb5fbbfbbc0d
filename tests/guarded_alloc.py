"""Guard bands and two-fill runs: what a call wrote OUTSIDE its buffers, and which returned bytes it never wrote.

Every other test of this suite asks whether the returned values are right.  The buffers they are read from come out of the caching
allocator, which rounds blocks up to 512 bytes, packs them into segments and hands a previous call's block back for the same shape:
a store one vector past the end lands in slack or in a neighbour without a fault, and an element the kernel never writes reads back
as a plausible (often the correct) value.  This module makes both visible without touching the allocator:

  proxy         a stand-in for the `torch` module AS SEEN BY ONE PROJECT MODULE (monkeypatch.setattr(functional, 'torch', proxy)).
                It delegates everything to the real torch except empty / empty_like / zeros / zeros_like.  An intercepted allocation
                of nbytes > 0 on the guarded device type becomes one uint8 buffer of G + nbytes + G' bytes, G = 4096, G' = 4096 +
                round-up of nbytes to 256, filled with the run's fill byte; the caller gets the slice [G, G + nbytes) in the dtype and
                shape it asked for (zeros: with the payload zeroed).  The payload start keeps the allocator's 256-byte alignment and
                the high guard starts at byte nbytes exactly -- no slack in between.  Zero-size requests and tensors on any other
                device type pass through unguarded.  Every allocation is logged with its buffer, byte count, dtype, shape and the
                file:line of the caller in the project module.
  check_guards  synchronise, then every guard byte must still equal the fill.
  run_twice     the same function under fill 0xCB and under fill 0x35 (the two differ in every byte of a buffer, neither is 0x00 or
                0xFF -- 0 and -1 are legitimate padding values -- and every 2- and 4-byte float read of either is finite), then
                  check 1  guards intact in both runs;
                  check 2  no returned element holds pattern A in run A AND pattern B in run B at the same position: such an
                           element was never written;
                  check 3  every returned tensor is bit-for-bit the same in both runs: nothing depends on what a workspace, an aux
                           buffer or an output held before the call (a missing memset in front of atomics, a flag word assumed zero).

What this cannot see: READS out of bounds (a load past the end changes no byte), and a stray write farther than G = 4096 bytes from
the payload (G is a condition, not a measurement: a multiple of 256, and larger than one wave of 16-byte stores, 1024 bytes).
"""
import os
import sys

import numpy as np
import torch as _torch

G = 4096
FILL_A, FILL_B = 0xCB, 0x35
_HERE = os.path.abspath(__file__)
_INTERCEPTED = ('empty', 'empty_like', 'zeros', 'zeros_like')


def high_guard_bytes(nbytes):
    return G + (int(nbytes) + 255) // 256 * 256


class Allocation(object):
    __slots__ = ('buf', 'nbytes', 'dtype', 'shape', 'site', 'kind')

    def __init__(self, buf, nbytes, dtype, shape, site, kind):
        self.buf, self.nbytes, self.dtype, self.shape, self.site, self.kind = buf, nbytes, dtype, shape, site, kind

    def describe(self):
        return '%s at %s, shape %s, %s (%d bytes)' % (self.kind, self.site, tuple(self.shape), self.dtype, self.nbytes)

    def payload(self):
        return self.buf[G:G + self.nbytes]


class GuardedAllocator(object):
    """One run's allocator: the fill byte, the device type it guards ('cuda' for the kernel cases, 'cpu' for the checker's own
    tests) and the log of what it handed out.  The log keeps every buffer alive, so no block is recycled before check_guards."""

    def __init__(self, fill, device_type='cuda'):
        assert 0 < fill < 255
        self.fill, self.device_type, self.log = int(fill), device_type, []

    def proxy(self, module=None):
        """The torch stand-in for `module` (None: for the test's own allocations; the call site is then the caller's)."""
        return _TorchProxy(self, getattr(module, '__file__', None))

    # -- the four intercepted constructors; `site_file`: the file whose frame names the call site ---------------------------------
    def _site(self, site_file):
        f = sys._getframe(2)
        first = None
        while f is not None:
            name = os.path.abspath(f.f_code.co_filename)
            if name != _HERE:
                if first is None:
                    first = f
                if site_file is None or name == os.path.abspath(site_file):
                    return '%s:%d' % (os.path.basename(name), f.f_lineno)
            f = f.f_back
        return '%s:%d' % (os.path.basename(first.f_code.co_filename), first.f_lineno) if first is not None else '?'

    def _guarded(self, shape, dtype, device, strides, zero, kind, site_file):
        shape = tuple(int(s) for s in shape)
        numel = int(np.prod(shape, dtype=np.int64)) if shape else 1
        nbytes = numel * _itemsize(dtype)
        total = G + nbytes + high_guard_bytes(nbytes)
        raw = _torch.full((total + 256,), self.fill, dtype=_torch.uint8, device=device)
        skip = -raw.data_ptr() % 256             # 0 on the GPU (the caching allocator aligns blocks to 512 bytes); the host's malloc does not
        buf = raw[skip:skip + total]
        assert device.type != 'cuda' or skip == 0, 'the caching allocator no longer aligns blocks to 256 bytes'
        pay = buf[G:G + nbytes]
        if zero:
            pay.zero_()
        out = pay.view(dtype)
        out = out.as_strided(shape, strides) if strides is not None else out.reshape(shape)
        self.log.append(Allocation(buf, nbytes, dtype, shape, self._site(site_file), kind))
        return out

    def _new(self, kind, site_file, args, kw):
        real = getattr(_torch, kind)
        kw = dict(kw)
        if set(kw) - {'dtype', 'device', 'requires_grad'}:
            return real(*args, **kw)                                  # out=, pin_memory=, memory_format=, layout=: not ours
        shape = args[0] if len(args) == 1 and isinstance(args[0], (tuple, list, _torch.Size)) else args
        if not all(isinstance(s, (int, np.integer)) for s in shape):
            return real(*args, **kw)
        dtype = kw.get('dtype') or _torch.get_default_dtype()
        device = _torch.device(kw['device']) if kw.get('device') is not None else _torch.empty(0).device
        numel = int(np.prod([int(s) for s in shape], dtype=np.int64)) if len(shape) else 1
        if device.type != self.device_type or numel == 0 or dtype.is_complex:
            return real(*args, **kw)
        out = self._guarded(shape, dtype, device, None, kind == 'zeros', kind, site_file)
        return out.requires_grad_(True) if kw.get('requires_grad') else out

    def _like(self, kind, site_file, t, kw):
        real = getattr(_torch, kind)
        if set(kw) - {'dtype', 'device'} or not isinstance(t, _torch.Tensor):
            return real(t, **kw)
        dtype = kw.get('dtype') or t.dtype
        device = _torch.device(kw['device']) if kw.get('device') is not None else t.device
        if device.type != self.device_type or t.numel() == 0 or dtype.is_complex:
            return real(t, **kw)
        # torch.preserve_format: a dense, non-overlapping tensor keeps its strides, anything else comes out contiguous
        strides = t.stride() if (not t.is_contiguous() and _dense(t)) else None
        return self._guarded(t.shape, dtype, device, strides, kind == 'zeros_like', kind, site_file)

    # -- the test's own buffers (calls that update caller-owned memory in place) ----------------------------------------------------
    def empty(self, *args, **kw):
        return self._new('empty', None, args, kw)

    def zeros(self, *args, **kw):
        return self._new('zeros', None, args, kw)

    def tensor(self, values, dtype=None, device=None):
        """A guarded copy of `values` (a numpy array or a tensor): a caller-owned buffer with known contents."""
        src = values if isinstance(values, _torch.Tensor) else _torch.as_tensor(np.asarray(values))
        if dtype is not None:
            src = src.to(dtype)
        dst = self._new('empty', None, (tuple(src.shape),), dict(dtype=src.dtype, device=device if device is not None else src.device))
        dst.copy_(src)
        return dst


def _itemsize(dtype):
    return _torch.empty(0, dtype=dtype).element_size()


def _dense(t):
    sizes_strides = sorted((st, sz) for sz, st in zip(t.shape, t.stride()) if sz > 1)
    expect = 1
    for st, sz in sizes_strides:
        if st != expect:
            return False
        expect *= sz
    return True


class _TorchProxy(object):
    """Delegates to the real torch module; empty / empty_like / zeros / zeros_like go through the run's GuardedAllocator."""

    def __init__(self, alloc, site_file):
        object.__setattr__(self, '_alloc', alloc)
        object.__setattr__(self, '_site_file', site_file)

    def __getattr__(self, name):
        return getattr(_torch, name)

    def empty(self, *args, **kw):
        return self._alloc._new('empty', self._site_file, args, kw)

    def zeros(self, *args, **kw):
        return self._alloc._new('zeros', self._site_file, args, kw)

    def empty_like(self, t, **kw):
        return self._alloc._like('empty_like', self._site_file, t, kw)

    def zeros_like(self, t, **kw):
        return self._alloc._like('zeros_like', self._site_file, t, kw)


# ---- check 1 ---------------------------------------------------------------------------------------------------------------------
def check_guards(alloc, what=''):
    """Every guard byte of every logged allocation still equals the fill.  The failure names the allocation (call site, shape,
    dtype), the side, the first and last offending byte -- low side: relative to the payload start (negative), high side: relative
    to the payload END (0 = the first byte behind it) -- and for the high side the same in elements."""
    if alloc.device_type == 'cuda':
        _torch.cuda.synchronize()
    if not alloc.log:
        return
    flags = _torch.stack([_torch.stack([(a.buf[:G] != alloc.fill).any(), (a.buf[G + a.nbytes:] != alloc.fill).any()]) for a in alloc.log])
    flags = flags.cpu().numpy()
    if not flags.any():
        return
    lines = []
    for a, (low, high) in zip(alloc.log, flags):
        if low:
            bad = np.flatnonzero(a.buf[:G].cpu().numpy() != alloc.fill)
            lines.append('low guard of %s: %d bytes overwritten, first at byte %d, last at byte %d relative to the payload start'
                         % (a.describe(), bad.size, int(bad[0]) - G, int(bad[-1]) - G))
        if high:
            bad = np.flatnonzero(a.buf[G + a.nbytes:].cpu().numpy() != alloc.fill)
            es = _itemsize(a.dtype)
            lines.append('high guard of %s: %d bytes overwritten, first at byte %d, last at byte %d past the payload end '
                         '(elements %d .. %d past the end)' % (a.describe(), bad.size, int(bad[0]), int(bad[-1]), int(bad[0]) // es,
                                                               int(bad[-1]) // es))
    raise AssertionError('%sstray write (fill 0x%02X):\n  %s' % (what, alloc.fill, '\n  '.join(lines)))


# ---- the two-fill protocol ----------------------------------------------------------------------------------------------------------
class TwoRuns(object):
    """outputs[i], inplace[i]: name -> tensor of run i (A, B); allocs[i]: that run's GuardedAllocator (its .log is the record)."""

    def __init__(self):
        self.outputs, self.inplace, self.allocs = [], [], []


def run_twice(fn, monkeypatch=None, modules=(), device_type='cuda', between=None):
    """fn(alloc) once under FILL_A and once under FILL_B.  fn builds fresh inputs and parameters from its own seed on every call and
    returns name -> tensor (the returned outputs), or a pair (outputs, inplace): `inplace` are caller-owned buffers the call updates
    (allocated by fn through alloc.empty / alloc.zeros / alloc.tensor), to which checks 1 and 3 apply but not check 2.
    modules: the project modules whose `torch` is replaced by the proxy for the duration of each run (pytest's monkeypatch).
    between: called in front of each run (functional.invalidate_cached_kernels: cached re-layouts are then allocated INSIDE the
    run).  The tensors of run A stay alive through run B, so the two runs cannot share a block."""
    res = TwoRuns()
    for fill in (FILL_A, FILL_B):
        alloc = GuardedAllocator(fill, device_type)
        if between is not None:
            between()
        if modules:
            with monkeypatch.context() as m:
                for mod in modules:
                    m.setattr(mod, 'torch', alloc.proxy(mod))
                out = fn(alloc)
        else:
            out = fn(alloc)
        outputs, inplace = out if isinstance(out, tuple) else (out, {})
        if device_type == 'cuda':
            _torch.cuda.synchronize()
        res.outputs.append({k: v.detach() for k, v in outputs.items() if v is not None})
        res.inplace.append({k: v.detach() for k, v in inplace.items() if v is not None})
        res.allocs.append(alloc)
    return res


def _bytes_of(t):
    """(elements, itemsize) uint8 image of a tensor in its logical (row-major) order."""
    t = t.detach()
    if t.dtype == _torch.bool:
        t = t.to(_torch.uint8)
    flat = t.contiguous().reshape(-1)
    return flat.view(_torch.uint8).cpu().numpy().reshape(flat.numel(), flat.element_size())


def _positions(flat, shape, limit=4):
    idx = [tuple(int(i) for i in np.unravel_index(int(f), shape)) if len(shape) else () for f in flat[:limit]]
    return ', '.join(str(i) for i in idx) + (', ...' if flat.size > limit else '')


def assert_guards_intact(res, what=''):
    for alloc, run in zip(res.allocs, 'AB'):
        check_guards(alloc, '%srun %s: ' % (what, run))


def assert_allocations_seen(res, what=''):
    for alloc, run in zip(res.allocs, 'AB'):
        assert alloc.log, '%srun %s: the proxy saw no allocation -- the buffers of this call did not come through the guarded ' \
            'allocator, so neither their guards nor their fill were checked' % (what, run)


def assert_no_stale_element(res, what=''):
    """Check 2.  Positions are reported as assert_equal_exact reports them: count, first, last, by index."""
    for name in res.outputs[0]:
        a, b = res.outputs[0][name], res.outputs[1][name]
        assert a.shape == b.shape and a.dtype == b.dtype, '%s%s: the two runs returned %s %s and %s %s' % (what, name, tuple(a.shape), a.dtype, tuple(b.shape), b.dtype)
        stale = np.flatnonzero((_bytes_of(a) == FILL_A).all(axis=1) & (_bytes_of(b) == FILL_B).all(axis=1))
        if stale.size:
            shape = tuple(a.shape)
            raise AssertionError('%s%s: %d of %d elements were never written (they hold the fill 0x%02X in run A and 0x%02X in run B)'
                                 '\n  first: index %s\n  last:  index %s\n  at: %s'
                                 % (what, name, stale.size, a.numel(), FILL_A, FILL_B, _positions(stale[:1], shape),
                                    _positions(stale[-1:], shape), _positions(stale, shape, 8)))


def first_bit_difference(a, b):
    """None when the two tensors are bit-for-bit equal, else (count, flat indices) of the elements that differ."""
    if a.shape != b.shape or a.dtype != b.dtype:
        return -1, np.zeros(0, dtype=np.int64)
    diff = np.flatnonzero((_bytes_of(a) != _bytes_of(b)).any(axis=1))
    return (int(diff.size), diff) if diff.size else None


def assert_bitwise_equal(res, what='', not_bitwise=None):
    """Check 3 on the returned tensors and on the in-place buffers.  not_bitwise: name -> callable(a, b, name) that compares the two
    runs of an output that is not bit-reproducible BY DESIGN with the tolerance of the entry point's own parity test."""
    for group in (res.outputs, res.inplace):
        for name in group[0]:
            a, b = group[0][name], group[1][name]
            if not_bitwise and name in not_bitwise:
                not_bitwise[name](a, b, name)
                continue
            d = first_bit_difference(a, b)
            if d is None:
                continue
            n, idx = d
            assert n >= 0, '%s%s: the two runs returned %s %s and %s %s' % (what, name, tuple(a.shape), a.dtype, tuple(b.shape), b.dtype)
            fa, fb = a.detach().contiguous().reshape(-1), b.detach().contiguous().reshape(-1)
            show = lambda t, i: t[int(i)].item() if not t.dtype.is_floating_point else float(t[int(i)])
            raise AssertionError('%s%s: %d of %d elements differ between the run under fill 0x%02X and the run under fill 0x%02X -- the '
                                 'result depends on what a buffer held before the call\n  first: index %s: %r vs %r\n  last:  index %s: %r vs %r'
                                 % (what, name, n, a.numel(), FILL_A, FILL_B, _positions(idx[:1], tuple(a.shape)), show(fa, idx[0]),
                                    show(fb, idx[0]), _positions(idx[-1:], tuple(a.shape)), show(fa, idx[-1]), show(fb, idx[-1])))


def assert_hygiene(res, what='', not_bitwise=None):
    """Checks 1, 2 and 3, and that the allocator was in the path at all."""
    assert_allocations_seen(res, what)
    assert_guards_intact(res, what)
    assert_no_stale_element(res, what)
    assert_bitwise_equal(res, what, not_bitwise)

"""Guard bands for device buffers: the instrument of tests/test_gpu_abi_bounds.py (a plain helper module, no conftest).

The C ABI takes raw pointers and no capacities, so a call that writes past the buffer it was given, or leaves part of it
unwritten, or reads a workspace it promised not to depend on, is invisible to a comparison of values.  ``guarded`` puts
one output (or workspace) between two canary regions of ONE allocation and prefills it with a pattern no finite input can
produce; ``frozen`` snapshots an input; ``patched_allocations`` does the former for every device buffer the Python facade
allocates inside a block.  Everything works on CPU tensors too (tests/test_redzone_cpu.py proves each detector fires).
"""
import contextlib

import numpy as np
import torch

GUARD_BYTE = 0xA5
GUARD_MIN = 64 * 1024          # bytes: a guard is a multiple of 256 bytes, at least this and at least the payload's size
ALIGN = 256


def _nbytes(shape, dtype):
    n = 1
    for s in shape:
        n *= int(s)
    return n * torch.empty((), dtype=dtype).element_size()


def _guard_bytes(payload_bytes):
    g = max(GUARD_MIN, payload_bytes)
    return (g + ALIGN - 1) // ALIGN * ALIGN


def _int_view(t):
    """flat integer view of a contiguous tensor's bits (NaN != NaN: bit patterns are compared as integers)"""
    flat = t.reshape(-1)
    if flat.dtype.is_complex:
        flat = torch.view_as_real(flat).reshape(-1)
    size = flat.element_size()
    return flat.view({1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[size])


class Guarded:
    """front guard | payload | back guard in one uint8 allocation ``base``; ``t`` is the payload as (shape, dtype)"""

    def __init__(self, shape, dtype, device, fill=0xFF):
        self.shape = tuple(int(s) for s in (shape if isinstance(shape, (tuple, list, torch.Size)) else (shape,)))
        self.dtype, self.fill = dtype, int(fill)
        self.nbytes = _nbytes(self.shape, dtype)
        self.guard = _guard_bytes(self.nbytes)
        # the payload starts and ends on its own bytes: a one-byte overrun on either side lands in a guard
        self.base = torch.full((2 * self.guard + self.nbytes,), GUARD_BYTE, dtype=torch.uint8, device=device)
        self.payload = self.base[self.guard:self.guard + self.nbytes]
        self.payload.fill_(self.fill)
        self.t = self.payload.view(dtype).reshape(self.shape)

    def refill(self, fill):
        """same buffer, payload prefilled anew (the stale-content runs: 0xFF, then 0x00)"""
        self.fill = int(fill)
        self.payload.fill_(self.fill)
        return self

    def _guard_report(self):
        out = []
        for name, lo in (('front', 0), ('back', self.guard + self.nbytes)):
            g = self.base[lo:lo + self.guard]
            bad = torch.nonzero(g != GUARD_BYTE).reshape(-1)
            if bad.numel():
                first, last = int(bad[0]), int(bad[-1])
                # offsets relative to the payload: negative = bytes before its start, >= 0 = bytes past its end
                rel = (lambda o: o - self.guard) if name == 'front' else (lambda o: o)
                out.append(f'{name} guard: {bad.numel()} byte(s) touched, first at payload{"" if name == "front" else " end"}'
                           f'{rel(first):+d}, last at {rel(last):+d}')
        return out

    def unwritten(self):
        """number of payload elements that still carry the prefill bit pattern"""
        if self.nbytes == 0:
            return 0
        iv = _int_view(self.t)
        pattern = torch.full((1,), self.fill, dtype=torch.uint8).repeat(iv.element_size()).view(iv.dtype)[0].item()
        return int((iv == pattern).sum())

    def check(self, written=False, what='buffer'):
        report = self._guard_report()
        assert not report, f'{what} {self.shape} {self.dtype}: write outside the payload of {self.nbytes} bytes; ' + '; '.join(report)
        if written:
            n = self.unwritten()
            assert n == 0, f'{what} {self.shape} {self.dtype}: {n} element(s) still hold the prefill 0x{self.fill:02X}'
        return self

    def bits(self):
        """host copy of the payload's bytes"""
        return self.payload.cpu().numpy().copy()


def guarded(shape, dtype, device, fill=0xFF):
    return Guarded(shape, dtype, device, fill)


class Frozen:
    """bitwise snapshot of an input tensor (any strides: the whole of what the tensor addresses is compared)"""

    def __init__(self, t):
        self.t = t
        self.snap = t.clone()

    def check(self, what='input'):
        a, b = _int_view(self.t.contiguous()), _int_view(self.snap.contiguous())
        bad = torch.nonzero(a != b).reshape(-1)
        assert bad.numel() == 0, (f'{what} {tuple(self.t.shape)} {self.t.dtype} was modified: {bad.numel()} word(s), first at '
                                  f'{int(bad[0]) if bad.numel() else -1}, last at {int(bad[-1]) if bad.numel() else -1}')
        return self


def frozen(t):
    return Frozen(t)


_PATCHED = ('empty', 'zeros', 'empty_like', 'zeros_like')


@contextlib.contextmanager
def patched_allocations():
    """Inside the block torch.empty / zeros / empty_like / zeros_like return guarded payloads for CUDA results (other
    results are untouched); every such buffer is registered and all guards are checked on a clean exit.  The originals are
    restored on every exit path.  Yields the list of registered Guarded buffers."""
    orig = {name: getattr(torch, name) for name in _PATCHED}
    registry = []

    def wrap(name):
        fn = orig[name]
        zero = name.startswith('zeros')

        def patched(*args, **kw):
            probe = fn(*args, **kw)
            # the factory's own result decides shape, dtype and device; only contiguous CUDA results are replaced
            if not probe.is_cuda or not probe.is_contiguous() or kw.get('out') is not None:
                return probe
            g = Guarded(tuple(probe.shape), probe.dtype, probe.device, fill=0x00 if zero else 0xFF)
            registry.append(g)
            return g.t
        patched.__name__ = name
        return patched

    for name in _PATCHED:
        setattr(torch, name, wrap(name))
    try:
        yield registry
    finally:
        for name in _PATCHED:
            setattr(torch, name, orig[name])
    for i, g in enumerate(registry):
        g.check(what=f'facade allocation #{i}')

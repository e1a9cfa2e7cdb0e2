"""Guard-band allocations for the kernel tests: every tensor a kernel may touch sits between two poisoned guards.

A wrapper's result comes from ``torch.empty`` of the exact size, in the slack of the caching allocator (512-byte rounding, parts of
2 MiB blocks): a store past the end corrupts a neighbour instead of the tensor under test, a skipped store finds the previous
correct result in the recycled block, and a tail read that is masked after the fact sees finite bits.  Here every allocation is a
view into a larger byte buffer ``[front guard | tensor | back guard]`` filled with the 16-bit pattern 0x7FC1 -- a NaN with a payload
as bf16, as fp16 and (doubled) as fp32, a recognisable value as an integer, and nothing a kernel computes from finite inputs.

    g = Guarded(K)                      # K = imagine360_amd.kernels (any module that reaches torch through its global `torch`)
    x = g.guard(x)                      # inputs / weights / tables / caller-owned destinations: copied between guards
    with g:                             # K.torch is a proxy: torch.empty / torch.zeros inside K come back guarded
        y = g.out(K.some_kernel(x))     # y must live in a guarded buffer (else AssertionError) and be written completely
    # leaving the block: synchronize, then check() -- guards and row gaps bit-identical to the pattern, outputs free of it

Only the name ``torch`` inside the module is replaced, and only while the block is active; the global torch is untouched.
"""
import torch as _torch

PATTERN = 0x7FC1                   # bf16 / fp16 NaN with a payload; 0x7FC17FC1 as fp32 is a NaN too
MIN_GUARD = 64 * 1024              # bytes, each side
GUARD_ROWS = 256                   # ... and at least this many rows of the last dimension of a tensor with rows (one GEMM row tile)
ALIGN = 256                        # alignment of the interior (the 16-byte checks of the launchers see production alignment)
_WORD = {1: _torch.uint8, 2: _torch.int16, 4: _torch.int32, 8: _torch.int64}
_SENTINEL = {2: PATTERN, 4: PATTERN << 16 | PATTERN, 8: ((PATTERN << 16 | PATTERN) << 32) | (PATTERN << 16 | PATTERN)}


def _round_up(v, m):
    return (v + m - 1) // m * m


def _expected(device, start, end):
    """The pattern's bytes at buffer offsets [start, end) (little endian: even offsets 0xC1, odd 0x7F)."""
    pat = _torch.tensor([PATTERN & 0xFF, PATTERN >> 8], dtype=_torch.uint8, device=device)
    return pat[_torch.arange(start, end, device=device) & 1]


class _Alloc:
    """One guarded buffer: ``raw`` (uint8, whole buffer), the interior at byte ``off`` spanning ``span`` bytes, ``view`` the tensor."""

    def __init__(self, shape, dtype, device, strides, misalign, label):
        shape = tuple(int(s) for s in shape)
        es = _torch.empty((), dtype=dtype).element_size()
        if strides is None:
            strides, acc = [], 1
            for s in reversed(shape):
                strides.append(acc)
                acc *= max(s, 1)
            strides = tuple(reversed(strides))
        strides = tuple(int(s) for s in strides)
        assert len(strides) == len(shape) and 0 <= misalign < ALIGN
        assert misalign % max(es, 2) == 0, "a tensor cannot start off its own element size (and the pattern is 2 bytes wide)"
        numel = 1
        for s in shape:
            numel *= s
        span_elems = (sum((s - 1) * st for s, st in zip(shape, strides)) + 1) if numel else 0
        # (a 1-D tensor -- a vector or a flat workspace -- has no rows: the 64 KiB minimum alone)
        row = max(shape[-1], strides[-2]) if len(shape) > 1 else 1
        guard = _round_up(max(MIN_GUARD, GUARD_ROWS * row * es), ALIGN)
        self.shape, self.dtype, self.strides, self.es, self.label = shape, dtype, strides, es, label
        self.span = span_elems * es
        total = ALIGN + guard + misalign + _round_up(self.span, ALIGN) + guard
        words = _torch.full((total // 2,), PATTERN, dtype=_torch.int16, device=device)
        self.raw = words.view(_torch.uint8)
        self.off = (-self.raw.data_ptr()) % ALIGN + guard + misalign
        self.dense = span_elems == numel
        self.view = self.raw[self.off:self.off + self.span].view(dtype).as_strided(shape, strides) if numel else _torch.empty(shape, dtype=dtype, device=device)
        self.begin = self.raw.data_ptr()
        self.end = self.begin + self.raw.numel()

    def describe(self):
        st = "" if self.dense else f" strides {self.strides}"
        return f"{self.label}: shape {self.shape} {self.dtype}{st}"

    def owns(self, t):
        return t.numel() == 0 or (t.device == self.raw.device and self.begin + self.off <= t.data_ptr() and
                                  t.data_ptr() + t.element_size() <= self.begin + self.off + self.span)

    def _range(self, bad, base):
        idx = bad.nonzero().flatten()
        return int(idx[0]) + base, int(idx[-1]) + base

    def corrupted(self):
        """[(side, first byte, last byte)] of the guard / gap bytes that no longer hold the pattern; offsets relative to the tensor
        (negative: front guard; >= span: back guard)."""
        found = []
        dev = self.raw.device
        for side, a, b in (("front guard", 0, self.off), ("back guard", self.off + self.span, self.raw.numel())):
            bad = self.raw[a:b] != _expected(dev, a, b)
            if bool(bad.any()):
                found.append((side,) + self._range(bad, a - self.off))
        if not self.dense and self.span:
            covered = _torch.zeros(self.span // self.es, dtype=_torch.bool, device=dev)
            covered.as_strided(self.shape, self.strides).fill_(True)
            bad = (self.raw[self.off:self.off + self.span] != _expected(dev, self.off, self.off + self.span)) & ~covered.repeat_interleave(self.es)
            if bool(bad.any()):
                found.append(("row gap",) + self._range(bad, 0))
        return found


def unwritten(t, alloc=None):
    """(count, first byte, last byte) of the elements of ``t`` that still hold the sentinel bits, or None.  Byte offsets are relative
    to the allocation's tensor (to ``t`` itself without one).  One-byte types: four consecutive pattern bytes (a 4-byte word of the
    buffer), since a single 0xC1 or 0x7F is an ordinary value."""
    if t.numel() == 0:
        return None
    es = t.element_size()
    base = 0 if alloc is None else t.data_ptr() - (alloc.begin + alloc.off)
    if es == 1:
        assert t.is_contiguous()
        flat = t.reshape(-1).view(_torch.uint8)
        start = (-(t.data_ptr() if alloc is None else alloc.off + base)) % 4
        n = (flat.numel() - start) // 4
        if n <= 0:
            return None
        first = (0 if alloc is None else alloc.off + base) + start
        hit = (flat[start:start + 4 * n] == _expected(t.device, first, first + 4 * n)).view(n, 4).all(dim=1)
        if not bool(hit.any()):
            return None
        idx = hit.nonzero().flatten()
        return int(hit.sum()) * 4, base + start + 4 * int(idx[0]), base + start + 4 * int(idx[-1]) + 3
    hit = t.view(_WORD[es]) == _SENTINEL[es]
    if not bool(hit.any()):
        return None
    nz = hit.nonzero()
    offs = (nz * _torch.tensor(t.stride(), device=nz.device)).sum(dim=1) * es + base
    return int(nz.shape[0]), int(offs.min()), int(offs.max()) + es - 1


class _TorchProxy:
    """Stands in for the name ``torch`` inside one module: everything is the real torch's, except ``empty`` and ``zeros``."""

    def __init__(self, owner):
        self.__dict__["_owner"] = owner

    def __getattr__(self, name):
        return getattr(_torch, name)

    def _alloc(self, kind, size, dtype, device, kw):
        assert not kw, f"torch.{kind} with {sorted(kw)} is not something the guarded proxy reproduces"
        if len(size) == 1 and not isinstance(size[0], int):
            size = tuple(size[0])
        return self._owner._new(size, dtype or _torch.get_default_dtype(), device or "cpu", None, 0, kind).view

    def empty(self, *size, dtype=None, device=None, **kw):
        return self._alloc("empty", size, dtype, device, kw)

    def zeros(self, *size, dtype=None, device=None, **kw):
        t = self._alloc("zeros", size, dtype, device, kw)
        t.zero_()
        return t


class Guarded:
    """See the module's docstring.  ``module``: the module whose global ``torch`` is replaced while the context is active."""

    def __init__(self, module):
        self.module = module
        self.allocs = []
        self.outputs = []
        self._saved = None

    # ---------------------------------------------------------------- allocations
    def _new(self, shape, dtype, device, strides, misalign, kind):
        a = _Alloc(shape, dtype, _torch.device(device), strides, misalign, f"{kind} #{len(self.allocs)}")
        self.allocs.append(a)
        return a

    def guard(self, t, strides=None, row_stride=None, misalign=0):
        """A copy of ``t`` between guards.  ``row_stride`` (elements, >= the last dimension): rows that far apart, the outer
        dimensions packed on top; ``strides``: every stride given (last one 1); the gaps are poisoned and checked.  ``misalign``:
        even byte offset of the tensor from its 256-byte alignment."""
        if row_stride is not None:
            assert strides is None and t.dim() >= 2 and row_stride >= t.shape[-1]
            strides, acc = [1], row_stride
            for s in reversed(t.shape[:-1]):
                strides.append(acc)
                acc *= s
            strides = tuple(reversed(strides))
        a = self._new(t.shape, t.dtype, t.device, strides, misalign, "guard")
        a.view.copy_(t)
        return a.view

    def empty(self, shape, dtype, device, strides=None, misalign=0):
        """A poisoned caller-owned destination (``out=`` / ``dst``): nothing copied in."""
        return self._new(shape, dtype, device, strides, misalign, "guard").view

    def find(self, t):
        for a in self.allocs:
            if a.owns(t):
                return a
        return None

    def out(self, *ts):
        """Name results: each must live in a guarded buffer (the bypass condition) and hold no sentinel when the context ends."""
        for t in ts:
            if self.find(t) is None:
                raise AssertionError(f"not guarded: a result of shape {tuple(t.shape)} {t.dtype} does not live in a guarded buffer -- "
                                     f"it was allocated by something other than torch.empty / torch.zeros of {self.module.__name__}")
            self.outputs.append(t)
        return ts[0] if len(ts) == 1 else ts

    # ---------------------------------------------------------------- the context
    def __enter__(self):
        assert self._saved is None
        self._saved = self.module.torch
        self.module.torch = _TorchProxy(self)
        return self

    def __exit__(self, exc_type, exc, tb):
        self.module.torch = self._saved
        self._saved = None
        if exc_type is None:
            self.check()
        return False

    def check(self):
        if any(a.raw.is_cuda for a in self.allocs):
            _torch.cuda.synchronize()
        problems = []
        for a in self.allocs:
            for side, lo, hi in a.corrupted():
                problems.append(f"{a.describe()}: {side} overwritten, bytes {lo}..{hi} relative to the tensor")
        for t in self.outputs:
            a = self.find(t)
            u = unwritten(t, a)
            if u is not None:
                problems.append(f"{a.describe()}: {u[0]} element(s) still hold the sentinel (never written, or a leaked "
                                f"tail read), bytes {u[1]}..{u[2]} relative to the tensor")
        if problems:
            raise AssertionError("guarded allocation check failed:\n  " + "\n  ".join(problems))

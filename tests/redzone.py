"""Redzone allocator for the GPU tests (test infrastructure).

Every parity test hands the kernels exact-size torch tensors from the caching allocator: a kernel that writes one row past its
output lands in allocator slack (blocks are rounded up to 512 bytes, freed blocks are recycled) and the test still passes.  Inside
`guarded()` every allocation call the host layer of articulated-pose_amd makes for a buffer it passes through the C ABI is intercepted:

      torch.empty  torch.zeros  torch.ones  torch.full       and their *_like forms

(outputs of single entries come from `empty`; the slot buffers of AncshPipeline, the depth front end's and the render-and-compare layer's
come from `zeros` / `full`).  On a HIP device each of them is carved out of a larger allocation instead:

      [ guard: PAD bytes of 0xA5 | body: the tensor | guard: PAD bytes of 0xA5 (+ alignment slack) ]

`check()` (called when the context exits) synchronises and asserts every guard byte.  An `empty` body is pre-filled with 0xFF bytes -- a
NaN for float32 / float64 and -1 for the integer types --, so an output element a kernel failed to write shows up in the test's own
equality check.  A `zeros`, `ones` or `full` body keeps the CALLER'S fill, not NaN / -1: the result is the original's in dtype, shape,
contiguity and value, and an unwritten element shows only where the caller asked for `empty`.
A call for another device, with pin_memory, with a memory format that is not contiguous, or with an argument the arena does not model
(out=, layout=, requires_grad=, a *_like of a tensor that is not contiguous) goes to the original function.
`misalign`: extra bytes in front of the body (rounded down to a multiple of the element size) for the entry points that promise no
alignment; entry points that require 16-byte alignment keep misalign = 0 (PAD is a multiple of 512).
`cpu=True` guards CPU tensors too (and those without a device): the arena's own arithmetic is tested without a GPU that way.
`guarded()` nests: an inner arena allocates from the unpatched torch, and the outer arena's functions are back when it exits.
"""
import contextlib

import torch

PAD = 4096
GUARD, BODY = 0xA5, 0xFF
PATCHED = ("empty", "zeros", "ones", "full", "empty_like", "zeros_like", "ones_like", "full_like")
_REAL = {name: getattr(torch, name) for name in PATCHED}       # torch's own, whatever arenas are live (this module is imported before any)
_UNMODELLED = ("out", "layout", "requires_grad", "names")


class RedzoneError(AssertionError):
    pass


class Arena(object):
    def __init__(self, misalign=0, cpu=False):
        self.blocks = []            # (raw uint8 tensor, body offset, body bytes, description)
        self.misalign = int(misalign)
        self.cpu = bool(cpu)
        self._empty = _REAL["empty"]

    # ---- which calls the arena takes -------------------------------------------------------------------------------------------------------------
    def _device(self, kw):
        """-> the device to carve the block on, or None: the call goes to the original function."""
        dev = kw.get("device")
        if kw.get("pin_memory") or kw.get("memory_format") not in (None, torch.contiguous_format) or any(kw.get(k) is not None and kw.get(k) is not False for k in _UNMODELLED):
            return None
        if dev is None:
            return torch.device("cpu") if self.cpu else None
        dev = torch.device(dev)
        return dev if dev.type == "cuda" or (self.cpu and dev.type == "cpu") else None

    @staticmethod
    def _shape(size):
        if len(size) == 1 and isinstance(size[0], (tuple, list, torch.Size)):
            return tuple(int(s) for s in size[0])
        return tuple(int(s) for s in size)

    def _carve(self, shape, dtype, dev, fill):
        """The block: guards, then the body as a contiguous `shape` tensor of `dtype`, filled with 0xFF bytes (fill None) or with `fill`."""
        item = self._empty((), dtype=dtype).element_size()
        n = 1
        for s in shape:
            n *= int(s)
        nbytes = n * item
        mis = (self.misalign // item) * item
        off = PAD + mis
        raw = self._empty((off + nbytes + PAD + 64,), dtype=torch.uint8, device=dev)
        raw.fill_(GUARD)
        t = raw[off:off + nbytes].view(dtype).view(shape)
        if fill is None:
            raw[off:off + nbytes].fill_(BODY)
        else:
            t.fill_(fill)
        self.blocks.append((raw, off, nbytes, "%s %s" % (str(dtype), shape)))
        return t

    def _new(self, name, size, fill, kw):
        dev = self._device(kw)
        if dev is None:
            return _REAL[name](*size, **kw) if name != "full" else _REAL[name](*size, fill, **kw)
        dtype = kw.get("dtype")
        if dtype is None:
            dtype = _REAL["full"]((), fill).dtype if name == "full" else torch.get_default_dtype()
        return self._carve(self._shape(size), dtype, dev, fill)

    def _like(self, name, t, fill, kw):
        dev = None
        if t.is_contiguous() and kw.get("memory_format") in (None, torch.preserve_format, torch.contiguous_format):
            dev = self._device(dict(kw, device=kw.get("device") or t.device, memory_format=None))
        if dev is None:
            return _REAL[name](t, **kw) if name != "full_like" else _REAL[name](t, fill, **kw)
        return self._carve(tuple(t.shape), kw.get("dtype") or t.dtype, dev, fill)

    # ---- torch's names ---------------------------------------------------------------------------------------------------------------------------
    def empty(self, *size, **kw):
        return self._new("empty", size, None, kw)

    def zeros(self, *size, **kw):
        return self._new("zeros", size, 0, kw)

    def ones(self, *size, **kw):
        return self._new("ones", size, 1, kw)

    def full(self, size, fill_value, **kw):
        return self._new("full", (size,), fill_value, kw)

    def empty_like(self, t, **kw):
        return self._like("empty_like", t, None, kw)

    def zeros_like(self, t, **kw):
        return self._like("zeros_like", t, 0, kw)

    def ones_like(self, t, **kw):
        return self._like("ones_like", t, 1, kw)

    def full_like(self, t, fill_value, **kw):
        return self._like("full_like", t, fill_value, kw)

    # ---- what the tests ask ----------------------------------------------------------------------------------------------------------------------
    def owns(self, t):
        """True when every byte t addresses lies inside the body of a live block (one made since the last check())."""
        if not isinstance(t, torch.Tensor):
            return False
        item = t.element_size()
        first = t.storage_offset() * item
        last = first + (sum((s - 1) * st for s, st in zip(t.shape, t.stride())) + 1) * item if t.numel() else first
        base = t.untyped_storage().data_ptr()
        for raw, off, nbytes, _ in self.blocks:
            if raw.untyped_storage().data_ptr() == base and raw.device == t.device and off <= first and last <= off + nbytes:
                return True
        return False

    @contextlib.contextmanager
    def patched(self):
        """torch's PATCHED names are this arena's for the duration, then what they were (an outer arena's included); no check on exit: for a
        second arena of another misalign next to guarded()'s, checked by hand."""
        before = {name: getattr(torch, name) for name in PATCHED}
        for name in PATCHED:
            setattr(torch, name, getattr(self, name))
        try:
            yield self
        finally:
            for name in PATCHED:
                setattr(torch, name, before[name])

    def check(self):
        if torch.cuda.is_available():
            torch.cuda.synchronize()
        bad = []
        for raw, off, nbytes, what in self.blocks:
            head, tail = raw[:off], raw[off + nbytes:]
            if not bool((head == GUARD).all()):
                i = int((head != GUARD).nonzero()[-1])
                bad.append("%s: %d byte(s) BEFORE the buffer overwritten (nearest: %d bytes before its start)" % (what, int((head != GUARD).sum()), off - i))
            if not bool((tail == GUARD).all()):
                i = int((tail != GUARD).nonzero()[0])
                bad.append("%s: %d byte(s) PAST the buffer overwritten (first: %d bytes past its end)" % (what, int((tail != GUARD).sum()), i))
        n = len(self.blocks)
        self.blocks = []
        if bad:
            raise RedzoneError("redzone violated:\n  " + "\n  ".join(bad))
        return n


@contextlib.contextmanager
def guarded(misalign=0, cpu=False):
    """with guarded() as arena: ...   -- patches torch's PATCHED names for the duration and puts back what they were, an outer arena's
    included; arena.check() runs on a clean exit (and can be called earlier; it returns the number of buffers it verified)."""
    arena = Arena(misalign, cpu=cpu)
    with arena.patched():
        yield arena
    arena.check()

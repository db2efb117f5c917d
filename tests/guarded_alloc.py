"""Guarded, poisoned allocations for the tests (test infrastructure only; the package never imports this).

Rule under test: a result never depends on bytes the call did not write, and no call writes outside its outputs and
its queried workspace.  Every wrapper of the package allocates its outputs and workspaces with ``torch.empty`` /
``torch.empty_like``; while a ``GuardedAlloc`` is active those two functions hand out, for the selected device, the
interior of a ``uint8`` slab of ``G + nbytes + G`` bytes that was filled with one pattern byte:

    [ G guard bytes | nbytes interior, viewed with the requested dtype / shape | G guard bytes ]

* an output tile or workspace slot the call never writes reads back as the pattern instead of as the previous call's
  (usually correct) value;
* a store before / past the interior lands in a guard and ``check()`` reports it;
* a test's inputs placed with ``guarded_from_numpy`` / ``guarded_clone`` are surrounded by the pattern too, so a load
  past either end reads poison.

The patterns are byte-repeating, so they hold at any size and alignment:

    0xFF  float32 / float64 NaN, byte 255, int64 -1
    0x7F  float32 +3.39e38, float64 +1.4e306, byte 127
    0xFE  float32 -1.69e38, float64 -5.4e303, byte 254

NaN alone is not enough: ``v > best``, ``fmaxf`` and ReLU swallow it; a huge finite value of either sign gets through.
Blind spots: a stray store farther than ``G`` from the interior, a store of the pattern's own byte value (hence three
patterns), and an out-of-extent load whose value is discarded.

Plain torch: nothing here inspects code objects, names an instruction, or touches the environment or process start-up.
"""
import os
import sys

import numpy as np
import pytest
import torch

G = 4096  # guard bytes on either side: a multiple of 256 keeps the interior's alignment; wider than one wave's widest store
PATTERNS = (0xFF, 0x7F, 0xFE)
PATTERN_IDS = ["0xFF", "0x7F", "0xFE"]

_THIS_FILE = os.path.abspath(__file__)
_TORCH_DIR = os.path.dirname(os.path.abspath(torch.__file__))
_ITEMSIZE = {}


def _itemsize(dtype):
    if dtype not in _ITEMSIZE:
        _ITEMSIZE[dtype] = torch.tensor([], dtype=dtype).element_size()
    return _ITEMSIZE[dtype]


def _call_site():
    """file:line (function) of the nearest frame that is neither this module nor torch: the wrapper that allocated"""
    f = sys._getframe(1)
    while f is not None:
        path = os.path.abspath(f.f_code.co_filename)
        if path != _THIS_FILE and not path.startswith(_TORCH_DIR):
            return "%s:%d (%s)" % (os.path.relpath(path, os.path.dirname(os.path.dirname(_THIS_FILE))), f.f_lineno,
                                   f.f_code.co_name)
        f = f.f_back
    return "<unknown>"


def _shape_of(size):
    if len(size) == 1 and not isinstance(size[0], (int, np.integer)):
        size = tuple(size[0])
    return tuple(int(s) for s in size)


class GuardViolation(AssertionError):
    """``violations``: one dict per damaged guard -- index, kind, shape, dtype, site, side ("front" | "rear"), count,
    first_offset / last_offset (bytes relative to the interior: the front guard is -G .. -1, the rear guard counts from
    the interior's end, 0 .. G-1) and first_value / last_value (the bytes found there)."""

    def __init__(self, violations, pattern):
        self.violations = violations
        lines = ["%d guard(s) no longer hold the pattern 0x%02X:" % (len(violations), pattern)]
        for v in violations:
            where = ("%d .. %d bytes before the interior" % (-v["first_offset"], -v["last_offset"]) if v["side"] == "front"
                     else "%d .. %d bytes past the interior's end" % (v["first_offset"], v["last_offset"]))
            lines.append("  #%d %s shape=%s dtype=%s (%d bytes) allocated at %s: %s guard, %d byte(s) changed, offsets %d "
                         ".. %d (%s); first 0x%02X, last 0x%02X"
                         % (v["index"], v["kind"], v["shape"], v["dtype"], v["nbytes"], v["site"], v["side"], v["count"],
                            v["first_offset"], v["last_offset"], where, v["first_value"], v["last_value"]))
        super().__init__("\n".join(lines))


class _Slab:
    __slots__ = ("index", "slab", "nbytes", "shape", "dtype", "site", "kind")

    def __init__(self, index, slab, nbytes, shape, dtype, site, kind):
        self.index, self.slab, self.nbytes, self.shape, self.dtype, self.site, self.kind = (
            index, slab, nbytes, shape, dtype, site, kind)


class GuardedAlloc:
    """Context manager: ``with GuardedAlloc("cuda", 0x7F) as g: ...; g.check()``.

    ``device``: the device whose allocations are guarded ("cpu" for the self-tests; "cuda" = the current GPU at the time
    of each allocation).  Allocations for any other device -- CPU and pinned memory when a GPU is selected -- go to the
    original functions untouched, as do requests the slab cannot represent (``out=``, a sparse layout, a channels-last
    memory format).  Every slab stays alive until the context exits (or ``release()``), so a workspace a wrapper dropped
    on return is still checked."""

    def __init__(self, device, pattern=0xFF, guard=G):
        self.device = torch.device(device)
        self.pattern = int(pattern)
        if not 0 <= self.pattern <= 255:
            raise ValueError("pattern must be one byte")
        if guard <= 0 or guard % 256:
            raise ValueError("guard must be a positive multiple of 256")
        self.guard = int(guard)
        self.count = 0      # allocations that went through the patched torch.empty / torch.empty_like
        self._slabs = []
        self._next = 0
        self._orig = None

    # ---- patching ----
    def __enter__(self):
        if self._orig is not None:
            raise RuntimeError("GuardedAlloc is not re-entrant")
        if getattr(torch.empty, "_guarded_alloc", False):
            raise RuntimeError("another GuardedAlloc is active")
        self._orig = (torch.empty, torch.empty_like)
        torch.empty, torch.empty_like = self._make_empty(), self._make_empty_like()
        return self

    def __exit__(self, *exc):
        torch.empty, torch.empty_like = self._orig
        self._orig = None
        self._slabs = []
        return False

    def _selected(self, device):
        if device is None:
            device = torch.get_default_device() if hasattr(torch, "get_default_device") else torch.device("cpu")
        device = torch.device(device)
        if device.type != self.device.type:
            return None
        if device.type == "cuda":
            if device.index is None:
                device = torch.device("cuda", torch.cuda.current_device())
            if self.device.index is not None and device.index != self.device.index:
                return None
        return device

    def _make_empty(self):
        orig = self._orig[0]

        def empty(*size, **kw):
            device = self._selected(kw.get("device"))
            plain = (device is not None and not kw.get("pin_memory") and kw.get("out") is None and "names" not in kw
                     and kw.get("layout", torch.strided) == torch.strided
                     and kw.get("memory_format", torch.contiguous_format) == torch.contiguous_format)
            if not plain:
                return orig(*size, **kw)
            if not size and "size" in kw:
                size = (kw["size"],)
            dtype = kw.get("dtype") or torch.get_default_dtype()
            t = self._alloc(_shape_of(size), dtype, device, "empty")
            self.count += 1
            return t.requires_grad_() if kw.get("requires_grad") else t

        empty._guarded_alloc = True
        return empty

    def _make_empty_like(self):
        orig = self._orig[1]

        def empty_like(input, **kw):
            device = self._selected(kw.get("device", input.device))
            plain = (device is not None and not kw.get("pin_memory") and kw.get("layout", torch.strided) == torch.strided
                     and input.layout == torch.strided
                     and kw.get("memory_format", torch.preserve_format) in (torch.preserve_format, torch.contiguous_format))
            if not plain:
                return orig(input, **kw)
            t = self._alloc(tuple(input.shape), kw.get("dtype") or input.dtype, device, "empty_like")
            self.count += 1
            return t.requires_grad_() if kw.get("requires_grad") else t

        empty_like._guarded_alloc = True
        return empty_like

    # ---- slabs ----
    def _raw_empty(self, *a, **kw):
        return (self._orig[0] if self._orig is not None else torch.empty)(*a, **kw)

    def _alloc(self, shape, dtype, device, kind):
        if any(s < 0 for s in shape):
            raise RuntimeError("negative dimension in %s" % (shape,))
        nbytes = int(np.prod(shape, dtype=np.int64)) * _itemsize(dtype)
        slab = self._raw_empty(self.guard + nbytes + self.guard, dtype=torch.uint8, device=device)
        slab.fill_(self.pattern)
        self._slabs.append(_Slab(self._next, slab, nbytes, shape, dtype, _call_site(), kind))
        self._next += 1
        return slab[self.guard:self.guard + nbytes].view(dtype).view(shape)

    def guarded_from_numpy(self, a):
        """a test INPUT on the selected device, surrounded by the pattern (a load past either end reads poison)"""
        a = np.ascontiguousarray(a)
        src = torch.from_numpy(a if a.flags.writeable else a.copy())
        dev = self._selected(self.device)
        t = self._alloc(tuple(a.shape), src.dtype, dev, "input")
        t.copy_(src)
        return t

    def guarded_clone(self, t):
        dev = self._selected(self.device)
        out = self._alloc(tuple(t.shape), t.dtype, dev, "input")
        out.copy_(t)
        return out

    def _find(self, t):
        if not isinstance(t, torch.Tensor):
            return None
        base, off = t.untyped_storage().data_ptr(), t.storage_offset() * t.element_size()
        for s in self._slabs:
            if s.slab.untyped_storage().data_ptr() == base and self.guard <= off <= self.guard + s.nbytes:
                return s
        return None

    def is_guarded(self, t):
        """True when ``t`` is (a view into) the interior of a live slab of this harness"""
        return self._find(t) is not None

    def refill(self, t):
        """write the pattern over the whole interior ``t`` lives in (a cached workspace between two calls)"""
        s = self._find(t)
        if s is None:
            raise ValueError("refill: not a guarded tensor")
        s.slab[self.guard:self.guard + s.nbytes].fill_(self.pattern)

    def release(self):
        """forget every slab allocated so far (after ``check()``), so the memory can be reused"""
        self._slabs = []

    @property
    def live(self):
        return len(self._slabs)

    # ---- the check ----
    def check(self):
        """synchronise, then assert that both guards of every live slab still hold the pattern"""
        if self.device.type == "cuda":
            torch.cuda.synchronize()
        if not self._slabs:
            return
        g = self.guard
        guards = torch.cat([torch.cat((s.slab[:g], s.slab[g + s.nbytes:])) for s in self._slabs])
        if not bool((guards != self.pattern).any()):
            return
        bad = (guards != self.pattern).view(len(self._slabs), 2, g).cpu().numpy()
        vals = guards.view(len(self._slabs), 2, g).cpu().numpy()
        violations = []
        for i, s in enumerate(self._slabs):
            for side, name, origin in ((0, "front", -g), (1, "rear", 0)):
                idx = np.flatnonzero(bad[i, side])
                if idx.size:
                    violations.append({"index": s.index, "kind": s.kind, "shape": s.shape, "dtype": s.dtype, "site": s.site,
                                       "nbytes": s.nbytes, "side": name, "count": int(idx.size),
                                       "first_offset": int(idx[0]) + origin, "last_offset": int(idx[-1]) + origin,
                                       "first_value": int(vals[i, side, idx[0]]), "last_value": int(vals[i, side, idx[-1]])})
        raise GuardViolation(violations, self.pattern)


def pattern_values(pattern):
    """what one interior element reads as before anything wrote it: {"float32", "float64", "uint8", "int64"}"""
    b = np.full(8, pattern, dtype=np.uint8)
    return {"float32": b[:4].view(np.float32)[0], "float64": b.view(np.float64)[0], "uint8": b[0], "int64": b.view(np.int64)[0]}


def same_bits(a, b):
    """bit equality of two tensors / arrays (NaN == NaN when the payloads agree); shapes and dtypes must match too"""
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    b = b.detach().cpu().numpy() if isinstance(b, torch.Tensor) else np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


@pytest.fixture
def guarded_alloc():
    """factory fixture: ``g = guarded_alloc(device, pattern)`` enters a GuardedAlloc (leaving the one the same test made
    before, if any); the last one is left at teardown, also when the test failed.  Import it into the test module that
    wants it (no conftest.py declares it)."""
    active = []

    def make(device, pattern=0xFF, guard=G):
        while active:
            active.pop().__exit__(None, None, None)
        g = GuardedAlloc(device, pattern, guard)
        g.__enter__()
        active.append(g)
        return g

    yield make
    while active:
        active.pop().__exit__(None, None, None)

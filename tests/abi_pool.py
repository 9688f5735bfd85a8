"""One device pool with guards, for the tests that call the C ABI the way a C caller does (tests/test_gpu_abi_buffers.py,
tests/test_gpu_abi_streams.py; include/arap_opt.h states the contract).

Every buffer of a call -- inputs, outputs, scratch -- is carved out of ONE uint8 array filled with 0xA5:
  * a buffer sits at the alignment asked for and no more: its address is a multiple of `align` and, unless `align` is
    already 256 or more, not a multiple of 2 * align (a buffer asked at 1 sits on an odd address);
  * at least GUARD bytes stand before the first buffer, between any two, and after the last.  GUARD is a condition, not
    a measurement: it is far wider than any single stray row or 256-byte rounding;
  * scratch and outputs are carved with exactly the bytes asked and left holding 0xA5, so a pixel a kernel forgets shows
    against the twin and a call that relies on clean scratch meets junk;
  * an output passed as NULL is not carved at all: it has no bytes of its own, every byte it could be mistaken for is guard.
check() then asserts that every guard byte still holds 0xA5 and every input still holds the bytes uploaded.

The arithmetic (Layout) is plain integers and knows no device; Pool puts it over a numpy array (the CPU test of
tests/test_abi_host.py) or over a CUDA tensor.  The storage's base is aligned to BASE, so the offsets' residues are the
addresses'."""
import numpy as np

GUARD = 4096
FILL = 0xA5
BASE = 512                   # what the storage's first byte is aligned to (torch's allocator gives 512)
KINDS = ("input", "output", "scratch")


def place(cursor, align):
    """the first offset >= cursor + GUARD that is a multiple of `align` and, for align < 256, an odd multiple of it"""
    assert align >= 1 and align & (align - 1) == 0, "alignment: a power of two"
    o = -(-(cursor + GUARD) // align) * align
    if align < 256 and o % (2 * align) == 0:
        o += align
    return o


class Layout:
    """offsets of the buffers of one pool: add() them in any order, then `total` bytes hold them and their guards"""

    def __init__(self):
        self.parts = {}              # name -> (offset, nbytes, align, kind)
        self.end = 0                 # one past the last buffer's last byte

    def add(self, name, nbytes, align, kind):
        assert kind in KINDS and name not in self.parts and nbytes > 0, (name, nbytes, kind)
        o = place(self.end, align)
        self.parts[name] = (o, int(nbytes), int(align), kind)
        self.end = o + int(nbytes)
        return o

    @property
    def total(self):
        return self.end + GUARD

    def guard_mask(self):
        """bool[total]: True on every byte that belongs to no buffer"""
        m = np.ones(self.total, bool)
        for o, n, _, _ in self.parts.values():
            m[o:o + n] = False
        return m


class Pool:
    """Layout + storage.  carve() every buffer, allocate(), upload() the inputs, hand out ptr()s, call, check()."""

    def __init__(self, device="cuda"):
        self.layout = Layout()
        self.device = device
        self.store = None            # uint8 numpy array or CUDA tensor of layout.total bytes, BASE-aligned
        self.expected = {}           # input name -> the bytes uploaded
        self._keep = None

    def carve(self, name, nbytes, align, kind):
        assert self.store is None, "carve before allocate"
        return self.layout.add(name, nbytes, align, kind)

    def allocate(self):
        n = self.layout.total
        if self.device == "numpy":
            self._keep = np.empty(n + BASE, np.uint8)
            skip = -self._keep.ctypes.data % BASE
            self.store = self._keep[skip:skip + n]
            self.store[:] = FILL
        else:
            import torch
            self.store = torch.full((n,), FILL, dtype=torch.uint8, device=self.device)
        assert self.base % BASE == 0, "the storage's base is %d-byte aligned" % BASE
        return self

    @property
    def base(self):
        return self.store.ctypes.data if self.device == "numpy" else self.store.data_ptr()

    def span(self, name):
        o, n, _, _ = self.layout.parts[name]
        return o, n

    def ptr(self, name):
        """the buffer's address; None (NULL) for a name that was not carved"""
        if name not in self.layout.parts:
            return None
        o, n, align, _ = self.layout.parts[name]
        p = self.base + o
        assert p % align == 0 and (align >= 256 or p % (2 * align) != 0)
        return p

    def view(self, name):
        """the buffer's bytes in the storage itself (a numpy or tensor slice)"""
        o, n = self.span(name)
        return self.store[o:o + n]

    @staticmethod
    def raw(array):
        return np.frombuffer(np.ascontiguousarray(array).tobytes(), np.uint8)

    def expect(self, name, array):
        """what check() must find in input `name`"""
        b = self.raw(array)
        assert self.layout.parts[name][3] == "input" and b.size == self.layout.parts[name][1], name
        self.expected[name] = b

    def upload(self, name, array):
        """write an input's bytes (on the current stream, from pageable memory) and expect them at check()"""
        self.expect(name, array)
        b = self.expected[name]
        if self.device == "numpy":
            self.view(name)[:] = b
        else:
            import torch
            self.view(name).copy_(torch.from_numpy(b.copy()))

    def snapshot(self):
        """the whole pool as a numpy array (the caller has synchronised)"""
        return self.store.copy() if self.device == "numpy" else self.store.cpu().numpy()

    def read(self, name, snap=None):
        o, n = self.span(name)
        return (self.snapshot() if snap is None else snap)[o:o + n].copy()

    def check(self, snap=None, pristine=False):
        """every guard byte 0xA5, every input the bytes uploaded; `pristine`: every output and the scratch 0xA5 too (what a
        refused call leaves).  Raises AssertionError naming the first fault."""
        snap = self.snapshot() if snap is None else snap
        assert snap.shape == (self.layout.total,)
        bad = np.flatnonzero((snap != FILL) & self.layout.guard_mask())
        if bad.size:
            raise AssertionError("%d guard bytes overwritten, the first at offset %d: %s" % (bad.size, bad[0], self.where(int(bad[0]))))
        for name, (o, n, _, kind) in self.layout.parts.items():
            if kind == "input":
                assert name in self.expected, "input %s was never uploaded" % name
                diff = np.flatnonzero(snap[o:o + n] != self.expected[name])
                assert not diff.size, "input %s: %d bytes changed, the first at byte %d" % (name, diff.size, diff[0])
            elif pristine:
                diff = np.flatnonzero(snap[o:o + n] != FILL)
                assert not diff.size, "%s %s: %d bytes written, the first at byte %d" % (kind, name, diff.size, diff[0])

    def where(self, offset):
        """an offset in words: which buffers it lies between"""
        before = [(o + n, name) for name, (o, n, _, _) in self.layout.parts.items() if o + n <= offset]
        after = [(o, name) for name, (o, n, _, _) in self.layout.parts.items() if o > offset]
        b, a = max(before, default=None), min(after, default=None)
        return "%s%s" % ("%d bytes past the end of %s" % (offset - b[0], b[1]) if b else "before the first buffer",
                         ", %d bytes before %s" % (a[0] - offset, a[1]) if a else "")

"""Helpers shared by the -m gpu parity tests (HIP path vs oracle on identical seeded inputs)."""
import numpy as np
import torch


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def host(t):
    return t.detach().cpu().numpy()


def rel_linf(a, b):
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def rel_l1(a, b):
    """The north-star metric: sum|a-b| / sum|b|."""
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    return float(np.abs(a - b).sum() / max(np.abs(b).sum(), 1e-30))


# ---- guarded device buffers (raw C-ABI tests: test_gpu_elementwise.py, test_gpu_stencil_edges.py) ---------------------------------------
class Out(object):
    """An output buffer: NaN everywhere, the tensor in front, a guard of one row (last extent) or one element behind it."""

    def __init__(self, shape, data=None):
        self.shape = tuple(shape)
        self.n = int(np.prod(self.shape)) if self.shape else 1
        self.buf = torch.full((self.n + (self.shape[-1] if self.shape else 1),), float("nan"), dtype=torch.float32, device="cuda")
        if data is not None:
            self.buf[:self.n] = torch.from_numpy(np.array(data, dtype=np.float32)).cuda().reshape(-1)
        self.ptr = self.buf.data_ptr()

    def get(self):
        assert bool(torch.isnan(self.buf[self.n:]).all()), "the guard behind the output was written"
        return host(self.buf[:self.n]).reshape(self.shape)


def assert_bits(got, want, what=""):
    """equal bit for bit: distinguishes -0.0 from +0.0, and a NaN left from the pre-fill never matches"""
    got = np.ascontiguousarray(got, np.float32); want = np.ascontiguousarray(want, np.float32)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = got.view(np.int32) != want.view(np.int32)
    if bad.any():
        i = np.unravel_index(int(np.argmax(bad)), bad.shape)
        raise AssertionError("%s: %d of %d elements differ, first at %s: got %r, want %r" % (what, int(bad.sum()), bad.size, i, got[i], want[i]))


GUARD = 64                  # floats per guard zone: 256 bytes, so the payload behind the front guard keeps the allocation's 16-byte alignment
NAN_BITS = 0x7FC5A5A5       # the fill: a quiet NaN with a payload no kernel produces


class Guarded(object):
    """``shape`` floats inside a larger allocation that holds NAN_BITS everywhere: GUARD floats in front, the payload, GUARD floats
    behind.  ``offset`` (floats) shifts the payload: 0 = 16-byte aligned, 1 = 4-byte aligned and not 8-byte aligned.  ``data`` fills
    the payload (an input operand); without it the payload is NaN too (an output, or a workspace).  The object owns the allocation:
    keep it in a named variable until the result has been read."""

    def __init__(self, shape, data=None, offset=0):
        self.shape = tuple(shape)
        self.n = int(np.prod(self.shape)) if self.shape else 1
        self.lo = GUARD + int(offset)
        self.bits = torch.full((self.lo + self.n + GUARD,), NAN_BITS, dtype=torch.int32, device="cuda")
        self.buf = self.bits.view(torch.float32)
        if data is not None:
            self.buf[self.lo:self.lo + self.n] = torch.from_numpy(np.array(data, dtype=np.float32)).cuda().reshape(-1)
        self.ptr = self.buf.data_ptr() + 4 * self.lo
        assert self.buf.data_ptr() % 16 == 0 and self.ptr % 16 == (4 * offset) % 16

    def payload(self):
        return self.buf[self.lo:self.lo + self.n]

    def refill(self):
        """the payload back to NaN (a workspace between two calls)"""
        self.bits[self.lo:self.lo + self.n] = NAN_BITS

    def check_guards(self, what=""):
        front, back = self.bits[:self.lo], self.bits[self.lo + self.n:]
        assert bool((front == NAN_BITS).all()), "%s: the guard in front of the buffer was written" % what
        assert bool((back == NAN_BITS).all()), "%s: the guard behind the buffer was written" % what

    def untouched(self):
        return bool((self.bits == NAN_BITS).all())

    def raw(self, what=""):
        """guards intact -> the payload's int32 words as a host array, NAN_BITS still in it wherever nothing was written (a strided
        output whose gaps must keep the fill; rows of fp64 halves, which may look like a NaN; results that hold a NaN on purpose)"""
        self.check_guards(what)
        return host(self.bits[self.lo:self.lo + self.n]).reshape(self.shape)

    def get(self, what=""):
        """guards intact, no NaN left inside -> the payload as a host array"""
        self.check_guards(what)
        got = host(self.payload()).reshape(self.shape)
        assert not np.isnan(got).any(), "%s: %d of %d elements were never written" % (what, int(np.isnan(got).sum()), got.size)
        return got


# ---- the byte and integer siblings of Guarded (tests/test_gpu_particle_edges.py: marks, flags, keep bytes; keys, ranges, counts, the sort order)
BYTE_FILL = 0xA5            # no mark, flags byte or keep byte of the tests takes this value
WORD_FILL = 0x5A5A5A5A      # no key, range, count or row index of the tests takes this value (int64: the word twice)


class _GuardedInts(object):
    """``shape`` elements of ``dtype`` inside a larger allocation that holds ``fill`` everywhere: 256 bytes in front, the payload, 256 bytes
    behind.  ``offset`` (elements) shifts the payload.  ``data`` fills the payload (an input operand); without it the payload holds the fill
    too (an output).  The object owns the allocation: keep it in a named variable until the result has been read."""
    dtype, fill = None, None

    def __init__(self, shape, data=None, offset=0):
        self.shape = tuple(shape)
        self.n = int(np.prod(self.shape)) if self.shape else 1
        size = torch.empty((), dtype=self.dtype).element_size()
        guard = 4 * GUARD // size
        self.lo = guard + int(offset)
        self.bits = torch.full((self.lo + self.n + guard,), self.fill, dtype=self.dtype, device="cuda")
        if data is not None:
            self.bits[self.lo:self.lo + self.n] = torch.from_numpy(np.ascontiguousarray(data).reshape(-1)).to(self.dtype).cuda()
        self.ptr = self.bits.data_ptr() + size * self.lo
        assert self.bits.data_ptr() % 16 == 0 and self.ptr % 16 == (size * offset) % 16

    def payload(self):
        return self.bits[self.lo:self.lo + self.n]

    def refill(self):
        self.bits[self.lo:self.lo + self.n] = self.fill

    def check_guards(self, what=""):
        front, back = self.bits[:self.lo], self.bits[self.lo + self.n:]
        assert bool((front == self.fill).all()), "%s: the guard in front of the buffer was written" % what
        assert bool((back == self.fill).all()), "%s: the guard behind the buffer was written" % what

    def raw(self, what=""):
        """guards intact -> the payload as a host array, the fill still in it wherever nothing was written"""
        self.check_guards(what)
        return host(self.payload()).reshape(self.shape)

    def get(self, what=""):
        """guards intact, no fill left inside -> the payload as a host array"""
        got = self.raw(what)
        left = int((got == self.fill).sum())
        assert left == 0, "%s: %d of %d elements were never written" % (what, left, got.size)
        return got


class GuardedBytes(_GuardedInts):
    dtype, fill = torch.uint8, BYTE_FILL


class GuardedInts(_GuardedInts):
    dtype, fill = torch.int32, WORD_FILL


class GuardedLongs(_GuardedInts):
    dtype, fill = torch.int64, (WORD_FILL << 32) | WORD_FILL

"""Guarded buffers: what a call writes outside the tensor it was given, and what it needs of that tensor's alignment.

`guarded(torch, n, shift, device, like=None)` allocates ONE int64 buffer of G + shift + n + G words, every word the bit pattern
SENTINEL (a quiet NaN with a payload: arithmetic gives the canonical NaN, never this one), and views it as float64.  The payload is
buf[G + shift : G + shift + n]; G = max(65536, n) rounded up to even, so the guards are at least as long as the payload itself and an
overrun of up to one whole output length in either direction lands in a guard.  Allocations are at least 16-byte aligned and G is
even, so the payload starts at an odd multiple of 8 bytes when `shift` is odd and at a multiple of 16 when it is even (asserted).
`like` (a tensor or an array of n doubles) is copied into the payload: an input.

Every comparison is made on the int64 view, so NaN compares like any other bit pattern:
  guards_intact()   both guards still hold the sentinel; otherwise an AssertionError with the first and last touched offsets
                    relative to the payload (negative: before it; >= n: past its end) and the number of touched words
  unwritten()       the payload positions that still hold the sentinel
  snapshot() / unchanged()   the whole buffer's bits, for inputs

WHAT THIS CANNOT SEE: a store further than G doubles from the payload -- from a wrapped 32-bit index, say -- lands in somebody
else's memory, not in a guard.  A store of the sentinel's own bits is invisible too.

Device-agnostic: torch is passed in, nothing is imported here, the same code guards CPU tensors (tests/test_guarded_cpu.py) and
device tensors (tests/test_gpu_write_sets.py).
"""
SENTINEL = 0x7FF8C7D15EED0001
MIN_GUARD = 65536


def guard_len(n):
    g = max(MIN_GUARD, int(n))
    return g + (g & 1)


class Guarded:
    def __init__(self, torch, n, shift, device, like=None):
        self.torch, self.n, self.shift = torch, int(n), int(shift)
        self.G = guard_len(n)
        self.lo = self.G + self.shift                   # first word of the payload
        self.buf = torch.full((self.lo + self.n + self.G,), SENTINEL, dtype=torch.int64, device=device)
        self.view = self.buf.view(torch.float64)[self.lo:self.lo + self.n]
        assert self.buf.data_ptr() % 16 == 0, "the allocation itself is 16-byte aligned"
        if self.n:                                      # (an empty tensor has no address)
            assert self.view.data_ptr() == self.buf.data_ptr() + 8 * self.lo
            assert self.view.data_ptr() % 16 == (8 if self.shift % 2 else 0), (self.view.data_ptr(), shift)
        if like is not None:
            src = like if hasattr(like, "is_cuda") else torch.from_numpy(like)
            assert src.numel() == self.n and src.dtype == torch.float64
            self.view.copy_(src.reshape(-1))
        self._snap = None

    def bits(self):
        """the payload as int64"""
        return self.buf[self.lo:self.lo + self.n]

    def touched(self):
        """offsets, relative to the payload, of the guard words that no longer hold the sentinel (ascending)"""
        torch = self.torch
        hi = self.lo + self.n
        below = torch.nonzero(self.buf[:self.lo] != SENTINEL).flatten() - self.lo
        above = torch.nonzero(self.buf[hi:] != SENTINEL).flatten() + self.n
        return torch.cat([below, above]).cpu().tolist()

    def guards_intact(self, what=""):
        hi = self.lo + self.n
        if bool((self.buf[:self.lo] == SENTINEL).all()) and bool((self.buf[hi:] == SENTINEL).all()):
            return True
        t = self.touched()
        raise AssertionError(f"{what}: {len(t)} guard word(s) written, offsets {t[0]} .. {t[-1]} relative to a payload of {self.n} "
                             f"(shift {self.shift}, guards of {self.G})")

    def unwritten(self):
        return self.torch.nonzero(self.bits() == SENTINEL).flatten().cpu().tolist()

    def snapshot(self):
        self._snap = self.buf.clone()
        return self

    def unchanged(self, what=""):
        assert self._snap is not None, "snapshot() first"
        if self.torch.equal(self.buf, self._snap):
            return True
        t = (self.torch.nonzero(self.buf != self._snap).flatten() - self.lo).cpu().tolist()
        raise AssertionError(f"{what}: {len(t)} word(s) of an input buffer changed, offsets {t[0]} .. {t[-1]} relative to a payload of "
                             f"{self.n} (shift {self.shift}, guards of {self.G})")


def guarded(torch, n, shift, device, like=None):
    return Guarded(torch, n, shift, device, like)

"""Tensors carved out of ONE flat buffer, each at a chosen offset from a 16-byte boundary and between two red zones.

The kernels choose their code path from `pointer & 15` and from whether a size divides by 4 or 8; a tensor that comes straight
from torch's allocator is 256-byte aligned and is followed by slack nobody looks at.  An Arena hands out contiguous views whose
address modulo 16 the test picks, and surrounds every view with RED_ZONE bytes of a known content on each side:

  * around an INPUT the test chooses the content so that a kernel which reads past the view and USES the value gives a wrong
    result (NaN for sums and products, +inf for max-pools, a copy of the first centre for a nearest-neighbour search, and
    for index inputs an IN-RANGE index, so that a stray read never turns into a stray gather);
  * around an OUTPUT the content is a fixed bit pattern, and check() asserts that every red zone of the arena still holds
    bit for bit what it was filled with: a write past either end of any view is seen, whichever view it came from.

A red zone is larger than any tile a kernel of this library moves at once, so an overrun of a whole tile stays inside the
arena.  Works on CPU tensors as well (tests/test_arena_host.py).  A helper module like detector_case.py: no fixtures here.
"""
import numpy as np
import torch

RED_ZONE = 64 * 1024            # bytes on each side of every view; a multiple of 16 and of every element size
OUT_BYTE = 0xA5                 # the fixed pattern of an output's red zones (as fp32: -2.87e-16, as int32: negative)


class Arena:
    def __init__(self, dev, nbytes=32 << 20):
        self.buf = torch.full((nbytes + 16,), OUT_BYTE, dtype=torch.uint8, device=dev)
        self.origin = -self.buf.data_ptr() % 16     # first 16-byte boundary of the buffer
        self.reset()

    def reset(self):
        """Forget every view and red zone; the buffer is handed out again from its start."""
        self.cursor = self.origin
        self.zones = []         # (lo, hi, expected bytes) of every red zone
        self.views = []         # (lo, hi) of every view

    def carve(self, shape, dtype, misalign_bytes=0, poison=None):
        """A contiguous `shape` view of `dtype` with data_ptr() % 16 == misalign_bytes and RED_ZONE bytes on each side.
        poison: None = the output pattern; a number = that value in the view's dtype; a sequence = that pattern repeated in
        phase with the view (red-zone element i, counted from the view's first element and negative in front of it, holds
        pattern[i mod len]: a flat (n, 3) coordinate table is continued by whole points).  The view itself is NOT filled."""
        if isinstance(shape, int):
            shape = (shape,)
        item = torch.empty((), dtype=dtype).element_size()
        assert 0 <= misalign_bytes < 16 and misalign_bytes % item == 0, (misalign_bytes, item)
        numel = int(np.prod(shape)) if len(shape) else 1
        lo = self.cursor + RED_ZONE + misalign_bytes           # cursor is a 16-byte boundary
        hi = lo + numel * item
        end = hi + RED_ZONE
        assert end <= self.buf.numel(), f"arena of {self.buf.numel()} bytes is full (this view ends at {end})"
        self.cursor = end + (-end % 16)
        if misalign_bytes:                                      # the bytes between the boundary and the zone stay OUT_BYTE
            self._zone(lo - RED_ZONE - misalign_bytes, lo - RED_ZONE, None, dtype, 0)
        self._zone(lo - RED_ZONE, lo, poison, dtype, -(RED_ZONE // item))
        self._zone(hi, end, poison, dtype, numel)
        self.views.append((lo, hi))
        view = self.buf[lo:hi].view(dtype).view(*shape)
        assert view.data_ptr() % 16 == misalign_bytes and view.is_contiguous()
        return view

    def put(self, src, misalign_bytes=0, poison=None):
        """carve() a view shaped and typed like `src` (a tensor or a numpy array) and copy it in."""
        src = torch.as_tensor(src)
        view = self.carve(tuple(src.shape), src.dtype, misalign_bytes, poison)
        view.copy_(src)
        return view

    def _zone(self, lo, hi, poison, dtype, first_index):
        z = self.buf[lo:hi]
        if poison is None:
            z.fill_(OUT_BYTE)
        elif np.ndim(poison) == 0:
            z.view(dtype).fill_(poison)
        else:
            pat = torch.as_tensor(poison).to(dtype).flatten().cpu()
            n = z.numel() // pat.element_size()
            k = (torch.arange(first_index, first_index + n) % pat.numel())
            z.view(dtype).copy_(pat[k])
        self.zones.append((lo, hi, z.clone()))

    def check(self):
        """Assert that every red zone holds, bit for bit, what it was filled with."""
        if not self.zones:
            return
        bad = torch.stack([(self.buf[lo:hi] != want).any() for lo, hi, want in self.zones]).cpu()
        for (lo, hi, want), b in zip(self.zones, bad.tolist()):
            if b:
                at = int((self.buf[lo:hi] != want).nonzero()[0])
                owner = min(self.views, key=lambda v: min(abs(v[0] - hi), abs(lo - v[1])))
                side = "in front of" if hi <= owner[0] else "behind"
                raise AssertionError(f"red zone [{lo}, {hi}) {side} the view [{owner[0]}, {owner[1]}) was written: "
                                     f"first changed byte at arena offset {lo + at}")

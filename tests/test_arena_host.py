"""tests/arena.py on CPU tensors: the carved offsets, the red zones' contents and what check() notices."""
import numpy as np
import pytest
import torch

from arena import OUT_BYTE, RED_ZONE, Arena


@pytest.mark.parametrize("dtype,offsets", [(torch.float32, [0, 4, 8, 12]), (torch.int32, [0, 4, 8, 12]),
                                           (torch.bfloat16, [0, 2, 8, 14]), (torch.uint8, [0, 1, 4, 15]),
                                           (torch.int64, [0, 8])])
def test_carved_views_sit_where_asked_between_whole_red_zones(dtype, offsets):
    a = Arena("cpu", 4 << 20)
    spans = []
    for k, off in enumerate(offsets):
        v = a.carve((3, 5 + k), dtype, off)
        assert v.data_ptr() % 16 == off and v.is_contiguous() and v.dtype == dtype and v.shape == (3, 5 + k)
        lo = v.data_ptr() - a.buf.data_ptr()
        spans.append((lo, lo + v.numel() * v.element_size()))
        v.fill_(1)                                              # writing the whole view touches no red zone
    a.check()
    for (lo, hi), nxt in zip(spans, spans[1:] + [(a.buf.numel() + RED_ZONE, None)]):
        assert bool((a.buf[lo - RED_ZONE:lo] == OUT_BYTE).all()) and bool((a.buf[hi:hi + RED_ZONE] == OUT_BYTE).all())
        assert nxt[0] - hi >= 2 * RED_ZONE or nxt[1] is None    # neighbours never share a red zone


def test_misaligned_offsets_must_be_whole_elements():
    a = Arena("cpu", 1 << 20)
    with pytest.raises(AssertionError):
        a.carve(4, torch.float32, 2)
    with pytest.raises(AssertionError):
        a.carve(4, torch.bfloat16, 3)
    with pytest.raises(AssertionError):
        a.carve(4, torch.float32, 16)


def test_a_full_arena_refuses_instead_of_overlapping():
    a = Arena("cpu", 4 * RED_ZONE)
    a.carve(16, torch.float32)
    with pytest.raises(AssertionError, match="full"):
        a.carve(RED_ZONE, torch.float32)


def test_scalar_poison_fills_both_zones_in_the_views_type():
    a = Arena("cpu", 1 << 20)
    v = a.put(np.arange(7, dtype=np.float32), 4, poison=float("nan"))
    lo = v.data_ptr() - a.buf.data_ptr()
    front = a.buf[lo - RED_ZONE:lo].view(torch.float32)
    back = a.buf[lo + 28:lo + 28 + RED_ZONE].view(torch.float32)
    assert bool(torch.isnan(front).all()) and bool(torch.isnan(back).all())
    assert torch.equal(v, torch.arange(7, dtype=torch.float32))
    a.check()                                                   # NaN zones compare by bits, not by value
    i = a.put(np.array([5, 6], dtype=np.int32), 8, poison=3)
    lo = i.data_ptr() - a.buf.data_ptr()
    assert bool((a.buf[lo - RED_ZONE:lo].view(torch.int32) == 3).all()) and bool((a.buf[lo + 8:lo + 8 + RED_ZONE].view(torch.int32) == 3).all())
    h = a.carve(5, torch.bfloat16, 2, poison=float("inf"))
    lo = h.data_ptr() - a.buf.data_ptr()
    assert bool(torch.isinf(a.buf[lo + 10:lo + 10 + RED_ZONE].view(torch.bfloat16)).all())
    a.check()


def test_pattern_poison_continues_the_table_in_phase():
    """a flat (n, 3) coordinate table: the elements behind it read as further whole points equal to the pattern, and so do
    those in front of it"""
    a = Arena("cpu", 1 << 20)
    pts = np.arange(15, dtype=np.float32).reshape(5, 3) + 100
    v = a.put(pts, 12, poison=[1.0, 2.0, 3.0])
    lo = v.data_ptr() - a.buf.data_ptr()
    flat = a.buf[lo - 3 * 4 * 4:lo + 60 + 3 * 4 * 4].view(torch.float32)
    assert flat[:12].tolist() == [1.0, 2.0, 3.0] * 4
    assert flat[12:27].tolist() == pts.flatten().tolist()
    assert flat[27:].tolist() == [1.0, 2.0, 3.0] * 4
    a.check()


@pytest.mark.parametrize("where", ["one byte behind", "one byte in front", "last byte of the zone behind", "first byte of the zone in front",
                                   "the bytes between the boundary and a misaligned view's zone"])
def test_check_fails_after_a_write_into_a_red_zone(where):
    a = Arena("cpu", 1 << 20)
    a.carve(10, torch.float32, 0, poison=float("nan"))
    v = a.carve(9, torch.float32, 4)
    a.carve(3, torch.int32, 8, poison=0)
    a.check()
    lo = v.data_ptr() - a.buf.data_ptr()
    hi = lo + 36
    at = {"one byte behind": hi, "one byte in front": lo - 1, "last byte of the zone behind": hi + RED_ZONE - 1,
          "first byte of the zone in front": lo - RED_ZONE, "the bytes between the boundary and a misaligned view's zone": lo - RED_ZONE - 1}[where]
    a.buf[at] = a.buf[at] ^ 1                                  # the deliberate stray write: one bit
    with pytest.raises(AssertionError, match=f"arena offset {at}"):
        a.check()
    a.buf[at] = a.buf[at] ^ 1
    a.check()


def test_check_sees_a_stray_float_store_past_an_output_and_reset_starts_over():
    a = Arena("cpu", 1 << 20)
    out = a.carve((4, 5), torch.float32, 12)
    flat = a.buf[out.data_ptr() - a.buf.data_ptr():].view(torch.uint8)[:21 * 4].view(torch.float32)   # one element too many
    flat[:20] = 1.0
    a.check()
    flat[20] = 1.0
    with pytest.raises(AssertionError, match="behind the view"):
        a.check()
    a.reset()
    a.check()
    again = a.carve((4, 5), torch.float32, 12)
    assert again.data_ptr() == out.data_ptr()
    a.check()

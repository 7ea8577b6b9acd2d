"""The shared CSR builder (csrc/csr.hip), hist_to_cursors (csrc/common.h) and the bf16 rounding (csrc/bf16.h), exactly.

The gradients that run through the inverted index add a target's terms in list order, and the lists are filled through an
LDS atomic cursor: the order is not fixed between launches.  With INTEGER data the order cannot matter: gradients are
integers in [-4, 4] (exact in bf16), group weights are 1, interpolation weights come from {0.25, 0.5}.  Every term is then a
multiple of 0.25 and every partial sum, in any order, is a multiple of 0.25 below 2^24 / 4 in magnitude: an exactly
representable fp32 number.  So the assertion is array_equal with a masked np.add.at in float64, cast to the output type; the
bound on the sums is asserted per case (on the sum of the terms' magnitudes, which bounds every partial sum).

Target counts {1, 63, 1024, 1025, 2049, 16384}: 1025 and 2049 give the scan chunks of 2 and 3 cells per thread with a ragged
or empty tail, 16384 is the only size above 16128, where the builder needs more than 64 KB of LDS granted.  In every case one
target (the LAST one: it sits in the ragged tail) holds half of all entries, one target holds none (count 1 has only its one
target) and four entries are out of range (-1 and the target count): they must be skipped.  They appear only in the idx of
the backward, which nothing but the builder dereferences."""
import numpy as np
import pytest
import torch

from pdm_ssd_amd import _native
from pdm_ssd_amd.pointnet2_batch import pointnet2_batch_hip as ext

pytestmark = pytest.mark.gpu

B = 2
NAN = float("nan")
COUNTS = [1, 63, 1024, 1025, 2049, 16384]
EXACT = 2.0 ** 24 / 4
_cache = {}


def cached(key, fn):
    if key not in _cache:
        _cache[key] = fn()
    return _cache[key]


def make_idx(ne, targets, seed):
    """(B, ne) int32: the last target holds half of the entries, target `empty` none, four entries are out of range"""
    rng = np.random.default_rng(seed)
    empty = targets // 2 if targets > 1 else -1
    idx = rng.integers(0, targets, (B, ne))
    idx[idx == empty] = (empty + 1) % targets
    idx[:, :ne // 2] = targets - 1
    for b in range(B):
        idx[b] = idx[b, rng.permutation(ne)]
        free = np.flatnonzero(idx[b] != targets - 1)[:4] if targets > 1 else np.arange(4)
        assert free.size == 4
        idx[b, free] = [-1, targets, -1, targets]
    assert ((idx == targets - 1).sum(1) >= ne // 2).all() and (empty < 0 or not (idx == empty).any())
    return idx.astype(np.int32), empty


def scatter_ref(idx, terms, targets):
    """out[b, k, :] = sum of terms[b, e, :] over idx[b, e] == k, in float64, and the largest sum of magnitudes"""
    out = np.zeros((B, targets, terms.shape[2]))
    mag = np.zeros_like(out)
    for b in range(B):
        ok = (idx[b] >= 0) & (idx[b] < targets)
        np.add.at(out[b], idx[b, ok], terms[b, ok])
        np.add.at(mag[b], idx[b, ok], np.abs(terms[b, ok]))
    return out, float(mag.max())


def int_grad(shape, seed):
    return torch.randint(-4, 5, shape, generator=torch.Generator().manual_seed(seed)).float()


# ------------------------------------------------------------------ pdm_group_concat_cl_grad_ld (the element payload)

@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("C,ld,bf16", [(5, 8, 0), (5, 8, 1), (8, 11, 1)], ids=["fp32-ld8", "bf16x4-ld8", "bf16-ld11"])
def test_group_concat_cl_grad_exact(dev, C, ld, bf16, n):
    """fp32 rows and bf16 rows of ld = 11 take gcl_grad_kernel, bf16 rows of ld = 8 gcl_grad_bf16x4_kernel (8-byte words)"""
    m, ns = 64, 8
    ne = m * ns
    idx, empty = cached(("gidx", n), lambda: make_idx(ne, n, 100 + n))
    go = cached(("ggo", ld), lambda: int_grad((B, m, ns, ld), ld))
    want, mag = scatter_ref(idx, go.reshape(B, ne, ld)[..., 3:3 + C].double().numpy(), n)
    assert mag < EXACT
    g = (go.bfloat16() if bf16 else go).to(dev)
    i = torch.from_numpy(idx).to(dev)
    out = torch.full((B, n, C), NAN, device=dev)      # "fully written"
    nbytes = _native.lib().pdm_group_concat_cl_grad_ws_bytes(B, n, m, ns)
    assert nbytes == B * ((n + 1) + ne) * 4 + 64
    ws = torch.zeros(nbytes, dtype=torch.uint8, device=dev)    # a start the builder skips reads as an empty list
    _native.call("pdm_group_concat_cl_grad_ld", _native.stream(dev), B, n, m, C, ns, g.data_ptr(), bf16, ld, i.data_ptr(), out.data_ptr(),
                 ws.data_ptr(), nbytes)
    got = out.cpu().numpy()
    np.testing.assert_array_equal(got, want.astype(np.float32))
    if empty >= 0:
        assert not got[:, empty].any()


# ------------------------------------------------------------------ pdm_interp_concat_rows_grad_out (row + weight payload)

def interp_case(m):
    n = 3000
    idx, empty = make_idx(3 * n, m, 200 + m)
    w = np.random.default_rng(m).choice(np.float32([0.25, 0.5]), (B, n, 3))
    return idx.reshape(B, n, 3), empty, w


@pytest.mark.parametrize("m", COUNTS)
@pytest.mark.parametrize("out_bf16", [0, 1], ids=["fp32", "bf16"])
@pytest.mark.parametrize("c2,ld", [(16, 16), (12, 24)], ids=["eight-channel", "element"])
def test_interp_concat_rows_grad_exact(dev, c2, ld, out_bf16, m):
    n = 3000
    idx, empty, w = cached(("iidx", m), lambda: interp_case(m))
    dx = cached(("idx_dx", ld), lambda: int_grad((B, n, ld), 7 * ld))
    terms = (dx[..., None, :c2].double().numpy() * w[..., None].astype(np.float64)).reshape(B, 3 * n, c2)
    want, mag = scatter_ref(idx.reshape(B, 3 * n), terms, m)
    assert mag < EXACT
    want = torch.from_numpy(want).to(torch.bfloat16 if out_bf16 else torch.float32)
    g = dx.bfloat16().to(dev)
    i, ww = torch.from_numpy(idx).to(dev), torch.from_numpy(w).to(dev)
    out = torch.full((B, m, c2), NAN, dtype=want.dtype, device=dev)     # "fully written"
    nbytes = _native.lib().pdm_three_interpolate_grad_ws_bytes(B, n, m)
    r16 = lambda x: (x + 15) // 16 * 16
    assert nbytes == r16(B * (m + 1) * 4) + r16(B * 3 * n * 2) + B * 3 * n * 4 + 64
    ws = torch.zeros(nbytes, dtype=torch.uint8, device=dev)    # a start the builder skips reads as an empty list
    _native.call("pdm_interp_concat_rows_grad_out", _native.stream(dev), B, n, m, c2, ld, g.data_ptr(), i.data_ptr(), ww.data_ptr(),
                 out.data_ptr(), out_bf16, ws.data_ptr(), nbytes)
    got = out.cpu()
    assert torch.equal(got.float(), want.float())
    if empty >= 0:
        assert not bool(got[:, empty].float().any())


# ------------------------------------------------------------------ the channel-major backward (csr_scatter_grad_launch)

@pytest.mark.parametrize("m", [1025, 16384])
def test_three_interpolate_grad_ws_exact(dev, m):
    n, c = 3000, 5
    idx, empty, w = cached(("iidx", m), lambda: interp_case(m))
    go = int_grad((B, c, n), 31)
    terms = (go.permute(0, 2, 1)[:, :, None, :].double().numpy() * w[..., None].astype(np.float64)).reshape(B, 3 * n, c)
    want, mag = scatter_ref(idx.reshape(B, 3 * n), terms, m)
    assert mag < EXACT
    out = torch.zeros(B, c, m, device=dev)            # the entry point adds into grad_points
    ext.three_interpolate_grad_wrapper(B, c, n, m, go.to(dev), torch.from_numpy(idx).to(dev), torch.from_numpy(w).to(dev), out)
    got = out.cpu().numpy()
    np.testing.assert_array_equal(got, want.transpose(0, 2, 1).astype(np.float32))
    assert not got[:, :, empty].any()


@pytest.mark.parametrize("n", [1025, 16384])
def test_group_points_grad_ws_exact(dev, n):
    npoints, ns, c = 64, 8, 5
    idx, empty = cached(("gidx", n), lambda: make_idx(npoints * ns, n, 100 + n))
    go = int_grad((B, c, npoints, ns), 37)
    want, mag = scatter_ref(idx, go.reshape(B, c, npoints * ns).permute(0, 2, 1).double().numpy(), n)
    assert mag < EXACT
    out = torch.zeros(B, c, n, device=dev)            # the entry point adds into grad_points
    ext.group_points_grad_wrapper(B, c, n, npoints, ns, go.to(dev), torch.from_numpy(idx.reshape(B, npoints, ns)).to(dev), out)
    got = out.cpu().numpy()
    np.testing.assert_array_equal(got, want.transpose(0, 2, 1).astype(np.float32))
    assert not got[:, :, empty].any()


# ------------------------------------------------------------------ f32_to_bf16 / pack_bf16x8

@pytest.mark.parametrize("ld", [8, 9], ids=["pack_bf16x8", "element"])
def test_bf16_rounding_ties_bit_exact(dev, ld):
    """Rows of eight floats through the skip columns of pdm_interp_concat_rows (passed through, then rounded): ld = 8 takes the
    eight-channel kernel (pack_bf16x8), ld = 9 the element kernel (f32_to_bf16).  Values k + half an ulp of bf16 for even and
    odd k, both signs (exact ties: to even), one fp32 ulp to either side of a tie, +-inf, the largest finite fp32 (rounds to
    inf), zeros, a denormal, NaNs.  Bit for bit torch's .bfloat16(), except for the NaNs: torch itself has no single NaN pattern
    (its vectorised CPU conversion writes 0xffff, its scalar one 0x7fc0).  They are pinned to the library's own rule instead:
    sign and upper payload kept, quiet bit set, which is 0x7fc0 for both inputs (one of them has its payload in the low bits only)."""
    bits = np.array([[0x3f808000, 0x3f818000, 0xbf808000, 0xbf818000, 0x3f807fff, 0x3f808001, 0x3f817fff, 0x3f818001],
                     [0x7f800000, 0xff800000, 0x7f7fffff, 0xff7fffff, 0x00000000, 0x80000000, 0x00008000, 0x00018000],
                     [0x7fc00000, 0x7f800001, 0x42f68000, 0x42f78000, 0xc2f68000, 0x477fff80, 0x3f7f8000, 0x33808000]], dtype=np.uint32)
    x = torch.from_numpy(bits.view(np.float32).copy()).reshape(1, 3, 8)
    out = torch.full((1, 3, ld), NAN, dtype=torch.bfloat16, device=dev)
    skip = x.to(dev)
    _native.call("pdm_interp_concat_rows", _native.stream(dev), 1, 3, 0, 0, 8, ld, 0, 0, skip.data_ptr(), 0, 0, 0, out.data_ptr())
    got = out.cpu().view(torch.int16).numpy().view(np.uint16)
    want = x.bfloat16().view(torch.int16).numpy().view(np.uint16)
    nan = np.isnan(x.numpy())
    assert nan.sum() == 2
    np.testing.assert_array_equal(got[..., :8][~nan], want[~nan])
    g = got[..., :8][nan]
    assert (g == 0x7fc0).all() and torch.isnan(x.bfloat16()[0][torch.from_numpy(nan[0])]).all()
    assert not got[..., 8:].any()

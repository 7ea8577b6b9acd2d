"""csrc/train_gemm.hip — the PERSISTENT walk of the forward / data-gradient contractions: shapes with more row tiles than slots, so
that workgroup slots 0 and 1 walk a second row tile (`for (; rt < row_tiles; rt += slots)` in tg_nt_kernel, the stage walk across a
tile boundary in tg_nt_deep_kernel): the prefetch of tile rt + slots, the weights kept in LDS across tiles (N <= 32, K <= 64), the
weights restaged from registers (one k-step, wider tiles) or reloaded (several k-steps), the statistics registers carried across
tiles and, in the deep kernel, the two register sets swapping roles at the boundary (odd number of k-steps).

    case   K    N     R       tile      row tiles / slots   kernels (plain | x_bn_coef | bs)
    1      8    8   262416   256 x 32    1026 / 1024        tg_nt_kernel<1,1,XF,BS,PL>, one k-step, weights resident
    2     72   64   262416   256 x 64    1026 / 1024        tg_nt_kernel<1,2,XF,BS,PL>, two k-steps, weights reloaded per tile
    3      8  128   131216   128 x 128   1026 / 1024        tg_nt_deep_kernel<XF,PL> | tg_nt_kernel<2,2,0,true>, one k-step
    4    136  264    43792   128 x 128    343 / 341 (x 3)   the same, three column tiles, three k-steps (odd: the sets swap)
    dy 2  72   64   131216   128 x 64    1026 / 1024        tg_nt_kernel<2,1,2,BS>
    dy 4 136  264    43792   128 x 128    343 / 341 (x 3)   tg_nt_kernel<2,2,2,BS>

slots = min(row tiles, clamp(1024 / column tiles, 64, 1024)) (tg_slots / tg_dy_slots; asserted through pdm_tg_stats_parts).  Every R is a
multiple of 16 (pooled groups) and leaves the last row tile partial.  References: the operation restated in torch float64 on integer /
half-integer data, where every fp32 sum of the kernels is exact — comparisons are torch.equal."""
import functools

import pytest
import torch

from pdm_ssd_amd import _native
from pdm_ssd_amd import train_gemm as tg
from test_train_gemm_gpu import _bn_coef as bn_coef, _bwd_stats_reference as bwd_stats_reference, bf16_of, bn_bwd64, check_pool, check_stats, ints, relu_bn64

pytestmark = pytest.mark.gpu

CASES = {1: (262416, 8, 8), 2: (262416, 72, 64), 3: (131216, 8, 128), 4: (43792, 136, 264)}
DY_CASES = {2: (131216, 72, 64), 4: (43792, 136, 264)}


@functools.lru_cache(maxsize=None)
def forward_case(case, dev):
    """inputs and the two float64 references (plain, through BatchNorm + ReLU) of a case: formed once, never written again"""
    R, K, N = CASES[case]
    bm, bn = (256, 32) if N <= 32 else (256, 64) if N <= 64 else (128, 128)
    slots = _native.lib().pdm_tg_stats_parts(R, N)
    tiles = (R + bm - 1) // bm
    assert slots == min(1024, max(64, 1024 // ((N + bn - 1) // bn))) and tiles == slots + 2 and R % bm != 0 and R % 16 == 0
    x = ints((R, K), -4, 4, 100 + case, dev).bfloat16()
    x[:, -1] = torch.arange(R, device=dev).remainder(5).bfloat16() - 2.0          # the row shows in the product: a swapped tile shows
    w32 = ints((N, K), -3, 3, 200 + case, dev)
    w32[0, :] = 1.0
    coef = bn_coef(K, dev, 300 + case)
    want = bf16_of(x.double() @ w32.double().t())
    want_bn = bf16_of(relu_bn64(x, coef) @ w32.double().t())
    return x, w32, tg.pack_weight(w32), coef, want, want_bn


@pytest.mark.parametrize("case", sorted(CASES))
@pytest.mark.parametrize("bn_in", [False, True])
def test_second_row_tile_of_gemm_nt(dev, case, bn_in):
    """y (plain call, stats=True, pool_ns=16) bit-equal to the float64 reference, the column sums over ALL slots' parts equal to the
    reference's, group extremes and first indices those of the reference y — without and with the BatchNorm + ReLU load path."""
    x, w32, w, coef, want, want_bn = forward_case(case, dev)
    xf, ref = (coef, want_bn) if bn_in else (None, want)
    assert torch.equal(tg.gemm_nt(x, w, x_bn_coef=xf), ref)
    y, st = tg.gemm_nt(x, w, stats=True, x_bn_coef=xf)
    assert torch.equal(y, ref) and st.shape[0] == _native.lib().pdm_tg_stats_parts(*ref.shape)
    check_stats(st, ref)
    y, st, (keep, idx) = tg.gemm_nt(x, w, stats=True, x_bn_coef=xf, pool_ns=16)
    assert torch.equal(y, ref)
    check_stats(st, ref)
    check_pool(ref, keep, idx, 16)


@pytest.mark.parametrize("case", sorted(CASES))
def test_second_row_tile_of_gemm_nt_bs(dev, case):
    """pdm_tg_gemm_nt_bs (tg_nt_kernel<WN,JT,0,true>; the wide cases take this kernel, not the deep one): the product is the
    reference's, the finalized gradient statistics are pdm_bn_relu_backward_stats' over the same tensors (2e-5 of each row's largest)."""
    x, w32, w, _, want, _ = forward_case(case, dev)
    R, N = want.shape
    bx = ints((R, N), -4, 4, 400 + case, dev).bfloat16()
    coef = bn_coef(N, dev, 500 + case)
    y, part = tg.gemm_nt_bs(x, w, bx, coef)
    assert torch.equal(y, want) and torch.equal(y, tg.gemm_nt(x, w)) and part.shape == (_native.lib().pdm_tg_stats_parts(R, N), N, 2)
    got, ref = tg.bn_bwd_finalize(R, coef, part), bwd_stats_reference(bx, y, coef)
    scale = ref.abs().amax(1, keepdim=True).clamp_min(1e-6)
    assert float(((got - ref).abs() / scale).max()) < 2e-5


@pytest.mark.parametrize("case", sorted(DY_CASES))
def test_second_row_tile_of_gemm_nt_dy(dev, case):
    """pdm_tg_gemm_nt_dy / _dy_bs (XF == 2): dy = bf16(scale (dz [bn(yp) > 0] - p - (yp - mean) q)) — p in {-1/2, 0, 1/2}, q in
    {-1/4, 0, 1/4}: multiples of 1/8 up to 20, exact in bf16 — and dx = bf16(dy . w^T), both bit-equal to float64; every row of dy
    is compared, so a row the walk skipped (column tile 0 writes it) or wrote from another tile shows."""
    R, K, N = DY_CASES[case]
    bn = 64 if N <= 64 else 128
    slots = _native.lib().pdm_tg_dy_stats_parts(R, N)
    assert slots == min(1024, max(64, 1024 // ((N + bn - 1) // bn))) and (R + 127) // 128 == slots + 2 and R % 128 != 0
    dz = ints((R, K), -3, 3, 600 + case, dev).bfloat16()
    yp = ints((R, K), -4, 4, 610 + case, dev).bfloat16()
    dz[:, 0] = torch.arange(R, device=dev).remainder(7).bfloat16() - 3.0
    icoef = bn_coef(K, dev, 620 + case)
    icoef[2, 0], icoef[3, 0] = 2.0, 1.5                       # channel 0 (the row marker): live for most rows
    igrads = torch.zeros((4, K), device=dev)
    igrads[2] = ints((K,), -1, 1, 630 + case, dev) * 0.5
    igrads[3] = ints((K,), -1, 1, 640 + case, dev) * 0.25
    w32 = ints((N, K), -2, 2, 650 + case, dev)
    w = tg.pack_weight(w32)
    dy64 = bn_bwd64(dz, yp, icoef, igrads)
    want_dy = bf16_of(dy64)
    assert torch.equal(want_dy.double(), dy64)                # the operand is exact in bf16
    want_dx = bf16_of(dy64 @ w32.double().t())
    dx, dy = tg.gemm_nt_dy(dz, yp, icoef, igrads, w)
    assert torch.equal(dy, want_dy) and torch.equal(dx, want_dx)
    bx = ints((R, N), -4, 4, 660 + case, dev).bfloat16()
    coef = bn_coef(N, dev, 670 + case)
    dx, dy, part = tg.gemm_nt_dy(dz, yp, icoef, igrads, w, bs=(bx, coef))
    assert torch.equal(dy, want_dy) and torch.equal(dx, want_dx) and part.shape == (slots, N, 2)
    got, ref = tg.bn_bwd_finalize(R, coef, part), bwd_stats_reference(bx, dx, coef)
    scale = ref.abs().amax(1, keepdim=True).clamp_min(1e-6)
    assert float(((got - ref).abs() / scale).max()) < 2e-5

"""pdm_bev_roi_crop and pdm_bev_roi_crop_fc (csrc/bev_roi_crop.hip) against the float64 restatement of
tests/bev_crop_reference.py, with every tensor carved from a poisoned Arena 4 bytes off a 16-byte boundary (the packed weight and
the workspace, which the operator requires 16-byte aligned, excepted).

Crop: |got - want64| <= delta (Lx_c + Ly_c) + 8 2^-24 T per element (bev_crop_reference's docstring: delta from the reference's own
deviation from float64 over these very cases), two runs bit-equal, rois wholly outside exactly 0, and the same rois sampled with
i / j transposed or x / y swapped leave the bound, so the test can fail.

Crop + FC: against float64 crop . W^T within (K + 8) 2^-24 T_fc + sum_k |W| (crop bound): the first term is the first-order bound
of an fp32 sum of K rounded products in any order (the operator's MFMA chains and fixed partials), T_fc = sum |W| |crop64|; the
second carries the crop's own bound through the contraction.  The epilogue against relu(raw * scale + shift) to 2^-23 relative, as
tests/test_sparse_fc_gpu.py does.
"""
import numpy as np
import pytest
import torch

import bev_crop_reference as bcr
from arena import Arena
from pdm_ssd_amd import bev_roi_ops

pytestmark = pytest.mark.gpu
U = bcr.U
NAN = float('nan')


@pytest.fixture(scope="module")
def arena(dev):
    return Arena(dev, nbytes=40 << 20)


@pytest.fixture(scope="module")
def maps():
    """the map of a (B, C, H, W) case, made once"""
    cache = {}

    def get(B, C, H, W):
        if (B, C, H, W) not in cache:
            cache[(B, C, H, W)] = bcr.make_map(B, C, H, W, seed=B + C + H)
        return cache[(B, C, H, W)]
    return get


def run_crop(arena, rois, feat, H, W, G, pad=5):
    arena.reset()
    B, n, C = rois.shape[0], rois.shape[1], feat.shape[1]
    t_rois = arena.put(rois, 4, NAN)
    t_feat = arena.put(feat, 4, NAN)
    out = arena.carve((B * n, C * G * G + pad), torch.float32, 4)
    out.fill_(NAN)
    got = bev_roi_ops.bev_roi_crop(t_rois, t_feat, bcr.pc_range(H, W), bcr.VOXEL, bcr.RATIO, G, out=out)
    torch.cuda.synchronize()
    arena.check()
    assert got is out and bool(torch.isnan(out[:, C * G * G:]).all()), 'the columns behind C G^2 are not the operator\'s'
    return out[:, :C * G * G].clone().view(B * n, C, G, G)


@pytest.mark.parametrize("name, C, G, B, n, stride, seed", bcr.crop_cases())
def test_crop_is_within_the_bound_of_float64(dev, arena, maps, name, C, G, B, n, stride, seed):
    H, W = bcr.CASES[name]
    rois, outside = bcr.make_rois(H, W, B, n, stride, seed)
    feat = maps(B, C, H, W)
    r = bcr.pc_range(H, W)
    want, T = bcr.crop64(rois, feat, r[0], r[1], bcr.CELL, bcr.CELL, G)
    bound = bcr.crop_bound(feat, n, T)
    out = run_crop(arena, rois, feat, H, W, G)
    assert torch.equal(out, run_crop(arena, rois, feat, H, W, G)), 'two runs differ'
    got = out.cpu().numpy().astype(np.float64)
    ratio = np.abs(got - want) / np.maximum(bound, 1e-300)
    print(name, 'C', C, 'G', G, 'B', B, 'n', n, 'stride', stride, 'max err / bound', float(ratio.max()), 'max err', float(np.abs(got - want).max()))
    assert np.isfinite(got).all() and (np.abs(got - want) <= bound).all()
    flat = outside.reshape(-1)
    assert (got[flat] == 0).all() and (want[flat] == 0).all(), 'a roi wholly outside the map crops exactly 0'
    if n > 1:       # the all-zero padding rows: every cell samples the map at the range's origin
        last = got.reshape(B, n, C, G * G)[:, -1]
        assert (rois[:, -1] == 0).all() and (last == last[..., :1]).all()
    # what a transposed lattice or swapped axes compute is outside the bound somewhere
    if (~flat).any():
        for wrong in ({'transpose_ij': True}, {'swap_xy': True}):
            other = bcr.crop64(rois, feat, r[0], r[1], bcr.CELL, bcr.CELL, G, **wrong)[0]
            assert (np.abs(got - other) > bound).any(), wrong


def test_fresh_output_and_the_torch_formulation_on_the_device(dev, maps):
    """without `out` the operator allocates (B n, C, G, G); bev_roi_crop_torch, the checker, on the same device tensors is within
    the two bounds of it"""
    H, W = bcr.CASES['small']
    rois, _ = bcr.make_rois(H, W, 3, 37, 9, seed=2)
    feat = maps(3, 5, H, W)
    r = bcr.pc_range(H, W)
    t_rois, t_feat = torch.from_numpy(rois).to(dev), torch.from_numpy(feat).to(dev)
    got = bev_roi_ops.bev_roi_crop(t_rois, t_feat, r, bcr.VOXEL, bcr.RATIO, 7)
    check = bev_roi_ops.bev_roi_crop_torch(t_rois, t_feat, r, bcr.VOXEL, bcr.RATIO, 7)
    _, T = bcr.crop64(rois, feat, r[0], r[1], bcr.CELL, bcr.CELL, 7)
    assert got.shape == (111, 5, 7, 7) and check.shape == got.shape
    assert ((got - check).abs().cpu().numpy() <= 2 * bcr.crop_bound(feat, 37, T)).all()


# ---- crop + first FC --------------------------------------------------------------------------------------------------------------

def fc_case(maps, C, cout, R, G=7, name='small'):
    H, W = bcr.CASES[name]
    B, n = (1, 1) if R == 1 else (1, R)
    rois, _ = bcr.make_rois(H, W, B, n, 7, seed=C + cout + R)
    feat = maps(B, C, H, W)
    r = bcr.pc_range(H, W)
    K = C * G * G
    rng = np.random.default_rng(C * cout + R)
    w = (rng.uniform(-1, 1, (cout, K, 1)) / np.sqrt(K)).astype(np.float32)
    crop, T = bcr.crop64(rois, feat, r[0], r[1], bcr.CELL, bcr.CELL, G)
    cbound = bcr.crop_bound(feat, n, T).reshape(B * n, K)
    x, w64 = crop.reshape(B * n, K), w[:, :, 0].astype(np.float64)
    want = x @ w64.T
    bound = (K + 8) * U * (np.abs(x) @ np.abs(w64).T) + cbound @ np.abs(w64).T
    # the same crop under the WRONG column order (i G + j) C + c: what a mis-packed weight computes
    wrong = crop.reshape(B * n, C, G * G).transpose(0, 2, 1).reshape(B * n, K) @ w64.T
    return dict(rois=rois, feat=feat, w=w, want=want, bound=bound, wrong=wrong, H=H, W=W, G=G, C=C)


def run_fc(arena, case, cout, w=None, scale=None, shift=None, relu=False):
    dev = arena.buf.device
    arena.reset()
    t_rois = arena.put(case['rois'], 4, NAN)
    t_feat = arena.put(case['feat'], 4, NAN)
    R = case['rois'].shape[0] * case['rois'].shape[1]
    out = arena.carve((R, cout), torch.float32, 4)
    out.fill_(NAN)
    wpack = bev_roi_ops.pack_crop_fc_weight(torch.from_numpy(case['w'] if w is None else w).to(dev), case['C'], case['G'])
    opt = [None if t is None else arena.put(t, 4, NAN) for t in (scale, shift)]
    bev_roi_ops.bev_roi_crop_fc(t_rois, t_feat, bcr.pc_range(case['H'], case['W']), bcr.VOXEL, bcr.RATIO, case['G'], wpack, cout, opt[0], opt[1],
                                relu, out=out)
    torch.cuda.synchronize()
    arena.check()
    return out.clone()


@pytest.mark.parametrize("R", [1, 37])
@pytest.mark.parametrize("cout", [16, 256])
@pytest.mark.parametrize("C", [16, 64])
def test_crop_fc_matches_float64(dev, arena, maps, C, cout, R):
    case = fc_case(maps, C, cout, R)
    raw = run_fc(arena, case, cout)
    assert torch.equal(raw, run_fc(arena, case, cout)), 'two runs differ'
    got = raw.cpu().numpy().astype(np.float64)
    ratio = np.abs(got - case['want']) / np.maximum(case['bound'], 1e-300)
    print('R', R, 'C', C, 'Cout', cout, 'chunks', bev_roi_ops.bev_roi_crop_fc_chunks(R, C, 7, cout), 'max err / bound', float(ratio.max()))
    assert np.isfinite(got).all() and (np.abs(got - case['want']) <= case['bound']).all()
    assert (np.abs(got - case['wrong']) > case['bound']).any(), 'the wrong column order is outside the bound: the test tells them apart'
    # the epilogue, from the operator's own raw output: one multiply and one add
    rng = np.random.default_rng(cout)
    scale = (rng.uniform(0.5, 1.5, cout) * rng.choice([-1, 1], cout)).astype(np.float32)
    shift = rng.uniform(-0.5, 0.5, cout).astype(np.float32)
    ep = run_fc(arena, case, cout, scale=scale, shift=shift, relu=True)
    sc, sh = torch.from_numpy(scale).to(dev), torch.from_numpy(shift).to(dev)
    want = torch.relu(raw * sc + sh)
    tol = 2.0 ** -23 * ((raw * sc).abs() + sh.abs())
    assert ((ep - want).abs() <= tol).all() and (ep >= 0).all()


@pytest.mark.parametrize("name, G, C", [('small', 7, 16), ('small', 2, 32), ('kitti', 7, 16)])
def test_a_unit_weight_block_reproduces_the_crops_bits(dev, arena, maps, name, G, C):
    """W = rows of the identity: output channel o is crop column cols[o], so the fused operator's crop (the same device routine)
    must have bev_roi_crop's bits; the columns straddle the stages of 128 and the channel blocks"""
    H, W = bcr.CASES[name]
    rois, _ = bcr.make_rois(H, W, 1, 37, 7, seed=G + C)
    feat = maps(1, C, H, W)
    K, cout = C * G * G, 32
    cols = np.unique(np.concatenate([[0, 1, K - 1, K // 2], np.arange(125, 131) % K, np.random.default_rng(0).integers(0, K, 24)]))[:cout]
    cols = np.resize(cols, cout)
    w = np.zeros((cout, K, 1), dtype=np.float32)
    w[np.arange(cout), cols, 0] = 1.0
    case = dict(rois=rois, feat=feat, w=w, H=H, W=W, G=G, C=C)
    got = run_fc(arena, case, cout)
    crop = run_crop(arena, rois, feat, H, W, G).view(37, K)
    assert torch.equal(got, crop[:, torch.from_numpy(cols).to(dev)])
    assert float(got.abs().max()) > 0

"""Voxel R-CNN's training form on the device (csrc/roi_grid_train.hip): the query, the pooling over kept groups and
the gradients as raw entry points against hand-derived answers and the numpy restatement of tests/voxel_rcnn_grad_reference.py,
then the module, the head and the detector against the composed formulation under torch autograd.  The raw entry points' inputs
and outputs are carved from a poisoned Arena, every fp32 tensor 4 bytes off a 16-byte boundary between NaN red zones.

Bounds.  pooled: 7t's 2 n 2^-24 A with n = 5 roundings against the winning expression on absolute values.  dfeatures_in, per
element: cnt 2^-41 max|gpool| + 2^-24 |value| (cnt addends, each rounded to a step of at most max|gpool| 2^-40, then one
rounding to fp32).  Parameter gradients, per element: M 2^-24 times the sum of the addends' absolute values (an fp32 sum of at
most M addends in any order).  Module and head against the composed path: 4 e per tensor, e = max|f32 - f64| / max|f64| of the
torch formulation on the CPU (7u's rule).
"""
import copy
import os

import numpy as np
import pytest
import torch

import sparse_conv_reference as scr
import voxel_rcnn_case as case
import voxel_rcnn_grad_reference as vg
from arena import Arena
from pdm_ssd_amd import _native, sparse_conv_ops

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
U = 2.0 ** -24
SOURCES = case.HEAD_CFG['ROI_GRID_POOL']['FEATURES_SOURCE']
POOL_CFG = case.HEAD_CFG['ROI_GRID_POOL']['POOL_LAYERS']
STRIDES = {name: stride for name, stride, _ in case.LEVEL_GEOMETRY}
NAN = float('nan')


@pytest.fixture(scope="module")
def ref():
    z = np.load(os.path.join(GOLDEN, "ref_voxel_rcnn.npz"))
    return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def tref():
    z = np.load(os.path.join(GOLDEN, "ref_voxel_rcnn_train.npz"))
    return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def arena(dev):
    return Arena(dev)


@pytest.fixture(scope="module")
def levels():
    return case.levels()


@pytest.fixture(scope="module")
def groups(ref, levels):
    """the restatement's kept groups per (level, G), computed once and shared: (rois, rows, offsets, counts)"""
    cache = {}

    def get(src, G):
        if (src, G) not in cache:
            cfg = POOL_CFG[src]
            rois = ref[f'g{G}.rois']
            hits, offs = vg.level_groups(rois, G, levels[src], cfg['QUERY_RANGES'][0], cfg['POOL_RADIUS'][0], cfg['NSAMPLE'][0])
            cache[(src, G)] = (rois,) + vg.kept(hits, offs, cfg['NSAMPLE'][0])
        return cache[(src, G)]
    return get


def put(arena, src, poison=NAN):
    src = torch.as_tensor(src)
    return arena.put(src, 4, poison) if src.numel() else src.to(arena.buf.device)


# ---- the raw entry points -----------------------------------------------------------------------------------------------------
def raw_query(arena, rois, G, indices, shape, stride, voxel, rng0, qr, radius, S):
    arena.reset()
    dev = arena.buf.device
    B, n = rois.shape[0], rois.shape[1]
    D, H, W = shape
    P, M = len(indices), B * n * G ** 3
    idx = put(arena, np.asarray(indices, np.int32).reshape(-1, 4), [0, 0, 0, 0])
    nbytes = _native.lib().pdm_sparse_index_workspace_bytes(P, B, D, H, W)
    ws = arena.carve(nbytes, torch.uint8, 8)
    _native.call("pdm_sparse_index", _native.stream(dev), P, idx.data_ptr(), B, D, H, W, ws.data_ptr(), nbytes)
    t_rois = put(arena, np.asarray(rois, np.float32))
    qbytes = _native.lib().pdm_roi_grid_query_workspace_bytes(M)
    qws = arena.carve(qbytes, torch.uint8, 8)
    rows = arena.carve((M, S), torch.int32, 4)
    offs = arena.carve((M, S, 3), torch.float32, 4)
    mom = arena.carve(9, torch.float64, 8)
    rows.fill_(-77)
    offs.fill_(NAN)
    mom.fill_(NAN)
    _native.call("pdm_roi_grid_query", _native.stream(dev), B, n, rois.shape[2], t_rois.data_ptr(), G, D, H, W, stride, *voxel, *rng0[:3], P, ws.data_ptr(),
                 nbytes, *qr, radius, S, rows.data_ptr(), offs.data_ptr(), mom.data_ptr(), qws.data_ptr(), qbytes)
    torch.cuda.synchronize()
    arena.check()
    return rows.cpu().numpy(), offs.cpu().numpy(), mom.cpu().numpy()


def raw_train(arena, f, rows, d, wp, sp, hp):
    arena.reset()
    dev = arena.buf.device
    (M, S), (P, C1) = rows.shape, f.shape
    t = [put(arena, np.asarray(a, np.float32)) for a in (f, d, wp, sp, hp)]
    t_rows = put(arena, np.asarray(rows, np.int32), [-1])
    pooled = arena.carve((M, C1), torch.float32, 4)
    arg = arena.carve((M, C1), torch.uint8, 1)
    pooled.fill_(NAN)
    arg.fill_(0x77)
    _native.call("pdm_roi_grid_pool_train", _native.stream(dev), M, S, P, C1, t_rows.data_ptr(), t[1].data_ptr(), t[0].data_ptr(), t[2].data_ptr(),
                 t[3].data_ptr(), t[4].data_ptr(), pooled.data_ptr(), arg.data_ptr())
    torch.cuda.synchronize()
    arena.check()
    return pooled.cpu().numpy(), arg.cpu().numpy()


def raw_grad(arena, g, arg, rows, d, wp, sp, P):
    arena.reset()
    dev = arena.buf.device
    (M, S), C1 = rows.shape, g.shape[1]
    t = [put(arena, np.asarray(a, np.float32)) for a in (g, d, wp, sp)]
    t_rows = put(arena, np.asarray(rows, np.int32), [-1])
    t_arg = put(arena, np.asarray(arg, np.uint8), 0xFF)
    nbytes = _native.lib().pdm_roi_grid_pool_grad_workspace_bytes(M, P, C1)
    ws = arena.carve(nbytes, torch.uint8, 8)
    outs = [arena.carve(shape, torch.float32, 4) for shape in ((P, C1), (C1, 3), (C1,), (C1,))]
    for o in outs:
        o.fill_(NAN)        # poisoned: every element must be written
    _native.call("pdm_roi_grid_pool_grad", _native.stream(dev), M, S, P, C1, t[0].data_ptr(), t_arg.data_ptr(), t_rows.data_ptr(), t[1].data_ptr(),
                 t[2].data_ptr(), t[3].data_ptr(), *(o.data_ptr() for o in outs), ws.data_ptr(), nbytes)
    torch.cuda.synchronize()
    arena.check()
    got = dict(zip(('dfeat', 'dwp', 'dscale', 'dshift'), (o.cpu().numpy() for o in outs)))
    assert all(np.isfinite(v).all() for v in got.values()), 'poison left in an output'
    return got


@pytest.mark.parametrize("G", case.GRID_SIZES)
@pytest.mark.parametrize("src", SOURCES)
def test_query_keeps_the_restatements_groups_offsets_and_moments(arena, levels, groups, src, G):
    """M = 120 (a last tile of 8 grid points) and 405 (a last tile of 5, several workgroups), the empty sample, the zero rois and the
    boxes that leave the range.  grp_row (so the counts too) equals the restatement's hit sets exactly; grp_off is within 4 2^-20 m
    of the float64 value (four roundings at |coordinate| <= 16 m) and 0 in unused slots; the moments are within N 2^-53 of a
    float64 numpy sum over the device's own groups, relative to the sum of the addends' absolute values; two runs give equal bytes."""
    lv, cfg = levels[src], POOL_CFG[src]
    rois, rows, d, cnt = groups(src, G)
    S, qr, radius = cfg['NSAMPLE'][0], cfg['QUERY_RANGES'][0], cfg['POOL_RADIUS'][0]
    args = (rois, G, lv['indices'], lv['shape'], lv['stride'], case.VOXEL, case.RANGE, qr, radius, S)
    g_rows, g_off, g_mom = raw_query(arena, *args)
    print(src, G, 'group sizes', np.bincount(cnt, minlength=S + 1).tolist())
    assert (cnt == 0).any() and (cnt == S).any()
    assert np.array_equal(g_rows, rows)
    assert (g_off[g_rows < 0] == 0).all()
    # the float64 offsets: centre and grid point from the fp32 inputs, in float64
    import voxel_rcnn_reference as vr
    pts = vr.grid_points(rois, G).astype(np.float64)
    cen = (lv['indices'][:, [3, 2, 1]].astype(np.float64) + 0.5) * (np.asarray(case.VOXEL, np.float32).astype(np.float64) * lv['stride']) \
        + np.asarray(case.RANGE[:3], np.float64)
    exact = cen[np.maximum(g_rows, 0)] - pts[:, None, :]
    err = np.abs(g_off.astype(np.float64) - exact)[g_rows >= 0]
    print(src, G, 'offset error (m)', float(err.max()), 'bound', 4 * 2.0 ** -20)
    assert float(err.max()) <= 4 * 2.0 ** -20
    _, dd = vg.padded(g_rows, g_off)
    want, scale = vg.moments(dd), vg.moments(np.abs(dd))
    N =dd.shape[0] * dd.shape[1]
    ratio = np.abs(g_mom - want) / (N * 2.0 ** -53 * scale)
    print(src, G, 'moments err / bound', float(ratio.max()))
    assert (ratio <= 1.0).all()
    again = raw_query(arena, *args)
    assert all(np.array_equal(a, b) for a, b in zip((g_rows, g_off, g_mom), again))


def test_known_answers_shared_row_tie_zero_empty_groups_and_padding(arena):
    """Grid (B 1, D 8, H 8, W 8) of unit voxels from the origin, G = 1 (the grid point is the RoI's centre), window 3 x 3 x 3, radius
    1.1, S = 4, C1 = 16.  Voxels A (z 4, y 4, x 4), B (z 4, y 4, x 5), C (z 1, y 6, x 1).  Grid points: p0 at A's centre: slots [A, B],
    offsets (0, 0, 0), (1, 0, 0); p1 at B's centre: slots [A, B], offsets (-1, 0, 0), (0, 0, 0); p2 over empty cells; p3 at
    (1.75, 6.5, 1.5): slot [C], offset (-0.25, 0, 0), cnt = 1.
    Moments over the padded tensor (S = 4): p0 adds (0) twice more, p1 (-1, 0, 0) twice more, p3 its offset three times more, p2 four
    zeros: sum x = 1 + (-1 - 2) + 4 (-0.25) = -3, sum xx = 1 + 3 + 4 / 16 = 4.25, the rest 0.
    scale_p = 1; Wp = 0 but Wp[3] = (2, 0, 0); shift_p = 0 for c < 4, +0.5 for even c >= 4, -0.5 for odd c >= 4; features 0 for c >= 4.
      c 0: A 2, B 1, C 1      -> A wins at p0 and p1: TWO grid points share the row, dfeatures_in[A][0] = g0 + g1
      c 1: A 3, B 3, C 1      -> a tie: the lower slot (A) wins at both
      c 2: A -5, B -5, C -5   -> pooled 0: arg 0xFF, no gradient anywhere
      c 3: A 1, B 4, C 1      -> p0: max(1 + 0, 4 + 2) = 6 slot 1; p1: max(1 - 2, 4 + 0) = 4 slot 1; p3: 1 - 0.5 = 0.5 slot 0
      even c >= 4: every group, the empty p2 included, pools 0.5 at slot 0: only dshift_p moves, by g0 + g1 + g2 + g3
      odd c >= 4: pooled 0 everywhere: nothing moves
    gpool[m][:] = 1, 2, 3, 8 for m = 0..3."""
    idx = np.array([[0, 4, 4, 4], [0, 4, 4, 5], [0, 1, 6, 1]], np.int32)
    rois = np.zeros((1, 4, 7), np.float32)
    rois[0, :, 3:6] = 1.0
    rois[0, :, 0:3] = [[4.5, 4.5, 4.5], [5.5, 4.5, 4.5], [1.5, 1.5, 5.5], [1.75, 6.5, 1.5]]
    rows, d, mom = raw_query(arena, rois, 1, idx, (8, 8, 8), 1, [1.0, 1.0, 1.0], [0.0, 0.0, 0.0], (1, 1, 1), 1.1, 4)
    assert rows.tolist() == [[0, 1, -1, -1], [0, 1, -1, -1], [-1, -1, -1, -1], [2, -1, -1, -1]]
    assert d[0, :2].tolist() == [[0, 0, 0], [1, 0, 0]] and d[1, :2].tolist() == [[-1, 0, 0], [0, 0, 0]] and d[3, 0].tolist() == [-0.25, 0, 0]
    assert mom.tolist() == [-3, 0, 0, 4.25, 0, 0, 0, 0, 0]

    C1 = 16
    f = np.zeros((3, C1), np.float32)
    f[:, :4] = [[2, 3, -5, 1], [1, 3, -5, 4], [1, 1, -5, 1]]
    wp = np.zeros((C1, 3), np.float32)
    wp[3] = [2, 0, 0]
    sp = np.ones(C1, np.float32)
    hp = np.where(np.arange(C1) < 4, 0.0, np.where(np.arange(C1) % 2 == 0, 0.5, -0.5)).astype(np.float32)
    pooled, arg = raw_train(arena, f, rows, d, wp, sp, hp)
    even, odd = [c for c in range(4, C1, 2)], [c for c in range(5, C1, 2)]
    assert pooled[:, :4].tolist() == [[2, 3, 0, 6], [2, 3, 0, 4], [0, 0, 0, 0], [1, 1, 0, 0.5]]
    assert (pooled[:, even] == 0.5).all() and (pooled[:, odd] == 0).all()
    assert arg[:, :4].tolist() == [[0, 0, 255, 1], [0, 0, 255, 1], [255, 255, 255, 255], [0, 0, 255, 0]]
    assert (arg[:, even] == 0).all() and (arg[:, odd] == 255).all()

    g = np.repeat(np.array([[1.0], [2.0], [3.0], [8.0]], np.float32), C1, 1)
    got = raw_grad(arena, g, arg, rows, d, wp, sp, 3)
    want = np.zeros((3, C1), np.float32)
    want[:, :4] = [[3, 3, 0, 0], [0, 0, 0, 3], [8, 8, 0, 8]]
    want[0, even], want[2, even] = 3, 8             # slot 0 of the non-empty groups; the empty p2 has no row to give to
    assert np.array_equal(got['dfeat'], want)
    shift = np.zeros(C1, np.float32)
    shift[[0, 1, 3]] = 11                           # p0, p1, p3; the empty p2 has shift_p = 0 there: nothing
    shift[even] = 14                                # every group, the empty one included
    assert np.array_equal(got['dshift'], shift)
    scale = np.zeros(C1, np.float32)
    scale[3] = 1 * 2 + 2 * 0 + 8 * -0.5             # g dot(Wp, d) of the winners
    assert np.array_equal(got['dscale'], scale)
    dwp = np.zeros((C1, 3), np.float32)
    dwp[0, 0] = dwp[1, 0] = 1 * 0 + 2 * -1 + 8 * -0.25      # slot 0 wins everywhere: offsets 0, -1, -0.25
    dwp[3, 0] = 1 * 1 + 2 * 0 + 8 * -0.25
    dwp[even, 0] = 1 * 0 + 2 * -1 + 8 * -0.25               # the empty group adds nothing
    assert np.array_equal(got['dwp'], dwp)


def random_parameters(c1, seed):
    rng = np.random.default_rng(seed)
    wp = rng.normal(0, 0.3, (c1, 3)).astype(np.float32)
    sp = (rng.uniform(0.5, 1.5, c1) * rng.choice([-1, 1], c1)).astype(np.float32)
    hp = rng.normal(0, 0.3, c1).astype(np.float32)
    return rng, wp, sp, hp


@pytest.mark.parametrize("c1", [16, 32, 64])
@pytest.mark.parametrize("G", case.GRID_SIZES)
@pytest.mark.parametrize("src", SOURCES)
def test_pooling_and_gradients_match_the_restatement(arena, levels, groups, src, G, c1):
    """pooled within 2 * 5 * 2^-24 * A, arg exact (the seeded inputs keep every winner further from the runner-up and from zero than
    twice that bound: asserted), dfeatures_in and the parameter gradients within the module docstring's bounds under a seeded normal
    cotangent, nothing left of the poison, two runs bit-equal."""
    _, rows, d, cnt = groups(src, G)
    P = len(levels[src]['indices'])
    rng, wp, sp, hp = random_parameters(c1, 1000 * c1 + 10 * G + STRIDES[src])
    f = rng.normal(0, 1, (P, c1)).astype(np.float32)
    want, want_arg, A, gap = vg.pool_train(f, rows, d, wp, sp, hp)
    bound = 2 * 5 * U * A
    assert gap > 2 * float(bound.max()), (gap, float(bound.max()))
    pooled, arg = raw_train(arena, f, rows, d, wp, sp, hp)
    ratio = np.abs(pooled - want) / bound
    print(src, G, c1, 'pooled err / bound', float(ratio.max()), 'winners', float((want_arg != 255).mean()))
    assert (ratio <= 1.0).all() and np.array_equal(arg, want_arg)
    assert ((arg == 0) & (rows[:, :1] < 0)).any() and ((arg == 255) & (rows[:, :1] < 0)).any()      # empty groups on both sides of 0

    g = rng.normal(0, 1, pooled.shape).astype(np.float32)
    got = raw_grad(arena, g, arg, rows, d, wp, sp, P)
    w = vg.pool_grad(g, arg, rows, d, wp, sp, P)
    fb = w['cnt'] * 2.0 ** -41 * float(np.abs(g).max()) + U * np.abs(w['dfeat'])
    err = np.abs(got['dfeat'] - w['dfeat'])
    assert (err <= fb).all(), float((err / np.maximum(fb, 1e-300)).max())
    assert float(w['cnt'].max()) > 1 and (got['dfeat'][w['cnt'] == 0] == 0).all()
    M = rows.shape[0]
    for name in ('dwp', 'dscale', 'dshift'):
        r = np.abs(got[name] - w[name]) / np.maximum(M * U * w['abs_' + name], 1e-300)
        print(src, G, c1, name, 'err / bound', float(r.max()))
        assert (r <= 1.0).all(), name
    again = raw_grad(arena, g, arg, rows, d, wp, sp, P)
    assert all(np.array_equal(got[k], again[k]) for k in got)


@pytest.mark.parametrize("c1", [16, 64])
def test_partition_edges_of_the_parameter_sums(arena, c1):
    """synthetic kept groups over 50 rows with M one below, at and one above the boundary between partials 8 and 9 and between 20
    and 21 (the partition: pdm_roi_grid_pool_grad_chunk_points, a function of M and C1 alone), against the restatement.  (Not at
    the first boundary: with M = 3 the bound M 2^-24 sum|addend| is smaller than the roundings inside one addend's fp32 dot product.)"""
    P, S = 50, 4
    for M0 in (8 * (256 // c1), 20 * (256 // c1)):
        for M in (M0 - 1, M0, M0 + 1):
            chunk = sparse_conv_ops.roi_grid_grad_chunk_points(M, c1)
            assert chunk == 256 // c1
            rng, wp, sp, hp = random_parameters(c1, 7 * M + c1)
            cnt = rng.integers(0, S + 1, M)
            rows = np.where(np.arange(S)[None] < cnt[:, None], rng.integers(0, P, (M, S)), -1).astype(np.int32)
            d = np.where(rows[..., None] >= 0, rng.normal(0, 1, (M, S, 3)), 0).astype(np.float32)
            f = rng.normal(0, 1, (P, c1)).astype(np.float32)
            want, want_arg, A, gap = vg.pool_train(f, rows, d, wp, sp, hp)
            assert gap > 4 * 5 * U * float(A.max())
            pooled, arg = raw_train(arena, f, rows, d, wp, sp, hp)
            assert np.array_equal(arg, want_arg) and (np.abs(pooled - want) <= 2 * 5 * U * A).all()
            g = rng.normal(0, 1, pooled.shape).astype(np.float32)
            got = raw_grad(arena, g, arg, rows, d, wp, sp, P)
            w = vg.pool_grad(g, arg, rows, d, wp, sp, P)
            assert (np.abs(got['dfeat'] - w['dfeat']) <= w['cnt'] * 2.0 ** -41 * float(np.abs(g).max()) + U * np.abs(w['dfeat'])).all()
            for name in ('dwp', 'dscale', 'dshift'):
                assert (np.abs(got[name] - w[name]) <= M * U * w['abs_' + name]).all(), (M, name)


def test_large_m_paths_of_the_gradients(arena):
    """M = 16 385 synthetic kept groups at C1 = 16: one more than 1024 partials of 256 / C1 points, so a partial holds 32 grid
    points and every thread of pdm_roi_grid_pool_grad's scatter walks its chunk in two steps; against the restatement, with the
    bounds of the module docstring."""
    M, c1, P, S = 16 * 1024 + 1, 16, 50, 4
    assert sparse_conv_ops.roi_grid_grad_chunk_points(M, c1) == 32
    rng, wp, sp, hp = random_parameters(c1, 99)
    cnt = rng.integers(0, S + 1, M)
    rows = np.where(np.arange(S)[None] < cnt[:, None], rng.integers(0, P, (M, S)), -1).astype(np.int32)
    d = np.where(rows[..., None] >= 0, rng.normal(0, 1, (M, S, 3)), 0).astype(np.float32)
    f = rng.normal(0, 1, (P, c1)).astype(np.float32)
    want, want_arg, A, _ = vg.pool_train(f, rows, d, wp, sp, hp)
    pooled, arg = raw_train(arena, f, rows, d, wp, sp, hp)
    assert (np.abs(pooled - want) <= 2 * 5 * U * A).all()
    # among 262 144 elements a winner may sit within the rounding of its runner-up: the gradients are held to the device's own arg
    assert float((arg != want_arg).mean()) <= 1e-4
    g = rng.normal(0, 1, pooled.shape).astype(np.float32)
    got = raw_grad(arena, g, arg, rows, d, wp, sp, P)
    w = vg.pool_grad(g, arg, rows, d, wp, sp, P)
    assert (np.abs(got['dfeat'] - w['dfeat']) <= w['cnt'] * 2.0 ** -41 * float(np.abs(g).max()) + U * np.abs(w['dfeat'])).all()
    for name in ('dwp', 'dscale', 'dshift'):
        r = np.abs(got[name] - w[name]) / (M * U * w['abs_' + name])
        print('M', M, name, 'err / bound', float(r.max()))
        assert (r <= 1.0).all(), name


def test_large_m_paths_of_the_query(arena, levels):
    """M = 3 * 128 * 8^3 = 196 608 grid points on the x_conv2 level: 12 288 tiles, so the waves of the 2048 workgroups walk the
    tiles with their stride and every thread of the moments' reduction adds a run of 48 tiles.  RoI j of a sample repeats RoI
    j mod 8, so the groups of the later tiles must equal, bit for bit, those of the first; the moments are held to a float64
    numpy sum over the device's own groups (N 2^-53 of the sum of the addends' absolute values)."""
    src, G, n = 'x_conv2', 8, 128
    lv, cfg = levels[src], POOL_CFG[src]
    S = cfg['NSAMPLE'][0]
    base = case.rois(np.random.default_rng(3))[:, :4]
    rois = np.concatenate([base, base[:, :, [1, 0, 2, 4, 3, 5, 6]] * np.float32(0.9)], 1)          # 8 distinct boxes a sample
    rois = np.ascontiguousarray(np.tile(rois, (1, n // 8, 1)).astype(np.float32))
    rows, off, mom = raw_query(arena, rois, G, lv['indices'], lv['shape'], lv['stride'], case.VOXEL, case.RANGE, cfg['QUERY_RANGES'][0],
                               cfg['POOL_RADIUS'][0], S)
    per = G ** 3
    r4, o4 = rows.reshape(case.B, n, per, S), off.reshape(case.B, n, per, S, 3)
    assert np.array_equal(r4, np.tile(r4[:, :8], (1, n // 8, 1, 1))) and np.array_equal(o4, np.tile(o4[:, :8], (1, n // 8, 1, 1, 1)))
    cnt = (rows >= 0).sum(1)
    assert (cnt == 0).any() and (cnt == S).any() and ((cnt > 0) & (cnt < S)).any() and (rows[cnt > 0] < len(lv['indices'])).all()
    _, dd = vg.padded(rows, off)
    want, scale = vg.moments(dd), vg.moments(np.abs(dd))
    ratio = np.abs(mom - want) / (rows.size * 2.0 ** -53 * scale)
    print('M', rows.shape[0], 'moments err / bound', float(ratio.max()))
    assert (ratio <= 1.0).all()


# ---- the module and the head --------------------------------------------------------------------------------------------------
def sparse_levels(features, levels, dev):
    from pdm_ssd_amd import spconv
    return {k: spconv.SparseConvTensor(features[k], torch.from_numpy(levels[k]['indices']).to(dev), levels[k]['shape'], case.B) for k in SOURCES}


def built_head(tref, dev, extra=None, dp=0.0):
    """the reduced head at G = 2 with the pool layers' parameters of the training fixture (winner margins searched there)"""
    from pdm_ssd_amd.config import cfg_from_dict
    from pdm_ssd_amd.roi_heads import VoxelRCNNHead
    cfg = case.head_cfg(2)
    cfg['DP_RATIO'] = dp
    cfg.update(extra or {})
    head = VoxelRCNNHead(backbone_channels=dict(case.BACKBONE_CHANNELS), model_cfg=cfg_from_dict(cfg), point_cloud_range=case.RANGE,
                         voxel_size=case.VOXEL, num_class=1)
    case.fill_module(head, 102)
    for i, layer in enumerate(head.roi_grid_pool_layers):
        layer.load_state_dict({k[len(f'layer{i}.state.'):]: torch.from_numpy(v) for k, v in tref.items() if k.startswith(f'layer{i}.state.')})
    return head.to(dev).train()


def cpu_error_scale(tref, groups, levels, layer):
    """per tensor e = max|f32 - f64| / max|f64| of the torch formulation on the CPU, and max|f64|"""
    src = SOURCES[layer]
    _, rows, d, _ = groups(src, 2)
    state = {k[len(f'layer{layer}.state.'):]: v for k, v in tref.items() if k.startswith(f'layer{layer}.state.')}
    res = {}
    for dtype in (torch.float64, torch.float32):
        mods = vg.scale_modules(state, '', 0, dtype)
        f = torch.from_numpy(case.level_features(src, len(levels[src]['indices']))).to(dtype).requires_grad_(True)
        out, _, _ = vg.train_forward(mods, f, rows, d)
        out.backward(torch.randn(out.shape, generator=torch.Generator().manual_seed(77 + layer), dtype=torch.float64).to(dtype))
        r = {'out': out.detach(), 'features.grad': f.grad}
        r.update({k + '.grad': p.grad for k, p in vg.named_parameters(mods).items()})
        r.update(vg.running_stats(mods))
        res[dtype] = {k: v.double().numpy() for k, v in r.items()}
    big = {k: max(float(np.abs(v).max()), 1e-30) for k, v in res[torch.float64].items()}
    return {k: float(np.abs(res[torch.float32][k] - res[torch.float64][k]).max()) / big[k] for k in big}, big


def pool_step(head, tref, ref, levels, dev):
    """one training forward + backward of head.roi_grid_pool under the fixture's cotangents -> per layer the tensors compared"""
    feats = {k: torch.from_numpy(case.level_features(k, len(levels[k]['indices']))).to(dev).requires_grad_(True) for k in SOURCES}
    bd = {'batch_size': case.B, 'rois': torch.from_numpy(ref['g2.rois']).to(dev), 'multi_scale_3d_features': sparse_levels(feats, levels, dev),
          'multi_scale_3d_strides': dict(STRIDES)}
    pooled = head.roi_grid_pool(bd).flatten(0, 1)
    cots = [torch.randn((pooled.shape[0], l.out_channels()[0]), generator=torch.Generator().manual_seed(77 + i), dtype=torch.float64).float()
            for i, l in enumerate(head.roi_grid_pool_layers)]
    head.zero_grad(set_to_none=True)
    pooled.backward(torch.cat(cots, 1).to(dev))
    out, at = [], 0
    for i, layer in enumerate(head.roi_grid_pool_layers):
        c2 = layer.out_channels()[0]
        r = {'out': pooled[:, at:at + c2].detach(), 'features.grad': feats[SOURCES[i]].grad}
        at += c2
        r.update({k.replace('.0.', '.', 1) + '.grad': p.grad for k, p in layer.named_parameters()})
        r.update({k.replace('.0.', '.', 1): v.clone() for k, v in layer.state_dict().items() if 'running' in k or 'tracked' in k})
        out.append({k: v.double().cpu().numpy() for k, v in r.items()})
    return out


def test_fused_training_form_matches_the_composed_module_on_the_device(tref, ref, levels, groups, dev):
    """head.roi_grid_pool in training mode, per level NeighborVoxelSAModuleMSG.forward_fused_train against the composed forward()
    under torch autograd, the same parameters: output, the three BatchNorms' running statistics and num_batches_tracked, every
    parameter gradient and the features' gradient within 4 e of the tensor's largest entry, and both within 1e-4 of the reference's
    own module (the training fixture)."""
    fused_head = built_head(tref, dev)
    composed_head = copy.deepcopy(fused_head)
    composed_head.use_fused_pool = False
    assert all(l.fused_train_supported(2) for l in fused_head.roi_grid_pool_layers)
    fused, composed = pool_step(fused_head, tref, ref, levels, dev), pool_step(composed_head, tref, ref, levels, dev)
    for i in range(len(SOURCES)):
        e, big = cpu_error_scale(tref, groups, levels, i)
        assert sorted(e) == sorted(fused[i]) == sorted(composed[i])
        for k in sorted(e):
            diff = float(np.abs(fused[i][k] - composed[i][k]).max()) / big[k]
            to_ref = max(float(np.abs(x[i][k].reshape(tref[f'layer{i}.{k}'].shape) - tref[f'layer{i}.{k}']).max()) for x in (fused, composed)) / big[k]
            print(f'{SOURCES[i]} {k}: e {e[k]:.3g}  fused-composed / e {diff / max(e[k], 1e-30):.3g}  worst against the reference {to_ref:.3g}')
            assert diff <= 4 * e[k], (SOURCES[i], k, diff, e[k])
            assert to_ref <= 1e-4, (SOURCES[i], k, to_ref)


def test_training_form_is_deterministic_graph_capturable_and_reads_nothing(tref, ref, levels, dev, monkeypatch):
    """two runs of forward_fused_train + backward give equal bits, and a torch.cuda.graph replay of the operators' chain (query,
    pooling, gradients) equals its eager run bit for bit; HOST_READS does not move.  The module's own forward refuses a capturing
    stream with a RuntimeError ("not captured"): checked with the stream query patched, no capture is begun."""
    head = built_head(tref, dev)
    layer, src = head.roi_grid_pool_layers[0], SOURCES[0]
    feats = torch.from_numpy(case.level_features(src, len(levels[src]['indices']))).to(dev).requires_grad_(True)
    rois = torch.from_numpy(ref['g2.rois']).to(dev)
    index = sparse_conv_ops.site_index(torch.from_numpy(levels[src]['indices']).to(dev), case.B, levels[src]['shape'])
    cot = torch.randn((rois.shape[0] * rois.shape[1] * 8, layer.out_channels()[0]), generator=torch.Generator().manual_seed(3)).to(dev)
    params = [feats] + list(layer.parameters())

    def step():
        out = layer.forward_fused_train(rois, 2, feats, index, STRIDES[src], case.VOXEL, case.RANGE)
        return [out] + list(torch.autograd.grad(out, params, cot))
    before = sparse_conv_ops.HOST_READS
    first = [t.clone() for t in step()]
    second = [t.clone() for t in step()]
    torch.cuda.synchronize()
    assert sparse_conv_ops.HOST_READS == before
    assert all(torch.equal(a, b) for a, b in zip(first, second)) and all(float(t.abs().max()) > 0 for t in first)
    # the three operators' launch chains, captured from this thread as the other operators' graph tests do (the module's own
    # forward and backward are torch's BatchNorm and autograd engine around exactly these calls)
    g = layer.groupers[0]
    f_in = torch.randn((feats.shape[0], 16), generator=torch.Generator().manual_seed(4)).to(dev)
    wp, sp, hp = (torch.randn(s, generator=torch.Generator().manual_seed(5)).to(dev) for s in ((16, 3), (16,), (16,)))
    gpool = torch.randn((cot.shape[0], 16), generator=torch.Generator().manual_seed(6)).to(dev)

    def chain():
        groups = sparse_conv_ops.roi_grid_query(rois, 2, index, STRIDES[src], case.VOXEL, case.RANGE, g.max_range, g.radius, g.nsample)
        pooled, arg = sparse_conv_ops.roi_grid_pool_train(f_in, wp, sp, hp, groups.rows, groups.offsets)
        return [groups.rows, groups.offsets, groups.moments, pooled, arg,
                *sparse_conv_ops.roi_grid_pool_grad(gpool, arg, groups.rows, groups.offsets, wp, sp, f_in.shape[0])]
    eager = [t.clone() for t in chain()]
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = chain()
    for t in captured:
        t.fill_(NAN) if t.is_floating_point() else t.fill_(0x55)
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(eager, captured)) and sparse_conv_ops.HOST_READS == before
    monkeypatch.setattr(torch.cuda, 'is_current_stream_capturing', lambda: True)
    with pytest.raises(RuntimeError, match='cannot be captured in a graph'):
        layer.forward_fused_train(rois, 2, feats, index, STRIDES[src], case.VOXEL, case.RANGE)


TRAIN_EXTRA = {'TARGET_CONFIG': {'BOX_CODER': 'ResidualCoder', 'ROI_PER_IMAGE': 8, 'FG_RATIO': 0.5, 'SAMPLE_ROI_BY_EACH_CLASS': True,
                                 'CLS_SCORE_TYPE': 'roi_iou', 'CLS_FG_THRESH': 0.75, 'CLS_BG_THRESH': 0.25, 'CLS_BG_THRESH_LO': 0.1,
                                 'HARD_BG_RATIO': 0.8, 'REG_FG_THRESH': 0.55},
               'LOSS_CONFIG': {'CLS_LOSS': 'BinaryCrossEntropy', 'REG_LOSS': 'smooth-l1', 'CORNER_LOSS_REGULARIZATION': True,
                               'LOSS_WEIGHTS': {'rcnn_cls_weight': 1.0, 'rcnn_reg_weight': 1.0, 'rcnn_corner_weight': 1.0, 'code_weights': [1.0] * 7}}}


def head_step(head, ref, levels, dev):
    rois = ref['g2.rois']
    gt = np.zeros((case.B, 3, 8), np.float32)
    gt[:, :, :7], gt[:, :, 7] = rois[:, :3], 1
    gt[:, :, 0] += 0.1          # near the first three rois: foreground rows for the regression losses
    feats = {k: torch.from_numpy(case.level_features(k, len(levels[k]['indices']))).to(dev).requires_grad_(True) for k in SOURCES}
    bd = {'batch_size': case.B, 'rois': torch.from_numpy(rois).to(dev), 'roi_scores': torch.zeros(rois.shape[:2], device=dev),
          'roi_labels': torch.ones(rois.shape[:2], dtype=torch.long, device=dev), 'gt_boxes': torch.from_numpy(gt).to(dev),
          'multi_scale_3d_features': sparse_levels(feats, levels, dev), 'multi_scale_3d_strides': dict(STRIDES)}
    torch.manual_seed(11)
    head(bd)
    loss, tb = head.get_loss()
    head.zero_grad(set_to_none=True)
    loss.backward()
    got = {'loss': loss.detach()}
    got.update({f'{k}.features.grad': v.grad for k, v in feats.items()})
    got.update({k + '.grad': p.grad for k, p in head.named_parameters()})
    return {k: v.double().cpu().numpy() for k, v in got.items()}, head.forward_ret_dict


def test_head_trains_fused_against_composed(tref, ref, levels, groups, dev):
    """VoxelRCNNHead.train() with gt_boxes and DP_RATIO 0: the same sampler seed and step on both, so the same sampled rois; the
    loss and every gradient (parameters and both levels' features) within 4 e of the tensor's largest entry, e the largest of the
    pooling's CPU fp32-against-float64 errors (the FC stacks behind the pooling carry its error on; they add none of their own
    between the two heads, which run the same torch modules).  One run with DP_RATIO 0.3 is finite."""
    e = max(max(cpu_error_scale(tref, groups, levels, i)[0].values()) for i in range(len(SOURCES)))
    fused = built_head(tref, dev, TRAIN_EXTRA)
    composed = copy.deepcopy(fused)
    composed.use_fused_pool = False
    a, ret_a = head_step(fused, ref, levels, dev)
    b, ret_b = head_step(composed, ref, levels, dev)
    assert torch.equal(ret_a['rois'], ret_b['rois']) and ret_a['rcnn_cls'].shape == (case.B * 8, 1)
    assert sorted(a) == sorted(b)
    worst = 0.0
    for k in sorted(a):
        big = max(float(np.abs(b[k]).max()), 1e-30)
        diff = float(np.abs(a[k] - b[k]).max()) / big
        worst = max(worst, diff)
        assert np.isfinite(a[k]).all() and diff <= 4 * e, (k, diff, e)
    print(f'head: e {e:.3g}, worst fused-composed / e {worst / e:.3g}, loss {float(a["loss"]):.6g}')
    assert float(np.abs(a['x_conv2.features.grad']).max()) > 0 and float(np.abs(a['x_conv4.features.grad']).max()) > 0
    dropped, _ = head_step(built_head(tref, dev, TRAIN_EXTRA, dp=0.3), ref, levels, dev)
    assert all(np.isfinite(v).all() for v in dropped.values())


# ---- the detector -------------------------------------------------------------------------------------------------------------
def test_build_voxel_rcnn_takes_a_training_step(dev):
    """a reduced VOXEL_RCNN_TRAIN_CFG on sparse_conv_reference.D1's grid: forward returns {'loss'}; loss.backward() leaves a finite
    gradient on every trainable parameter; loss_rcnn alone reaches the backbone's convolutions up to conv4 through the pooling; an
    optimizer step changes the pool layers; the eval forward afterwards equals its own second run bit for bit."""
    from pdm_ssd_amd import detector_config as dc
    torch.manual_seed(5)
    g = scr.D1
    cfg = copy.deepcopy(dc.VOXEL_RCNN_TRAIN_CFG)
    cfg['ROI_HEAD']['NMS_CONFIG']['TRAIN'].update(NMS_PRE_MAXSIZE=64, NMS_POST_MAXSIZE=16)
    cfg['ROI_HEAD']['NMS_CONFIG']['TEST'].update(NMS_PRE_MAXSIZE=48, NMS_POST_MAXSIZE=8)
    cfg['ROI_HEAD']['TARGET_CONFIG']['ROI_PER_IMAGE'] = 8
    cfg['ROI_HEAD']['ROI_GRID_POOL']['GRID_SIZE'] = 2
    cfg['ROI_HEAD'].update(SHARED_FC=[32, 32], CLS_FC=[32, 32], REG_FC=[32, 32])
    cfg['POST_PROCESSING']['SCORE_THRESH'] = 0.0
    model = dc.build_voxel_rcnn(cfg, dataset=dc.voxel_dataset(4, g['range'], g['voxel'], g['grid'])).to(dev).train()
    rng = np.random.default_rng(21)
    n = 3000
    centres = rng.uniform([1, -3, -2.5], [15, 3, 0.5], (12, 3))
    p = centres[rng.integers(0, 12, n)] + rng.normal(0, 0.6, (n, 3))
    pts = torch.from_numpy(np.concatenate([rng.integers(0, 2, (n, 1)), p, rng.uniform(0, 1, (n, 1))], 1).astype(np.float32)).to(dev)
    gt = np.zeros((g['B'], 3, 8), dtype=np.float32)
    gt[0, 0] = [6.0, 1.0, -1.0, 3.9, 1.6, 1.5, 0.3, 1]
    gt[0, 1] = [12.0, -3.0, -0.8, 0.8, 0.6, 1.7, -1.2, 2]
    gt[1, 0] = [14.0, -2.2, -0.9, 1.7, 0.6, 1.7, 2.1, 3]
    batch = {'batch_size': g['B'], 'points': pts, 'gt_boxes': torch.from_numpy(gt).to(dev)}
    ret, tb, _ = model(dict(batch))
    assert set(ret) == {'loss'} and torch.isfinite(ret['loss']) and 'rcnn_loss' in tb
    assert all(l.fused_train_supported(2) for l in model.roi_head.roi_grid_pool_layers)
    loss_rcnn, _ = model.roi_head.get_loss()
    loss_rcnn.backward(retain_graph=True)
    bb = model.backbone_3d
    for name in ('conv_input', 'conv1', 'conv2', 'conv3', 'conv4'):
        grads = [q.grad for q in getattr(bb, name).parameters() if q.dim() > 1]
        assert grads and all(x is not None and torch.isfinite(x).all() for x in grads) and any(bool(x.any()) for x in grads), name
    model.zero_grad(set_to_none=True)
    ret['loss'].backward()
    for name, q in model.named_parameters():
        if q.requires_grad:
            assert q.grad is not None and torch.isfinite(q.grad).all(), name
    before = [q.detach().clone() for q in model.roi_head.roi_grid_pool_layers.parameters()]
    opt = torch.optim.SGD(model.parameters(), lr=0.01)
    opt.step()
    after = list(model.roi_head.roi_grid_pool_layers.parameters())
    assert any(not torch.equal(a, b) for a, b in zip(before, after))
    model.eval()
    with torch.no_grad():
        one, _ = model(dict(batch))
        two, _ = model(dict(batch))
    assert len(one) == g['B'] and all(torch.equal(a[k], b[k]) for a, b in zip(one, two) for k in ('pred_boxes', 'pred_scores', 'pred_labels'))

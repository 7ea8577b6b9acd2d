"""Voxel R-CNN on the device (csrc/sparse_conv.hip pdm_sparse_index, csrc/roi_grid_pool.hip, roi_heads/voxelrcnn_head.py): the
site index row for row, the fused RoI-grid pooling against hand-derived answers, against the numpy restatement of
tests/voxel_rcnn_reference.py and against the composed module on the device, the head against the reference's own
(tests/golden/ref_voxel_rcnn.npz, gen_voxel_rcnn_fixtures.py) and the detector end to end.  Inputs and outputs of the raw entry
points are carved from a poisoned Arena, features 4 bytes off a 16-byte boundary between NaN red zones.

The bound of the pooling tests, per element: |err| <= 2 n 2^-24 A with n = C1 + 4 and A the pooling's own expression evaluated on
absolute values in float64, A = (|Wout| max_group(|f| + (|Wp| |d|) |scale_p| + |shift_p|)) |scale_o| + |shift_o|.  Derivation: a
pooled value is formed by 4 rounded operations on top of its inputs (the 3-term dot product counts 2 beyond its first product,
the fma 1, the addition of the feature 1; the maximum and the ReLU are 1-Lipschitz and round nothing), each at most 2^-24 of
the absolute-value expression; the output layer sums C1 products in fp32, any order of which errs by at most C1 2^-24 of the
absolute-value sum to first order, and its fma adds one more rounding, which the 4 of the pooled value's bound already exceed
when taken against A.  So n = C1 + 4 roundings against A to first order, doubled as in the sparse-convolution tests.
"""
import copy
import os

import numpy as np
import pytest
import torch

import sparse_conv_reference as scr
import voxel_rcnn_case as case
import voxel_rcnn_reference as vr
from arena import Arena
from pdm_ssd_amd import _native, sparse_conv_ops

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
U = 2.0 ** -24
STRIDES = {name: stride for name, stride, _ in case.LEVEL_GEOMETRY}
# per level: window half-widths (z, y, x), radius, nsample
QUERY = {'x_conv2': ((1, 2, 3), 1.6, 4), 'x_conv3': ((2, 3, 4), 2.45, 8), 'x_conv4': ((4, 4, 4), 5.0, 16)}


@pytest.fixture(scope="module")
def ref():
    z = np.load(os.path.join(GOLDEN, "ref_voxel_rcnn.npz"))
    return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def arena(dev):
    return Arena(dev)


@pytest.fixture(scope="module")
def levels():
    return case.levels()


@pytest.fixture(scope="module")
def hit_cache(ref, levels):
    """numpy hit sets per (rois tag, level), computed once and shared: (rois, G, hits, offsets)"""
    cache = {}

    def get(tag, src):
        if (tag, src) not in cache:
            G = 2 if tag == 'small' else 3
            rois = ref['g2.rois'][:, 1:2] if tag == 'small' else ref['g3.rois']      # small: one turned box a sample
            lv, (qr, radius, nsample) = levels[src], QUERY[src]
            pts = vr.grid_points(rois, G)
            sample = np.repeat(np.arange(case.B), rois.shape[1] * G ** 3)
            cell = vr.cells(pts, case.RANGE, case.VOXEL, lv['stride'])
            hits, offs, margin = vr.hit_sets(pts, sample, cell, lv['indices'], lv['shape'], lv['stride'], case.VOXEL, case.RANGE, qr, radius, nsample)
            # the inputs' own clearance from a last-ulp difference of cosf / sinf, as the generator demands of its cases
            real = np.repeat(np.abs(rois.reshape(-1, 7)).sum(1) > 0, G ** 3)
            c = vr.cell_coordinate(pts[real], case.RANGE, case.VOXEL).astype(np.float64) / lv['stride']
            assert np.abs(c - np.round(c)).min() >= 1e-3 and margin >= 1e-4, (tag, src, margin)
            cache[(tag, src)] = (rois, G, hits, offs)
        return cache[(tag, src)]
    return get


def put(arena, src, misalign_bytes=0, poison=None):
    src = torch.as_tensor(src)
    return arena.put(src, misalign_bytes, poison) if src.numel() else src.to(arena.buf.device)


# ---- the site index -------------------------------------------------------------------------------------------------------
def raw_site_index(arena, idx_np, B, shape):
    arena.reset()
    D, H, W = shape
    P = len(idx_np)
    idx = put(arena, idx_np.reshape(-1, 4), misalign_bytes=4, poison=[0, 1, 1, 1])
    nbytes = _native.lib().pdm_sparse_index_workspace_bytes(P, B, D, H, W)
    assert nbytes > 0
    ws = arena.carve(nbytes, torch.uint8, 8)
    _native.call("pdm_sparse_index", _native.stream(ws), P, idx.data_ptr(), B, D, H, W, ws.data_ptr(), nbytes)
    torch.cuda.synchronize()
    arena.check()
    return ws.cpu().numpy().copy()


def index_sections(ws, P, ncell):
    """(bits as one bool per cell, gprefix, row_of_rank) of a site-index workspace (the layout of csrc/sc_index.h)"""
    a256 = lambda v: (v + 255) & ~255      # noqa: E731
    ngroups = (ncell + 255) // 256
    nwords, ntiles = 8 * ngroups, (ngroups + 2047) // 2048
    at_prefix = a256(4 * nwords)
    at_rows = at_prefix + a256(4 * ngroups) + a256(4 * ntiles)
    words = ws[:4 * nwords].view(np.uint32)
    bits = ((words[:, None] >> np.arange(32, dtype=np.uint32)) & 1).astype(bool).reshape(-1)
    return bits, ws[at_prefix:at_prefix + 4 * ngroups].view(np.int32), ws[at_rows:at_rows + 4 * P].view(np.int32)


@pytest.mark.parametrize("P", [1, 65, None])
def test_site_index_returns_every_row_and_nothing_else(arena, P):
    """row_of_rank[rank(key)] is the row, for rows in shuffled order; exactly the P cells of the rows are set, so an unset cell
    tests false; the group prefixes are the popcounts in front of each group of 256 cells; two runs give equal bytes."""
    idx = scr.r1_indices(P)
    D, H, W = scr.R1_SHAPE
    ncell = scr.R1_B * D * H * W
    ws = raw_site_index(arena, idx, scr.R1_B, scr.R1_SHAPE)
    bits, gprefix, row_of_rank = index_sections(ws, len(idx), ncell)
    key = scr.site_key(idx, scr.R1_SHAPE)
    assert bits[key].all() and int(bits.sum()) == len(idx) and not bits[ncell:].any()
    before = np.concatenate([[0], np.cumsum(bits)])            # set cells in front of every cell
    assert np.array_equal(row_of_rank[before[key]], np.arange(len(idx)))
    assert np.array_equal(gprefix, before[np.arange(len(gprefix)) * 256])
    assert np.array_equal(ws, raw_site_index(arena, idx, scr.R1_B, scr.R1_SHAPE))


def test_site_index_of_no_row_and_its_host_reads(dev):
    before = sparse_conv_ops.HOST_READS
    empty = sparse_conv_ops.site_index(torch.zeros((0, 4), dtype=torch.int32, device=dev), 2, (5, 2, 3))
    full = sparse_conv_ops.site_index(torch.from_numpy(scr.r1_indices()).to(dev), scr.R1_B, scr.R1_SHAPE)
    torch.cuda.synchronize()
    assert sparse_conv_ops.HOST_READS == before
    assert empty.num_rows == 0 and not bool(empty.workspace[:8].any()) and full.spatial_shape == scr.R1_SHAPE


# ---- the fused pooling, raw -----------------------------------------------------------------------------------------------
def run_pool(arena, rois, G, indices, shape, stride, voxel, rng0, f_in, wp, sp, hp, qr, radius, nsample, wout, so, ho, out_stride=None, out_offset=0):
    """pdm_sparse_index + pdm_roi_grid_pool on arena views -> (M, C2) numpy; the other columns of the output rows must stay as carved"""
    arena.reset()
    dev = arena.buf.device
    B, n = rois.shape[0], rois.shape[1]
    D, H, W = shape
    P, C1, C2 = len(indices), wp.shape[0], wout.shape[0]
    M = B * n * G ** 3
    out_stride = C2 if out_stride is None else out_stride
    nan = float('nan')
    idx = put(arena, np.asarray(indices, np.int32).reshape(-1, 4), 4, [0, 0, 0, 0])
    nbytes = _native.lib().pdm_sparse_index_workspace_bytes(P, B, D, H, W)
    ws = arena.carve(nbytes, torch.uint8, 8)
    _native.call("pdm_sparse_index", _native.stream(dev), P, idx.data_ptr(), B, D, H, W, ws.data_ptr(), nbytes)
    t_rois = put(arena, np.asarray(rois, np.float32), 4, nan)
    t_f = put(arena, np.asarray(f_in, np.float32), 4, nan)
    small = [put(arena, np.asarray(t, np.float32), 4, nan) for t in (wp, sp, hp, so, ho)]
    wpack = sparse_conv_ops.pack_weight(torch.from_numpy(np.asarray(wout, np.float32)).to(dev).reshape(C2, 1, 1, 1, C1))
    out = arena.carve((M, out_stride), torch.float32, 4)
    out.fill_(-7.0)
    _native.call("pdm_roi_grid_pool", _native.stream(dev), B, n, rois.shape[2], t_rois.data_ptr(), G, D, H, W, stride, *voxel, *rng0[:3], P,
                 ws.data_ptr(), nbytes, C1, t_f.data_ptr(), small[0].data_ptr(), small[1].data_ptr(), small[2].data_ptr(), *qr, radius, nsample, C2,
                 wpack.data_ptr(), small[3].data_ptr(), small[4].data_ptr(), out.data_ptr(), out_stride, out_offset)
    torch.cuda.synchronize()
    arena.check()
    got = out.cpu().numpy()
    untouched = np.ones(out_stride, bool)
    untouched[out_offset:out_offset + C2] = False
    assert (got[:, untouched] == -7.0).all(), 'columns outside [out_offset, out_offset + C2) were written'
    return got[:, out_offset:out_offset + C2]


def test_known_answers_first_nsample_in_window_order_empty_group_and_no_wrap(arena):
    """Grid (B 2, D 8, H 8, W 8) of unit voxels from the origin, G = 1 (the grid point is the RoI's centre), window 3 x 3 x 3,
    radius 1.1, nsample 3, C1 = C2 = 16, Wp = 0, Wout = identity, scale 1, shift_p[c] = 0.25 (c even) / -0.5 (c odd), shift_o = 0:
    out[c] = max over the group of relu(f[row][c] + shift_p[c]).
    RoI 0 at the centre of cell (4, 4, 4) with all 27 cells of its window set: the 7 cells within 1.1 are, in window order (z
    outermost, x innermost), z-1, y-1, x-1, centre, x+1, y+1, z+1; the first 3 carry f = 1, 2, 3, the other four 100 and the 20
    cells out of the radius 1000: out = 3.25 / 2.5.  The same cells of sample 1 carry 5000 and must not be taken.
    RoI 1 at the centre of cell z = 7, y = 2, x = 7 (the last z and x): only that cell is set around it (f = 7), and the cell
    (z 0, y 3, x 7), whose key follows it, and (z 0, y 0, x 0) of sample 1 carry 9000: out = 7.25 / 6.5.
    RoI 2 over empty cells: an empty group, out = relu(shift_p) = 0.25 / 0.  Sample 1's RoIs: two over empty cells and one at the
    centre of (4, 4, 4), which takes sample 1's own first three cells: 5000.25 / 4999.5."""
    order = [(-1, 0, 0), (0, -1, 0), (0, 0, -1), (0, 0, 0), (0, 0, 1), (0, 1, 0), (1, 0, 0)]
    idx, f = [], []
    for b, scale in ((0, 1.0), (1, None)):
        for dz in (-1, 0, 1):
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    idx.append((b, 4 + dz, 4 + dy, 4 + dx))
                    k = order.index((dz, dy, dx)) if (dz, dy, dx) in order else -1
                    f.append(5000.0 if scale is None else (1000.0 if k < 0 else (float(k + 1) if k < 3 else 100.0)))
    idx += [(0, 7, 2, 7), (0, 0, 3, 7), (1, 0, 0, 0)]
    f += [7.0, 9000.0, 9000.0]
    rng = np.random.default_rng(1)
    perm = rng.permutation(len(idx))
    idx, f = np.array(idx, np.int32)[perm], np.array(f, np.float32)[perm]
    f_in = np.repeat(f[:, None], 16, 1)
    rois = np.zeros((2, 3, 7), np.float32)
    rois[0, 0] = [4.5, 4.5, 4.5, 2.0, 1.0, 3.0, 0.7]
    rois[0, 1] = [7.5, 2.5, 7.5, 1.0, 1.0, 1.0, 0.0]
    rois[0, 2] = [1.5, 6.5, 1.5, 1.0, 1.0, 1.0, 0.0]
    rois[1, 0] = [1.5, 6.5, 1.5, 1.0, 1.0, 1.0, 0.0]
    rois[1, 1] = [4.5, 4.5, 4.5, 1.0, 1.0, 1.0, 0.0]
    rois[1, 2] = [6.5, 1.5, 6.5, 1.0, 1.0, 1.0, 0.0]
    hp = np.where(np.arange(16) % 2 == 0, 0.25, -0.5).astype(np.float32)
    one = np.ones(16, np.float32)
    got = run_pool(arena, rois, 1, idx, (8, 8, 8), 1, [1.0, 1.0, 1.0], [0.0, 0.0, 0.0], f_in, np.zeros((16, 3), np.float32), one, hp, (1, 1, 1), 1.1, 3,
                   np.eye(16, dtype=np.float32), one, np.zeros(16, np.float32))
    want = np.stack([np.maximum(v + hp, 0) for v in (3.0, 7.0, 0.0, 0.0, 5000.0, 0.0)])
    assert np.array_equal(got, want), got[:, :2]


@pytest.mark.parametrize("src", list(STRIDES))
def test_hit_sets_agree_exactly_with_the_numpy_restatement(arena, levels, hit_cache, src):
    """Wp = 0, shift_p = 0, Wout = identity over C1 = C2 = 64: out[m][c] is exactly max over the group of f[row][c], 0 for an empty
    group.  With distinct positive random features a missing or an extra row changes the maximum of some channel unless it is the
    largest of its group in none of the 64 (at most (15 / 16)^64 = 1.6 % for a row of a full group of 16); two feature draws."""
    lv, (qr, radius, nsample) = levels[src], QUERY[src]
    rois, G, hits, _ = hit_cache('full', src)
    sizes = np.bincount([len(h) for h in hits], minlength=nsample + 1)
    print(src, 'group sizes', sizes.tolist())
    assert sizes[0] > 0 and sizes[nsample] > 0
    one, zero = np.ones(64, np.float32), np.zeros(64, np.float32)
    for seed in (1, 2):
        f = np.random.default_rng(seed).uniform(0.5, 1.5, (len(lv['indices']), 64)).astype(np.float32)
        want = np.stack([f[h].max(0) if h else zero for h in hits])
        got = run_pool(arena, rois, G, lv['indices'], lv['shape'], lv['stride'], case.VOXEL, case.RANGE, f, np.zeros((64, 3), np.float32), one, zero,
                       qr, radius, nsample, np.eye(64, dtype=np.float32), one, zero)
        assert np.array_equal(got, want)


@pytest.mark.parametrize("c1, c2", [(16, 16), (16, 32), (32, 32), (64, 64)])
@pytest.mark.parametrize("src", list(STRIDES))
@pytest.mark.parametrize("tag", ['small', 'full'])
def test_fused_pooling_matches_the_numpy_restatement(arena, levels, hit_cache, tag, src, c1, c2):
    """small: 3 rois x G = 2, 24 grid points (a partial 16-row tile, a partial workgroup); full: 15 rois x G = 3, 405 grid points
    (several workgroups) with the empty sample, the zero rois and the boxes that leave the range (negative cells).  Strides 2, 4, 8 with three
    windows; the output goes to columns [8, 8 + C2) of rows 8 + C2 + 4 wide.  Bound: the module docstring.  Two runs bit-equal."""
    lv, (qr, radius, nsample) = levels[src], QUERY[src]
    rois, G, hits, offs = hit_cache(tag, src)
    rng = np.random.default_rng(1000 * c1 + c2 + lv['stride'])
    P = len(lv['indices'])
    f = rng.normal(0, 1, (P, c1)).astype(np.float32)
    wp = (rng.normal(0, 0.3, (c1, 3))).astype(np.float32)
    sp, so = (rng.uniform(0.5, 1.5, c).astype(np.float32) * rng.choice([-1, 1], c).astype(np.float32) for c in (c1, c2))
    hp, ho = rng.normal(0, 0.3, c1).astype(np.float32), rng.normal(0, 0.3, c2).astype(np.float32)
    wout = (rng.normal(0, 1, (c2, c1)) / np.sqrt(c1)).astype(np.float32)
    want, A, _ = vr.pool(f, hits, offs, wp, sp, hp, wout, so, ho)
    args = (rois, G, lv['indices'], lv['shape'], lv['stride'], case.VOXEL, case.RANGE, f, wp, sp, hp, qr, radius, nsample, wout, so, ho, c2 + 12, 8)
    got = run_pool(arena, *args)
    ratio = np.abs(got - want) / (2 * (c1 + 4) * U * A)
    print(tag, src, c1, c2, 'grid points', len(hits), 'max err / bound', float(ratio.max()), 'nonzero outputs', float((want > 0).mean()))
    assert np.isfinite(got).all() and (ratio <= 1.0).all()
    assert np.array_equal(got, run_pool(arena, *args)), 'two runs differ'


# ---- the module and the head ----------------------------------------------------------------------------------------------
def sparse_levels(ref, levels, dev):
    from pdm_ssd_amd import spconv
    return {k: spconv.SparseConvTensor(torch.from_numpy(ref[f'{k}.features']).to(dev), torch.from_numpy(levels[k]['indices']).to(dev),
                                       levels[k]['shape'], case.B) for k in case.HEAD_CFG['ROI_GRID_POOL']['FEATURES_SOURCE']}


def built_head(ref, G, dev):
    from pdm_ssd_amd.config import cfg_from_dict
    from pdm_ssd_amd.roi_heads import VoxelRCNNHead
    head = VoxelRCNNHead(backbone_channels=dict(case.BACKBONE_CHANNELS), model_cfg=cfg_from_dict(case.head_cfg(G)), point_cloud_range=case.RANGE,
                         voxel_size=case.VOXEL, num_class=1)
    case.fill_module(head, 100 + G)
    for k, v in head.state_dict().items():
        assert np.array_equal(v.numpy(), ref[f'g{G}.state.{k}']), f'{k}: not the generator\'s parameters'
    return head.to(dev).eval()


def head_batch(ref, levels, G, dev):
    return {'batch_size': case.B, 'rois': torch.from_numpy(ref[f'g{G}.rois']).to(dev),
            'roi_labels': torch.ones(ref[f'g{G}.rois'].shape[:2], dtype=torch.long, device=dev),
            'multi_scale_3d_features': sparse_levels(ref, levels, dev), 'multi_scale_3d_strides': {k: STRIDES[k] for k in STRIDES}}


@pytest.mark.parametrize("G", case.GRID_SIZES)
def test_fused_pooling_matches_the_composed_module_on_the_device(ref, levels, dev, G):
    """The same inputs through NeighborVoxelSAModuleMSG's plain path (dense voxel -> row table, VoxelQueryAndGrouping, Conv2d +
    BatchNorm2d, max-pool, Conv1d + BatchNorm1d) and through the fused operator, level by level, within the module docstring's
    bound (A from the numpy restatement of the same module), and both within it of the restatement."""
    head = built_head(ref, G, dev)
    bd = head_batch(ref, levels, G, dev)
    with torch.no_grad():
        fused = head.roi_grid_pool(bd).flatten(0, 1).cpu().numpy()
        head.use_fused_pool = False
        composed = head.roi_grid_pool(bd).flatten(0, 1).cpu().numpy()
    state = {k[len(f'g{G}.state.'):]: v for k, v in ref.items() if k.startswith(f'g{G}.state.')}
    at = 0
    for i, src in enumerate(case.HEAD_CFG['ROI_GRID_POOL']['FEATURES_SOURCE']):
        cfg = case.HEAD_CFG['ROI_GRID_POOL']['POOL_LAYERS'][src]
        want, _, A, c1 = vr.module_forward(state, f'roi_grid_pool_layers.{i}.', 0, ref[f'g{G}.rois'], G, levels[src]['indices'], ref[f'{src}.features'],
                                           levels[src]['shape'], STRIDES[src], case.VOXEL, case.RANGE, cfg['QUERY_RANGES'][0], cfg['POOL_RADIUS'][0],
                                           cfg['NSAMPLE'][0], with_bound=True)
        bound = 2 * (c1 + 4) * U * A
        cols = slice(at, at + want.shape[1])
        at += want.shape[1]
        worst = [float((np.abs(a - b) / bound).max()) for a, b in ((fused[:, cols], composed[:, cols]), (fused[:, cols], want), (composed[:, cols], want))]
        print(f'G={G} {src}: fused-composed, fused-numpy, composed-numpy err / bound', worst)
        assert max(worst) <= 1.0
    assert at == fused.shape[1]


@pytest.mark.parametrize("G", case.GRID_SIZES)
def test_head_eval_forward_matches_the_reference(ref, levels, dev, G):
    """rcnn_cls, rcnn_reg and batch_box_preds within 1e-4 of the reference's own head on the CPU (the project's fp32 feature
    parity; the generator kept only cases whose outputs move by less than 1e-4 under +-2e-5 on the grid points, and saw 8e-6).  Two runs are
    bit-equal, a graph capture and replay of roi_grid_pool equals the eager run bit for bit, and the pooling reads nothing on the
    host."""
    head = built_head(ref, G, dev)
    bd = head_batch(ref, levels, G, dev)
    before = sparse_conv_ops.HOST_READS
    with torch.no_grad():
        out = head(dict(bd))
    for k in ('rcnn_cls', 'rcnn_reg', 'batch_box_preds', 'batch_cls_preds'):
        err = float(np.abs(out[k].cpu().numpy() - ref[f'g{G}.{k}']).max())
        print(f'G={G} {k}: max err {err:.3g}')
        assert out[k].shape == ref[f'g{G}.{k}'].shape and err <= 1e-4, k
    assert out['cls_preds_normalized'] is False
    with torch.no_grad():
        again = head(dict(bd))
        eager = head.roi_grid_pool(bd).clone()
    assert sparse_conv_ops.HOST_READS == before
    assert all(torch.equal(out[k], again[k]) for k in ('rcnn_cls', 'rcnn_reg', 'batch_box_preds'))
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        replayed = head.roi_grid_pool(bd)
    replayed.fill_(float('nan'))
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(replayed, eager) and float(eager.abs().max()) > 0


def test_a_level_the_fused_operator_refuses_is_pooled_by_the_composed_path(ref, levels, dev):
    """avg_pool on one level: that level takes the plain path, the other the fused one, and the max_pool level's columns are
    the all-fused head's bit for bit"""
    head = built_head(ref, 2, dev)
    bd = head_batch(ref, levels, 2, dev)
    with torch.no_grad():
        fused = head.roi_grid_pool(bd).clone()
        head.roi_grid_pool_layers[0].pool_method = 'avg_pool'
        assert not head.roi_grid_pool_layers[0].fused_supported(2) and head.roi_grid_pool_layers[1].fused_supported(2)
        mixed = head.roi_grid_pool(bd)
    assert torch.equal(mixed[..., 16:], fused[..., 16:]) and torch.isfinite(mixed).all() and not torch.equal(mixed[..., :16], fused[..., :16])


# ---- the detector ---------------------------------------------------------------------------------------------------------
def test_build_voxel_rcnn_eval_forward(dev):
    """sparse_conv_reference.D1's grid, 3000 synthetic points, 2 samples: pred_dicts of the right length with finite boxes and
    scores and labels in range (taken from roi_labels: the anchor head has three class columns); the rois fed to the second
    stage are NMS_POST_MAXSIZE a sample and the pooled features are finite."""
    from pdm_ssd_amd import detector_config as dc
    torch.manual_seed(5)
    g = scr.D1
    cfg = copy.deepcopy(dc.VOXEL_RCNN_CFG)
    cfg['ROI_HEAD']['NMS_CONFIG']['TEST'].update(NMS_PRE_MAXSIZE=48, NMS_POST_MAXSIZE=8)
    cfg['POST_PROCESSING']['SCORE_THRESH'] = 0.0
    model = dc.build_voxel_rcnn(cfg, dataset=dc.voxel_dataset(4, g['range'], g['voxel'], g['grid'])).to(dev).eval()
    assert [type(m).__name__ for m in model.module_list] == ['DynamicMeanVFE', 'VoxelBackBone8x', 'HeightCompression', 'BaseBEVBackbone',
                                                             'AnchorHeadSingle', 'VoxelRCNNHead']
    rng = np.random.default_rng(21)
    n = 3000
    centres = rng.uniform([1, -3, -2.5], [15, 3, 0.5], (12, 3))
    p = centres[rng.integers(0, 12, n)] + rng.normal(0, 0.6, (n, 3))
    pts = torch.from_numpy(np.concatenate([rng.integers(0, 2, (n, 1)), p, rng.uniform(0, 1, (n, 1))], 1).astype(np.float32)).to(dev)
    seen = {}
    model.roi_head.register_forward_hook(lambda m, a, out: seen.update(rois=out['rois'], labels=out['roi_labels'], cls=out['rcnn_cls']))
    with torch.no_grad():
        pred, _ = model({'batch_size': g['B'], 'points': pts})
    assert seen['rois'].shape == (g['B'], 8, 7) and seen['cls'].shape == (g['B'] * 8, 1) and torch.isfinite(seen['cls']).all()
    assert len(pred) == g['B']
    total = 0
    for b, d in enumerate(pred):
        k = d['pred_boxes'].shape[0]
        total += k
        assert d['pred_boxes'].shape == (k, 7) and d['pred_scores'].shape == (k,) and d['pred_labels'].shape == (k,)
        assert torch.isfinite(d['pred_boxes']).all() and torch.isfinite(d['pred_scores']).all()
        assert bool(((d['pred_labels'] >= 1) & (d['pred_labels'] <= 3)).all())
        assert set(d['pred_labels'].tolist()) <= set(seen['labels'][b].tolist())
    assert total > 0

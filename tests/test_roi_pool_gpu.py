"""RoI point pooling and RoI-aware pooling on the device (csrc/roi_pool.hip) against the numpy restatement of the
reference launchers (tests/roi_pool_reference.py), the reference's own Python run (tests/golden/ref_roi.npz) and the
existing pdm_points_in_boxes kernel."""
import ctypes
import os

import numpy as np
import pytest
import torch

import roi_pool_reference as rp
from pdm_ssd_amd import _native

HERE = os.path.dirname(os.path.abspath(__file__))
F = np.float32


@pytest.fixture(scope='module', autouse=True)
def _oracle(oracle):
    return oracle


@pytest.fixture(scope='module')
def fix():
    return dict(np.load(os.path.join(HERE, 'golden', 'ref_roi.npz')))


def stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


def bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


def c_point_pool(dev, xyz, boxes, feats, S, fill=7.0):
    """pdm_roipoint_pool3d over `fill`-filled rows and -5 flags -> (pooled, flag) numpy."""
    B, N, M, C = xyz.shape[0], xyz.shape[1], boxes.shape[1], feats.shape[2]
    t = [torch.from_numpy(np.ascontiguousarray(a, dtype=F)).to(dev) for a in (xyz, boxes, feats)]
    pooled = torch.full((B, M, S, 3 + C), fill, dtype=torch.float32, device=dev)
    flag = torch.full((B, M), -5, dtype=torch.int32, device=dev)
    _native.call('pdm_roipoint_pool3d', stream(dev), B, N, M, C, S, t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(),
                 pooled.data_ptr(), flag.data_ptr())
    torch.cuda.synchronize()
    return pooled.cpu().numpy(), flag.cpu().numpy()


def restated_point_pool(xyz, boxes, feats, S, fill=7.0):
    pooled = np.full((xyz.shape[0], boxes.shape[1], S, 3 + feats.shape[2]), fill, dtype=F)
    flag = np.zeros((xyz.shape[0], boxes.shape[1]), dtype=np.int32)     # the kernel writes every flag: 0 unless empty
    rp.roipoint_pool3d(F(xyz), F(boxes), F(feats), pooled, flag)
    return pooled, flag


def clear_scene(seed, B, N, M, C):
    """uniform points in a 10 x 10 x 2 block, M boxes with random headings (the last one far away: empty), no point
    within 1e-4 of a face plane (so host and device cosf cannot disagree on a membership)."""
    while True:
        rng = np.random.default_rng(seed)
        xyz = np.stack([rng.uniform(0, 10, (B, N)), rng.uniform(0, 10, (B, N)), rng.uniform(-1, 1, (B, N))], -1).astype(F)
        boxes = np.zeros((B, M, 7), dtype=F)
        boxes[..., 0:2] = rng.uniform(2, 8, (B, M, 2))
        boxes[..., 3:6] = rng.uniform(1.5, 5, (B, M, 3))
        boxes[..., 6] = rng.uniform(-np.pi, np.pi, (B, M))
        if M > 1:
            boxes[:, -1, 0] += 50
        feats = rng.standard_normal((B, N, C)).astype(F)
        if all(rp.face_clearance(xyz[b], boxes[b]) > 1e-4 for b in range(B)):
            return xyz, boxes, feats
        seed += 1000


@pytest.mark.gpu
def test_point_pool_abi_matches_the_restatement_on_the_fixture_scene(dev, fix):
    boxes = fix['a_boxes'] + F([0, 0, 0, 0.2, 0.2, 0.2, 0])
    got, flag = c_point_pool(dev, fix['a_xyz'], boxes, fix['a_feats'], 16)
    want, wflag = restated_point_pool(fix['a_xyz'], boxes, fix['a_feats'], 16)
    assert (flag == wflag).all() and flag[:, 4].tolist() == [1, 1] and flag[:, :4].sum() == 0
    assert (bits(got) == bits(want)).all()
    assert (got[:, 4] == 7.0).all()                     # the empty box's rows are not written
    assert (got[:, :4, :, 0:3] != 7.0).any()


@pytest.mark.gpu
@pytest.mark.parametrize('B,N,M,C,S', [(1, 7, 3, 2, 4),        # fewer points than a wave; a 5-float row
                                         (2, 300, 4, 5, 1),      # S = 1
                                         (1, 40, 3, 1, 64),      # S > N
                                         (2, 300, 4, 0, 16),     # no features: rows of 3 floats
                                         (2, 1500, 3, 130, 24)])  # several blocks of 256 points, a 133-float row
def test_point_pool_abi_shapes(dev, B, N, M, C, S):
    xyz, boxes, feats = clear_scene(B * 7 + N, B, N, M, C)
    boxes[0, 0] = 0                                    # an all-zero padding row: holds no point
    got, flag = c_point_pool(dev, xyz, boxes, feats, S)
    want, wflag = restated_point_pool(xyz, boxes, feats, S)
    assert (flag == wflag).all() and flag[0, 0] == 1 and (flag == 0).any()
    assert (bits(got) == bits(want)).all()


@pytest.mark.gpu
def test_point_pool_abi_more_hits_than_the_index_list_holds(dev):
    """The kernel keeps 2048 hit indices between its search and its row copies: S = 3000 with 5000 hits takes two rounds
    (the second resumes inside a block of points), and 2048 < cnt < S wraps by re-reading the rows already written."""
    N, S = 5000, 3000
    seed = 77
    while True:
        rng = np.random.default_rng(seed)
        xyz = np.stack([rng.uniform(0, 10, (1, N)), rng.uniform(0, 10, (1, N)), rng.uniform(-1, 1, (1, N))], -1).astype(F)
        boxes = F([[[5, 5, 0, 30, 30, 10, 0.3], [5, 2.5, 0, 12, 5.2, 4, 0.0], [5, 5, 0, 3, 3, 1, -1.1]]])
        counts = [int(rp.in_box_mask(xyz[0], bx).sum()) for bx in boxes[0]]
        if rp.face_clearance(xyz[0], boxes[0]) > 1e-4 and counts[0] == N and 2048 < counts[1] < S and 0 < counts[2] < 2048:
            break
        seed += 1
    feats = np.arange(N, dtype=F).reshape(1, N, 1)
    got, flag = c_point_pool(dev, xyz, boxes, feats, S)
    want, _ = restated_point_pool(xyz, boxes, feats, S)
    assert (flag == 0).all()
    assert (bits(got) == bits(want)).all()


@pytest.mark.gpu
def test_point_pool_abi_zero_sizes_write_nothing(dev):
    xyz, boxes, feats = clear_scene(5, 1, 20, 2, 1)
    for B, N, M, S in [(0, 20, 2, 4), (1, 20, 0, 4), (1, 0, 2, 4), (1, 20, 2, 0)]:
        got, flag = c_point_pool(dev, xyz[:B, :N], boxes[:B, :M], feats[:B, :N], S)
        assert (got == 7.0).all() and (flag == -5).all()


@pytest.mark.gpu
def test_point_pool_agrees_with_points_in_boxes_next_to_the_faces(dev):
    """GPU against GPU, no host trigonometry: with S = N nothing is truncated, so the set of pooled point indices of a box
    is exactly the set of points pdm_points_in_boxes assigns to that box alone — including 200 points placed within 1e-6
    of the faces, where the outcome hangs on the last bit of the shared device function."""
    from pdm_ssd_amd.iou3d_nms.iou3d_nms_utils import points_in_boxes_gpu
    B, N, M = 2, 2048, 8
    rng = np.random.default_rng(31)
    xyz = np.stack([rng.uniform(0, 20, (B, N)), rng.uniform(0, 20, (B, N)), rng.uniform(-1, 1, (B, N))], -1)
    boxes = np.zeros((B, M, 7))
    boxes[..., 0:2] = rng.uniform(4, 16, (B, M, 2))
    boxes[..., 3:6] = rng.uniform(2, 6, (B, M, 3))
    boxes[..., 6] = rng.uniform(-np.pi, np.pi, (B, M))
    for b in range(B):
        for j in range(100):                                           # 100 per sample: 200 in all
            bx = boxes[b, rng.integers(M)]
            local = rng.uniform(-0.5, 0.5, 3) * bx[3:6]
            axis = rng.integers(3)
            local[axis] = (bx[3 + axis] / 2 + rng.uniform(-1e-6, 1e-6)) * rng.choice([-1, 1])
            c, s = np.cos(bx[6]), np.sin(bx[6])
            xyz[b, j] = [bx[0] + local[0] * c - local[1] * s, bx[1] + local[0] * s + local[1] * c, bx[2] + local[2]]
    xyz, boxes = xyz.astype(F), boxes.astype(F)
    index = np.broadcast_to(np.arange(N, dtype=F)[None, :, None], (B, N, 1))
    got, flag = c_point_pool(dev, xyz, boxes, index, N)
    near = 0
    for m in range(M):
        owner = points_in_boxes_gpu(torch.from_numpy(xyz).to(dev), torch.from_numpy(boxes[:, m:m + 1].copy()).to(dev)).cpu().numpy()
        for b in range(B):
            want = set(np.nonzero(owner[b] == 0)[0].tolist())
            have = set() if flag[b, m] == 1 else set(got[b, m, :, 3].astype(np.int64).tolist())
            assert have == want, (b, m, sorted(have ^ want))
            assert (flag[b, m] == 1) == (len(want) == 0)
            near += len(want & set(range(100)))
    assert near > 20        # the face points do fall on both sides


@pytest.mark.gpu
def test_point_pool_module_matches_the_reference_module_bit_for_bit(dev, fix):
    from pdm_ssd_amd.roipoint_pool3d.roipoint_pool3d_utils import RoIPointPool3d
    layer = RoIPointPool3d(num_sampled_points=16, pool_extra_width=[0.2, 0.2, 0.2])
    feats = torch.from_numpy(fix['a_feats']).to(dev).requires_grad_(True)
    pooled, flag = layer(torch.from_numpy(fix['a_xyz']).to(dev), feats, torch.from_numpy(fix['a_boxes']).to(dev))
    assert flag.dtype == torch.int32 and not flag.requires_grad
    assert (flag.cpu().numpy() == fix['a_flag']).all()
    assert (bits(pooled.detach().cpu().numpy()) == bits(fix['a_pooled'])).all()
    with pytest.raises(NotImplementedError):
        pooled.sum().backward()


@pytest.mark.gpu
@pytest.mark.parametrize('case', ['d', 'e'])
def test_canonical_pool_matches_the_reference_head_pooling(dev, fix, case):
    """Fixture (c): PointRCNNHead.roipool3d_gpu of the reference.  Local coordinates are below 8 m and take four fp32
    roundings of 2^-24 relative each: the error stays below about 2e-6; 1e-5 leaves 5x."""
    from pdm_ssd_amd.roipoint_pool3d.roipoint_pool3d_utils import roipoint_pool3d_canonical
    import roi_head_case
    rois, feats = fix[f'{case}_rois'], fix[f'{case}_feats_all']
    B = rois.shape[0]
    xyz = fix[f'{case}_coords'][:, 1:4].reshape(B, -1, 3)
    pooled, flag = roipoint_pool3d_canonical(torch.from_numpy(xyz).to(dev), torch.from_numpy(feats.reshape(B, xyz.shape[1], -1)).to(dev),
                                             torch.from_numpy(rois).to(dev), roi_head_case.HEAD_CFG['ROI_POINT_POOL']['POOL_EXTRA_WIDTH'], 32)
    got = pooled.cpu().numpy().reshape(fix[f'{case}_pooled'].shape)
    want = fix[f'{case}_pooled']
    assert np.abs(got[..., 0:3] - want[..., 0:3]).max() <= 1e-5
    assert (bits(got[..., 3:]) == bits(want[..., 3:])).all()
    empty = flag.cpu().numpy().reshape(-1) == 1
    assert empty.tolist() == [False] * 4 + [True] * 2 + [False] * 4 + [True] * 2
    assert (bits(got[empty]) == 0).all()                # exact zeros although `pooled` was torch.empty


# ---- RoI-aware pooling -----------------------------------------------------------------------------------------------------
def c_aware(dev, rois, pts, feats, out, max_pts, method):
    """pdm_roiaware_pool3d_forward over garbage-filled index / argmax tensors and zero-filled pooled -> numpy."""
    out = (out,) * 3 if isinstance(out, int) else tuple(out)
    t = [torch.from_numpy(np.ascontiguousarray(a, dtype=F)).to(dev) for a in (rois, pts, feats)]
    K, P, C = t[0].shape[0], t[1].shape[0], t[2].shape[1]
    idx = torch.full((K, *out, max_pts), -77, dtype=torch.int32, device=dev)
    am = torch.full((K, *out, C), -77, dtype=torch.int32, device=dev)
    pooled = torch.zeros((K, *out, C), dtype=torch.float32, device=dev)
    nbytes = _native.lib().pdm_roiaware_pool3d_workspace_bytes(K, *out)
    ws = torch.empty(max(nbytes, 8), dtype=torch.uint8, device=dev)
    _native.call('pdm_roiaware_pool3d_forward', stream(dev), K, P, C, max_pts, *out, t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(),
                 method, ws.data_ptr(), nbytes, idx.data_ptr(), am.data_ptr(), pooled.data_ptr())
    torch.cuda.synchronize()
    return idx.cpu().numpy(), am.cpu().numpy(), pooled.cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize('tag,out', [('b3', (3, 2, 4)), ('b1', 1)])
@pytest.mark.parametrize('method', ['max', 'avg'])
def test_aware_forward_matches_the_reference_bit_for_bit(dev, fix, tag, out, method):
    idx, am, pooled = c_aware(dev, fix[f'{tag}_rois'], fix[f'{tag}_pts'], fix[f'{tag}_feats'], out, 4, 0 if method == 'max' else 1)
    assert (idx == fix[f'{tag}_{method}_pts_idx']).all()            # fully written: the -77 fill is gone
    assert (bits(pooled) == bits(fix[f'{tag}_{method}_pooled'])).all()
    if method == 'max':
        assert (am == fix[f'{tag}_max_argmax']).all()
    else:
        assert (am == -77).all()                                   # avg mode does not write argmax
    # and through the module
    from pdm_ssd_amd.roiaware_pool3d.roiaware_pool3d_utils import RoIAwarePool3d
    res = RoIAwarePool3d(out, 4)(torch.from_numpy(fix[f'{tag}_rois']).to(dev), torch.from_numpy(fix[f'{tag}_pts']).to(dev),
                                 torch.from_numpy(fix[f'{tag}_feats']).to(dev), pool_method=method)
    assert (bits(res.cpu().numpy()) == bits(fix[f'{tag}_{method}_pooled'])).all()


@pytest.mark.gpu
def test_aware_forward_hand_cases_on_the_device(dev):
    box = F([[4, 2, 0, 4, 2, 2, 0]])
    idx, _, _ = c_aware(dev, box, [[6, 2, 0], [2, 2, 0]], [[1], [2]], (4, 1, 1), 4, 0)       # on the +dx/2 and -dx/2 faces
    assert idx[0, 3, 0, 0].tolist() == [1, 0, 0, 0] and idx[0, 0, 0, 0].tolist() == [1, 1, 0, 0] and (idx[0, 1:3, 0, 0] == 0).all()
    pts = [[4 + 0.125 * i, 2, 0] for i in range(6)]
    idx, am, pooled = c_aware(dev, box, pts, [[1], [9], [3], [50], [60], [70]], 1, 4, 0)       # the cap max_pts - 1
    assert idx[0, 0, 0, 0].tolist() == [3, 0, 1, 2] and am[0, 0, 0, 0, 0] == 1 and pooled[0, 0, 0, 0, 0] == 9
    pts = [[4, 2, 0], [4.5, 2, 0], [5, 2, 0]]
    _, am, pooled = c_aware(dev, box, pts, [[5, -3, np.nan], [5, -2, -np.inf], [1, -2, -4]], 1, 8, 0)   # ties, negatives, NaN
    assert am[0, 0, 0, 0].tolist() == [0, 1, 2] and pooled[0, 0, 0, 0].tolist() == [5, -2, -4]
    _, am, pooled = c_aware(dev, box, [[50, 2, 0]], [[5, -3]], 1, 8, 0)                        # no point: -1, pooled untouched
    assert am[0, 0, 0, 0].tolist() == [-1, -1] and pooled[0, 0, 0, 0].tolist() == [0, 0]
    a, b, c = F(2 ** 24), F(1), F(-2 ** 24)
    _, _, pooled = c_aware(dev, box, pts, [[a, a], [b, c], [c, b]], 1, 8, 1)                   # the average's sum order
    assert pooled[0, 0, 0, 0].tolist() == [0, F(1) / F(3)]


@pytest.mark.gpu
def test_aware_forward_counts_in_the_workspace_for_a_large_grid(dev, fix):
    """more than 8192 voxels per box: the counters live in the caller's workspace (same lists as the restatement)."""
    rois, pts, feats = fix['b3_rois'][:2], fix['b3_pts'], fix['b3_feats']
    out = (32, 32, 9)
    assert _native.lib().pdm_roiaware_pool3d_workspace_bytes(2, *out) == 2 * 32 * 32 * 9 * 4
    assert rp.voxel_clearance(pts, rois, out) > 1e-4
    idx, am, pooled = c_aware(dev, rois, pts, feats, out, 3, 0)
    widx = np.zeros(idx.shape, dtype=np.int32)
    wam, wp = np.zeros(am.shape, dtype=np.int32), np.zeros(pooled.shape, dtype=F)
    rp.roiaware_pool3d_forward(rois, pts, feats, wam, widx, wp, 0)
    assert (idx == widx).all() and (am == wam).all() and (bits(pooled) == bits(wp)).all()


@pytest.mark.gpu
def test_aware_forward_workspace_counters_with_crowded_voxels(dev):
    """A grid above 8192 voxels (counters in the workspace) with 1500 points crowded into a few dozen voxels: every
    voxel is revisited across many groups of 64 points and most lists overflow the cap."""
    out, max_pts, P = (32, 32, 9), 6, 1500
    seed = 11
    while True:
        rng = np.random.default_rng(seed)
        rois = F([[3, 3, 0, 6.4, 6.4, 1.8, 0.4], [3.2, 2.9, 0.1, 6.0, 5.0, 1.7, -0.9]])
        pts = np.concatenate([rng.normal([3.3, 2.7, 0.1], [0.25, 0.25, 0.15], (P - 300, 3)),
                              np.stack([rng.uniform(0, 6, 300), rng.uniform(0, 6, 300), rng.uniform(-1, 1, 300)], -1)]).astype(F)
        pts = pts[rng.permutation(P)]
        if rp.face_clearance(pts, rois) > 1e-4 and rp.voxel_clearance(pts, rois, out) > 1e-4:
            break
        seed += 1
    feats = rng.standard_normal((P, 2)).astype(F)
    assert _native.lib().pdm_roiaware_pool3d_workspace_bytes(2, *out) > 0
    for method in (0, 1):
        idx, am, pooled = c_aware(dev, rois, pts, feats, out, max_pts, method)
        widx = np.zeros(idx.shape, dtype=np.int32)
        wam, wp = np.full(am.shape, -77, dtype=np.int32), np.zeros(pooled.shape, dtype=F)
        rp.roiaware_pool3d_forward(rois, pts, feats, wam, widx, wp, method)
        assert (widx[..., 0] == max_pts - 1).sum() > 20          # many capped lists
        assert (idx == widx).all() and (am == wam).all() and (bits(pooled) == bits(wp)).all()


@pytest.mark.gpu
@pytest.mark.parametrize('method', ['max', 'avg'])
def test_aware_backward_through_autograd(dev, fix, method):
    """fp32 sums of a few terms against a float64 accumulation: within 1e-6 of the sum of the absolute terms."""
    from pdm_ssd_amd.roiaware_pool3d.roiaware_pool3d_utils import RoIAwarePool3d
    rois, pts, feats = (torch.from_numpy(fix[f'b3_{k}']).to(dev) for k in ('rois', 'pts', 'feats'))
    lists, am = fix[f'b3_{method}_pts_idx'], fix['b3_max_argmax']
    in0, in1 = set(lists[0, ..., 1:][lists[0, ..., 1:] > 0].tolist()), set(lists[1, ..., 1:][lists[1, ..., 1:] > 0].tolist())
    shared = in0 & in1
    assert shared                                                   # a point listed by both overlapping boxes
    grad_out = np.random.default_rng(3).standard_normal(fix[f'b3_{method}_pooled'].shape).astype(F)
    want = np.zeros(fix['b3_feats'].shape, dtype=np.float64)
    scale = rp.roiaware_pool3d_backward(lists, am, grad_out, want, 0 if method == 'max' else 1)
    runs = []
    for _ in range(2):
        f = feats.clone().requires_grad_(True)
        res = RoIAwarePool3d((3, 2, 4), 4)(rois, pts, f, pool_method=method)
        res.backward(torch.from_numpy(grad_out).to(dev))
        runs.append(f.grad.cpu().numpy())
    assert (bits(runs[0]) == bits(runs[1])).all()
    assert (np.abs(runs[0] - want) <= 1e-6 * scale).all()
    assert (scale[sorted(shared)] > 0).any() and (scale == 0).any()
    # the C entry point over a garbage-filled grad_in: fully overwritten, same bits
    g = torch.full(feats.shape, float('nan'), dtype=torch.float32, device=dev)
    idx_t, am_t, go = torch.from_numpy(lists).to(dev), torch.from_numpy(am).to(dev), torch.from_numpy(grad_out).to(dev)
    _native.call('pdm_roiaware_pool3d_backward', stream(dev), 4, 200, 3, 4, 3, 2, 4, rois.data_ptr(), pts.data_ptr(), idx_t.data_ptr(),
                 am_t.data_ptr(), go.data_ptr(), 0 if method == 'max' else 1, g.data_ptr())
    torch.cuda.synchronize()
    assert (bits(g.cpu().numpy()) == bits(runs[0])).all()


def test_bad_arguments_are_refused_before_any_launch():
    """(no GPU is touched: the checks come first)"""
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    fwd = lambda *a: _native.call('pdm_roiaware_pool3d_forward', 0, *a)     # noqa: E731
    with pytest.raises(_native.NativeLibraryError, match='out size'):
        fwd(1, 4, 1, 4, 257, 2, 2, p, p, p, 0, None, 0, p, p, p)
    with pytest.raises(_native.NativeLibraryError, match='max_pts'):
        fwd(1, 4, 1, 1, 2, 2, 2, p, p, p, 0, None, 0, p, p, p)
    with pytest.raises(_native.NativeLibraryError, match='null pointer'):
        fwd(1, 4, 1, 4, 2, 2, 2, None, p, p, 0, None, 0, p, p, p)
    with pytest.raises(_native.NativeLibraryError, match='workspace'):
        fwd(1, 4, 1, 4, 64, 64, 64, p, p, p, 0, None, 0, p, p, p)
    with pytest.raises(_native.NativeLibraryError, match='out size'):
        _native.call('pdm_roiaware_pool3d_backward', 0, 1, 4, 1, 4, 2, 0, 2, p, p, p, p, p, 0, p)
    with pytest.raises(_native.NativeLibraryError, match='null pointer'):
        _native.call('pdm_roiaware_pool3d_backward', 0, 1, 4, 1, 4, 2, 2, 2, p, p, p, p, p, 0, None)
    with pytest.raises(_native.NativeLibraryError, match='null pointer'):
        _native.call('pdm_roipoint_pool3d', 0, 1, 4, 1, 1, 4, p, None, p, p, p)
    with pytest.raises(_native.NativeLibraryError, match='null pointer'):
        _native.call('pdm_roipoint_pool3d_canonical', 0, 1, 4, 1, 1, 4, p, p, 7, 0.0, 0.0, 0.0, None, p, p)
    with pytest.raises(_native.NativeLibraryError, match='roi_stride'):
        _native.call('pdm_roipoint_pool3d_canonical', 0, 1, 4, 1, 1, 4, p, p, 6, 0.0, 0.0, 0.0, p, p, p)
    with pytest.raises(_native.NativeLibraryError, match='S=-1'):
        _native.call('pdm_roipoint_pool3d', 0, 1, 4, 1, 1, -1, p, p, p, p, p)

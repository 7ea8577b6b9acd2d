"""PV-RCNN on the device: pdm_bev_interpolate against bilinear_interpolate_torch on the device and the CPU
fixture, bit for bit, in a poisoned arena; pdm_roi_keypoint_query against pointnet2_stack.ball_query on its own grid points,
exactly; VoxelSetAbstraction, PointHeadSimple and PVRCNNHead against the reference's own modules (tests/golden/ref_pv_rcnn.npz);
build_pv_rcnn() end to end on a small grid."""
import copy
import os
import warnings

import numpy as np
import pytest
import torch

import pv_rcnn_case as case
import pv_rcnn_reference as pr
import sparse_conv_reference as scr
from arena import Arena
from pdm_ssd_amd import _native, pv_rcnn_ops
from pdm_ssd_amd.backbones_3d.pfe.voxel_set_abstraction import VoxelSetAbstraction, bilinear_interpolate_torch
from pdm_ssd_amd.config import cfg_from_dict
from pdm_ssd_amd.pointnet2_stack import pointnet2_utils

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def ref():
    z = np.load(os.path.join(GOLDEN, "ref_pv_rcnn.npz"))
    return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def arena(dev):
    return Arena(dev, 8 << 20)


def load(module, ref, prefix, dev):
    module.load_state_dict({k[len(prefix):]: torch.from_numpy(v) for k, v in ref.items() if k.startswith(prefix)})
    return module.to(dev).eval()


# ---------------------------------------------------------------------------------------------------------------- bev

def bev_case(C):
    """counts [7, 70] on a 6 x 5 map at stride 2 of 0.5 m voxels from (0, -2): keypoints on integer coordinates, beyond each of the
    four borders, at negative coordinates, and random ones"""
    rng = np.random.default_rng(5 + C)
    H, W, cell = 6, 5, 1.0
    special = np.array([[0, 0.0, -2.0, 0], [0, 2.0, 1.0, 0], [0, -0.7, -1.0, 0], [0, 6.3, 0.5, 0], [0, 1.5, -3.2, 0], [0, 2.5, 5.1, 0],
                        [0, -3.0, -6.0, 0]], dtype=np.float32)
    assert len(special) == 7
    rest = np.stack([np.ones(70), rng.uniform(-1.0, W * cell + 1.0, 70), rng.uniform(-3.0, H * cell - 1.0, 70), rng.uniform(-1, 1, 70)], 1)
    rest[:8, 1] = np.arange(8) - 1.0                     # integer x coordinates, two of them outside
    rest[:8, 2] = np.arange(8) - 3.0
    kp = np.concatenate([special, rest]).astype(np.float32)
    bev = rng.normal(0, 1, (2, C, H, W)).astype(np.float32)
    return kp, bev, [0.0, -2.0, -3.0], [0.5, 0.5, 0.1], 2


@pytest.mark.parametrize("C", [5, 64])
def test_bev_interpolate_is_bit_equal_in_a_poisoned_arena(dev, arena, C):
    kp_np, bev_np, r0, vs, stride = bev_case(C)
    arena.reset()
    kp = arena.put(kp_np, poison=[0.0, 1.0, 1.0, 0.0])
    bev = arena.put(bev_np, poison=float('nan'))
    ld = C + 7
    out = arena.carve((len(kp_np), ld), torch.float32)
    out.fill_(-7.0)
    pv_rcnn_ops.bev_interpolate(kp, bev, r0, vs, stride, out=out, col0=3)
    torch.cuda.synchronize()
    arena.check()
    assert bool((out[:, :3] == -7.0).all()) and bool((out[:, 3 + C:] == -7.0).all())
    got = out[:, 3:3 + C]
    x = (kp[:, 1] - kp.new_tensor(r0[0])) / kp.new_tensor(vs[0]) / kp.new_tensor(float(stride))
    y = (kp[:, 2] - kp.new_tensor(r0[1])) / kp.new_tensor(vs[1]) / kp.new_tensor(float(stride))
    want = torch.cat([bilinear_interpolate_torch(bev[b].permute(1, 2, 0), x[kp[:, 0] == b], y[kp[:, 0] == b]) for b in range(2)])
    assert torch.equal(got, want)
    assert np.array_equal(got.cpu().numpy(), pr.bev_interpolate(kp_np, bev_np, r0, vs, stride))
    again = torch.empty_like(out)
    pv_rcnn_ops.bev_interpolate(kp, bev, r0, vs, stride, out=again, col0=3)
    assert torch.equal(again[:, 3:3 + C], got)


def test_bev_interpolate_matches_the_cpu_fixture(ref, dev):
    got = pv_rcnn_ops.bev_interpolate(torch.from_numpy(ref['point_coords']).to(dev), torch.from_numpy(ref['bev']).to(dev), case.RANGE,
                                      case.VOXEL, case.BEV_STRIDE)
    assert np.array_equal(got.cpu().numpy(), ref['point_features_before_fusion'][:, :case.BEV_SHAPE[0]])


# -------------------------------------------------------------------------------------------------------------- query

QUERY_COUNTS = (70, 5, 130)
QUERY_R = 1.2


def query_case(dev):
    rng = np.random.default_rng(23)
    xyz = np.concatenate([np.stack([rng.uniform(1, 9, n), rng.uniform(-3, 3, n), rng.uniform(-2, 0, n)], 1) for n in QUERY_COUNTS]).astype(np.float32)
    xyz[70 + 5:70 + 5 + 60] = np.float32([5.0, 0.0, -1.0]) + rng.normal(0, 0.35, (60, 3)).astype(np.float32)      # a dense blob: more than nsample hits
    rois = case.rois(np.random.default_rng(3))
    rois[2, 0, 0:3] = [5.0, 0.0, -1.0]
    return torch.from_numpy(rois).to(dev), torch.from_numpy(xyz).to(dev), torch.tensor(QUERY_COUNTS, dtype=torch.int32, device=dev)


@pytest.mark.parametrize("G", [2, 3])
def test_roi_keypoint_query_equals_ball_query_on_its_own_grid_points(dev, G):
    rois, xyz, cnt = query_case(dev)
    scales = ((QUERY_R, 16), (2 * QUERY_R, 32))
    grid, idx, empty = pv_rcnn_ops.roi_keypoint_query(rois, G, xyz, cnt, max(QUERY_COUNTS), [s[0] for s in scales], [s[1] for s in scales])
    B, n = rois.shape[:2]
    per = n * G ** 3
    assert per in (40, 135) and grid.shape == (B * per, 3)
    new_cnt = torch.full((B,), per, dtype=torch.int32, device=dev)
    starts = torch.repeat_interleave(torch.cumsum(cnt, 0) - cnt, per)
    sizes = set()
    for s, (radius, ns) in enumerate(scales):
        want_idx, want_empty = pointnet2_utils.ball_query(radius, ns, xyz, cnt, grid, new_cnt)
        assert torch.equal(idx[s], (want_idx + starts[:, None]).int()) and torch.equal(empty[s], want_empty)
        _, _, size, _ = pr.ball_query(radius, ns, xyz.cpu().numpy(), QUERY_COUNTS, grid.cpu().numpy(), [per] * B)
        sizes |= {0 if k == 0 else (1 if k < ns else (2 if k == ns else 3)) for k in size.tolist()}
    assert {0, 1, 3} <= sizes                      # empty balls, partly filled ones, overflowing ones
    # the grid points: three fp32 roundings and the trigonometry away from a float64 evaluation; the torch formulation likewise
    r = rois.view(-1, 7).double().cpu().numpy()
    lattice = np.stack(np.meshgrid(np.arange(G), np.arange(G), np.arange(G), indexing='ij'), -1).reshape(-1, 3)
    local = (lattice[None] + 0.5) / G * r[:, None, 3:6] - r[:, None, 3:6] / 2
    c, s_ = np.cos(r[:, 6])[:, None], np.sin(r[:, 6])[:, None]
    exact = np.stack([local[..., 0] * c - local[..., 1] * s_, local[..., 0] * s_ + local[..., 1] * c, local[..., 2]], -1) + r[:, None, 0:3]
    bound = 4 * 2.0 ** -23 * (np.abs(r[:, None, 0:3]) + np.linalg.norm(r[:, 3:6] / 2, axis=1)[:, None, None])
    assert (np.abs(grid.double().cpu().numpy().reshape(exact.shape) - exact) <= bound).all()
    from pdm_ssd_amd.roi_heads import PVRCNNHead
    head = PVRCNNHead(input_channels=16, model_cfg=cfg_from_dict(case.head_cfg(G)), num_class=1)
    torch_points, _ = head.get_global_grid_points_of_roi(rois, grid_size=G)        # the composed path's grid points, on the device
    assert torch_points.is_cuda and (np.abs(torch_points.double().cpu().numpy().reshape(exact.shape) - exact) <= bound).all()
    assert (np.abs(pr.grid_points(rois.cpu().numpy(), G).astype(np.float64).reshape(exact.shape) - exact) <= bound).all()
    grid2, idx2, empty2 = pv_rcnn_ops.roi_keypoint_query(rois, G, xyz, cnt, max(QUERY_COUNTS), [s[0] for s in scales], [s[1] for s in scales])
    assert torch.equal(grid, grid2) and all(torch.equal(a, b) for a, b in zip(idx + empty, idx2 + empty2))


def test_roi_keypoint_query_refuses_a_count_above_the_cap(dev):
    rois, xyz, cnt = query_case(dev)
    with pytest.raises(_native.NativeLibraryError, match="exceed the cap of 4096"):
        pv_rcnn_ops.roi_keypoint_query(rois, 2, xyz, cnt, pv_rcnn_ops.roi_keypoint_query_cap() + 1, [1.0], [16])


# -------------------------------------------------------------------------------------------------------------- modules

def front_batch(ref, dev):
    levels = {name: type('Level', (), dict(indices=torch.from_numpy(ref[f'{name}.indices']).to(dev),
                                           features=torch.from_numpy(ref[f'{name}.features']).to(dev)))() for name, _, _ in case.LEVELS}
    return {'batch_size': case.B, 'points': torch.from_numpy(ref['points']).to(dev), 'spatial_features': torch.from_numpy(ref['bev']).to(dev),
            'spatial_features_stride': case.BEV_STRIDE, 'multi_scale_3d_features': levels}


def host_reads(fn):
    """the synchronising device-to-host copies torch reports while fn() runs"""
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('warn')
    try:
        with warnings.catch_warnings(record=True) as seen:
            warnings.simplefilter('always')
            out = fn()
    finally:
        torch.cuda.set_sync_debug_mode('default')
    return out, sum('synchroniz' in str(w.message).lower() for w in seen)


def test_voxel_set_abstraction_matches_the_reference(ref, dev):
    """keypoints index-exact; point_features_before_fusion and point_features within 1e-4 of the reference's own module on the CPU
    (the project's fp32 feature parity); ONE host read a batch, the stack FPS wrapper's."""
    from pdm_ssd_amd.dense_heads import PointHeadSimple
    vsa = load(VoxelSetAbstraction(model_cfg=cfg_from_dict(case.pfe_cfg()), voxel_size=case.VOXEL, point_cloud_range=case.RANGE,
                                   num_bev_features=case.BEV_SHAPE[0], num_rawpoint_features=case.NUM_RAWPOINT_FEATURES), ref, 'pfe.state.', dev)
    vsa(front_batch(ref, dev))                       # (packs the weights: cached afterwards)
    batch = front_batch(ref, dev)                    # (uploaded before the count starts)
    out, reads = host_reads(lambda: vsa(batch))
    assert np.array_equal(out['keypoint_indices'].cpu().numpy(), ref['keypoint_rows'])
    assert np.array_equal(out['point_coords'].cpu().numpy(), ref['point_coords'])
    worst = {k: float(np.abs(out[k].cpu().numpy() - ref[k]).max()) for k in ('point_features_before_fusion', 'point_features')}
    print('VoxelSetAbstraction against the reference:', worst, 'host reads', reads)
    assert max(worst.values()) <= 1e-4
    assert reads == 1
    # the fixture's widths are multiples of 4, so every source was written in place at its column offset (8, 24, 40 of 60); a
    # destination that is not (57 columns, offset 5) takes sa_into's copy branch and gives the same bits
    from pdm_ssd_amd.backbones_3d.pfe.voxel_set_abstraction import sa_into
    from pdm_ssd_amd.pv_rcnn_ops import sample_counts
    assert out['point_features_before_fusion'].shape[1] % 4 == 0 and case.BEV_SHAPE[0] % 4 == 0
    raw, odd = batch['points'], torch.full((case.B * case.NUM_KEYPOINTS, 57), -7.0, device=dev)
    with torch.no_grad():
        end = sa_into(vsa.SA_rawpoints, raw[:, 1:4].contiguous(), sample_counts(raw[:, 0], case.B), out['point_coords'][:, 1:4].contiguous(),
                      torch.full((case.B,), case.NUM_KEYPOINTS, dtype=torch.int32, device=dev), raw[:, 4:].contiguous(), odd, 5)
    assert end == 21 and torch.equal(odd[:, 5:21], out['point_features_before_fusion'][:, 8:24])
    assert bool((odd[:, :5] == -7.0).all()) and bool((odd[:, 21:] == -7.0).all())
    head = load(PointHeadSimple(num_class=1, input_channels=case.NUM_BEFORE_FUSION, model_cfg=cfg_from_dict(case.POINT_HEAD_CFG)), ref,
                'point_head.state.', dev)
    with torch.no_grad():
        scores = head(out)['point_cls_scores']
    assert float(np.abs(scores.cpu().numpy() - ref['point_cls_scores']).max()) <= 1e-4


def built_head(ref, G, dev):
    from pdm_ssd_amd.roi_heads import PVRCNNHead
    return load(PVRCNNHead(input_channels=16, model_cfg=cfg_from_dict(case.head_cfg(G)), num_class=1), ref, f'g{G}.state.', dev)


def head_batch(ref, G, dev):
    t = lambda k: torch.from_numpy(ref[k]).to(dev)      # noqa: E731
    rois = t(f'g{G}.rois')
    return {'batch_size': case.B, 'rois': rois, 'roi_labels': torch.ones(rois.shape[:2], dtype=torch.long, device=dev),
            'point_coords': t('point_coords'), 'point_features': t('point_features'), 'point_cls_scores': t('point_cls_scores'),
            'point_coords_max_per_sample': case.NUM_KEYPOINTS}


@pytest.mark.parametrize("G", case.GRID_SIZES)
def test_head_matches_the_reference(ref, dev, G):
    """fused and composed pooling within the fused-SA bound of the stack tests (1e-4); rcnn_cls, rcnn_reg, batch_box_preds and
    batch_cls_preds within 1e-4 of the reference's own head on the CPU; two runs bit-equal; a graph replay of roi_grid_pool equals
    the eager run; the pooling reads nothing on the host; above the cap the head pools through the composed path."""
    head = built_head(ref, G, dev)
    bd = head_batch(ref, G, dev)
    with torch.no_grad():
        out = head(dict(bd))
    assert head.last_pool_path == 'fused' and out['cls_preds_normalized'] is False
    worst = {k: float(np.abs(out[k].cpu().numpy() - ref[f'g{G}.{k}']).max()) for k in ('rcnn_cls', 'rcnn_reg', 'batch_box_preds', 'batch_cls_preds')}
    print(f'PVRCNNHead G={G} against the reference:', worst)
    assert max(worst.values()) <= 1e-4
    with torch.no_grad():
        again = head(dict(bd))
    assert all(torch.equal(out[k], again[k]) for k in ('rcnn_cls', 'rcnn_reg', 'batch_box_preds'))
    eager, reads = host_reads(lambda: head.roi_grid_pool(bd).clone())
    assert reads == 0
    assert float((eager.view(-1, eager.shape[-1]).cpu() - torch.from_numpy(ref[f'g{G}.pooled'])).abs().max()) <= 1e-4
    head.use_fused_pool = False
    composed = head.roi_grid_pool(bd)
    assert head.last_pool_path == 'composed'
    assert float((composed - eager).abs().max()) <= 1e-4
    head.use_fused_pool = True
    over = dict(bd, point_coords_max_per_sample=pv_rcnn_ops.roi_keypoint_query_cap() + 1)
    assert float((head.roi_grid_pool(over) - eager).abs().max()) <= 1e-4 and head.last_pool_path == 'composed'
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        replayed = head.roi_grid_pool(bd)
    assert head.last_pool_path == 'fused'
    replayed.fill_(float('nan'))
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(replayed, eager) and float(eager.abs().max()) > 0


def test_build_pv_rcnn_runs_end_to_end(dev):
    """the D1 grid, 3000 synthetic points, 2 samples, 256 keypoints, 8 test rois: module order, shapes, finite results, labels in
    range, at least one box at SCORE_THRESH 0"""
    from pdm_ssd_amd import detector_config as dc
    cfg = copy.deepcopy(dc.PV_RCNN_CFG)
    cfg['PFE']['NUM_KEYPOINTS'] = 256
    cfg['ROI_HEAD']['NMS_CONFIG']['TEST'].update(NMS_POST_MAXSIZE=8, NMS_PRE_MAXSIZE=256)
    cfg['POST_PROCESSING']['SCORE_THRESH'] = 0.0
    d = scr.D1
    torch.manual_seed(0)
    model = dc.build_pv_rcnn(cfg, dataset=dc.voxel_dataset(4, d['range'], d['voxel'], d['grid'])).to(dev).eval()
    assert [type(m).__name__ for m in model.module_list] == ['DynamicMeanVFE', 'VoxelBackBone8x', 'HeightCompression', 'VoxelSetAbstraction',
                                                             'BaseBEVBackbone', 'AnchorHeadSingle', 'PointHeadSimple', 'PVRCNNHead']
    rng = np.random.default_rng(1)
    lo, hi = np.array(d['range'][:3]) + 0.05, np.array(d['range'][3:]) - 0.05
    pts = np.concatenate([np.repeat(np.arange(2), 1500)[:, None], rng.uniform(lo, hi, (3000, 3)), rng.uniform(0, 1, (3000, 1))], 1).astype(np.float32)
    bd = {'batch_size': 2, 'points': torch.from_numpy(pts).to(dev)}
    seen = {}
    model.roi_head.register_forward_hook(lambda m, i, out: seen.update(out))
    with torch.no_grad():
        preds, _ = model(bd)
    assert seen['point_coords'].shape == (512, 4) and seen['rois'].shape[:2] == (2, 8) and model.roi_head.last_pool_path == 'fused'
    assert len(preds) == 2 and sum(len(p['pred_boxes']) for p in preds) >= 1
    for p in preds:
        assert bool(torch.isfinite(p['pred_boxes']).all()) and bool(torch.isfinite(p['pred_scores']).all())
        assert bool(((p['pred_labels'] >= 1) & (p['pred_labels'] <= 3)).all())

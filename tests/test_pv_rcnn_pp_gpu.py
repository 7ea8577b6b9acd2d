"""PV-RCNN++ on the device: pdm_spc_partition against the numpy restatement (tests/pv_rcnn_pp_reference.py), exactly,
in a poisoned arena; sector_fps_batch against the restatement and the composed (reference) formulation on the device;
VoxelSetAbstractionSPC end to end inside build_pv_rcnn_plusplus()."""
import contextlib
import copy
import warnings

import numpy as np
import pytest
import torch

import pv_rcnn_pp_case as case
import pv_rcnn_pp_reference as ppr
import sparse_conv_reference as scr
from arena import Arena
from pdm_ssd_amd import _native, spc_ops

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def arena(dev):
    return Arena(dev, 8 << 20)


@pytest.fixture(scope="module")
def cases():
    """the planted clouds, built once: {counts: (xyz, counts, rois)}"""
    return {c: case.partition_case(c) for c in (case.SMALL, case.LARGE)}


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


def run_partition(arena, dev, xyz_np, counts, rois_np, S, fallback=True):
    """the operator with every tensor between red zones: inputs continued by NaN points / huge counts / NaN rois, outputs pre-filled
    with a pattern; -> (outputs as numpy, the pattern)"""
    arena.reset()
    N, B = len(xyz_np), len(counts)
    nseg = max(S, 1)
    xyz = arena.put(xyz_np, misalign_bytes=4, poison=float('nan'))
    cnt = arena.put(np.array(counts, dtype=np.int32), misalign_bytes=4, poison=1 << 20)
    rois = arena.put(rois_np, misalign_bytes=8, poison=float('nan'))
    out = dict(seg_xyz=arena.carve((N, 3), torch.float32, 4), seg_row=arena.carve((N,), torch.int32, 12),
               seg_cnt=arena.carve((B * nseg,), torch.int32, 4), seg_take=arena.carve((B * S,), torch.int32, 8) if S else None,
               kept_cnt=arena.carve((B,), torch.int32, 4), mask=arena.carve((N,), torch.bool, 3))
    need = int(_native.lib().pdm_spc_partition_ws_bytes(N, B, S))
    ws = arena.carve((need,), torch.uint8, 8)
    for t in out.values():
        if t is not None:
            t.view(torch.uint8).fill_(0x5b)
    ws.fill_(0x5b)
    spc_ops.spc_partition_into(xyz, cnt, rois, case.RADIUS, S, case.K, fallback, out, workspace=ws)
    torch.cuda.synchronize()
    arena.check()
    return {k: (v.cpu().numpy() if v is not None else None) for k, v in out.items()}


def check_partition(got, want, N, S):
    T = len(want['seg_row'])
    assert np.array_equal(got['seg_cnt'], want['seg_cnt']) and np.array_equal(got['kept_cnt'], want['kept_cnt'])
    assert int(want['seg_cnt'].sum()) == T
    assert np.array_equal(got['seg_row'][:T], want['seg_row'])
    assert np.array_equal(got['seg_xyz'][:T].view(np.uint32), want['seg_xyz'].view(np.uint32))
    assert np.array_equal(got['mask'], want['mask'])
    if S:
        assert np.array_equal(got['seg_take'], want['seg_take'])
    # past the kept total nothing was written
    assert (got['seg_row'][T:].view(np.uint8) == 0x5b).all() and (got['seg_xyz'][T:].view(np.uint8) == 0x5b).all()


def test_partition_small_case_with_everything_planted(dev, arena, cases):
    """counts [300, 37, 0], S = 6, K = 50: the fallback point, empty sectors, the point on the negative x axis, 25 kept rows with 7 in
    one sector (N' < K: every kept row is taken; ceil(7 / 25 * 50) is 15 in double, above the count, so the min decides: the
    four-sample case holds the triple at which the double and the integer evaluation part ways), an empty sample"""
    xyz, counts, rois = cases[case.SMALL]
    want = ppr.partition(xyz, counts, rois, case.RADIUS, case.S, case.K)
    assert want['kept_cnt'].tolist() == [25, 1, 0]
    c0 = want['seg_cnt'][:6].tolist()
    axis = int(ppr.sector_index(np.float32([case.AXIS_POINT]), case.S)[0][0])
    print('sector counts of sample 0:', c0, '; the axis point has sector index', axis)
    assert sorted(c0)[:3] == [0, 0, 0] and 7 in c0 and sum(c0) == (24 if axis == case.S else 25)
    assert want['seg_take'][:6].tolist() == c0 and int(want['seg_cnt'][6:12].sum()) == 1 and not want['mask'][300:].any()
    got = run_partition(arena, dev, xyz, counts, rois, case.S)
    check_partition(got, want, len(xyz), case.S)
    again = run_partition(arena, dev, xyz, counts, rois, case.S)
    assert all(np.array_equal(got[k].view(np.uint8), again[k].view(np.uint8)) for k in got)


@pytest.mark.parametrize("fallback", [True, False])
def test_partition_filter_only(dev, arena, cases, fallback):
    xyz, counts, rois = cases[case.SMALL]
    want = ppr.partition(xyz, counts, rois, case.RADIUS, 0, case.K, fallback=fallback)
    assert want['seg_cnt'].tolist() == [25, 1 if fallback else 0, 0]
    got = run_partition(arena, dev, xyz, counts, rois, 0, fallback)
    check_partition(got, want, len(xyz), 0)
    again = run_partition(arena, dev, xyz, counts, rois, 0, fallback)
    assert all(np.array_equal(got[k].view(np.uint8), again[k].view(np.uint8)) for k in got if got[k] is not None)


def test_partition_samples_over_several_workgroups(dev, arena, cases):
    """counts [700, 37, 0, 1500]: a sample of two tiles, tiles of four samples in one launch; sample 3 keeps exactly 100 rows, 28 of
    them in sector 0, and K = 50 must take 15 there, not the 14 of ceil(28 * 50 / 100)"""
    xyz, counts, rois = cases[case.LARGE]
    want = ppr.partition(xyz, counts, rois, case.RADIUS, case.S, case.K)
    assert want['kept_cnt'].tolist() == [145, 1, 0, 100]
    assert want['seg_cnt'][18:24].tolist() == [28, 0, 30, 42, 0, 0] and want['seg_take'][18:24].tolist() == [15, 0, 15, 21, 0, 0]
    kept3 = np.flatnonzero(want['mask'][737:])
    assert kept3.min() < 1024 <= kept3.max()                    # kept rows in both tiles of the sample
    got = run_partition(arena, dev, xyz, counts, rois, case.S)
    check_partition(got, want, len(xyz), case.S)
    again = run_partition(arena, dev, xyz, counts, rois, case.S)
    assert all(np.array_equal(got[k].view(np.uint8), again[k].view(np.uint8)) for k in got)


def test_partition_replays_in_a_graph(dev, cases):
    xyz_np, counts, rois_np = cases[case.LARGE]
    xyz, rois = torch.from_numpy(xyz_np).to(dev), torch.from_numpy(rois_np).to(dev)
    cnt = torch.tensor(counts, dtype=torch.int32, device=dev)
    eager, reads = host_reads(lambda: spc_ops.spc_partition(xyz, cnt, rois, case.RADIUS, case.S, case.K, want_mask=True))
    assert reads == 0
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        replayed = spc_ops.spc_partition(xyz, cnt, rois, case.RADIUS, case.S, case.K, want_mask=True)
    T = int(eager['seg_cnt'].sum())
    for k in ('seg_cnt', 'seg_take', 'kept_cnt', 'seg_row'):
        replayed[k].fill_(-1)
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(replayed[k], eager[k]) for k in ('seg_cnt', 'seg_take', 'kept_cnt', 'mask'))
    assert torch.equal(replayed['seg_row'][:T], eager['seg_row'][:T]) and torch.equal(replayed['seg_xyz'][:T], eager['seg_xyz'][:T])


def test_sector_fps_batch_matches_the_restatement_and_the_composed_path(dev, cases):
    from pdm_ssd_amd.backbones_3d.pfe import voxel_set_abstraction_spc as vsp
    xyz_np, counts, rois_np = cases[case.LARGE]
    xyz, rois = torch.from_numpy(xyz_np).to(dev), torch.from_numpy(rois_np).to(dev)
    cnt = torch.tensor(counts, dtype=torch.int32, device=dev)
    (kp, rows, per, per_host), reads = host_reads(lambda: spc_ops.sector_fps_batch(xyz, cnt, rois, case.RADIUS, case.S, case.K))
    assert reads == 1
    want_kp, want_rows, want_per = ppr.keypoints(xyz_np, counts, rois_np, case.RADIUS, case.S, case.K)
    assert per_host == want_per.tolist() == per.tolist() and max(per_host) <= case.K + case.S
    assert np.array_equal(rows.cpu().numpy(), want_rows) and np.array_equal(kp.cpu().numpy(), want_kp)
    start, composed = 0, []
    for b, n in enumerate(counts):
        if n:
            filtered, _ = vsp.sample_points_with_roi(rois[b], xyz[start:start + n], case.RADIUS)
            composed.append(vsp.sector_fps(filtered, case.K, case.S))
        start += n
    assert torch.equal(torch.cat(composed), kp)


# ------------------------------------------------------------------------------------------------------------ end to end

def small_model(dev):
    """the D1 grid, 256 keypoints, 8 test rois, SCORE_THRESH 0"""
    from pdm_ssd_amd import detector_config as dc
    cfg = copy.deepcopy(dc.PV_RCNN_PP_CFG)
    cfg['PFE']['NUM_KEYPOINTS'] = 256
    cfg['ROI_HEAD']['NMS_CONFIG']['TEST'].update(NMS_POST_MAXSIZE=8, NMS_PRE_MAXSIZE=256)
    cfg['POST_PROCESSING']['SCORE_THRESH'] = 0.0
    d = scr.D1
    torch.manual_seed(0)
    model = dc.build_pv_rcnn_plusplus(cfg, dataset=dc.voxel_dataset(4, d['range'], d['voxel'], d['grid'])).to(dev).eval()
    rng = np.random.default_rng(1)
    lo, hi = np.array(d['range'][:3]) + 0.05, np.array(d['range'][3:]) - 0.05
    pts = np.concatenate([np.repeat(np.arange(2), 1500)[:, None], rng.uniform(lo, hi, (3000, 3)), rng.uniform(0, 1, (3000, 1))], 1).astype(np.float32)
    return model, torch.from_numpy(pts).to(dev)


@contextlib.contextmanager
def deterministic_convolutions():
    """torch's own convolutions (BaseBEVBackbone, the heads' Conv1d stacks) pick reproducible algorithms: without the flag two calls
    on identical input differ in the last bits on this device, whatever stands in front of them"""
    before = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    try:
        yield
    finally:
        torch.backends.cudnn.deterministic = before


def test_build_pv_rcnn_plusplus_runs_end_to_end(dev):
    """module order, ragged keypoints within NUM_KEYPOINTS + NUM_SECTORS a sample, finite results; two runs bit-equal in every output,
    the final predictions included; the fused and the composed sampling give identical point_coords; the encoder's host reads are
    the number its docstring states"""
    model, pts = small_model(dev)
    assert [type(m).__name__ for m in model.module_list] == ['DynamicMeanVFE', 'VoxelBackBone8x', 'HeightCompression', 'VoxelSetAbstractionSPC',
                                                             'BaseBEVBackbone', 'AnchorHeadSingle', 'PointHeadSimple', 'PVRCNNHead']
    seen = {}
    model.roi_head.register_forward_hook(lambda m, i, out: seen.update(out))
    runs = []
    with deterministic_convolutions():
        for fused in (True, True, False):
            model.pfe.use_fused_spc = fused
            with torch.no_grad():
                preds, _ = model({'batch_size': 2, 'points': pts})
            runs.append((preds, dict(seen)))
    (preds, first), (preds2, second), (_, composed) = runs
    per = first['keypoint_batch_cnt'].tolist()
    print('keypoints a sample:', per, 'rois', tuple(first['rois'].shape))
    assert first['rois'].shape[:2] == (2, 8) and model.roi_head.last_pool_path == 'composed'
    assert all(0 < k <= 256 + 6 for k in per) and first['point_coords'].shape == (sum(per), 4)
    assert first['point_coords_max_per_sample'] == 262
    assert torch.equal(pts[first['keypoint_indices'], 1:4], first['point_coords'][:, 1:4])       # (the points are sample-major already)
    assert len(preds) == 2 and sum(len(p['pred_boxes']) for p in preds) >= 1
    for p, q in zip(preds, preds2):
        assert bool(torch.isfinite(p['pred_boxes']).all()) and bool(torch.isfinite(p['pred_scores']).all())
        assert bool(((p['pred_labels'] >= 1) & (p['pred_labels'] <= 3)).all())
        assert all(torch.equal(p[k], q[k]) for k in ('pred_boxes', 'pred_scores', 'pred_labels'))
    tensors = [k for k, v in first.items() if torch.is_tensor(v)]
    assert {'rois', 'keypoint_indices', 'keypoint_batch_cnt', 'point_coords', 'point_features_before_fusion', 'point_features',
            'point_cls_scores', 'rcnn_cls', 'rcnn_reg', 'batch_cls_preds', 'batch_box_preds', 'spatial_features_2d'} <= set(tensors)
    differing = [k for k in tensors if not torch.equal(first[k], second[k])]
    assert not differing, differing
    assert torch.equal(first['point_coords'], composed['point_coords'])
    assert float((first['point_features'] - composed['point_features']).abs().max()) <= 1e-4
    # the encoder alone on the batch the detector left in front of it
    model.pfe.use_fused_spc = True
    front = {k: first[k] for k in ('batch_size', 'points', 'voxel_coords', 'spatial_features', 'spatial_features_stride',
                                   'multi_scale_3d_features', 'rois') if k in first}
    out, n = host_reads(lambda: model.pfe(dict(front)))
    print('host reads of the encoder:', n)
    assert torch.equal(out["point_coords"], first["point_coords"]) and n == model.pfe.host_reads_per_batch() == 8


# ------------------------------------------------------------------------------------------------------------ the fixture

import os  # noqa: E402

from pdm_ssd_amd.config import cfg_from_dict  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def ref():
    z = np.load(os.path.join(GOLDEN, "ref_pv_rcnn_pp.npz"))
    return {k: z[k] for k in z.files}


def load(module, ref, prefix, dev):
    module.load_state_dict({k[len(prefix):]: torch.from_numpy(v) for k, v in ref.items() if k.startswith(prefix)})
    return module.to(dev).eval()


@pytest.mark.parametrize("tag,counts", [('small', case.SMALL), ('large', case.LARGE)])
def test_sector_fps_batch_matches_the_reference_fixture(dev, cases, ref, tag, counts):
    """what the reference's own sample_points_with_roi + sector_fps gave on the CPU, the planted axis point's sector included"""
    xyz_np, counts, rois_np = cases[counts]
    assert int(ref['op.axis_sector']) == int(ppr.sector_index(np.float32([case.AXIS_POINT]), case.S)[0][0])
    kp, rows, per, per_host = spc_ops.sector_fps_batch(torch.from_numpy(xyz_np).to(dev), torch.tensor(counts, dtype=torch.int32, device=dev),
                                                       torch.from_numpy(rois_np).to(dev), case.RADIUS, case.S, case.K)
    assert per_host == ref[f'op.{tag}.per'].tolist()
    assert np.array_equal(kp.cpu().numpy(), ref[f'op.{tag}.keypoints']) and np.array_equal(rows.cpu().numpy(), ref[f'op.{tag}.rows'])


def front_batch(ref, dev):
    levels = {name: type('Level', (), dict(indices=torch.from_numpy(ref[f'{name}.indices']).to(dev),
                                           features=torch.from_numpy(ref[f'{name}.features']).to(dev)))() for name, _, _ in case.LEVELS}
    rois = torch.from_numpy(ref['rois']).to(dev)
    return {'batch_size': case.B, 'points': torch.from_numpy(ref['points']).to(dev), 'spatial_features': torch.from_numpy(ref['bev']).to(dev),
            'spatial_features_stride': case.BEV_STRIDE, 'multi_scale_3d_features': levels, 'rois': rois,
            'roi_labels': torch.ones(rois.shape[:2], dtype=torch.long, device=dev)}


def test_modules_match_the_reference(ref, dev):
    """VoxelSetAbstractionSPC (SPC keypoints, a plain and two filtered VectorPool sources), PointHeadSimple and PVRCNNHead (VectorPool
    pool) against the reference's own modules on the CPU: keypoints exact, features and rcnn outputs within 1e-4 (the project's fp32
    parity); the composed sampling gives the same keypoints; the encoder's host reads are what it states"""
    from pdm_ssd_amd.backbones_3d.pfe import VoxelSetAbstractionSPC
    from pdm_ssd_amd.dense_heads import PointHeadSimple
    from pdm_ssd_amd.roi_heads import PVRCNNHead
    vsa = load(VoxelSetAbstractionSPC(model_cfg=cfg_from_dict(case.pfe_cfg()), voxel_size=case.VOXEL, point_cloud_range=case.RANGE,
                                      num_bev_features=case.BEV_SHAPE[0], num_rawpoint_features=case.NUM_RAWPOINT_FEATURES), ref, 'pfe.state.', dev)
    point_head = load(PointHeadSimple(num_class=1, input_channels=case.NUM_BEFORE_FUSION, model_cfg=cfg_from_dict(case.POINT_HEAD_CFG)), ref,
                      'point_head.state.', dev)
    head = load(PVRCNNHead(input_channels=16, model_cfg=cfg_from_dict(case.head_cfg()), num_class=1), ref, 'head.state.', dev)
    vsa(front_batch(ref, dev))                       # (packs the weights: cached afterwards)
    batch = front_batch(ref, dev)
    out, reads = host_reads(lambda: vsa(batch))
    assert np.array_equal(out['point_coords'].cpu().numpy(), ref['point_coords'])
    assert np.array_equal(out['keypoint_indices'].cpu().numpy(), ref['keypoint_rows'])
    assert out['keypoint_batch_cnt'].tolist() == ref['keypoint_cnt'].tolist() and out['point_coords_max_per_sample'] == case.K + case.S
    with torch.no_grad():
        out = head(point_head(out))
    assert head.last_pool_path == 'composed'
    keys = ('point_features_before_fusion', 'point_features', 'point_cls_scores', 'rcnn_cls', 'rcnn_reg', 'batch_box_preds', 'batch_cls_preds')
    worst = {k: float(np.abs(out[k].cpu().numpy() - ref[k]).max()) for k in keys}
    print('PV-RCNN++ modules against the reference:', worst, 'host reads of the encoder', reads)
    assert max(worst.values()) <= 1e-4
    assert reads == vsa.host_reads_per_batch() == 2 + 4
    vsa.use_fused_spc = False
    composed = vsa(front_batch(ref, dev))
    assert torch.equal(composed['point_coords'], out['point_coords'])
    assert float((composed['point_features_before_fusion'] - out['point_features_before_fusion']).abs().max()) <= 1e-4


def test_voxel_centers_as_the_point_source(ref, dev):
    """POINT_SOURCE voxel_centers: the keypoints are sampled from the centres of voxel_coords (the stride-1 level's cells here); fused,
    composed and the restatement (with the oracle's FPS: lattice points tie, and the tie order is the kernels' tree) agree exactly,
    and the rows index the sample-major centres"""
    from pdm_ssd_amd.backbones_3d.pfe import VoxelSetAbstractionSPC
    cfg = case.pfe_cfg()
    cfg['POINT_SOURCE'] = 'voxel_centers'
    vsa = load(VoxelSetAbstractionSPC(model_cfg=cfg_from_dict(cfg), voxel_size=case.VOXEL, point_cloud_range=case.RANGE,
                                      num_bev_features=case.BEV_SHAPE[0], num_rawpoint_features=case.NUM_RAWPOINT_FEATURES), ref, 'pfe.state.', dev)
    level = dict(indices=ref['x_conv1.indices'], stride=1)
    centres, cnt = case.level_xyz(level), np.bincount(level['indices'][:, 0], minlength=case.B)
    assert case.partition_is_clear(centres, cnt, ref['rois'], case.RADIUS, True)
    from oracle import cpu_oracle
    tree_fps = lambda xyz, n: cpu_oracle.stack_furthest_point_sample(xyz, [len(xyz)], [n]).astype(np.int64)      # noqa: E731
    want_kp, want_rows, want_per = ppr.keypoints(centres, cnt, ref['rois'], case.RADIUS, case.S, case.K, fps=tree_fps)   # (lattice: ties)
    batch = dict(front_batch(ref, dev), voxel_coords=torch.from_numpy(level['indices']).to(dev))
    out = vsa(dict(batch))
    assert np.array_equal(out['point_coords'][:, 1:4].cpu().numpy(), want_kp) and np.array_equal(out['keypoint_indices'].cpu().numpy(), want_rows)
    assert out['keypoint_batch_cnt'].tolist() == want_per.tolist()
    assert out['point_features'].shape == (len(want_kp), 16) and bool(torch.isfinite(out['point_features']).all())
    vsa.use_fused_spc = False
    assert torch.equal(vsa(dict(batch))['point_coords'], out['point_coords'])


def test_fps_sampling_equals_the_plain_class(dev):
    """SAMPLE_METHOD FPS on the new class, PV-RCNN's own reduced config (tests/pv_rcnn_case.py, no rois in the batch): every output
    bit-equal to VoxelSetAbstraction's; keypoint_indices is its (B, K) table flattened, the counts are K each"""
    import pv_rcnn_case as pcase
    from pdm_ssd_amd.backbones_3d.pfe import VoxelSetAbstraction, VoxelSetAbstractionSPC
    z = np.load(os.path.join(GOLDEN, "ref_pv_rcnn.npz"))
    build = lambda cls: cls(model_cfg=cfg_from_dict(pcase.pfe_cfg()), voxel_size=pcase.VOXEL, point_cloud_range=pcase.RANGE,      # noqa: E731
                            num_bev_features=pcase.BEV_SHAPE[0], num_rawpoint_features=pcase.NUM_RAWPOINT_FEATURES)
    state = {k[len('pfe.state.'):]: torch.from_numpy(z[k]) for k in z.files if k.startswith('pfe.state.')}
    plain, new = build(VoxelSetAbstraction), build(VoxelSetAbstractionSPC)
    for m in (plain, new):
        m.load_state_dict(state)
        m.to(dev).eval()

    def batch():
        levels = {name: type('Level', (), dict(indices=torch.from_numpy(z[f'{name}.indices']).to(dev),
                                               features=torch.from_numpy(z[f'{name}.features']).to(dev)))() for name, _, _ in pcase.LEVELS}
        return {'batch_size': pcase.B, 'points': torch.from_numpy(z['points']).to(dev), 'spatial_features': torch.from_numpy(z['bev']).to(dev),
                'spatial_features_stride': pcase.BEV_STRIDE, 'multi_scale_3d_features': levels}
    want, got = plain(batch()), new(batch())
    assert all(torch.equal(want[k], got[k]) for k in ('point_coords', 'point_features_before_fusion', 'point_features'))
    assert torch.equal(got['keypoint_indices'], want['keypoint_indices'].view(-1)) and np.array_equal(got['keypoint_indices'].cpu().numpy(), z['keypoint_rows'].reshape(-1))
    assert got['keypoint_batch_cnt'].tolist() == [pcase.NUM_KEYPOINTS] * pcase.B and got['point_coords_max_per_sample'] == pcase.NUM_KEYPOINTS

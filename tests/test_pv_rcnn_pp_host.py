"""PV-RCNN++ without a GPU: the numpy restatement of the proposal-centric partition (tests/pv_rcnn_pp_reference.py) against what the
reference's own functions gave (tests/golden/ref_pv_rcnn_pp.npz, gen_pv_rcnn_pp_fixtures.py), state_dict keys and shapes against
the reference's, the registries and build_pv_rcnn_plusplus()'s module order, the argument checks of pdm_spc_partition (an error code
before any launch), the take counts in python's arithmetic, and the training-mode refusal."""
import ctypes as C
import json
import math
import os

import numpy as np
import pytest

import pv_rcnn_case as pcase
import pv_rcnn_pp_case as case
import pv_rcnn_pp_reference as ppr

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def ref():
    z = np.load(os.path.join(GOLDEN, "ref_pv_rcnn_pp.npz"))
    return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def manifest():
    with open(os.path.join(GOLDEN, "ref_pv_rcnn_pp_manifest.json")) as f:
        return json.load(f)


def test_take_counts_are_pythons():
    """min(c, ceil(c / N' * K)) in python floats: 7 / 25 * 50 is 14.000000000000002, so the ceiling is 15 (the count then caps the
    take at 7); with 28 of 100 the same quotient takes 15 where the integer form ceil(28 * 50 / 100) takes 14"""
    assert math.ceil(7 / 25 * 50) == 15 and -(-7 * 50 // 25) == 14
    assert ppr.take_counts([7], 25, 50) == [min(7, math.ceil(7 / 25 * 50))] == [7]
    assert ppr.take_counts([28, 0, 30, 42], 100, 50) == [15, 0, 15, 21] and -(-28 * 50 // 100) == 14
    assert ppr.take_counts([3, 0], 3, 50) == [3, 0]


def test_case_is_the_fixture_and_is_clear(ref, manifest):
    seed = manifest['seeds']['points_and_rois']
    pts, rois = pcase.points(seed), pcase.rois(np.random.default_rng(seed))
    assert np.array_equal(pts, ref['points']) and np.array_equal(rois, ref['rois']) and np.array_equal(pcase.bev_features(), ref['bev'])
    assert (rois[:, -1] == 0).all()                                # the all-zero padding row
    levels = pcase.levels(pts)
    for name, lv in levels.items():
        assert np.array_equal(lv['indices'], ref[f'{name}.indices']) and np.array_equal(lv['features'], ref[f'{name}.features'])
    assert case.partition_is_clear(pts[:, 1:4], case.COUNTS, rois, case.RADIUS, True)
    assert case.partition_is_clear(pts[:, 1:4], case.COUNTS, rois, case.FILTER_RADII['raw_points'], False)
    lv = levels['x_conv3']
    assert case.partition_is_clear(case.level_xyz(lv), np.bincount(lv['indices'][:, 0], minlength=case.B), rois, case.FILTER_RADII['x_conv3'], False)


def test_restated_keypoints_are_the_references(ref):
    """module case and both operator cases: keypoints bit-equal to the reference's sample_points_with_roi + sector_fps; the operator
    cases hold what they say they plant"""
    kp, rows, per = ppr.keypoints(ref['points'][:, 1:4], case.COUNTS, ref['rois'], case.RADIUS, case.S, case.K)
    assert np.array_equal(kp, ref['point_coords'][:, 1:4]) and np.array_equal(rows, ref['keypoint_rows']) and per.tolist() == ref['keypoint_cnt'].tolist()
    assert min(per) < case.K < max(per) <= case.K + case.S         # a sample with N' < K, and ragged counts above K
    for tag, counts in (('small', case.SMALL), ('large', case.LARGE)):
        xyz, counts, rois = case.partition_case(counts)
        kp, rows, per = ppr.keypoints(xyz, counts, rois, case.RADIUS, case.S, case.K)
        assert np.array_equal(kp, ref[f'op.{tag}.keypoints']) and np.array_equal(rows, ref[f'op.{tag}.rows']) and per.tolist() == ref[f'op.{tag}.per'].tolist()
    part = ppr.partition(xyz, counts, rois, case.RADIUS, case.S, case.K)
    assert part['kept_cnt'].tolist() == [145, 1, 0, 100] and part['seg_take'][18:24].tolist() == [15, 0, 15, 21, 0, 0]
    assert int(ref['op.axis_sector']) == case.S == int(ppr.sector_index(np.float32([case.AXIS_POINT]), case.S)[0][0])


def test_state_dicts_match_the_reference(manifest):
    from pdm_ssd_amd import detector_config as dc
    from pdm_ssd_amd.backbones_3d.pfe import VoxelSetAbstractionSPC
    from pdm_ssd_amd.config import cfg_from_dict
    from pdm_ssd_amd.dense_heads import PointHeadSimple
    from pdm_ssd_amd.roi_heads import PVRCNNHead
    shapes = lambda m: {k: list(v.shape) for k, v in m.state_dict().items()}      # noqa: E731
    vsa = VoxelSetAbstractionSPC(model_cfg=cfg_from_dict(case.pfe_cfg()), voxel_size=case.VOXEL, point_cloud_range=case.RANGE,
                                 num_bev_features=case.BEV_SHAPE[0], num_rawpoint_features=case.NUM_RAWPOINT_FEATURES)
    assert shapes(vsa) == manifest['VoxelSetAbstraction(reduced: tests/pv_rcnn_pp_case.py PFE_CFG)']
    assert vsa.num_point_features_before_fusion == case.NUM_BEFORE_FUSION and vsa.host_reads_per_batch() == 6
    point_head = PointHeadSimple(num_class=1, input_channels=case.NUM_BEFORE_FUSION, model_cfg=cfg_from_dict(case.POINT_HEAD_CFG))
    assert shapes(point_head) == manifest['PointHeadSimple(reduced: tests/pv_rcnn_pp_case.py POINT_HEAD_CFG, num_class=1)']
    head = PVRCNNHead(input_channels=16, model_cfg=cfg_from_dict(case.head_cfg()), num_class=1)
    assert shapes(head) == manifest['PVRCNNHead(reduced: tests/pv_rcnn_pp_case.py HEAD_CFG, num_class=1)']
    model = dc.build_pv_rcnn_plusplus()
    assert shapes(model.pfe) == manifest['VoxelSetAbstraction(PV_RCNN_PP_CFG, 256 bev features, 4 raw point features)']
    assert shapes(model.roi_head) == manifest['PVRCNNHead(PV_RCNN_PP_CFG, 90 point features, num_class=1)']


def test_registries_and_module_order():
    from pdm_ssd_amd import detector_config as dc
    from pdm_ssd_amd import detectors
    from pdm_ssd_amd.backbones_3d import pfe
    from pdm_ssd_amd.backbones_3d.pfe import voxel_set_abstraction_spc as vsp
    assert detectors.__all__['PVRCNNPlusPlus'].__name__ == 'PVRCNNPlusPlus' and pfe.__all__['VoxelSetAbstractionSPC'] is vsp.VoxelSetAbstractionSPC
    assert issubclass(vsp.VoxelSetAbstractionSPC, pfe.VoxelSetAbstraction)
    model = dc.build_pv_rcnn_plusplus()
    assert [type(m).__name__ for m in model.module_list] == ['DynamicMeanVFE', 'VoxelBackBone8x', 'HeightCompression', 'VoxelSetAbstractionSPC',
                                                             'BaseBEVBackbone', 'AnchorHeadSingle', 'PointHeadSimple', 'PVRCNNHead']
    assert model.pfe.use_fused_spc is True and model.pfe.host_reads_per_batch() == 8
    assert model.pfe.num_point_features == 90 and model.pfe.num_point_features_before_fusion == 256 + 32 + 128 + 128


def test_training_mode_is_refused():
    from pdm_ssd_amd import detector_config as dc
    model = dc.build_pv_rcnn_plusplus().train()
    for module in (model, model.pfe, model.point_head, model.roi_head):
        with pytest.raises(NotImplementedError, match='eval mode only'):
            module({})


def test_plain_class_still_refuses_and_says_where_to_look():
    from pdm_ssd_amd.backbones_3d.pfe import VoxelSetAbstraction
    from pdm_ssd_amd.config import cfg_from_dict
    with pytest.raises(NotImplementedError, match='SAMPLE_METHOD.*VoxelSetAbstractionSPC'):
        VoxelSetAbstraction(model_cfg=cfg_from_dict(case.pfe_cfg()), voxel_size=case.VOXEL, point_cloud_range=case.RANGE,
                            num_bev_features=case.BEV_SHAPE[0], num_rawpoint_features=case.NUM_RAWPOINT_FEATURES)


def test_spc_partition_validates_its_arguments_before_any_launch():
    from pdm_ssd_amd import _native, spc_ops
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p)
    lib = _native.lib()
    assert spc_ops.max_rois() == 1024 and lib.pdm_spc_partition_max_sectors() == 64
    assert lib.pdm_spc_partition_ws_bytes(100, 2, 6) >= 100 and lib.pdm_spc_partition_ws_bytes(100, 2, 65) == 0
    ws_bytes = lib.pdm_spc_partition_ws_bytes(4, 1, 6)

    def call(N=4, xyz=p, B=1, cnt=p, n=2, stride=7, rois=p, radius=1.0, S=6, K=8, seg_take=p, ws=p, ws_bytes=ws_bytes):
        _native.call("pdm_spc_partition", 0, N, xyz, B, cnt, n, stride, rois, radius, S, K, 1, p, p, p, seg_take, p, None, ws, ws_bytes)
    for kw in (dict(xyz=None), dict(cnt=None), dict(rois=None), dict(seg_take=None)):
        with pytest.raises(_native.NativeLibraryError, match="null pointer"):
            call(**kw)
    with pytest.raises(_native.NativeLibraryError, match="null workspace"):
        call(ws=None)
    with pytest.raises(_native.NativeLibraryError, match="exceed the cap of 1024"):
        call(n=1025)
    with pytest.raises(_native.NativeLibraryError, match="0 rois a sample"):
        call(n=0)
    for S in (-1, 65):
        with pytest.raises(_native.NativeLibraryError, match=f"{S} sectors"):
            call(S=S)
    with pytest.raises(_native.NativeLibraryError, match="num_keypoints 0"):
        call(K=0)
    with pytest.raises(_native.NativeLibraryError, match="rois of 6 columns"):
        call(stride=6)
    with pytest.raises(_native.NativeLibraryError, match="at most 1024 samples"):
        call(B=1025)
    with pytest.raises(_native.NativeLibraryError, match="radius is NaN"):
        call(radius=float('nan'))
    with pytest.raises(_native.NativeLibraryError, match="workspace of 8 bytes"):
        call(ws_bytes=8)
    with pytest.raises(_native.NativeLibraryError, match="8-byte aligned"):
        call(ws=C.c_void_p(C.addressof(buf) + 4))

"""PV-RCNN without a GPU: the numpy restatement of the keypoint path (tests/pv_rcnn_reference.py) against the reference's own
VoxelSetAbstraction and PVRCNNHead (tests/golden/ref_pv_rcnn.npz, gen_pv_rcnn_fixtures.py), state_dict keys and shapes against
the reference's, the registries and build_pv_rcnn()'s module order, the refused config keys, the argument checks of the two new
entry points (an error code before any launch) and the training-mode refusal."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import pv_rcnn_case as case
import pv_rcnn_reference as pr

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
KEYS = ('VoxelSetAbstraction(reduced: tests/pv_rcnn_case.py PFE_CFG)', 'PointHeadSimple(reduced: tests/pv_rcnn_case.py POINT_HEAD_CFG, num_class=1)')


@pytest.fixture(scope="module")
def ref():
    z = np.load(os.path.join(GOLDEN, "ref_pv_rcnn.npz"))
    return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def manifest():
    with open(os.path.join(GOLDEN, "ref_pv_rcnn_manifest.json")) as f:
        return json.load(f)


def sources(ref):
    """(name, state prefix, cfg, xyz, counts, features) in the reference's column order: raw_points, then the levels"""
    pts = ref['points']
    yield 'raw_points', 'SA_rawpoints.', case.PFE_CFG['SA_LAYER']['raw_points'], pts[:, 1:4], list(case.COUNTS), pts[:, 4:]
    for k, (name, stride, _) in enumerate(case.LEVELS):
        idx = ref[f'{name}.indices']
        xyz = ((idx[:, [3, 2, 1]].astype(np.float32) + np.float32(0.5)) * (np.float32(case.VOXEL) * np.float32(stride))
               + np.float32(case.RANGE[:3])).astype(np.float32)
        yield name, f'SA_layers.{k}.', case.PFE_CFG['SA_LAYER'][name], xyz, np.bincount(idx[:, 0], minlength=case.B), ref[f'{name}.features']


def test_case_is_the_fixture(ref, manifest):
    pts = case.points(manifest['seeds']['points'])
    assert np.array_equal(pts, ref['points']) and np.array_equal(case.bev_features(), ref['bev'])
    for name, lv in case.levels(pts).items():
        assert np.array_equal(lv['indices'], ref[f'{name}.indices']) and np.array_equal(lv['features'], ref[f'{name}.features'])
    assert min(case.COUNTS) < case.NUM_KEYPOINTS < max(case.COUNTS)


def test_keypoints_and_bev_features_are_bit_equal(ref):
    """keypoint rows index-exact (the sample with 30 points repeats its picks: slot j reads pick j mod 30), the interpolated BEV
    columns bit-equal to the reference's bilinear_interpolate_torch"""
    rows = pr.keypoint_rows(ref['points'], case.COUNTS, case.NUM_KEYPOINTS)
    assert np.array_equal(rows, ref['keypoint_rows'])
    assert np.array_equal(ref['points'][rows.reshape(-1), 1:4], ref['point_coords'][:, 1:4])
    assert np.array_equal(rows[1, 30:], rows[1, :18]) and len(set(rows[1, :30])) == 30
    got = pr.bev_interpolate(ref['point_coords'], ref['bev'], case.RANGE, case.VOXEL, case.BEV_STRIDE)
    assert np.array_equal(got, ref['point_features_before_fusion'][:, :case.BEV_SHAPE[0]])


def test_numpy_restatement_matches_the_reference_encoder(ref):
    """ball indices bit-equal, pooled columns and fused features within 2e-5 (the Voxel R-CNN host test's bound for its
    restatement: fp32 there, float64 behind fp32 geometry here, features of order 1)"""
    state = {k[len('pfe.state.'):]: v for k, v in ref.items() if k.startswith('pfe.state.')}
    new_xyz, new_cnt = ref['point_coords'][:, 1:4], [case.NUM_KEYPOINTS] * case.B
    cols, col = [ref['point_features_before_fusion'][:, :case.BEV_SHAPE[0]].astype(np.float64)], case.BEV_SHAPE[0]
    for name, prefix, cfg, xyz, cnt, feats in sources(ref):
        y, idxs, empties, _, _ = pr.sa_msg(state, prefix, cfg['POOL_RADIUS'], cfg['NSAMPLE'], xyz, cnt, new_xyz, new_cnt, feats)
        for s in range(2):
            assert np.array_equal(idxs[s], ref[f'{name}.idx{s}']) and np.array_equal(empties[s], ref[f'{name}.empty{s}'])
        assert float(np.abs(y - ref['point_features_before_fusion'][:, col:col + y.shape[1]]).max()) <= 2e-5
        cols.append(y)
        col += y.shape[1]
    assert col == case.NUM_BEFORE_FUSION
    fused = pr.linear_bn_relu(np.concatenate(cols, 1), state, 'vsa_point_feature_fusion.')
    assert float(np.abs(fused - ref['point_features']).max()) <= 2e-5


@pytest.mark.parametrize("G", case.GRID_SIZES)
def test_numpy_restatement_matches_the_reference_head_pooling(ref, G):
    state = {k[len(f'g{G}.state.'):]: v for k, v in ref.items() if k.startswith(f'g{G}.state.')}
    pool = case.HEAD_CFG['ROI_GRID_POOL']
    rois = ref[f'g{G}.rois']
    weighted = ref['point_features'] * ref['point_cls_scores'][:, None]
    y, idxs, empties, sizes, _ = pr.sa_msg(state, 'roi_grid_pool_layer.', pool['POOL_RADIUS'], pool['NSAMPLE'], ref['point_coords'][:, 1:4],
                                          [case.NUM_KEYPOINTS] * case.B, pr.grid_points(rois, G), [rois.shape[1] * G ** 3] * case.B, weighted)
    for s in range(2):
        assert np.array_equal(idxs[s], ref[f'g{G}.idx{s}']) and np.array_equal(empties[s], ref[f'g{G}.empty{s}'])
    assert empties[0].any() and (sizes[1] > 16).any()
    assert float(np.abs(y - ref[f'g{G}.pooled']).max()) <= 2e-5


def test_state_dict_keys_and_shapes_match_the_reference(manifest):
    from pdm_ssd_amd import detector_config as dc
    from pdm_ssd_amd.backbones_3d.pfe import VoxelSetAbstraction
    from pdm_ssd_amd.config import cfg_from_dict
    from pdm_ssd_amd.dense_heads import PointHeadSimple
    from pdm_ssd_amd.roi_heads import PVRCNNHead
    shapes = lambda m: {k: list(v.shape) for k, v in m.state_dict().items()}      # noqa: E731
    vsa = VoxelSetAbstraction(model_cfg=cfg_from_dict(case.pfe_cfg()), voxel_size=case.VOXEL, point_cloud_range=case.RANGE,
                              num_bev_features=case.BEV_SHAPE[0], num_rawpoint_features=case.NUM_RAWPOINT_FEATURES)
    assert shapes(vsa) == manifest[KEYS[0]] and vsa.num_point_features_before_fusion == case.NUM_BEFORE_FUSION
    ph = PointHeadSimple(num_class=1, input_channels=case.NUM_BEFORE_FUSION, model_cfg=cfg_from_dict(case.POINT_HEAD_CFG))
    assert shapes(ph) == manifest[KEYS[1]]
    for G in case.GRID_SIZES:
        head = PVRCNNHead(input_channels=16, model_cfg=cfg_from_dict(case.head_cfg(G)), num_class=1)
        assert shapes(head) == manifest[f'PVRCNNHead(reduced: tests/pv_rcnn_case.py HEAD_CFG, GRID_SIZE={G}, num_class=1)']
    model = dc.build_pv_rcnn()
    assert shapes(model.pfe) == manifest['VoxelSetAbstraction(PV_RCNN_CFG, 256 bev features, 4 raw point features)']
    assert shapes(model.point_head) == manifest['PointHeadSimple(PV_RCNN_CFG, num_class=1)']
    want = manifest['PVRCNNHead(PV_RCNN_CFG, 128 point features, num_class=1)']
    assert shapes(model.roi_head) == want
    assert 'shared_fc_layer.4.weight' in want and 'shared_fc_layer.3.weight' not in want      # the Dropout at child 3 shifts the indices
    assert [type(m).__name__ for m in model.module_list] == ['DynamicMeanVFE', 'VoxelBackBone8x', 'HeightCompression', 'VoxelSetAbstraction',
                                                             'BaseBEVBackbone', 'AnchorHeadSingle', 'PointHeadSimple', 'PVRCNNHead']
    assert model.pfe.num_point_features_before_fusion == 640 and model.roi_head.use_fused_pool


@pytest.mark.parametrize("edit, word", [
    (lambda c: c.update(SAMPLE_METHOD='SPC'), 'SAMPLE_METHOD'),
    (lambda c: c.update(POINT_SOURCE='voxel_centers'), 'POINT_SOURCE'),
    (lambda c: c['SA_LAYER']['raw_points'].update(FILTER_NEIGHBOR_WITH_ROI=True), 'FILTER_NEIGHBOR_WITH_ROI'),
    (lambda c: c['SA_LAYER']['x_conv3'].update(NAME='VectorPoolAggregationModuleMSG'), 'VectorPoolAggregationModuleMSG'),
])
def test_refused_config_keys_raise(edit, word):
    from pdm_ssd_amd.backbones_3d.pfe import VoxelSetAbstraction
    from pdm_ssd_amd.config import cfg_from_dict
    cfg = case.pfe_cfg()
    edit(cfg)
    with pytest.raises(NotImplementedError, match=word):
        VoxelSetAbstraction(model_cfg=cfg_from_dict(cfg), voxel_size=case.VOXEL, point_cloud_range=case.RANGE,
                            num_bev_features=case.BEV_SHAPE[0], num_rawpoint_features=case.NUM_RAWPOINT_FEATURES)


def test_training_mode_is_refused():
    from pdm_ssd_amd import detector_config as dc
    model = dc.build_pv_rcnn().train()
    for module in (model, model.pfe, model.point_head, model.roi_head):
        with pytest.raises(NotImplementedError, match='eval mode only'):
            module({})


def test_entry_points_validate_their_arguments_before_any_launch():
    from pdm_ssd_amd import _native, pv_rcnn_ops
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p)
    assert pv_rcnn_ops.roi_keypoint_query_cap() == 4096
    with pytest.raises(_native.NativeLibraryError, match=r"columns \[3, 8\) do not fit rows of 7"):
        _native.call("pdm_bev_interpolate", 0, 4, p, 1, 5, 4, 6, p, 0.0, 0.0, 0.5, 0.5, 4, p, 7, 3)
    with pytest.raises(_native.NativeLibraryError, match="bad voxel size or stride"):
        _native.call("pdm_bev_interpolate", 0, 4, p, 1, 5, 4, 6, p, 0.0, 0.0, 0.5, 0.5, 0, p, 8, 3)
    with pytest.raises(_native.NativeLibraryError, match="null pointer"):
        _native.call("pdm_bev_interpolate", 0, 4, p, 1, 5, 4, 6, None, 0.0, 0.0, 0.5, 0.5, 4, p, 8, 3)
    query = lambda **kw: _native.call("pdm_roi_keypoint_query", 0, 1, 2, 7, p, kw.get('G', 2), 8, p, p, kw.get('bound', 8), kw.get('scales', 2), 1.0,  # noqa: E731
                                      kw.get('ns', 16), 2.0, 16, p, p, p, kw.get('idx1', p), p)
    with pytest.raises(_native.NativeLibraryError, match="exceed the cap of 4096"):
        query(bound=4097)
    with pytest.raises(_native.NativeLibraryError, match="grid size 9"):
        query(G=9)
    with pytest.raises(_native.NativeLibraryError, match="nsample 65"):
        query(ns=65)
    with pytest.raises(_native.NativeLibraryError, match="3 scales"):
        query(scales=3)
    with pytest.raises(_native.NativeLibraryError, match="null pointer"):
        query(idx1=None)
    with pytest.raises(_native.NativeLibraryError, match="no keypoint at all"):
        _native.call("pdm_roi_keypoint_query", 0, 1, 2, 7, p, 2, 0, p, p, 8, 1, 1.0, 16, 0.0, 0, p, p, p, None, None)


def test_get_voxel_centers_is_bit_equal_to_the_tensor_form():
    """common_utils.get_voxel_centers forms the centres with python constants (nothing is uploaded, so the host never waits for the
    stream); the bits are those of the reference's tensor form: float(c) + 0.5, times fp32(voxel) * stride, plus fp32(minimum)"""
    import torch

    from pdm_ssd_amd.utils import common_utils

    def tensor_form(coords, stride, voxel, rng):
        c = coords[:, [2, 1, 0]].float()
        return (c + 0.5) * (torch.tensor(voxel).float() * stride) + torch.tensor(rng[0:3]).float()
    coords = torch.randint(0, 1600, (50000, 3), dtype=torch.int32, generator=torch.Generator().manual_seed(3))
    for stride in (1, 2, 4, 8):
        for voxel, rng in (([0.05, 0.05, 0.1], [0, -40, -3, 70.4, 40, 1]), (case.VOXEL, case.RANGE), ([0.16, 0.16, 4], [0, -39.68, -3, 69.12, 39.68, 1])):
            assert torch.equal(common_utils.get_voxel_centers(coords, stride, voxel, rng), tensor_form(coords, stride, voxel, rng))

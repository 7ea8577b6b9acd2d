"""Host-side checks of the RoI pooling operators and the PointRCNN second stage: hand-derived known answers for the numpy
restatement of the reference launchers (tests/roi_pool_reference.py), ResidualCoder and generate_predicted_boxes against
the reference's own run (tests/golden/ref_roi.npz, written by tests/golden/gen_roi_fixtures.py), and the state_dict
manifests.  No GPU is used."""
import copy
import json
import os

import numpy as np
import pytest
import torch

import roi_head_case
import roi_pool_reference as rp

HERE = os.path.dirname(os.path.abspath(__file__))
F = np.float32


@pytest.fixture(scope='module', autouse=True)
def _oracle(oracle):
    return oracle


@pytest.fixture(scope='module')
def fix():
    return dict(np.load(os.path.join(HERE, 'golden', 'ref_roi.npz')))


@pytest.fixture(scope='module')
def manifest():
    with open(os.path.join(HERE, 'golden', 'ref_roi_manifest.json')) as f:
        return json.load(f)


# a heading-0 box centred at (4, 2, 0), 4 x 2 x 2; all coordinates dyadic, so every fp32 operation is exact
BOX = F([4, 2, 0, 4, 2, 2, 0])


def pool(points, S, box=BOX, C=1):
    xyz = F(points)[None]
    feats = np.arange(len(points) * C, dtype=F).reshape(1, -1, C) + 100
    pooled = np.full((1, 1, S, 3 + C), 7.0, dtype=F)
    flag = np.zeros((1, 1), dtype=np.int32)
    rp.roipoint_pool3d(xyz, F(box)[None, None], feats, pooled, flag)
    return pooled[0, 0], int(flag[0, 0])


def test_point_pool_keeps_the_first_s_points_in_index_order():
    pts = [[9, 9, 0], [3, 2, 0], [4, 2.5, 0.5], [20, 2, 0], [5, 1.5, -0.5], [4.5, 2, 0], [2.5, 1.25, 0.75]]   # 1, 2, 4, 5, 6 inside
    rows, flag = pool(pts, 3)
    assert flag == 0
    assert rows[:, 3].tolist() == [101, 102, 104]
    assert rows[:, 0:3].tolist() == [pts[1], pts[2], pts[4]]


@pytest.mark.parametrize('inside,S', [([2], 4), ([1, 3, 4], 4)])      # cnt = 1 and cnt = S - 1
def test_point_pool_wraps_modulo_the_count(inside, S):
    pts = [[50 + i, 0, 0] for i in range(6)]
    for i in inside:
        pts[i] = [4 + 0.25 * i, 2, 0]
    rows, flag = pool(pts, S)
    assert flag == 0
    assert rows[:, 3].tolist() == [100 + inside[k % len(inside)] for k in range(S)]


def test_point_pool_empty_box_sets_the_flag_and_leaves_the_rows():
    rows, flag = pool([[50, 0, 0], [4, 2, 1.5], [6.5, 2, 0]], 3)      # above the box; beyond +dx/2 by 0.5
    assert flag == 1
    assert (rows == 7.0).all()


def aware(points, feats, out, max_pts, method, box=BOX):
    out = (out,) * 3 if isinstance(out, int) else out
    C = F(feats).shape[1]
    idx = np.zeros((1, *out, max_pts), dtype=np.int32)
    am = np.full((1, *out, C), -9, dtype=np.int32)
    pooled = np.zeros((1, *out, C), dtype=F)
    rp.roiaware_pool3d_forward(F(box)[None], F(points), F(feats), am, idx, pooled, method)
    return idx[0], am[0], pooled[0]


def test_aware_point_on_the_far_face_lands_in_the_last_voxel():
    # x = cx + dx/2 exactly: inside by the 1e-5 margin, (local + dx/2) / res = out -> clamped to out - 1; the -dx/2 face -> 0
    idx, _, _ = aware([[6, 2, 0], [2, 2, 0]], [[1], [2]], (4, 1, 1), 4, 0)
    assert idx[3, 0, 0].tolist() == [1, 0, 0, 0]
    assert idx[0, 0, 0].tolist() == [1, 1, 0, 0]
    assert idx[1:3, 0, 0, 0].tolist() == [0, 0]


def test_aware_list_is_capped_and_ascending():
    pts = [[4 + 0.125 * i, 2, 0] for i in range(6)]
    idx, am, pooled = aware(pts, [[1], [9], [3], [50], [60], [70]], 1, 4, 0)
    assert idx[0, 0, 0].tolist() == [3, 0, 1, 2]          # count capped at max_pts - 1, the first three indices
    assert am[0, 0, 0, 0] == 1 and pooled[0, 0, 0, 0] == 9  # the capped-out points take no part


def test_aware_max_first_index_wins_ties_and_negative_maximum_is_kept():
    pts = [[4, 2, 0], [4.5, 2, 0], [5, 2, 0]]
    _, am, pooled = aware(pts, [[5, -3], [5, -2], [1, -2]], 1, 8, 0)
    assert am[0, 0, 0].tolist() == [0, 1]
    assert pooled[0, 0, 0].tolist() == [5, -2]
    # a voxel without points: argmax -1, pooled untouched (0 from the caller)
    _, am, pooled = aware([[50, 2, 0]], [[5, -3]], 1, 8, 0)
    assert am[0, 0, 0].tolist() == [-1, -1] and pooled[0, 0, 0].tolist() == [0, 0]
    # NaN and -inf never win
    _, am, pooled = aware(pts, [[np.nan], [-np.inf], [-4]], 1, 8, 0)
    assert am[0, 0, 0].tolist() == [2] and pooled[0, 0, 0].tolist() == [-4]


def test_aware_average_adds_in_list_order_in_fp32():
    pts = [[4, 2, 0], [4.5, 2, 0], [5, 2, 0]]
    a, b, c = F(2 ** 24), F(1), F(-2 ** 24)
    _, _, pooled = aware(pts, [[a], [b], [c]], 1, 8, 1)
    assert pooled[0, 0, 0, 0] == ((a + b) + c) / F(3) == 0          # (2^24 + 1) rounds to 2^24: another order gives 1/3
    _, _, pooled = aware(pts, [[a], [c], [b]], 1, 8, 1)
    assert pooled[0, 0, 0, 0] == F(1) / F(3)


def test_backward_restatement_known_answer():
    pts = [[4, 2, 0], [4.5, 2, 0], [50, 2, 0]]
    idx, am, _ = aware(pts, [[5, -3], [5, -2], [0, 0]], 1, 8, 0)
    g = np.zeros((3, 2))
    rp.roiaware_pool3d_backward(idx[None], am[None], F([[[[[2, 3]]]]]), g, 0)
    assert g.tolist() == [[2, 0], [0, 3], [0, 0]]
    g = np.zeros((3, 2))
    rp.roiaware_pool3d_backward(idx[None], None, F([[[[[2, 3]]]]]), g, 1)
    assert g.tolist() == [[1, 1.5], [1, 1.5], [0, 0]]


# ---- the second stage against the reference's own run ---------------------------------------------------------------------
def test_residual_coder_matches_the_reference(fix):
    from pdm_ssd_amd.utils.box_coder_utils import ResidualCoder
    for tag, coder in (('coder', ResidualCoder()), ('coder_sincos', ResidualCoder(encode_angle_by_sincos=True))):
        assert coder.code_size == (8 if 'sincos' in tag else 7)
        boxes, anchors = torch.from_numpy(fix['coder_boxes'].copy()), torch.from_numpy(fix['coder_anchors'].copy())
        code = coder.encode_torch(boxes, anchors)
        np.testing.assert_allclose(code.numpy(), fix[f'{tag}_code'], rtol=1e-6, atol=1e-6)
        dec = coder.decode_torch(torch.from_numpy(fix[f'{tag}_code']), torch.from_numpy(fix['coder_anchors'].copy()))
        np.testing.assert_allclose(dec.numpy(), fix[f'{tag}_decoded'], rtol=1e-6, atol=1e-6)


def reduced_head():
    from pdm_ssd_amd.config import cfg_from_dict
    from pdm_ssd_amd.roi_heads import PointRCNNHead
    return PointRCNNHead(input_channels=roi_head_case.HEAD_INPUT_CHANNELS, model_cfg=cfg_from_dict(copy.deepcopy(roi_head_case.HEAD_CFG)),
                         num_class=1)


@pytest.mark.parametrize('case', ['d', 'e'])
def test_generate_predicted_boxes_matches_the_reference(fix, case):
    head = reduced_head()
    cls, box = head.generate_predicted_boxes(2, torch.from_numpy(fix[f'{case}_rois']), torch.from_numpy(fix[f'{case}_rcnn_cls']),
                                             torch.from_numpy(fix[f'{case}_rcnn_reg']))
    np.testing.assert_allclose(cls.numpy(), fix[f'{case}_batch_cls_preds'], rtol=1e-6, atol=1e-6)
    np.testing.assert_allclose(box.numpy(), fix[f'{case}_batch_box_preds'], rtol=1e-6, atol=1e-6)


def test_head_state_dict_manifest_equals_the_reference(manifest):
    from pdm_ssd_amd.config import cfg_from_dict
    from pdm_ssd_amd.detector_config import POINT_RCNN_CFG
    from pdm_ssd_amd.roi_heads import PointRCNNHead
    got = {k: list(v.shape) for k, v in reduced_head().state_dict().items()}
    assert got == manifest['PointRCNNHead(reduced: tests/roi_head_case.py HEAD_CFG, input_channels=16, num_class=1)']
    full = PointRCNNHead(input_channels=128, model_cfg=cfg_from_dict(copy.deepcopy(POINT_RCNN_CFG['ROI_HEAD'])), num_class=1)
    assert {k: list(v.shape) for k, v in full.state_dict().items()} == \
        manifest['PointRCNNHead(POINT_RCNN_CFG, input_channels=128, num_class=1)']


def test_reduced_point_rcnn_builds_with_the_recorded_keys(manifest):
    from pdm_ssd_amd.detector_config import build_point_rcnn
    model = build_point_rcnn(roi_head_case.REDUCED_POINT_RCNN_CFG)
    assert type(model).__name__ == 'PointRCNN' and type(model.roi_head).__name__ == 'PointRCNNHead'
    assert model.module_list[-1] is model.roi_head and model.point_head.predict_boxes_when_training
    got = {k: list(v.shape) for k, v in model.state_dict().items()}
    assert got == manifest['PointRCNN(tests/roi_head_case.py REDUCED_POINT_RCNN_CFG, 4 point features, 3 classes)']


def test_pdm_ssd_still_refuses_a_roi_head():
    from pdm_ssd_amd.detector_config import PDM_SSD_CFG, POINT_RCNN_CFG, build_pdm_ssd
    with pytest.raises(AssertionError, match='ROI_HEAD'):
        build_pdm_ssd(dict(PDM_SSD_CFG, ROI_HEAD=copy.deepcopy(POINT_RCNN_CFG['ROI_HEAD'])))


def test_pool_extra_width_scalar_means_all_three_sizes():
    from pdm_ssd_amd.roipoint_pool3d.roipoint_pool3d_utils import RoIPointPool3d, _extra_width
    assert _extra_width(1.0) == [1.0, 1.0, 1.0] and _extra_width([0.1, 0.2, 0.3]) == [0.1, 0.2, 0.3]
    assert RoIPointPool3d().pool_extra_width == 1.0 and RoIPointPool3d().num_sampled_points == 512

"""Second-stage training, the part that needs no GPU: the numpy restatement's known answers, the torch formulation of the
rcnn losses against the values the REFERENCE's own code gave (tests/golden/ref_roi_targets.npz, written by
tests/golden/gen_roi_target_fixtures.py), the corner helpers, and the configuration rule."""
import copy

import numpy as np
import pytest
import torch

import roi_target_reference as rt

from roi_target_case import FIXTURE, SAMPLER, check_losses_against_reference, template_head


@pytest.fixture(scope='module')
def fix():
    return dict(np.load(FIXTURE))


def test_restatement_known_heading_folds():
    for roi_h, gt_h, want in rt.KNOWN_FOLDS:
        roi = np.array([1, 2, 3, 4, 2, 1.5, roi_h], dtype=np.float32)
        g = np.array([1.5, 2.5, 3.2, 4, 2, 1.5, gt_h, 2], dtype=np.float32)
        got = rt.canonical(roi, g)
        assert abs(float(got[6]) - want) < 2e-6, (roi_h, gt_h, float(got[6]), want)
        assert -np.pi / 2 - 1e-6 <= float(got[6]) <= np.pi / 2 + 1e-6 and got[7] == 2 and (got[3:6] == g[3:6]).all()


def test_restatement_canonical_position_known_answer():
    # RoI at (1, 2, 3) facing +y (pi / 2); the ground truth 2 m further along +y and 1 m up: 2 m ahead in the RoI's frame
    got = rt.canonical(np.array([1, 2, 3, 4, 2, 1.5, np.pi / 2], dtype=np.float32), np.array([1, 4, 4, 4, 2, 1.5, np.pi / 2, 1], dtype=np.float32))
    np.testing.assert_allclose(got[0:3], [2, 0, 1], atol=1e-6)
    assert abs(float(got[6])) < 1e-6


def test_restatement_known_counts():
    for (n_fg, n_hard, n_easy), want in rt.KNOWN_COUNTS:
        assert rt.counts(n_fg, n_hard, n_easy, 16, 8, 0.8) == want, (n_fg, n_hard, n_easy)
    assert int(np.round(0.5 * 16)) == 8 and int(np.round(0.5 * 5)) == 2       # np.round: half to even, as the reference


def test_restatement_draw_rule_properties():
    for n in (1, 2, 3, 7, 16, 17, 70, 1024):
        perm = [rt.feistel_perm(i, n, 0x1234567) for i in range(n)]
        assert sorted(perm) == list(range(n))
    assert rt.fmix32(0) == 0 and rt.fmix32(1) == 0x514E28B7                   # murmur3's finaliser
    idx = [rt.draw_index(rt.draw_key(5, 0, 1, 3), j, 8) for j in range(64)]
    assert min(idx) >= 0 and max(idx) < 8 and len(set(idx)) > 1
    assert rt.draw_key(5, 0, 1, 3) != rt.draw_key(5, 1, 1, 3) != rt.draw_key(5, 1, 2, 3)


def test_restatement_row_rule_and_ties():
    gt = np.zeros((5, 8), dtype=np.float32)
    gt[0] = [0, 0, 0, 2, 2, 2, 0, 1]
    gt[2] = [0, 0, 0, 2, 2, 2, 0, 1]          # identical to row 0: a tie
    assert rt.live_rows(gt).shape[0] == 3      # the interior zero row stays, the trailing two go
    assert rt.live_rows(np.zeros((4, 8), dtype=np.float32)).shape == (1, 8)
    assert rt.live_rows(np.zeros((0, 8), dtype=np.float32)).shape == (1, 8)


def test_restatement_reproduces_the_reference_run(fix, oracle):
    for tag in ('cls', 'roi_iou'):
        ref = rt.proposal_targets(fix['rois'], fix['roi_scores'], fix['roi_labels'], fix['gt_boxes'], dict(SAMPLER, CLS_SCORE_TYPE=tag),
                                  int(fix['draw'][0]), int(fix['draw'][1]))
        assert (ref['sampled_inds'] == fix[f'{tag}.sampled_inds']).all() and not ref['failed'].any()
        for key in ('rois', 'roi_labels', 'roi_scores', 'reg_valid_mask', 'gt_of_rois_src'):
            assert (ref[key] == fix[f'{tag}.{key}']).all(), key
        np.testing.assert_allclose(ref['gt_iou_of_rois'], fix[f'{tag}.gt_iou_of_rois'], atol=1e-6)
        np.testing.assert_allclose(ref['gt_of_rois'], fix[f'{tag}.gt_of_rois'], atol=1e-5)
        np.testing.assert_allclose(ref['rcnn_cls_labels'], fix[f'{tag}.rcnn_cls_labels'], atol=1e-6)
    # the tie rule: a RoI equally on two identical boxes goes to the first
    gt = np.zeros((1, 3, 8), dtype=np.float32)
    gt[0, 0] = gt[0, 1] = [5, 5, 0, 3.9, 1.6, 1.5, 0.3, 1]
    mo, ga = rt.assign(gt[0, :1, 0:7].copy(), np.array([1]), gt[0, :2], True)
    assert ga[0] == 0 and mo[0] > 0.99


def test_torch_loss_formulation_matches_the_reference_run(fix):
    head = template_head(fix)
    head.use_fused_loss = True           # (not on the GPU: the torch formulation runs whatever the switch says)
    check_losses_against_reference(head, fix, torch.device('cpu'))


def test_corner_helpers_match_the_reference(fix):
    from pdm_ssd_amd.utils import box_utils, loss_utils
    a, b = torch.from_numpy(fix['corner_boxes_a']), torch.from_numpy(fix['corner_boxes_b'])
    np.testing.assert_allclose(box_utils.boxes_to_corners_3d(a).numpy(), fix['corners_a'], rtol=0, atol=1e-5)
    np.testing.assert_allclose(loss_utils.get_corner_loss_lidar(a, b).numpy(), fix['corner_loss'], rtol=1e-5, atol=1e-6)
    # a box against itself turned by pi: the same solid, no loss
    turned = a.clone()
    turned[:, 6] += np.pi
    assert float(loss_utils.get_corner_loss_lidar(a, turned).max()) < 1e-5


def test_config_rule():
    from pdm_ssd_amd import detector_config as dc
    from pdm_ssd_amd.config import cfg_from_dict
    from pdm_ssd_amd.roi_heads import PointRCNNHead
    from pdm_ssd_amd.roi_heads.target_assigner import ProposalTargetLayer
    assert dc.POINT_RCNN_CFG['ROI_HEAD']['TARGET_CONFIG'] == {'BOX_CODER': 'ResidualCoder'} and 'LOSS_CONFIG' not in dc.POINT_RCNN_CFG['ROI_HEAD']
    t = dc.POINT_RCNN_TRAIN_CFG['ROI_HEAD']
    assert t['TARGET_CONFIG'] == {'BOX_CODER': 'ResidualCoder', 'ROI_PER_IMAGE': 128, 'FG_RATIO': 0.5, 'SAMPLE_ROI_BY_EACH_CLASS': True,
                                  'CLS_SCORE_TYPE': 'cls', 'CLS_FG_THRESH': 0.6, 'CLS_BG_THRESH': 0.45, 'CLS_BG_THRESH_LO': 0.1,
                                  'HARD_BG_RATIO': 0.8, 'REG_FG_THRESH': 0.55}
    assert t['LOSS_CONFIG'] == {'CLS_LOSS': 'BinaryCrossEntropy', 'REG_LOSS': 'smooth-l1', 'CORNER_LOSS_REGULARIZATION': True,
                                'LOSS_WEIGHTS': {'rcnn_cls_weight': 1.0, 'rcnn_reg_weight': 1.0, 'rcnn_corner_weight': 1.0,
                                                 'code_weights': [1.0] * 7}}
    rest = copy.deepcopy(dc.POINT_RCNN_TRAIN_CFG)
    rest['ROI_HEAD']['TARGET_CONFIG'] = {'BOX_CODER': 'ResidualCoder'}
    del rest['ROI_HEAD']['LOSS_CONFIG']
    assert rest == dc.POINT_RCNN_CFG
    plain = PointRCNNHead(input_channels=128, model_cfg=cfg_from_dict(copy.deepcopy(dc.POINT_RCNN_CFG['ROI_HEAD'])), num_class=1)
    assert plain.proposal_target_layer is None and not plain.has_training_half
    with pytest.raises(NotImplementedError, match='ProposalTargetLayer and the rcnn losses are not built'):
        plain.get_loss()
    full = PointRCNNHead(input_channels=128, model_cfg=cfg_from_dict(copy.deepcopy(t)), num_class=1, seed=7)
    assert isinstance(full.proposal_target_layer, ProposalTargetLayer) and full.proposal_target_layer.seed == 7
    assert full.has_training_half and full.use_fused_loss and full.reg_loss_func.code_weights.tolist() == [1.0] * 7
    assert set(plain.state_dict()) == set(full.state_dict())       # the training half adds no parameter or buffer
    model = dc.build_point_rcnn(model_cfg=dc.POINT_RCNN_TRAIN_CFG)
    assert isinstance(model.roi_head.proposal_target_layer, ProposalTargetLayer)


def test_wider_boxes_are_refused():
    from pdm_ssd_amd.roi_heads.target_assigner import ProposalTargetLayer
    layer = ProposalTargetLayer(SAMPLER)
    bd = {'batch_size': 1, 'rois': torch.zeros(1, 4, 8), 'roi_scores': torch.zeros(1, 4), 'roi_labels': torch.ones(1, 4, dtype=torch.long),
          'gt_boxes': torch.zeros(1, 2, 9)}
    with pytest.raises(ValueError, match='code size 7'):
        layer(bd)


def test_entry_points_validate_their_arguments_before_any_launch():
    """no GPU is touched: the checks come first (R <= 1024, M <= 256, rows <= 262144, the workspace size)"""
    import ctypes as C

    from pdm_ssd_amd import _native
    ptr = C.cast((C.c_float * 64)(), C.c_void_p)

    def targets(B, R, M, S, fg=8):
        _native.call('pdm_proposal_targets', 0, B, R, M, S, ptr, ptr, ptr, ptr, 1, fg, 0.8, 0.55, 0.6, 0.45, 0.1, 0, 0, *([ptr] * 11))
    for R, M in ((1025, 4), (4, 257)):
        with pytest.raises(_native.NativeLibraryError, match='code -2'):
            targets(1, R, M, 16)
    for bad in ((1, 0, 4, 16), (1, 4, 4, 0), (-1, 4, 4, 16), (1, 4, 4, 16, 17)):
        with pytest.raises(_native.NativeLibraryError, match='code -1'):
            targets(*bad)
    targets(0, 4, 4, 16)                                  # an empty batch is served without a launch
    assert _native.lib().pdm_rcnn_loss_workspace_bytes(1000) == 16 + 4 * 3 * 4
    with pytest.raises(_native.NativeLibraryError, match='code -2'):
        _native.call('pdm_rcnn_loss', 0, 262145, *([ptr] * 7), 0, ptr, 0.1, 1.0, 1.0, 1.0, 1, *([ptr] * 7), ptr, 1 << 30)
    with pytest.raises(_native.NativeLibraryError, match='workspace too small'):
        _native.call('pdm_rcnn_loss', 0, 1000, *([ptr] * 7), 0, ptr, 0.1, 1.0, 1.0, 1.0, 1, *([ptr] * 7), ptr, 16)
    with pytest.raises(_native.NativeLibraryError, match='code -1'):
        _native.call('pdm_rcnn_loss', 0, 0, *([ptr] * 7), 0, ptr, 0.1, 1.0, 1.0, 1.0, 1, *([ptr] * 7), ptr, 1 << 20)

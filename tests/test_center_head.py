"""CenterHead on the CPU against the reference's own Python (tests/golden/ref_center_head.npz): the torch formulations of
utils/centernet_utils.py and utils/loss_utils.py, the head's targets, losses and gradients, and its constructor."""
import copy

import numpy as np
import pytest
import torch

import center_head_case as case
from center_head_case import B, H, W, close, fixture
from pdm_ssd_amd.utils import centernet_utils, loss_utils


def test_state_dict_keys_and_shapes_are_the_reference_s():
    for key, want in case.manifest().items():
        names = case.HEADS['one'] if "'Car', 'Pedestrian', 'Cyclist'" in key else case.HEADS['two']
        got = {k: list(v.shape) for k, v in case.build_head(names).state_dict().items()}
        assert got == want
    keys = list(case.build_head(case.HEADS['two']).state_dict())
    assert 'shared_conv.0.weight' in keys and 'shared_conv.1.running_mean' in keys
    assert 'heads_list.1.hm.1.bias' in keys and 'heads_list.0.center_z.0.0.weight' in keys


def test_initialisation_follows_the_reference():
    head = case.build_head(case.HEADS['one'])
    h = head.heads_list[0]
    assert torch.all(h.hm[-1].bias == -2.19)
    for name in case.MAPS:
        assert torch.all(getattr(h, name)[-1].bias == 0) and float(getattr(h, name)[-1].weight.detach().std()) > 0


@pytest.mark.parametrize("tag", ["10", "all"])
def test_decode_formulation_matches_the_reference(tag):
    fx = fixture()
    K = 10 if tag == "10" else H * W
    thresh = float(fx[f'dec_thresh_{tag}'])
    m = case.decode_maps()
    kw = dict(heatmap=m['hm'].sigmoid(), rot_cos=m['rot'][:, 0:1], rot_sin=m['rot'][:, 1:2], center=m['center'], center_z=m['center_z'],
              dim=m['dim'].exp(), point_cloud_range=case.PC_RANGE, voxel_size=case.VOXEL, feature_map_stride=case.STRIDE, K=K)
    ranked = centernet_utils.decode_bbox_from_heatmap(score_thresh=None, post_center_limit_range=[-1e9] * 3 + [1e9] * 3, **kw)
    assert all(len(d['pred_boxes']) == K for d in ranked)
    case.check_decode_conditions(fx['dec_hm'], K, thresh, np.stack([d['pred_boxes'].numpy() for d in ranked]))
    got = centernet_utils.decode_bbox_from_heatmap(score_thresh=thresh, post_center_limit_range=case.LIMIT, **kw)
    assert len(got) == B
    for b, d in enumerate(got):
        assert np.array_equal(d['pred_labels'].numpy().astype(np.int64), fx[f'dec{tag}.labels.{b}'])
        close(d['pred_boxes'].numpy(), fx[f'dec{tag}.boxes.{b}'])
        close(d['pred_scores'].numpy(), fx[f'dec{tag}.scores.{b}'])
    if tag == "10":
        assert 0 < len(got[0]['pred_boxes']) < K and len(got[1]['pred_boxes']) == 0     # filtered by range and threshold; no survivor


def test_topk_is_two_stage_and_rejects_k_beyond_the_map():
    m = case.decode_maps()
    scores = m['hm'].sigmoid()
    s, cells, classes, ys, xs = centernet_utils._topk(scores, K=7)
    flat_s, flat_i = torch.topk(scores.flatten(1), 7)
    assert torch.equal(s, flat_s) and torch.equal(cells, flat_i % (H * W)) and torch.equal(classes.long(), flat_i // (H * W))
    assert torch.equal(ys, (cells // W).float()) and torch.equal(xs, (cells % W).float())
    with pytest.raises(RuntimeError):
        centernet_utils._topk(scores, K=H * W + 1)
    feat = centernet_utils._transpose_and_gather_feat(m['dim'], cells)
    assert torch.equal(feat[1, 3], m['dim'][1, :, int(ys[1, 3]), int(xs[1, 3])])


def test_circle_nms_stays_unsupported():
    m = case.decode_maps()
    with pytest.raises(AssertionError, match="circle_nms"):
        centernet_utils.decode_bbox_from_heatmap(m['hm'].sigmoid(), m['rot'][:, 0:1], m['rot'][:, 1:2], m['center'], m['center_z'], m['dim'],
                                                 point_cloud_range=case.PC_RANGE, voxel_size=case.VOXEL, feature_map_stride=8, K=5,
                                                 circle_nms=True, post_center_limit_range=case.LIMIT)


def test_reg_loss_formulation_matches_the_reference():
    fx = fixture()
    pred = torch.from_numpy(fx['reg_pred']).requires_grad_(True)
    mask, inds, target = (torch.from_numpy(fx[k]) for k in ('reg_mask', 'reg_inds', 'reg_target'))
    w = torch.from_numpy(fx['reg_code_weights'])
    per_code = loss_utils.RegLossCenterNet()(pred, mask, inds, target)
    (per_code * w).sum().mul(float(fx['reg_loc_weight'])).backward()
    finite = [0, 1, 2, 3, 5, 6, 7]                      # code 4 holds the NaN target element: NaN in the reference, left out here
    assert np.isnan(fx['reg_per_code'][4])
    close(per_code.detach().numpy()[finite], fx['reg_per_code'][finite])
    clean = target.clone()
    clean[0, 1, 4] = pred[0, 4].flatten()[inds[0, 1]].detach()            # a target equal to the prediction adds nothing either
    close(per_code.detach().numpy(), loss_utils.RegLossCenterNet()(pred.detach(), mask, inds, clean).numpy(), tol=1e-6)
    close(pred.grad.numpy(), fx['reg_grad'])
    pred0 = torch.from_numpy(fx['reg_pred']).requires_grad_(True)
    zero = loss_utils.RegLossCenterNet()(pred0, torch.zeros_like(mask), inds, target)
    zero.sum().backward()
    close(zero.detach().numpy(), fx['reg_zero_per_code'])
    assert torch.count_nonzero(pred0.grad) == 0 and not fx['reg_zero_grad'].any()


@pytest.mark.parametrize("tag", ["one", "two"])
def test_head_on_the_cpu_matches_the_reference(tag):
    fx = fixture()
    head = case.build_head(case.HEADS[tag], tag).train()
    gt = torch.from_numpy(fx['gt_boxes'].copy())
    head({'batch_size': B, 'spatial_features_2d': torch.from_numpy(fx['spatial_features_2d']), 'gt_boxes': gt})
    assert torch.equal(gt, torch.from_numpy(fx['gt_boxes'])), 'assign_targets must leave gt_boxes untouched'
    td, preds = head.forward_ret_dict['target_dicts'], head.forward_ret_dict['pred_dicts']
    assert set(td) == {'heatmaps', 'target_boxes', 'inds', 'masks', 'heatmap_masks', 'target_boxes_src'}
    case.check_targets(td, f'{tag}.targets')
    for h, pd in enumerate(preds):
        for name in ('hm',) + case.MAPS:
            close(pd[name].detach().numpy(), fx[f'{tag}.pred.{name}.{h}'])
            pd[name].retain_grad()
    loss, tb = head.get_loss()
    assert set(tb) == {f'{k}_loss_head_{h}' for h in range(len(preds)) for k in ('hm', 'loc')} | {'rpn_loss'}
    for k, v in tb.items():
        assert torch.is_tensor(v) and not v.requires_grad
        close(float(v), float(fx[f'{tag}.tb.{k}']))
    close(float(loss.detach()), float(fx[f"{tag}.loss"]))
    loss.backward()
    for h, pd in enumerate(preds):
        for name in ('hm',) + case.MAPS:
            close(pd[name].grad.numpy(), fx[f'{tag}.grad.{name}.{h}'])


def test_only_the_first_num_max_objs_boxes_take_part():
    head = case.build_head(case.HEADS['one'])
    over = torch.from_numpy(fixture()['gt_boxes_over'].copy())
    assert int((over[0, :, 7] > 0).sum()) > 6
    case.check_targets(head.assign_targets(over, feature_map_size=(H, W)), 'one.targets_over')


def test_interleaved_heads_see_only_their_own_classes():
    head = case.build_head([['Car', 'Cyclist'], ['Pedestrian']])
    gt = torch.from_numpy(fixture()['gt_boxes'].copy())
    td = head.assign_targets(gt, feature_map_size=(H, W))
    assert torch.equal(gt, torch.from_numpy(fixture()['gt_boxes']))
    for h, (src, inds, mask) in case.interleaved_expectation().items():
        assert np.array_equal(td['target_boxes_src'][h].numpy(), src), h
        assert np.array_equal(td['inds'][h].numpy(), inds) and np.array_equal(td['masks'][h].numpy(), mask), h
        assert td['heatmaps'][h].shape == (B, 2 - h, H, W)
        peaks = (td['heatmaps'][h] == 1).nonzero().tolist()
        want = sorted([0, int(src[0, k, 7]) - 1, int(inds[0, k]) // W, int(inds[0, k]) % W] for k in range(6) if mask[0, k])
        assert sorted(peaks) == want, h


@pytest.mark.parametrize("edit, word", [
    (lambda c: c['POST_PROCESSING']['NMS_CONFIG'].update(NMS_TYPE='class_specific_nms'), 'class_specific_nms'),
    (lambda c: c['POST_PROCESSING']['NMS_CONFIG'].update(NMS_TYPE='circle_nms'), 'circle_nms'),
    (lambda c: c['SEPARATE_HEAD_CFG']['HEAD_DICT'].update(iou={'out_channels': 1, 'num_conv': 2}), 'iou'),
    (lambda c: c.update(IOU_REG_LOSS=True), 'IOU_REG_LOSS'),
    (lambda c: c['POST_PROCESSING'].update(USE_IOU_TO_RECTIFY_SCORE=True), 'USE_IOU_TO_RECTIFY_SCORE'),
])
def test_constructor_rejects_what_is_out_of_scope(edit, word):
    from pdm_ssd_amd.dense_heads import CenterHead
    cfg = copy.deepcopy(case.head_cfg(case.HEADS['one']))
    edit(cfg)
    with pytest.raises(NotImplementedError, match=word):
        CenterHead(model_cfg=cfg, input_channels=8, num_class=3, class_names=case.CLASS_NAMES, grid_size=[160, 96, 40],
                   point_cloud_range=case.PC_RANGE, voxel_size=case.VOXEL)


def test_reorder_rois_pads_to_the_longest_sample():
    from pdm_ssd_amd.dense_heads import CenterHead
    dicts = [{'pred_boxes': torch.ones(2, 7), 'pred_scores': torch.tensor([0.9, 0.8]), 'pred_labels': torch.tensor([1, 3])},
             {'pred_boxes': torch.zeros(0, 7), 'pred_scores': torch.zeros(0), 'pred_labels': torch.zeros(0, dtype=torch.long)}]
    rois, scores, labels = CenterHead.reorder_rois_for_refining(2, dicts)
    assert rois.shape == (2, 2, 7) and labels.dtype == torch.int64 and labels.tolist() == [[1, 3], [0, 0]]
    assert scores[0].tolist() == pytest.approx([0.9, 0.8]) and not rois[1].any()


def test_center_pdm_config_builds_a_centerpoint():
    from pdm_ssd_amd.detector_config import CENTER_PDM_CFG, build_center_pdm
    from pdm_ssd_amd.detectors import CenterPoint
    model = build_center_pdm()
    assert isinstance(model, CenterPoint) and type(model.dense_head).__name__ == 'CenterHead' and model.point_head is None
    assert CENTER_PDM_CFG['DENSE_HEAD']['CLASS_NAMES_EACH_HEAD'] == [['Car', 'Pedestrian', 'Cyclist']]
    ta, pp = CENTER_PDM_CFG['DENSE_HEAD']['TARGET_ASSIGNER_CONFIG'], CENTER_PDM_CFG['DENSE_HEAD']['POST_PROCESSING']
    assert (ta['FEATURE_MAP_STRIDE'], ta['NUM_MAX_OBJS'], pp['MAX_OBJ_PER_SAMPLE']) == (8, 500, 500)
    assert not model.dense_head.predict_boxes_when_training


def test_entry_points_validate_their_arguments_before_any_launch():
    import ctypes as C

    from pdm_ssd_amd import _native
    buf = (C.c_float * 64)()
    ptr = C.cast(buf, C.c_void_p)
    table = C.cast((C.c_int * 8)(0, 1, 2, 3), C.c_void_p)
    with pytest.raises(_native.NativeLibraryError, match="out of range"):      # K > H * W, as torch.topk
        _native.call("pdm_center_decode", 0, 1, 3, 4, 5, 21, ptr, ptr, ptr, 0.1, ptr, 0.0, 0.0, 0.05, 0.05, 8.0, table, ptr, ptr, ptr, ptr)
    with pytest.raises(_native.NativeLibraryError, match="class table"):
        _native.call("pdm_center_targets", 0, 1, 4, 8, 2, 4, 5, ptr, 3, table, 0.0, 0.0, 0.05, 0.05, 8.0, 6, 0.1, 2, ptr, ptr, ptr, ptr, ptr)
    with pytest.raises(_native.NativeLibraryError, match="bad size"):          # 17 regression channels
        _native.call("pdm_center_reg_loss", 0, 1, 6, 17, 4, 5, ptr, ptr, ptr, ptr, ptr, ptr, ptr, 1.0, ptr, ptr, ptr, ptr, 1024)
    assert _native.lib().pdm_center_reg_loss_workspace_bytes(32, 8) == 32 * 9 * 8

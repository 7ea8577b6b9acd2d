"""PointRCNN's second stage on the device: the eval forward of PointRCNNHead against the reference's own head
(tests/golden/ref_roi.npz, written by tests/golden/gen_roi_fixtures.py), proposal_layer, and the detector end to end."""
import copy
import os

import numpy as np
import pytest
import torch

import roi_head_case

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope='module')
def fix():
    return dict(np.load(os.path.join(HERE, 'golden', 'ref_roi.npz')))


def reduced_head(fix, dev):
    from pdm_ssd_amd.config import cfg_from_dict
    from pdm_ssd_amd.roi_heads import PointRCNNHead
    head = PointRCNNHead(input_channels=roi_head_case.HEAD_INPUT_CHANNELS, model_cfg=cfg_from_dict(copy.deepcopy(roi_head_case.HEAD_CFG)),
                         num_class=1)
    head.load_state_dict({k[len('head_state.'):]: torch.from_numpy(v) for k, v in fix.items() if k.startswith('head_state.')})
    return head.to(dev).eval()


@pytest.mark.gpu
@pytest.mark.parametrize('case', ['d', 'e'])     # (d) all headings exactly 0: bit-equal canonical points; (e) random headings
def test_eval_forward_matches_the_reference_head(dev, fix, case):
    """the project's fp32-feature parity bound (README): allclose(rtol=1e-4, atol=1e-4)"""
    head = reduced_head(fix, dev)
    bd = {'batch_size': 2, 'point_coords': torch.from_numpy(fix[f'{case}_coords']).to(dev),
          'point_features': torch.from_numpy(fix[f'{case}_feats']).to(dev),
          'point_cls_scores': torch.from_numpy(fix[f'{case}_scores']).to(dev), 'rois': torch.from_numpy(fix[f'{case}_rois']).to(dev)}
    with torch.no_grad():
        pooled = head.roipool3d_gpu(bd).cpu().numpy()
        out = head(bd)
    if case == 'd':
        assert (pooled[..., 0:3].view(np.uint32) == fix['d_pooled'][..., 0:3].view(np.uint32)).all()
    for key, got in (('rcnn_cls', out['rcnn_cls']), ('rcnn_reg', out['rcnn_reg']), ('batch_box_preds', out['batch_box_preds']),
                     ('batch_cls_preds', out['batch_cls_preds'])):
        want = fix[f'{case}_{key}']
        got = got.cpu().numpy()
        assert got.shape == want.shape, (key, got.shape, want.shape)
        print(case, key, 'max abs difference', float(np.abs(got - want).max()), 'scale', float(np.abs(want).max()))
        np.testing.assert_allclose(got, want, rtol=1e-4, atol=1e-4, err_msg=key)
    assert out['cls_preds_normalized'] is False


@pytest.mark.gpu
def test_training_mode_says_what_is_not_built(dev, fix):
    head = reduced_head(fix, dev).train()
    with pytest.raises(NotImplementedError, match='ProposalTargetLayer and the rcnn losses are not built'):
        head({'batch_size': 2})


@pytest.mark.gpu
def test_proposal_layer(dev, fix):
    head = reduced_head(fix, dev)
    cfg = {'NMS_TYPE': 'nms_gpu', 'MULTI_CLASSES_NMS': False, 'NMS_PRE_MAXSIZE': 64, 'NMS_POST_MAXSIZE': 8, 'NMS_THRESH': 0.5}
    rng = np.random.default_rng(4)
    n = 64
    boxes = np.zeros((2 * n, 7), dtype=np.float32)
    gx, gy = np.meshgrid(np.arange(8), np.arange(8))
    boxes[:n, 0], boxes[:n, 1] = gx.ravel() * 10.0, gy.ravel() * 10.0          # sample 0: 64 boxes far apart, all survive
    boxes[n:, 0:2] = np.array([[5, 5], [25, 5], [45, 5]], dtype=np.float32)[np.arange(n) % 3] + rng.uniform(-1e-3, 1e-3, (n, 2))
    boxes[:, 3:6] = [3.9, 1.6, 1.5]                                            # sample 1: three piles of near-copies
    boxes[:, 6] = rng.uniform(-0.02, 0.02, 2 * n)                              # (near-copies overlap at IoU > 0.9)
    cls = rng.standard_normal((2 * n, 3)).astype(np.float32)
    index = np.repeat(np.arange(2), n).astype(np.float32)
    bd = {'batch_size': 2, 'batch_box_preds': torch.from_numpy(boxes).to(dev), 'batch_cls_preds': torch.from_numpy(cls).to(dev),
          'batch_index': torch.from_numpy(index).to(dev)}
    out = head.proposal_layer(bd, nms_config=cfg)
    rois, scores, labels = out['rois'].cpu().numpy(), out['roi_scores'].cpu().numpy(), out['roi_labels'].cpu().numpy()
    assert rois.shape == (2, 8, 7) and scores.shape == (2, 8) and labels.shape == (2, 8) and out['roi_labels'].dtype == torch.long
    assert out['has_class_labels'] is True and 'batch_index' not in out
    best = cls.max(1)
    top = np.argsort(-best[:n], kind='stable')[:8]
    assert (rois[0] == boxes[:n][top]).all() and (scores[0] == best[:n][top]).all()
    assert (labels[0] == cls[:n][top].argmax(1) + 1).all()
    kept = int((np.abs(rois[1]).sum(1) > 0).sum())
    assert kept == 3                                                           # one survivor per pile
    assert (rois[1, kept:] == 0).all() and (scores[1, kept:] == 0).all()        # zero padding behind the kept rows
    assert (np.diff(scores[1, :kept]) <= 0).all()
    assert ((labels >= 1) & (labels <= 3)).all()
    # a batch_dict that already holds rois is returned as it is
    given = {'batch_size': 2, 'rois': out['rois']}
    assert head.proposal_layer(given, nms_config=cfg) is given and set(given) == {'batch_size', 'rois'}
    with pytest.raises(NotImplementedError):
        head.proposal_layer({'batch_size': 2, 'batch_box_preds': bd['batch_box_preds'], 'batch_cls_preds': bd['batch_cls_preds'],
                             'batch_index': torch.from_numpy(index).to(dev)}, nms_config=dict(cfg, MULTI_CLASSES_NMS=True))


@pytest.mark.gpu
def test_point_rcnn_end_to_end_in_eval(dev):
    from detector_case import scene_boxes
    from pdm_ssd_amd import synthetic
    from pdm_ssd_amd.detector_config import build_point_rcnn
    torch.manual_seed(3)
    model = build_point_rcnn(roi_head_case.REDUCED_POINT_RCNN_CFG).to(dev).eval()
    B, N = 2, 1024
    cl = synthetic.lidar_like_clouds(B, N, 5)
    gt = scene_boxes(B, 6, 3)
    cl[:, :200, :3] = gt[:, :1, :3] + np.random.default_rng(0).normal(0, 0.5, (B, 200, 3)).astype(np.float32)
    batch = {'batch_size': B, 'points': torch.from_numpy(synthetic.to_batch_points(cl)).to(dev), 'gt_boxes': torch.from_numpy(gt).to(dev)}
    with torch.no_grad():
        pred_dicts, recall_dict = model(batch)
    assert len(pred_dicts) == B
    for d in pred_dicts:
        k = d['pred_boxes'].shape[0]
        assert d['pred_boxes'].shape == (k, 7) and d['pred_scores'].shape == (k,) and d['pred_labels'].shape == (k,)
        assert torch.isfinite(d['pred_boxes']).all() and torch.isfinite(d['pred_scores']).all()
        assert k <= 16 and ((d['pred_labels'] >= 1) & (d['pred_labels'] <= 3)).all()
    assert {'gt', 'roi_0.3', 'rcnn_0.3', 'roi_0.7', 'rcnn_0.7'} <= set(recall_dict) and recall_dict['gt'] == 11
    model.roi_head.train()
    with pytest.raises(NotImplementedError, match='ProposalTargetLayer and the rcnn losses are not built'):
        with torch.no_grad():
            model(dict(batch))

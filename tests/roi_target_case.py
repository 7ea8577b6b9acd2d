"""What tests/test_roi_targets_host.py and tests/test_roi_targets_gpu.py share: the sampler settings of the fixture case
(tests/golden/gen_roi_target_fixtures.py), a bare RoIHeadTemplate under them, the recorded loss inputs, and the check of
the rcnn losses and their gradients against the values the reference's own code gave."""
import os

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, 'golden', 'ref_roi_targets.npz')
SAMPLER = {'BOX_CODER': 'ResidualCoder', 'ROI_PER_IMAGE': 16, 'FG_RATIO': 0.5, 'SAMPLE_ROI_BY_EACH_CLASS': True, 'CLS_SCORE_TYPE': 'cls',
           'CLS_FG_THRESH': 0.6, 'CLS_BG_THRESH': 0.45, 'CLS_BG_THRESH_LO': 0.1, 'HARD_BG_RATIO': 0.8, 'REG_FG_THRESH': 0.55}


def template_head(fix, score_type='cls', **kwargs):
    """a bare RoIHeadTemplate with the fixture's sampler and loss settings"""
    from pdm_ssd_amd.config import cfg_from_dict
    from pdm_ssd_amd.roi_heads import RoIHeadTemplate
    w = fix['loss_weights']
    cfg = {'TARGET_CONFIG': dict(SAMPLER, CLS_SCORE_TYPE=score_type),
           'LOSS_CONFIG': {'CLS_LOSS': 'BinaryCrossEntropy', 'REG_LOSS': 'smooth-l1', 'CORNER_LOSS_REGULARIZATION': True,
                           'LOSS_WEIGHTS': {'rcnn_cls_weight': float(w[0]), 'rcnn_reg_weight': float(w[1]), 'rcnn_corner_weight': float(w[2]),
                                            'code_weights': [float(v) for v in fix['code_weights']]}}}
    return RoIHeadTemplate(num_class=1, model_cfg=cfg_from_dict(cfg), **kwargs)


def loss_inputs(fix, tag, dev, rows=slice(None)):
    keys = ('rois', 'gt_of_rois', 'gt_of_rois_src', 'reg_valid_mask', 'rcnn_cls_labels')
    ret = {k: torch.from_numpy(fix[f'{tag}.{k}'][rows].copy()).to(dev) for k in keys}
    B, S = fix['cls.rois'].shape[:2]
    ret['rcnn_cls'] = torch.from_numpy(fix['rcnn_cls'].reshape(B, S, 1)[rows].reshape(-1, 1).copy()).to(dev).requires_grad_(True)
    ret['rcnn_reg'] = torch.from_numpy(fix['rcnn_reg'].reshape(B, S, 7)[rows].reshape(-1, 7).copy()).to(dev).requires_grad_(True)
    return ret


def close(got, want, rel, what):
    got, want = (float(v.detach()) if isinstance(v, torch.Tensor) else float(v) for v in (got, want))
    print(what, 'got', got, 'want', want)
    assert abs(got - want) <= rel * max(abs(want), 1e-30) + (1e-12 if want == 0 else 0), (what, got, want)


def grad_close(got, want, what):
    got, want = got.detach().cpu().numpy().reshape(want.shape), np.asarray(want)
    scale = float(np.abs(want).max())
    err = float(np.abs(got - want).max())
    print(what, 'max abs difference', err, 'scale', scale)
    assert err <= 1e-4 * scale + (1e-12 if scale == 0 else 0), (what, err, scale)


def check_losses_against_reference(head, fix, dev):
    """losses to 1e-5 relative, gradients to 1e-4 of their scale (the bounds of
    test_point_head_fused_loss_equals_torch_formulation), for the int64-label case, the float-label case and a case
    without any fg row"""
    ret = loss_inputs(fix, 'cls', dev)
    head.forward_ret_dict = ret
    loss, tb = head.get_loss()
    assert set(tb) == {'rcnn_loss_cls', 'rcnn_loss_reg', 'rcnn_loss_corner', 'rcnn_loss'}
    assert all(isinstance(v, torch.Tensor) and v.dim() == 0 and not v.requires_grad for v in tb.values())
    close(tb['rcnn_loss_cls'], fix['loss.cls'], 1e-5, 'loss_cls')
    close(tb['rcnn_loss_reg'], fix['loss.reg'], 1e-5, 'loss_reg')
    close(tb['rcnn_loss_corner'], fix['loss.corner'], 1e-5, 'loss_corner')
    close(loss, float(fix['loss.cls']) + float(fix['loss.reg']) + float(fix['loss.corner']), 1e-5, 'rcnn_loss')
    close(tb['rcnn_loss'], loss, 0, 'tb rcnn_loss')
    g_cls, g_reg = torch.autograd.grad(loss, [ret['rcnn_cls'], ret['rcnn_reg']])
    grad_close(g_cls, fix['loss.g_cls'], 'd loss / d rcnn_cls')
    grad_close(g_reg, fix['loss.g_reg_total'], 'd loss / d rcnn_reg')
    # the smooth-L1 part alone: the gradient of the tb value's own tensor
    ret = loss_inputs(fix, 'cls', dev)
    loss_reg_total, tb = head.get_box_reg_layer_loss(ret)
    close(loss_reg_total, float(fix['loss.reg']) + float(fix['loss.corner']), 1e-5, 'loss_reg + loss_corner')
    # float labels ('roi_iou')
    ret = loss_inputs(fix, 'roi_iou', dev)
    assert ret['rcnn_cls_labels'].dtype == torch.float32
    head.forward_ret_dict = ret
    loss, tb = head.get_loss()
    close(tb['rcnn_loss_cls'], fix['loss_iou.cls'], 1e-5, 'roi_iou loss_cls')
    close(tb['rcnn_loss_reg'], fix['loss_iou.reg'], 1e-5, 'roi_iou loss_reg')
    close(tb['rcnn_loss_corner'], fix['loss_iou.corner'], 1e-5, 'roi_iou loss_corner')
    g_cls, g_reg = torch.autograd.grad(loss, [ret['rcnn_cls'], ret['rcnn_reg']])
    grad_close(g_cls, fix['loss_iou.g_cls'], 'roi_iou d loss / d rcnn_cls')
    grad_close(g_reg, fix['loss_iou.g_reg_total'], 'roi_iou d loss / d rcnn_reg')
    # no fg row at all (sample 1): reg and corner are 0 (the key is present), their gradients 0
    ret = loss_inputs(fix, 'cls', dev, rows=slice(1, 2))
    assert int((ret['reg_valid_mask'] > 0).sum()) == 0
    head.forward_ret_dict = ret
    loss, tb = head.get_loss()
    close(tb['rcnn_loss_cls'], fix['loss_nofg.cls'], 1e-5, 'no-fg loss_cls')
    assert float(tb['rcnn_loss_reg']) == 0 and float(tb['rcnn_loss_corner']) == 0
    g_cls, g_reg = torch.autograd.grad(loss, [ret['rcnn_cls'], ret['rcnn_reg']], allow_unused=True)
    grad_close(g_cls, fix['loss_nofg.g_cls'], 'no-fg d loss / d rcnn_cls')
    assert g_reg is None or not g_reg.any()

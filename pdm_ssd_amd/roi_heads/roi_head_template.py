"""Base class of the RoI heads: /root/reference/pcdet/models/roi_heads/roi_head_template.py, restated — make_fc_layers
(:29-43), proposal_layer (:45-102), assign_targets (:104-134), the rcnn losses (:136-231) and generate_predicted_boxes
(:233-261) with the reference's names, arguments, config keys, batch_dict keys and state_dict keys.

The training half exists when TARGET_CONFIG holds the sampler's settings (ROI_PER_IMAGE, ...) and the head's config a
LOSS_CONFIG; a head built without them (POINT_RCNN_CFG) runs in eval mode only.  Targets come from ONE device operator
(pdm_proposal_targets), the losses and their gradients from another (pdm_rcnn_loss, `use_fused_loss`, default on); a
plain torch formulation of the losses is the checker of the fused operator and the path for what it does not cover
(encode_angle_by_sincos, CLS_LOSS 'CrossEntropy', predictions off the GPU).  No `.item()` anywhere: tb_dict holds
detached 0-dim tensors.
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from ..iou3d_nms.iou3d_nms_utils import class_agnostic_nms
from ..utils import box_coder_utils, loss_utils
from ..utils.common_utils import rotate_points_along_z
from .target_assigner.proposal_target_layer import ProposalTargetLayer


def _get(cfg, key, default=None):
    return cfg.get(key, default) if isinstance(cfg, dict) else getattr(cfg, key, default)


class RoIHeadTemplate(nn.Module):
    def __init__(self, num_class, model_cfg, **kwargs):
        super().__init__()
        self.model_cfg = model_cfg
        self.num_class = num_class
        target_cfg = _get(model_cfg, 'TARGET_CONFIG')
        coder = getattr(box_coder_utils, _get(target_cfg, 'BOX_CODER'))
        self.box_coder = coder(**(_get(target_cfg, 'BOX_CODER_CONFIG', None) or {}))
        self.forward_ret_dict = None
        # the training half: the proposal-target sampler and the loss modules, when the configuration holds their settings
        self.use_fused_loss = True
        self.proposal_target_layer = None
        if _get(target_cfg, 'ROI_PER_IMAGE') is not None:
            self.proposal_target_layer = ProposalTargetLayer(roi_sampler_cfg=target_cfg, seed=kwargs.get('seed', 0),
                                                             check=kwargs.get('check', False))
            self.build_losses(_get(model_cfg, 'LOSS_CONFIG'))

    @property
    def has_training_half(self):
        return self.proposal_target_layer is not None

    def _require_training_half(self, who):
        if not self.has_training_half:
            raise NotImplementedError(f"{who} training: ProposalTargetLayer and the rcnn losses are not built for this head — its "
                                      "TARGET_CONFIG holds no ROI_PER_IMAGE (the proposal-target sampler's settings) and no "
                                      "LOSS_CONFIG is read; build it from POINT_RCNN_TRAIN_CFG or a dict like it")

    def build_losses(self, losses_cfg):
        self.add_module('reg_loss_func', loss_utils.WeightedSmoothL1Loss(
            code_weights=_get(_get(losses_cfg, 'LOSS_WEIGHTS'), 'code_weights')))

    def make_fc_layers(self, input_channels, output_channels, fc_list):
        """A per-RoI MLP over (rois, channels, 1): [Conv1d(k=1, no bias), BatchNorm1d, ReLU] per width of fc_list, then a
        biased Conv1d to output_channels.  With DP_RATIO >= 0 a Dropout follows the FIRST block; it holds no parameter but
        shifts the indices of the children behind it, and with them the reference's state_dict keys."""
        drop = _get(self.model_cfg, 'DP_RATIO')
        layers, width = [], input_channels
        for depth, hidden in enumerate(fc_list):
            layers += [nn.Conv1d(width, hidden, kernel_size=1, bias=False), nn.BatchNorm1d(hidden), nn.ReLU()]
            if depth == 0 and drop >= 0:
                layers.append(nn.Dropout(drop))
            width = hidden
        layers.append(nn.Conv1d(width, output_channels, kernel_size=1, bias=True))
        return nn.Sequential(*layers)

    @torch.no_grad()
    def proposal_layer(self, batch_dict, nms_config):
        """First-stage predictions -> at most NMS_POST_MAXSIZE proposals per sample.

        Reads batch_cls_preds (B, n, num_class | 1) and batch_box_preds (B, n, 7 + C), or both stacked over the samples,
        (N1 + N2 + ..., ..), with batch_index (N1 + N2 + ...).  Per sample: best class per box, class_agnostic_nms on the
        raw scores (no score threshold), survivors in NMS order.  Writes rois (B, NMS_POST_MAXSIZE, 7 + C), roi_scores
        (B, ..) and roi_labels (B, ..) int64 = best class + 1, with zero rows (label 1, as the reference) behind each
        sample's survivors, has_class_labels = more than one class column, and removes batch_index.  A batch_dict that
        already holds rois is returned untouched.  MULTI_CLASSES_NMS is not implemented, as in the reference."""
        if batch_dict.get('rois', None) is not None:
            return batch_dict
        if _get(nms_config, 'MULTI_CLASSES_NMS'):
            raise NotImplementedError('proposal_layer: MULTI_CLASSES_NMS')
        all_boxes, all_logits = batch_dict['batch_box_preds'], batch_dict['batch_cls_preds']
        sample_of_row = batch_dict.get('batch_index', None)
        stacked = sample_of_row is not None
        assert all_logits.dim() == (2 if stacked else 3)
        num_samples, room = batch_dict['batch_size'], int(_get(nms_config, 'NMS_POST_MAXSIZE'))
        rois = all_boxes.new_zeros((num_samples, room, all_boxes.shape[-1]))
        roi_scores = all_boxes.new_zeros((num_samples, room))
        roi_classes = torch.zeros((num_samples, room), dtype=torch.long, device=all_boxes.device)
        for b in range(num_samples):
            rows = (sample_of_row == b) if stacked else b
            boxes, logits = all_boxes[rows], all_logits[rows]
            best, best_class = logits.max(dim=1)
            kept, _ = class_agnostic_nms(box_scores=best, box_preds=boxes, nms_config=nms_config)
            k = kept.numel()
            rois[b, :k] = boxes[kept]
            roi_scores[b, :k] = best[kept]
            roi_classes[b, :k] = best_class[kept]
        batch_dict.update(rois=rois, roi_scores=roi_scores, roi_labels=roi_classes + 1,
                          has_class_labels=bool(all_logits.shape[-1] > 1))
        batch_dict.pop('batch_index', None)
        return batch_dict

    # ------------------------------------------------------------------ targets

    def assign_targets(self, batch_dict):
        """rois, roi_scores, roi_labels, gt_boxes -> targets_dict of ProposalTargetLayer plus gt_of_rois_src (the assigned
        ground truth as it was) and gt_of_rois in the canonical form of ref :113-132: relative to the RoI's centre, turned
        by minus the RoI's heading (mod 2 pi), the heading relative to the RoI's and folded into [-pi / 2, pi / 2] (a box
        that faces the other way is the same solid).  One operator forms all of it (csrc/roi_targets.hip)."""
        self._require_training_half(type(self).__name__)
        with torch.no_grad():
            return self.proposal_target_layer(batch_dict, with_canonical=True)

    # ------------------------------------------------------------------ losses

    def _loss_cfg(self):
        cfg = _get(self.model_cfg, 'LOSS_CONFIG')
        return cfg, _get(cfg, 'LOSS_WEIGHTS')

    def _fused_loss_applies(self, ret):
        cfg, _ = self._loss_cfg()
        cls, reg = ret['rcnn_cls'], ret['rcnn_reg']
        return (self.use_fused_loss and cls.is_cuda and reg.is_cuda
                and _get(cfg, 'CLS_LOSS') == 'BinaryCrossEntropy' and _get(cfg, 'REG_LOSS') == 'smooth-l1'
                and not self.box_coder.encode_angle_by_sincos and self.box_coder.code_size == 7 and reg.shape[-1] == 7
                and cls.numel() == reg.shape[0] and ret['rois'].shape[-1] == 7 and ret['gt_of_rois'].shape[-1] == 8
                and ret['rcnn_cls_labels'].dtype in (torch.int64, torch.float32))

    def _fused_losses(self, ret):
        """(loss_cls, loss_reg, loss_corner) from pdm_rcnn_loss, once per forward_ret_dict"""
        if 'fused_losses' not in ret:
            from .. import roi_targets
            cfg, w = self._loss_cfg()
            cw = self.reg_loss_func.code_weights
            cw = [1.0] * 7 if cw is None else [float(v) for v in cw]
            ret['fused_losses'] = roi_targets.rcnn_loss(
                ret['rcnn_cls'].float(), ret['rcnn_reg'].float(), ret['rois'].reshape(-1, 7), ret['gt_of_rois'].reshape(-1, 8),
                ret['gt_of_rois_src'].reshape(-1, 8), ret['reg_valid_mask'].reshape(-1), ret['rcnn_cls_labels'].reshape(-1), cw,
                self.reg_loss_func.beta, w['rcnn_cls_weight'], w['rcnn_reg_weight'], w['rcnn_corner_weight'],
                bool(_get(cfg, 'CORNER_LOSS_REGULARIZATION')))
        return ret['fused_losses']

    def get_box_reg_layer_loss(self, forward_ret_dict):
        """-> (rcnn_loss_reg + rcnn_loss_corner, {'rcnn_loss_reg', 'rcnn_loss_corner'}): smooth-L1 between rcnn_reg and the
        canonical ground truth coded against the RoI with centre and heading zeroed, over the rows of reg_valid_mask,
        divided by their number (at least 1); with CORNER_LOSS_REGULARIZATION the corner loss of the decoded boxes against
        gt_of_rois_src, averaged over the same rows.  'rcnn_loss_corner' is ALWAYS present and is 0 without such a row or
        without the regularisation (the reference leaves the key out then); the values are detached 0-dim tensors."""
        cfg, w = self._loss_cfg()
        if self._fused_loss_applies(forward_ret_dict):
            _, loss_reg, loss_corner, _ = self._fused_losses(forward_ret_dict)
            return loss_reg + loss_corner, {'rcnn_loss_reg': loss_reg.detach(), 'rcnn_loss_corner': loss_corner.detach()}
        if _get(cfg, 'REG_LOSS') != 'smooth-l1':
            raise NotImplementedError(_get(cfg, 'REG_LOSS'))
        width = self.box_coder.code_size
        box_width = forward_ret_dict['rois'].shape[-1]
        fg = forward_ret_dict['reg_valid_mask'].view(-1) > 0
        fg_rows = fg.sum()
        rois = forward_ret_dict['rois'].detach().reshape(-1, box_width)
        canonical = forward_ret_dict['gt_of_rois'][..., 0:box_width].reshape(-1, box_width).clone()
        source = forward_ret_dict['gt_of_rois_src'][..., 0:box_width].reshape(-1, box_width)
        rcnn_reg = forward_ret_dict['rcnn_reg'].float().view(rois.shape[0], -1)
        anchors = rois.clone()
        anchors[:, 0:3] = 0
        anchors[:, 6] = 0
        targets = self.box_coder.encode_torch(canonical, anchors)
        per_code = self.reg_loss_func(rcnn_reg.unsqueeze(0), targets.unsqueeze(0)).view(rois.shape[0], -1)
        # (rows outside the mask are switched off by selection: the reference multiplies them by 0)
        loss_reg = torch.where(fg[:, None], per_code, torch.zeros_like(per_code)).sum() / fg_rows.clamp(min=1).float()
        loss_reg = loss_reg * w['rcnn_reg_weight']
        loss_corner = loss_reg.new_zeros(())
        if _get(cfg, 'CORNER_LOSS_REGULARIZATION'):
            # every row is decoded and the mean is taken over the masked rows: no boolean-mask indexing, whose result size
            # the host would have to read back
            at_origin = rois.clone()
            at_origin[:, 0:3] = 0
            # (rows outside the mask decode zeros: an overflowing exp there would turn the masked-out gradient into NaN)
            codes = torch.where(fg[:, None], rcnn_reg, torch.zeros_like(rcnn_reg))
            local = self.box_coder.decode_torch(codes.view(1, -1, width), at_origin.view(1, -1, box_width)).view(-1, 1, box_width)
            boxes = rotate_points_along_z(local, rois[:, 6]).view(-1, box_width)
            boxes = torch.cat([boxes[:, 0:3] + rois[:, 0:3], boxes[:, 3:]], dim=1)
            per_row = loss_utils.get_corner_loss_lidar(boxes[:, 0:7], source[:, 0:7])
            loss_corner = torch.where(fg, per_row, torch.zeros_like(per_row)).sum() / fg_rows.clamp(min=1).float()
            loss_corner = loss_corner * w['rcnn_corner_weight']
        return loss_reg + loss_corner, {'rcnn_loss_reg': loss_reg.detach(), 'rcnn_loss_corner': loss_corner.detach()}

    def get_box_cls_layer_loss(self, forward_ret_dict):
        """-> (rcnn_loss_cls, {'rcnn_loss_cls'}).  BinaryCrossEntropy: of sigmoid(rcnn_cls) against the label (int64 with -1 =
        ignored, or the float 'roi_iou' label) over the rows with label >= 0, divided by their number (at least 1), in the
        logit form — the reference's F.binary_cross_entropy clamps its logs at -100, which differs for |logit| >= 88 only.
        CrossEntropy: F.cross_entropy with ignore_index -1, the same normalisation."""
        cfg, w = self._loss_cfg()
        if self._fused_loss_applies(forward_ret_dict):
            loss_cls = self._fused_losses(forward_ret_dict)[0]
            return loss_cls, {'rcnn_loss_cls': loss_cls.detach()}
        rcnn_cls = forward_ret_dict['rcnn_cls'].float()
        labels = forward_ret_dict['rcnn_cls_labels'].view(-1)
        valid = labels >= 0
        if _get(cfg, 'CLS_LOSS') == 'BinaryCrossEntropy':
            per_row = F.binary_cross_entropy_with_logits(rcnn_cls.view(-1), labels.float(), reduction='none')
        elif _get(cfg, 'CLS_LOSS') == 'CrossEntropy':
            per_row = F.cross_entropy(rcnn_cls, labels, reduction='none', ignore_index=-1)
        else:
            raise NotImplementedError(_get(cfg, 'CLS_LOSS'))
        loss_cls = torch.where(valid, per_row, torch.zeros_like(per_row)).sum() / valid.sum().float().clamp(min=1.0)
        loss_cls = loss_cls * w['rcnn_cls_weight']
        return loss_cls, {'rcnn_loss_cls': loss_cls.detach()}

    def get_loss(self, tb_dict=None):
        """-> (rcnn_loss, tb_dict) with rcnn_loss_cls, rcnn_loss_reg, rcnn_loss_corner and rcnn_loss as detached 0-dim tensors
        (the reference reads each back with .item(): four synchronisations per step)."""
        self._require_training_half(type(self).__name__)
        tb_dict = {} if tb_dict is None else tb_dict
        loss_cls, cls_tb = self.get_box_cls_layer_loss(self.forward_ret_dict)
        loss_reg, reg_tb = self.get_box_reg_layer_loss(self.forward_ret_dict)
        rcnn_loss = loss_cls + loss_reg
        tb_dict.update(cls_tb)
        tb_dict.update(reg_tb)
        tb_dict['rcnn_loss'] = rcnn_loss.detach()
        return rcnn_loss, tb_dict

    def generate_predicted_boxes(self, batch_size, rois, cls_preds, box_preds):
        """rois (B, N, 7 [+ C]), cls_preds (B N, num_class | 1), box_preds (B N, code_size) -> batch_cls_preds
        (B, N, num_class | 1), batch_box_preds (B, N, code_size).  The codes are relative to each RoI's own frame: decode
        them against the RoI moved to the origin, turn the result by the RoI's heading about z, move it to the RoI's
        centre."""
        width = self.box_coder.code_size
        at_origin = rois.detach().clone()
        at_origin[..., 0:3] = 0
        local = self.box_coder.decode_torch(box_preds.view(batch_size, -1, width), at_origin).view(-1, 1, width)
        boxes = rotate_points_along_z(local, rois[..., 6].reshape(-1)).view(-1, width)
        boxes[:, 0:3] += rois[..., 0:3].reshape(-1, 3)
        return cls_preds.view(batch_size, -1, cls_preds.shape[-1]), boxes.view(batch_size, -1, width)

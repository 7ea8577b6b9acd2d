"""AnchorHeadTemplate: anchors, target assignment, the three loss terms and the box decode of the anchor heads — the
reference's pcdet/models/dense_heads/anchor_head_template.py on this repository's operators.

Constructor signature, config keys and behaviour are the reference's.  What differs is where the work runs: on the GPU the
targets of the whole batch are one launch chain (pdm_anchor_targets), the losses and their gradients one operator that reads
the conv outputs as they are (pdm_anchor_head_loss: no permuted copies, no one-hot tensor, no repeated anchors) and the decode
one launch (pdm_anchor_decode); a training step has no host read.  On CPU tensors (and with use_fused = False) the torch
formulations get_cls_layer_loss / get_box_reg_layer_loss / the decode below run instead.  tb_dict holds detached 0-dim tensors.

The anchors are plain attributes as in the reference (no buffers: they are not in the state_dict); they follow the module
through .to() / .cuda().

Refused with NotImplementedError: TARGET_ASSIGNER_CONFIG.NAME ATSS, USE_MULTIHEAD, MATCH_HEIGHT, POS_FRACTION >= 0.
"""
import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from ..utils import box_coder_utils, common_utils, loss_utils
from .point_head_template import _get
from .target_assigner import AnchorGenerator, AxisAlignedTargetAssigner


class AnchorHeadTemplate(nn.Module):
    def __init__(self, model_cfg, num_class, class_names, grid_size, point_cloud_range, predict_boxes_when_training):
        super().__init__()
        self.model_cfg = model_cfg
        self.num_class = num_class
        self.class_names = class_names
        self.predict_boxes_when_training = predict_boxes_when_training
        self.use_multihead = _get(model_cfg, 'USE_MULTIHEAD', False)
        if self.use_multihead:
            raise NotImplementedError('AnchorHeadTemplate: USE_MULTIHEAD is not supported by this build')

        anchor_target_cfg = _get(model_cfg, 'TARGET_ASSIGNER_CONFIG')
        self.box_coder = getattr(box_coder_utils, _get(anchor_target_cfg, 'BOX_CODER'))(
            num_dir_bins=_get(anchor_target_cfg, 'NUM_DIR_BINS', 6), **dict(_get(anchor_target_cfg, 'BOX_CODER_CONFIG', {})))
        assert self.box_coder.code_size == 7, 'the anchor head codes boxes in 7 columns (ResidualCoder without encode_angle_by_sincos)'

        anchor_generator_cfg = _get(model_cfg, 'ANCHOR_GENERATOR_CONFIG')
        anchors, self.num_anchors_per_location = self.generate_anchors(
            anchor_generator_cfg, grid_size=grid_size, point_cloud_range=point_cloud_range, anchor_ndim=self.box_coder.code_size)
        assert all(a.shape[0] == 1 for a in anchors), 'one anchor_bottom_heights entry per anchor set'
        assert len({tuple(a.shape[:3]) for a in anchors}) == 1, 'every anchor set on the same feature map'
        self.anchors = anchors
        self._flat_anchors = torch.cat(anchors, dim=-3).view(-1, 7)             # (H W A_loc, 7): y, x, set, size, rotation
        self._anchor_rot = self._flat_anchors[:sum(self.num_anchors_per_location), 6].tolist()
        self.target_assigner = self.get_target_assigner(anchor_target_cfg)
        self.forward_ret_dict = {}
        self.use_fused = True                       # False: the torch formulations on any device
        self.build_losses(_get(model_cfg, 'LOSS_CONFIG'))

    def _apply(self, fn, *args, **kwargs):
        """the anchors follow the module's device and never its dtype: only the device `fn` leads to is taken from it, so
        .half() / .bfloat16() / .to(dtype) leave every anchor value as it is"""
        super()._apply(fn, *args, **kwargs)
        device = fn(self._flat_anchors.new_empty(0)).device
        self.anchors = [a.to(device) for a in self.anchors]
        self._flat_anchors = self._flat_anchors.to(device)
        return self

    @staticmethod
    def generate_anchors(anchor_generator_cfg, grid_size, point_cloud_range, anchor_ndim=7):
        """-> (per anchor set a (1, ny, nx, #sizes, #rotations, anchor_ndim) table, per set the anchors of one location); a
        set's map is the grid divided by its feature_map_stride; columns beyond the seventh are zeros"""
        map_sizes = [np.asarray(grid_size)[:2] // _get(config, 'feature_map_stride') for config in anchor_generator_cfg]
        tables, per_location = AnchorGenerator(point_cloud_range, anchor_generator_cfg).generate_anchors(map_sizes)
        if anchor_ndim > 7:
            tables = [F.pad(t, (0, anchor_ndim - 7)) for t in tables]
        return tables, per_location

    def get_target_assigner(self, anchor_target_cfg):
        name = _get(anchor_target_cfg, 'NAME')
        if name == 'ATSS':
            raise NotImplementedError('AnchorHeadTemplate: TARGET_ASSIGNER_CONFIG.NAME ATSS is not supported by this build')
        if name != 'AxisAlignedTargetAssigner':
            raise NotImplementedError(f'AnchorHeadTemplate: TARGET_ASSIGNER_CONFIG.NAME {name}')
        return AxisAlignedTargetAssigner(model_cfg=self.model_cfg, class_names=self.class_names, box_coder=self.box_coder,
                                         match_height=_get(anchor_target_cfg, 'MATCH_HEIGHT', False))

    def build_losses(self, losses_cfg):
        self.add_module('cls_loss_func', loss_utils.SigmoidFocalClassificationLoss(alpha=0.25, gamma=2.0))
        reg_loss_name = _get(losses_cfg, 'REG_LOSS_TYPE', None) or 'WeightedSmoothL1Loss'
        assert reg_loss_name == 'WeightedSmoothL1Loss', f'REG_LOSS_TYPE {reg_loss_name}: only WeightedSmoothL1Loss'
        self.add_module('reg_loss_func', loss_utils.WeightedSmoothL1Loss(code_weights=_get(losses_cfg, 'LOSS_WEIGHTS')['code_weights']))
        self.add_module('dir_loss_func', loss_utils.WeightedCrossEntropyLoss())

    def assign_targets(self, gt_boxes):
        """gt_boxes (B, M, 8) -> box_cls_labels (B, A) int32, box_reg_targets (B, A, 7), reg_weights (B, A), num_pos (B)"""
        self.target_assigner.use_fused = self.use_fused
        return self.target_assigner.assign_targets(self.anchors, gt_boxes, flat_anchors=self._flat_anchors)

    # ---- the torch formulations (CPU tensors) -------------------------------------------------------------------------------
    def _nhwc(self, key):
        """a conv output (B, C, H, W) as the reference's forward stores it: (B, H, W, C) contiguous, fp32"""
        t = self.forward_ret_dict.get(key, None)
        return None if t is None else t.float().permute(0, 2, 3, 1).contiguous()

    def get_cls_layer_loss(self):
        """sigmoid focal loss over the anchors with label >= 0, each sample divided by max(#positives, 1), then by B"""
        logits = self._nhwc('cls_preds')
        labels = self.forward_ret_dict['box_cls_labels']
        batch_size = logits.shape[0]
        positive = labels > 0
        weights = (labels >= 0).float() / positive.sum(dim=1, keepdim=True).clamp(min=1).float()
        column = positive.long() if self.num_class == 1 else labels.clamp(min=0).long()    # one class: every positive is class 1
        target = F.one_hot(column, self.num_class + 1)[..., 1:].to(logits.dtype)           # column 0 = background: dropped
        per_anchor = self.cls_loss_func(logits.view(batch_size, -1, self.num_class), target, weights=weights)
        cls_loss = per_anchor.sum() / batch_size * _get(_get(self.model_cfg, 'LOSS_CONFIG'), 'LOSS_WEIGHTS')['cls_weight']
        return cls_loss, {'rpn_loss_cls': cls_loss.detach()}

    def get_box_reg_layer_loss(self):
        """smooth-L1 over the positives with the heading compared as sin(p - t) = sin p cos t - cos p sin t (the two
        products stand in column 6 of prediction and target), and with a direction map the cross-entropy of the bin of
        target heading + anchor rotation; each sample divided by max(#positives, 1), then by B"""
        codes = self._nhwc('box_preds')
        dir_logits = self._nhwc('dir_cls_preds')
        targets = self.forward_ret_dict['box_reg_targets']
        batch_size = codes.shape[0]
        weights_cfg = _get(_get(self.model_cfg, 'LOSS_CONFIG'), 'LOSS_WEIGHTS')
        positive = self.forward_ret_dict['box_cls_labels'] > 0
        weights = positive.float() / positive.sum(dim=1, keepdim=True).float().clamp(min=1.0)
        codes = codes.view(batch_size, -1, 7)
        p, t = codes[..., 6:7], targets[..., 6:7]
        pred = torch.cat([codes[..., :6], p.sin() * t.cos()], dim=-1)
        want = torch.cat([targets[..., :6], p.cos() * t.sin()], dim=-1)
        loc_loss = self.reg_loss_func(pred, want, weights=weights).sum() / batch_size * weights_cfg['loc_weight']
        box_loss, tb_dict = loc_loss, {'rpn_loss_loc': loc_loss.detach()}
        if dir_logits is not None:
            num_bins = _get(self.model_cfg, 'NUM_DIR_BINS')
            heading = targets[..., 6] + self._flat_anchors[:, 6].to(targets.device)
            folded = common_utils.limit_period(heading - _get(self.model_cfg, 'DIR_OFFSET'), 0, 2 * np.pi)
            bins = (folded / (2 * np.pi / num_bins)).floor().long().clamp(min=0, max=num_bins - 1)
            per_anchor = self.dir_loss_func(dir_logits.view(batch_size, -1, num_bins), bins, weights=weights)
            dir_loss = per_anchor.sum() / batch_size * weights_cfg['dir_weight']
            box_loss = box_loss + dir_loss
            tb_dict['rpn_loss_dir'] = dir_loss.detach()
        return box_loss, tb_dict

    # ---- the loss -----------------------------------------------------------------------------------------------------------
    def get_loss(self):
        """-> (rpn_loss, tb_dict) with rpn_loss_cls, rpn_loss_loc, rpn_loss_dir (with the direction classifier) and rpn_loss as
        detached 0-dim tensors: no .item(), no host read."""
        fr = self.forward_ret_dict
        cls_preds, box_preds, dir_preds = fr['cls_preds'], fr['box_preds'], fr.get('dir_cls_preds', None)
        maps = [t for t in (cls_preds, box_preds, dir_preds) if t is not None]
        if self.use_fused and cls_preds.is_cuda and all(t.dtype in (torch.float32, torch.bfloat16) for t in maps):
            from .. import anchor_head_ops
            weights = _get(_get(self.model_cfg, 'LOSS_CONFIG'), 'LOSS_WEIGHTS')
            num_pos = fr['num_pos'] if 'num_pos' in fr else (fr['box_cls_labels'] > 0).sum(dim=1).int()
            cls_loss, loc_loss, dir_loss = anchor_head_ops.anchor_head_loss(
                cls_preds, box_preds, dir_preds, fr['box_cls_labels'].int(), fr['box_reg_targets'], num_pos, self._anchor_rot,
                weights['code_weights'], self.num_class, num_dir_bins=_get(self.model_cfg, 'NUM_DIR_BINS', 2),
                cls_weight=weights['cls_weight'], loc_weight=weights['loc_weight'], dir_weight=weights.get('dir_weight', 0.0),
                dir_offset=_get(self.model_cfg, 'DIR_OFFSET', 0.0), beta=self.reg_loss_func.beta, alpha=self.cls_loss_func.alpha,
                gamma=self.cls_loss_func.gamma)
            tb_dict = {'rpn_loss_cls': cls_loss.detach(), 'rpn_loss_loc': loc_loss.detach()}
            rpn_loss = cls_loss + loc_loss
            if dir_preds is not None:
                tb_dict['rpn_loss_dir'] = dir_loss.detach()
                rpn_loss = rpn_loss + dir_loss
        else:
            cls_loss, tb_dict = self.get_cls_layer_loss()
            box_loss, tb_dict_box = self.get_box_reg_layer_loss()
            tb_dict.update(tb_dict_box)
            rpn_loss = cls_loss + box_loss
        tb_dict['rpn_loss'] = rpn_loss.detach()
        return rpn_loss, tb_dict

    # ---- boxes --------------------------------------------------------------------------------------------------------------
    def generate_predicted_boxes(self, batch_size, cls_preds, box_preds, dir_cls_preds=None):
        """the conv outputs (B, C, H, W) -> batch_cls_preds (B, A, num_class) fp32 (a permuted view's reshape),
        batch_box_preds (B, A, 7): ResidualCoder.decode_torch against the anchors, then with a direction map the arg-max bin
        (the lower bin on equal logits) and the heading folded into the bin's period."""
        batch_cls_preds = cls_preds.permute(0, 2, 3, 1).reshape(batch_size, -1, self.num_class).float()
        dir_offset, dir_limit_offset = _get(self.model_cfg, 'DIR_OFFSET', 0.0), _get(self.model_cfg, 'DIR_LIMIT_OFFSET', 0.0)
        num_bins = _get(self.model_cfg, 'NUM_DIR_BINS', 2)
        if self.use_fused and box_preds.is_cuda and box_preds.dtype in (torch.float32, torch.bfloat16):
            from .. import anchor_head_ops
            return batch_cls_preds, anchor_head_ops.anchor_decode(box_preds, dir_cls_preds, self._flat_anchors, num_bins, dir_offset, dir_limit_offset)
        anchors = self._flat_anchors.to(box_preds.device)
        codes = box_preds.float().permute(0, 2, 3, 1).reshape(batch_size, anchors.shape[0], -1)
        boxes = self.box_coder.decode_torch(codes, anchors.expand(batch_size, -1, -1))
        if dir_cls_preds is not None:
            bins = dir_cls_preds.float().permute(0, 2, 3, 1).reshape(batch_size, anchors.shape[0], -1).argmax(dim=-1)
            period = 2 * np.pi / num_bins                            # the heading folded into bin 0's period, then moved to its bin
            folded = common_utils.limit_period(boxes[..., 6] - dir_offset, dir_limit_offset, period)
            boxes = torch.cat([boxes[..., :6], (folded + dir_offset + period * bins.to(boxes.dtype)).unsqueeze(-1)], dim=-1)
        return batch_cls_preds, boxes

    def forward(self, **kwargs):
        raise NotImplementedError

"""SECOND-IoU's second stage: behaviour, constructor signature, config keys and state_dict keys (shared_fc_layer, iou_layers) of the
reference's pcdet/models/roi_heads/second_head.py (SECONDHead), restated.

Per RoI a G x G crop of the 2-D backbone's map under the RoI's rotated rectangle (ROI_GRID_POOL: GRID_SIZE, IN_CHANNEL,
DOWNSAMPLE_RATIO), flattened channels-first to (C G^2) and put through shared_fc_layer ([Conv1d, BatchNorm1d, ReLU] per width of
SHARED_FC, a Dropout behind every block but the last when DP_RATIO > 0) and iou_layers (make_fc_layers over IOU_FC to ONE output):
the predicted IoU of the RoI with its object, which SECONDNetIoU uses to re-score the first stage's boxes.  The boxes themselves
are not refined: batch_box_preds = rois.

point_cloud_range and voxel_size come from the keywords build_roi_head passes (the reference reads them from
batch_dict['dataset_cfg'] on every forward; a dataset_cfg in the batch is ignored here).

Three formulations of the pooling + first block, in eval mode:
  * use_fused_pool and use_fused_fc: bev_roi_ops.bev_roi_crop_fc, the crop and shared_fc_layer[0:3] (Conv1d, eval BatchNorm1d folded,
    ReLU) in two launches without the (R, C G^2) tensor; for what the operator refuses (C or the first width no multiple of 16,
    widths above its limits, a first block that is not Conv1d / BatchNorm1d / ReLU, CPU tensors) the next one;
  * use_fused_pool only: bev_roi_ops.bev_roi_crop (one launch for the batch) and the torch stack;
  * neither: bev_roi_ops.bev_roi_crop_torch, the crop in torch's operators: the checker, and what CPU tensors take in any case.
`last_path` tells which ran: 'fused_fc', 'crop' or 'torch'.  use_fused_fc's default is what tools/second_iou_rate.py measured
(profiles/second_iou_rate.json; README).

Training: proposals under NMS_CONFIG.TRAIN, the one-operator ProposalTargetLayer (CLS_SCORE_TYPE 'roi_iou'), the sampled rois
cropped by bev_roi_crop without a gradient (the reference detaches the map and the rois here), the torch stack under autograd: the
gradient of rcnn_loss reaches shared_fc_layer and iou_layers and nothing in front of them.  get_loss takes the four IOU_LOSS
kinds; no `.item()`: tb_dict holds detached 0-dim tensors.
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import bev_roi_ops, spconv
from ..utils import loss_utils
from .roi_head_template import RoIHeadTemplate, _get

# whether eval takes the crop + first FC operator where it applies: tools/second_iou_rate.py's verdict, (c) against (b) at bs = 32
# and bs = 4 (profiles/second_iou_rate.json: 1.13 ms against 1.64 ms and 0.22 ms against 0.33 ms on an MI355X)
FUSED_FC_DEFAULT = True


class SECONDHead(RoIHeadTemplate):
    def __init__(self, input_channels, model_cfg, num_class=1, **kwargs):
        super().__init__(num_class=num_class, model_cfg=model_cfg, **kwargs)
        self.pool_cfg = _get(model_cfg, 'ROI_GRID_POOL')
        if kwargs.get('point_cloud_range') is None or kwargs.get('voxel_size') is None:
            raise ValueError('SECONDHead: point_cloud_range and voxel_size keywords (build_roi_head passes them)')
        self.point_cloud_range = [float(v) for v in kwargs['point_cloud_range']]
        self.voxel_size = [float(v) for v in kwargs['voxel_size']]
        self.grid_size = int(_get(self.pool_cfg, 'GRID_SIZE'))
        self.in_channel = int(_get(self.pool_cfg, 'IN_CHANNEL'))
        pre_channel = self.in_channel * self.grid_size * self.grid_size
        widths, drop = list(_get(model_cfg, 'SHARED_FC')), _get(model_cfg, 'DP_RATIO')
        shared = []
        for k, width in enumerate(widths):
            shared += [nn.Conv1d(pre_channel, width, kernel_size=1, bias=False), nn.BatchNorm1d(width), nn.ReLU()]
            pre_channel = width
            if k != len(widths) - 1 and drop > 0:       # (holds no parameter but shifts the children behind it: the reference's keys)
                shared.append(nn.Dropout(drop))
        self.shared_fc_layer = nn.Sequential(*shared)
        self.iou_layers = self.make_fc_layers(input_channels=pre_channel, output_channels=1, fc_list=_get(model_cfg, 'IOU_FC'))
        self.use_fused_pool = True
        self.use_fused_fc = FUSED_FC_DEFAULT
        self.last_path = None
        self._fc_cache = None       # (parameter versions, (packed weight, scale, shift)) of shared_fc_layer[0:2]
        self.init_weights(weight_init='xavier')

    def init_weights(self, weight_init='xavier'):
        init_func = {'kaiming': nn.init.kaiming_normal_, 'xavier': nn.init.xavier_normal_, 'normal': nn.init.normal_}.get(weight_init)
        if init_func is None:
            raise NotImplementedError(weight_init)
        for m in self.modules():
            if isinstance(m, (nn.Conv2d, nn.Conv1d)):
                if weight_init == 'normal':
                    init_func(m.weight, mean=0, std=0.001)
                else:
                    init_func(m.weight)
                if m.bias is not None:
                    nn.init.constant_(m.bias, 0)

    # ------------------------------------------------------------------ pooling

    def _crop_args(self, batch_dict):
        rois = batch_dict['rois'].detach().float()
        feat = batch_dict['spatial_features_2d'].detach().float()
        if feat.shape[1] != self.in_channel:
            raise ValueError(f'SECONDHead: the map has {feat.shape[1]} channels, ROI_GRID_POOL.IN_CHANNEL is {self.in_channel}')
        return rois, feat, self.point_cloud_range, self.voxel_size, _get(self.pool_cfg, 'DOWNSAMPLE_RATIO'), self.grid_size

    def roi_grid_pool(self, batch_dict):
        """batch_size, rois (B, n, 7 + C), spatial_features_2d (B, C, H, W) -> (B n, C, G, G), without a gradient (both inputs are
        detached, as in the reference): one launch of pdm_bev_roi_crop on the device with use_fused_pool, the torch formulation
        otherwise"""
        args = self._crop_args(batch_dict)
        if self.use_fused_pool and args[0].is_cuda:
            return bev_roi_ops.bev_roi_crop(*args)
        return bev_roi_ops.bev_roi_crop_torch(*args)

    def _fused_fc_applies(self, batch_dict):
        if not (self.use_fused_pool and self.use_fused_fc) or self.training or len(self.shared_fc_layer) < 3:
            return False
        conv, bn, act = self.shared_fc_layer[0], self.shared_fc_layer[1], self.shared_fc_layer[2]
        return (batch_dict['rois'].is_cuda and isinstance(conv, nn.Conv1d) and conv.bias is None and isinstance(bn, nn.BatchNorm1d)
                and not bn.training and bn.track_running_stats and isinstance(act, nn.ReLU) and self.in_channel % 16 == 0
                and self.in_channel <= 512 and conv.out_channels % 16 == 0 and conv.out_channels <= 1024
                and conv.weight.dtype == torch.float32)

    def _packed_fc(self):
        """shared_fc_layer[0] repacked and shared_fc_layer[1] folded, once per version of their tensors"""
        conv, bn = self.shared_fc_layer[0], self.shared_fc_layer[1]
        sources = [conv.weight, bn.weight, bn.bias, bn.running_mean, bn.running_var]
        key = tuple((t.data_ptr(), t._version) for t in sources)
        if self._fc_cache is None or self._fc_cache[0] != key:
            with torch.no_grad():
                scale, shift = spconv.fold_norm(bn, None, conv.out_channels, conv.weight)
                self._fc_cache = (key, (bev_roi_ops.pack_crop_fc_weight(conv.weight, self.in_channel, self.grid_size), scale, shift))
        return self._fc_cache[1]

    def _shared_features(self, batch_dict):
        """-> (R, SHARED_FC[-1], 1)"""
        if self._fused_fc_applies(batch_dict):
            wpack, scale, shift = self._packed_fc()
            first = bev_roi_ops.bev_roi_crop_fc(*self._crop_args(batch_dict), wpack, self.shared_fc_layer[0].out_channels, scale, shift,
                                                relu=True)
            self.last_path = 'fused_fc'
            shared = first.unsqueeze(-1)
            for layer in list(self.shared_fc_layer)[3:]:
                shared = layer(shared)
            return shared
        pooled = self.roi_grid_pool(batch_dict)
        self.last_path = 'crop' if (self.use_fused_pool and pooled.is_cuda) else 'torch'
        return self.shared_fc_layer(pooled.view(pooled.shape[0], -1, 1))

    # ------------------------------------------------------------------ forward

    def forward(self, batch_dict):
        """proposals (unless rois are given) -> rcnn_iou (R, 1).  Eval: batch_cls_preds (B, n, 1) = the IoU logits,
        batch_box_preds = rois, cls_preds_normalized = False.  Training: the proposals go through assign_targets first and
        forward_ret_dict holds the targets with rcnn_iou for get_loss."""
        if self.training:
            self._require_training_half(type(self).__name__)
        self.proposal_layer(batch_dict, nms_config=_get(self.model_cfg, 'NMS_CONFIG')['TRAIN' if self.training else 'TEST'])
        if self.training:
            targets_dict = self.assign_targets(batch_dict)
            batch_dict['rois'] = targets_dict['rois']
            batch_dict['roi_labels'] = targets_dict['roi_labels']
        shared = self._shared_features(batch_dict)
        rcnn_iou = self.iou_layers(shared).transpose(1, 2).contiguous().squeeze(dim=1)       # (R, 1)
        if self.training:
            targets_dict['rcnn_iou'] = rcnn_iou
            self.forward_ret_dict = targets_dict
            return batch_dict
        batch_dict.update(batch_cls_preds=rcnn_iou.view(batch_dict['batch_size'], -1, rcnn_iou.shape[-1]),
                          batch_box_preds=batch_dict['rois'], cls_preds_normalized=False)
        return batch_dict

    # ------------------------------------------------------------------ losses

    def get_box_iou_layer_loss(self, forward_ret_dict):
        """-> (rcnn_loss_iou, {'rcnn_loss_iou'}): LOSS_CONFIG.IOU_LOSS of rcnn_iou against rcnn_cls_labels ('roi_iou': the IoU
        mapped onto [0, 1], -1 = ignored) per row — 'BinaryCrossEntropy' on the logit, 'L2', 'smoothL1' with the knee at 1/9,
        'focalbce' (loss_utils.sigmoid_focal_cls_loss) — over the rows with label >= 0, divided by their number (at least 1),
        times LOSS_WEIGHTS.rcnn_iou_weight.  The tb_dict value is a detached 0-dim tensor."""
        cfg = _get(self.model_cfg, 'LOSS_CONFIG')
        logits = forward_ret_dict['rcnn_iou'].float().view(-1)
        labels = forward_ret_dict['rcnn_cls_labels'].view(-1).float()
        kind = _get(cfg, 'IOU_LOSS')
        if kind == 'BinaryCrossEntropy':
            per_row = F.binary_cross_entropy_with_logits(logits, labels, reduction='none')
        elif kind == 'L2':
            per_row = F.mse_loss(logits, labels, reduction='none')
        elif kind == 'smoothL1':
            per_row = loss_utils.WeightedSmoothL1Loss.smooth_l1_loss(logits - labels, 1.0 / 9.0)
        elif kind == 'focalbce':
            per_row = loss_utils.sigmoid_focal_cls_loss(logits, labels)
        else:
            raise NotImplementedError(kind)
        valid = labels >= 0
        # (rows outside the mask are switched off by selection: the reference multiplies them by 0)
        loss = torch.where(valid, per_row, torch.zeros_like(per_row)).sum() / valid.sum().float().clamp(min=1.0)
        loss = loss * _get(cfg, 'LOSS_WEIGHTS')['rcnn_iou_weight']
        return loss, {'rcnn_loss_iou': loss.detach()}

    def get_loss(self, tb_dict=None):
        """-> (rcnn_loss, tb_dict) with rcnn_loss_iou and rcnn_loss as detached 0-dim tensors (the reference reads each back with
        .item())"""
        self._require_training_half(type(self).__name__)
        tb_dict = {} if tb_dict is None else tb_dict
        rcnn_loss, iou_tb = self.get_box_iou_layer_loss(self.forward_ret_dict)
        tb_dict.update(iou_tb)
        tb_dict['rcnn_loss'] = rcnn_loss.detach()
        return rcnn_loss, tb_dict

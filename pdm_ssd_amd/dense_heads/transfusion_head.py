"""TransFusionHead (LiDAR branch): BEV map -> heat-map queries -> one transformer decoder layer -> boxes, the
reference's pcdet/models/dense_heads/transfusion_head.py on this repository's operators.

Constructor signature, config keys, initialisation and state_dict keys (shared_conv.*, heatmap_head.{0.conv,0.bn,1}.*,
class_encoding.*, decoder.*, prediction_head.{center,height,dim,rot,vel,heatmap}.*) are the reference's.  What differs is
where the work runs.  On the GPU with use_fused (the default):
  * the queries come from transfusion_ops.proposals (local-maximum filter and a rank select of the P best cells, where the
    reference sorts all C * H * W scores of every sample),
  * both attentions of the decoder run in attention_ops.mha_forward (utils/transfusion_utils.py),
  * the boxes come from transfusion_ops.decode, padded, and ONE device-to-host read of the counts serves the batch.
On the CPU (and with use_fused = False) the torch formulations next to those operators run instead.

The key positional embedding is the same for every sample in eval mode: it is computed for one sample per call and
broadcast (it is not cached across calls).

Training is opt-in by a key of this build, TARGET_ASSIGNER_CONFIG.ASSIGN_ON_DEVICE.  Without it forward() in training mode
raises NotImplementedError and the constructor builds no assigner.  With it the constructor builds bbox_assigner
(HungarianAssigner3D) and reads the loss weights; forward() in training mode runs predict under autograd (the decoder through
nn.MultiheadAttention with its dropout; query_heatmap_score carries no gradient), then transfusion_ops.assign and
transfusion_ops.loss for the whole batch with no host read (the reference walks the samples, calls scipy's
linear_sum_assignment on the host and ends in four .item() calls), and sets batch_dict['loss'] and batch_dict['tb_dict']
(detached device tensors).  On the CPU assign_torch and loss_torch run instead.

A second key of this build, FUSED_ATTENTION_TRAIN (default False), sends the decoder's two attentions in training mode through
attention_ops.mha_qkv / mha_kv and their HIP backward instead of nn.MultiheadAttention; the attention dropout then draws from
ATTENTION_DROPOUT_SEED (default 0) and the decoder's device step counters (utils/transfusion_utils.py), not from torch's generator.
"""
import copy

import torch
from torch import nn

from .. import transfusion_ops
from ..utils.basic_block_2d import BasicBlock2D
from ..utils.transfusion_utils import PositionEmbeddingLearned, TransformerDecoderLayer
from .point_head_template import _get


class SeparateHead_Transfusion(nn.Module):
    """One Conv1d stack per entry of sep_head_dict ({name: {out_channels, num_conv}}), each an attribute of that name:
    (num_conv - 1) x [conv, BatchNorm1d, ReLU], then a biased conv.  Every layer keeps torch's default initialisation: the
    reference's special cases look for 'hm' in the name and for nn.Conv2d layers, and this head has neither."""

    def __init__(self, input_channels, head_channels, kernel_size, sep_head_dict, init_bias=-2.19, use_bias=False):
        super().__init__()
        self.sep_head_dict = sep_head_dict
        pad = kernel_size // 2
        for name in sep_head_dict:
            out_channels, num_conv = sep_head_dict[name]['out_channels'], sep_head_dict[name]['num_conv']
            layers = [nn.Sequential(nn.Conv1d(input_channels, head_channels, kernel_size, stride=1, padding=pad, bias=use_bias),
                                    nn.BatchNorm1d(head_channels), nn.ReLU()) for _ in range(num_conv - 1)]
            layers.append(nn.Conv1d(head_channels, out_channels, kernel_size, stride=1, padding=pad, bias=True))
            stack = nn.Sequential(*layers)
            if 'hm' in name:
                stack[-1].bias.data.fill_(init_bias)
            setattr(self, name, stack)

    def forward(self, x):
        return {name: getattr(self, name)(x) for name in self.sep_head_dict}


class TransFusionHead(nn.Module):
    def __init__(self, model_cfg, input_channels, num_class, class_names, grid_size, point_cloud_range, voxel_size,
                 predict_boxes_when_training=True):
        super().__init__()
        self.model_cfg = model_cfg
        self.grid_size, self.point_cloud_range, self.voxel_size = grid_size, point_cloud_range, voxel_size
        self.num_classes = num_class
        assigner_cfg = _get(model_cfg, 'TARGET_ASSIGNER_CONFIG')
        self.feature_map_stride = _get(assigner_cfg, 'FEATURE_MAP_STRIDE', None)
        self.dataset_name = _get(assigner_cfg, 'DATASET', 'nuScenes')
        hidden = _get(model_cfg, 'HIDDEN_CHANNEL')
        self.num_proposals = int(_get(model_cfg, 'NUM_PROPOSALS'))
        self.bn_momentum = _get(model_cfg, 'BN_MOMENTUM')
        self.nms_kernel_size = int(_get(model_cfg, 'NMS_KERNEL_SIZE'))
        bias = _get(model_cfg, 'USE_BIAS_BEFORE_NORM', False)
        loss_cls = _get(_get(model_cfg, 'LOSS_CONFIG'), 'LOSS_CLS')
        self.use_sigmoid_cls = _get(loss_cls, 'use_sigmoid', False)
        if not self.use_sigmoid_cls:
            self.num_classes += 1
        self.code_size = 10

        self.shared_conv = nn.Conv2d(in_channels=input_channels, out_channels=hidden, kernel_size=3, padding=1)
        self.heatmap_head = nn.Sequential(BasicBlock2D(hidden, hidden, kernel_size=3, padding=1, bias=bias),
                                          nn.Conv2d(in_channels=hidden, out_channels=num_class, kernel_size=3, padding=1))
        self.class_encoding = nn.Conv1d(num_class, hidden, 1)
        self.decoder = TransformerDecoderLayer(
            hidden, _get(model_cfg, 'NUM_HEADS'), _get(model_cfg, 'FFN_CHANNEL'), _get(model_cfg, 'DROPOUT'), _get(model_cfg, 'ACTIVATION'),
            self_posembed=PositionEmbeddingLearned(2, hidden), cross_posembed=PositionEmbeddingLearned(2, hidden))
        head_dict = _get(_get(model_cfg, 'SEPARATE_HEAD_CFG'), 'HEAD_DICT')
        heads = {k: dict(out_channels=_get(v, 'out_channels'), num_conv=_get(v, 'num_conv')) for k, v in copy.deepcopy(dict(head_dict)).items()}
        heads['heatmap'] = dict(out_channels=self.num_classes, num_conv=_get(model_cfg, 'NUM_HM_CONV'))
        self.prediction_head = SeparateHead_Transfusion(hidden, 64, 1, heads, use_bias=bias)
        self.init_weights()
        # opt-in keys of this build: training mode through attention_ops.mha_kv / mha_qkv and their HIP backward, the
        # attention dropout drawn from ATTENTION_DROPOUT_SEED (data-parallel ranks: decoder.set_attention_seed(seed + rank))
        self.decoder.fused_train = bool(_get(model_cfg, 'FUSED_ATTENTION_TRAIN', False))
        self.decoder.set_attention_seed(int(_get(model_cfg, 'ATTENTION_DROPOUT_SEED', 0)))

        # the key positions of the cross-attention, already in (x, y) order: the reference's table runs over
        # (x_size, y_size) in `ij` order, entry n = (n // y_size + 0.5, n % y_size + 0.5), and is flipped before use
        x_size, y_size = int(self.grid_size[0]) // self.feature_map_stride, int(self.grid_size[1]) // self.feature_map_stride
        self.y_size = y_size
        n = torch.arange(x_size * y_size)
        self.register_buffer('bev_pos', torch.stack((n % y_size, n // y_size), dim=-1).float()[None] + 0.5, persistent=False)
        self.use_fused = True                       # False: the torch formulations on any device
        self.forward_ret_dict = {}
        # the training half is opt-in: without the key the head is the eval-only head (no assigner, training refused)
        self.assign_on_device = bool(_get(assigner_cfg, 'ASSIGN_ON_DEVICE', False))
        if self.assign_on_device:
            from .target_assigner.hungarian_assigner import HungarianAssigner3D
            costs = _get(assigner_cfg, 'HUNGARIAN_ASSIGNER')
            self.bbox_assigner = HungarianAssigner3D(**{k: dict(_get(costs, k)) for k in ('cls_cost', 'reg_cost', 'iou_cost')})
            weights = _get(_get(model_cfg, 'LOSS_CONFIG'), 'LOSS_WEIGHTS')
            self.loss_cls_weight, self.loss_bbox_weight = _get(weights, 'cls_weight'), _get(weights, 'bbox_weight')
            self.loss_heatmap_weight, self.code_weights = _get(weights, 'hm_weight'), list(_get(weights, 'code_weights'))
            self.loss_cls_alpha, self.loss_cls_gamma = float(_get(loss_cls, 'alpha')), float(_get(loss_cls, 'gamma'))
            self.head_order = list(_get(_get(model_cfg, 'SEPARATE_HEAD_CFG'), 'HEAD_ORDER'))
            if tuple(self.head_order) != transfusion_ops.HEAD_ORDER[:len(self.head_order)] or len(self.head_order) < 4:
                raise ValueError(f'HEAD_ORDER {self.head_order}: training needs the order of the box code, {list(transfusion_ops.HEAD_ORDER)}')
            self.gaussian_overlap, self.min_radius = _get(assigner_cfg, 'GAUSSIAN_OVERLAP'), _get(assigner_cfg, 'MIN_RADIUS')

    def init_weights(self):
        for p in self.decoder.parameters():
            if p.dim() > 1:
                nn.init.xavier_uniform_(p)
        for m in self.modules():
            if isinstance(m, (nn.BatchNorm2d, nn.BatchNorm1d)):
                m.momentum = self.bn_momentum

    def _on_device(self, x):
        return self.use_fused and x.is_cuda and x.dtype == torch.float32

    def predict(self, inputs):
        """(B, C_in, H, W) -> the prediction head's dict: center (query position added), height, dim, rot, vel, heatmap, each
        (B, c, P), plus query_heatmap_score (B, C, P) and dense_heatmap (B, C, H, W); self.query_labels = the queries' classes"""
        B = inputs.shape[0]
        lidar_feat = self.shared_conv(inputs)
        flat = lidar_feat.flatten(2)                                  # (B, hidden, H * W)
        dense_heatmap = self.heatmap_head(lidar_feat)
        exempt = transfusion_ops.exempt_classes(self.dataset_name, dense_heatmap.shape[1])
        pick = transfusion_ops.proposals if self._on_device(dense_heatmap) else transfusion_ops.proposals_torch
        index, cls, qhs, query_pos = pick(dense_heatmap, self.num_proposals, self.nms_kernel_size, exempt, self.y_size)
        self.query_labels = cls
        query_feat = flat.gather(2, index[:, None, :].expand(-1, flat.shape[1], -1))
        # the class encoding of a one-hot column is that class's weight column plus the bias
        w = self.class_encoding.weight[:, :, 0].t()                   # (C, hidden)
        query_feat = query_feat + (w[cls] + self.class_encoding.bias).transpose(1, 2)
        self.decoder.use_fused = self.use_fused
        query_feat = self.decoder(query_feat, flat, query_pos, self.bev_pos)     # one sample's key positions, broadcast
        res = self.prediction_head(query_feat)
        res['center'] = res['center'] + query_pos.permute(0, 2, 1)
        res['query_heatmap_score'] = qhs
        res['dense_heatmap'] = dense_heatmap
        return res

    def decode_padded(self, res):
        """-> boxes (B, P, 7 | 9), scores (B, P), labels (B, P) int64 (1-based), count (B) int32, survivors first"""
        post = _get(self.model_cfg, 'POST_PROCESSING')
        fn = transfusion_ops.decode if self._on_device(res['heatmap']) else transfusion_ops.decode_torch
        return fn(res['heatmap'], res['center'], res['height'], res['dim'], res['rot'], res.get('vel', None), self.query_labels,
                  res['query_heatmap_score'], _get(post, 'SCORE_THRESH'), list(_get(post, 'POST_CENTER_RANGE')),
                  self.point_cloud_range[0], self.point_cloud_range[1], self.voxel_size[0], self.voxel_size[1], self.feature_map_stride)

    @torch.no_grad()
    def get_bboxes(self, res):
        """-> the reference's list of per-sample dicts pred_boxes (n, 7 | 9), pred_scores (n), pred_labels (n) int32 (1-based)"""
        boxes, scores, labels, count = self.decode_padded(res)
        counts = count.tolist()                                       # the one device-to-host read
        return [{'pred_boxes': boxes[k, :n], 'pred_scores': scores[k, :n], 'pred_labels': labels[k, :n].int()} for k, n in enumerate(counts)]

    # ---- training (TARGET_ASSIGNER_CONFIG.ASSIGN_ON_DEVICE) ------------------------------------------------------------------
    def _assign_args(self):
        a = self.bbox_assigner
        H, W = int(self.grid_size[1]) // self.feature_map_stride, int(self.grid_size[0]) // self.feature_map_stride
        return (a.cls_cost, a.reg_cost, a.iou_cost, list(self.point_cloud_range), list(self.voxel_size), self.feature_map_stride, (H, W),
                self.gaussian_overlap, self.min_radius, self.num_classes)

    def encode_bbox(self, bboxes):
        return transfusion_ops.encode_bbox_torch(bboxes, self.point_cloud_range, self.voxel_size, self.feature_map_stride,
                                                 10 if bboxes.shape[1] >= 9 else 8)

    def _targets(self, gt_boxes, pred_dicts):
        """gt_boxes (B, M, 8 | 10) with the 1-based class last -> transfusion_ops.assign's dict: one launch chain for the batch
        on the GPU, the per-sample torch formulation elsewhere"""
        fn = transfusion_ops.assign if self._on_device(pred_dicts['heatmap']) else transfusion_ops.assign_torch
        return fn(*[pred_dicts[k] for k in ('heatmap', 'center', 'height', 'dim', 'rot')], pred_dicts.get('vel', None), gt_boxes,
                  *self._assign_args())

    def get_targets(self, gt_bboxes_3d, gt_labels_3d, pred_dicts):
        """the reference's tuple (labels, label_weights, bbox_targets, bbox_weights, num_pos, matched_ious, heatmap); num_pos and
        matched_ious stay 0-dim tensors on the device"""
        gt_boxes = torch.cat([gt_bboxes_3d, (gt_labels_3d + 1).to(gt_bboxes_3d.dtype).unsqueeze(-1)], dim=-1)
        t = self._targets(gt_boxes, pred_dicts)
        return t['labels'], t['label_weights'], t['bbox_targets'], t['bbox_weights'], t['num_pos'], t['matched_ious'], t['heatmap']

    def get_targets_single(self, gt_bboxes_3d, gt_labels_3d, preds_dict):
        """one sample: gt_bboxes_3d (G, 7 | 9), gt_labels_3d (G) 0-based, preds_dict of (1, c, P) maps -> get_targets' tuple"""
        return self.get_targets(gt_bboxes_3d[None], gt_labels_3d[None], preds_dict)

    def loss(self, gt_bboxes_3d, gt_labels_3d, pred_dicts, **kwargs):
        """-> (loss_trans, tb_dict); every entry of tb_dict is a detached tensor on the device (no .item())"""
        gt_boxes = torch.cat([gt_bboxes_3d, (gt_labels_3d + 1).to(gt_bboxes_3d.dtype).unsqueeze(-1)], dim=-1)
        return self._loss(gt_boxes, pred_dicts)

    def _loss(self, gt_boxes, pred_dicts):
        targets = self._targets(gt_boxes, pred_dicts)
        fn = transfusion_ops.loss if self._on_device(pred_dicts['heatmap']) else transfusion_ops.loss_torch
        loss_cls, loss_bbox, loss_heatmap = fn(
            *[pred_dicts[k] for k in ('heatmap', 'center', 'height', 'dim', 'rot')], pred_dicts.get('vel', None), pred_dicts['dense_heatmap'],
            targets, self.code_weights, self.loss_cls_weight, self.loss_bbox_weight, self.loss_heatmap_weight, self.loss_cls_alpha,
            self.loss_cls_gamma)
        loss_all = loss_heatmap + loss_cls + loss_bbox
        tb_dict = {'loss_heatmap': loss_heatmap.detach(), 'loss_cls': loss_cls.detach(), 'loss_bbox': loss_bbox.detach(),
                   'matched_ious': targets['matched_ious'], 'loss_trans': loss_all.detach()}
        self.forward_ret_dict['targets'] = targets
        return loss_all, tb_dict

    def forward(self, batch_dict):
        if self.training and self.assign_on_device:
            res = self.predict(batch_dict['spatial_features_2d'])       # under autograd; the queries carry no gradient
            self.forward_ret_dict['pred_dicts'] = res
            batch_dict['loss'], batch_dict['tb_dict'] = self._loss(batch_dict['gt_boxes'], res)
            return batch_dict
        if self.training:
            raise NotImplementedError('TransFusionHead: training needs the Hungarian assigner (HungarianAssigner3D), which this '
                                      'build does not have; the head runs in eval mode only')
        with torch.no_grad():
            res = self.predict(batch_dict['spatial_features_2d'])
            batch_dict['final_box_dicts'] = self.get_bboxes(res)
        self.forward_ret_dict['pred_dicts'] = res
        return batch_dict

"""CenterHead: BEV map -> boxes, the reference's pcdet/models/dense_heads/center_head.py on this repository's operators.

Constructor signature, config keys, initialisation and state_dict keys (shared_conv.{0,1}.*,
heads_list.{i}.{center,center_z,dim,rot,hm}.{j}.*) are the reference's.  What differs is where the work runs: on the GPU
every head's targets, decode and regression loss are one launch chain for the whole batch (center_head_ops.py,
csrc/center_head.hip) with no host read in a training step, where the reference loops over heads x samples x boxes on
the host (center_head.py:141-162, :191-220), gathers whole maps (centernet_utils.py:155-241) and calls .item() per term
(:255-256, :294).  On the CPU (and with use_fused = False) the torch formulations of utils/centernet_utils.py and
utils/loss_utils.py run instead.

Out of scope, rejected by the constructor: NMS_TYPE class_specific_nms / circle_nms, an `iou` head, IOU_REG_LOSS and
USE_IOU_TO_RECTIFY_SCORE.
"""
import copy
from functools import partial

import torch
import torch.nn as nn
from torch.nn.init import kaiming_normal_

from ..iou3d_nms import iou3d_nms_utils
from ..utils import centernet_utils, loss_utils
from .point_head_template import _get


class SeparateHead(nn.Module):
    """One 3x3 convolution stack per entry of sep_head_dict ({name: {out_channels, num_conv}}), each an attribute of
    that name: (num_conv - 1) x [conv, norm, ReLU], then a biased conv.  `hm` ends on bias init_bias (sigmoid(-2.19) =
    0.1); the regression stacks are Kaiming-initialised with zero bias."""

    def __init__(self, input_channels, sep_head_dict, init_bias=-2.19, use_bias=False, norm_func=None):
        super().__init__()
        self.sep_head_dict = sep_head_dict
        norm = nn.BatchNorm2d if norm_func is None else norm_func
        for name in sep_head_dict:
            out_channels, num_conv = sep_head_dict[name]['out_channels'], sep_head_dict[name]['num_conv']
            layers = [nn.Sequential(nn.Conv2d(input_channels, input_channels, 3, stride=1, padding=1, bias=use_bias),
                                    norm(input_channels), nn.ReLU()) for _ in range(num_conv - 1)]
            layers.append(nn.Conv2d(input_channels, out_channels, 3, stride=1, padding=1, bias=True))
            stack = nn.Sequential(*layers)
            if 'hm' in name:
                stack[-1].bias.data.fill_(init_bias)
            else:
                for m in stack.modules():
                    if isinstance(m, nn.Conv2d):
                        kaiming_normal_(m.weight.data)
                        if m.bias is not None:
                            nn.init.constant_(m.bias, 0)
            setattr(self, name, stack)

    def forward(self, x):
        return {name: getattr(self, name)(x) for name in self.sep_head_dict}


class CenterHead(nn.Module):
    def __init__(self, model_cfg, input_channels, num_class, class_names, grid_size, point_cloud_range, voxel_size,
                 predict_boxes_when_training=True):
        super().__init__()
        self.model_cfg = model_cfg
        self.num_class = num_class
        self.grid_size = grid_size
        self.point_cloud_range = point_cloud_range
        self.voxel_size = voxel_size
        self.feature_map_stride = _get(_get(model_cfg, 'TARGET_ASSIGNER_CONFIG'), 'FEATURE_MAP_STRIDE', None)
        self.class_names = list(class_names)
        self.class_names_each_head = []
        self.class_id_mapping_each_head = []        # per head: 0-based global class of each of its classes (a CPU tensor)
        for names in _get(model_cfg, 'CLASS_NAMES_EACH_HEAD'):
            mine = [x for x in names if x in self.class_names]
            self.class_names_each_head.append(mine)
            self.class_id_mapping_each_head.append(torch.tensor([self.class_names.index(x) for x in mine], dtype=torch.int64))
        total = sum(len(x) for x in self.class_names_each_head)
        assert total == len(self.class_names), f'class_names_each_head={self.class_names_each_head}'

        self.separate_head_cfg = _get(model_cfg, 'SEPARATE_HEAD_CFG')
        head_dict, self.head_order = _get(self.separate_head_cfg, 'HEAD_DICT'), list(_get(self.separate_head_cfg, 'HEAD_ORDER'))
        post_cfg = _get(model_cfg, 'POST_PROCESSING', None)
        nms_type = _get(_get(post_cfg, 'NMS_CONFIG', {}), 'NMS_TYPE', 'nms_gpu') if post_cfg is not None else 'nms_gpu'
        for bad, why in ((nms_type not in ('nms_gpu', 'nms_normal_gpu'), f'NMS_TYPE {nms_type}: only nms_gpu / nms_normal_gpu'),
                         ('iou' in head_dict, 'an `iou` head'), (bool(_get(model_cfg, 'IOU_REG_LOSS', False)), 'IOU_REG_LOSS'),
                         (post_cfg is not None and bool(_get(post_cfg, 'USE_IOU_TO_RECTIFY_SCORE', False)), 'USE_IOU_TO_RECTIFY_SCORE')):
            if bad:
                raise NotImplementedError(f'CenterHead: {why} is not supported by this build')
        assert self.head_order[:4] == ['center', 'center_z', 'dim', 'rot'] and self.head_order[4:] in ([], ['vel']), \
            f'HEAD_ORDER {self.head_order}: center, center_z, dim, rot[, vel]'

        norm_func = partial(nn.BatchNorm2d, eps=_get(model_cfg, 'BN_EPS', 1e-5), momentum=_get(model_cfg, 'BN_MOM', 0.1))
        width = _get(model_cfg, 'SHARED_CONV_CHANNEL')
        self.shared_conv = nn.Sequential(
            nn.Conv2d(input_channels, width, 3, stride=1, padding=1, bias=_get(model_cfg, 'USE_BIAS_BEFORE_NORM', False)),
            norm_func(width), nn.ReLU())
        self.heads_list = nn.ModuleList()
        for names in self.class_names_each_head:
            cur = {k: dict(out_channels=_get(v, 'out_channels'), num_conv=_get(v, 'num_conv')) for k, v in copy.deepcopy(dict(head_dict)).items()}
            cur['hm'] = dict(out_channels=len(names), num_conv=_get(model_cfg, 'NUM_HM_CONV'))
            self.heads_list.append(SeparateHead(input_channels=width, sep_head_dict=cur, init_bias=-2.19,
                                                use_bias=_get(model_cfg, 'USE_BIAS_BEFORE_NORM', False), norm_func=norm_func))
        self.predict_boxes_when_training = predict_boxes_when_training
        self.forward_ret_dict = {}
        self.use_fused = True                       # False: the torch formulations on any device
        self.build_losses()

    def build_losses(self):
        self.add_module('hm_loss_func', loss_utils.FocalLossCenterNet())
        self.add_module('reg_loss_func', loss_utils.RegLossCenterNet())

    # ---- targets ---------------------------------------------------------------------------------------------------
    def _local_of(self, head_idx):
        """global class g (1-based; 0 = padding) -> this head's 1-based class, 0 = not this head's"""
        table = [0] * (len(self.class_names) + 1)
        for local, g in enumerate(self.class_id_mapping_each_head[head_idx].tolist()):
            table[g + 1] = local + 1
        return table

    def assign_target_of_single_head(self, num_classes, gt_boxes, feature_map_size, feature_map_stride, num_max_objs=500,
                                     gaussian_overlap=0.1, min_radius=2):
        """The torch formulation for one sample (the reference's center_head.py:106-162 without its loop over boxes):
        gt_boxes (n, 8 + E) of this head, class (the head's, 1-based) last; feature_map_size [x, y] ->
        heatmap (C, H, W), ret_boxes (N, 8 + E), inds (N), mask (N), ret_boxes_src (N, 8 + E).  Only the first
        num_max_objs boxes take part; one host read (the largest radius sizes the batched gaussian window)."""
        W, H = int(feature_map_size[0]), int(feature_map_size[1])
        gt_boxes = gt_boxes[:num_max_objs]
        n, cols = gt_boxes.shape
        heatmap = gt_boxes.new_zeros(num_classes, H, W)
        ret_boxes = gt_boxes.new_zeros((num_max_objs, cols))
        inds = gt_boxes.new_zeros(num_max_objs).long()
        mask = gt_boxes.new_zeros(num_max_objs).long()
        ret_boxes_src = gt_boxes.new_zeros(num_max_objs, cols)
        ret_boxes_src[:n] = gt_boxes
        if n == 0:
            return heatmap, ret_boxes, inds, mask, ret_boxes_src
        coord_x = torch.clamp((gt_boxes[:, 0] - self.point_cloud_range[0]) / self.voxel_size[0] / feature_map_stride, min=0, max=W - 0.5)
        coord_y = torch.clamp((gt_boxes[:, 1] - self.point_cloud_range[1]) / self.voxel_size[1] / feature_map_stride, min=0, max=H - 0.5)
        center = torch.stack((coord_x, coord_y), dim=-1)
        center_int = center.int()
        dx = gt_boxes[:, 3] / self.voxel_size[0] / feature_map_stride
        dy = gt_boxes[:, 4] / self.voxel_size[1] / feature_map_stride
        valid = (dx > 0) & (dy > 0)
        one = torch.ones_like(dx)
        radius = centernet_utils.gaussian_radius(torch.where(valid, dx, one), torch.where(valid, dy, one), min_overlap=gaussian_overlap)
        radius = torch.clamp_min(radius.int(), min=min_radius).long()
        inds[:n] = torch.where(valid, center_int[:, 1].long() * W + center_int[:, 0].long(), torch.zeros_like(inds[:n]))
        mask[:n] = valid.long()
        safe = torch.where(valid[:, None], gt_boxes, torch.ones_like(gt_boxes))
        rows = torch.cat((center - center_int.float(), safe[:, 2:3], safe[:, 3:6].log(), torch.cos(safe[:, 6:7]),
                          torch.sin(safe[:, 6:7]), safe[:, 7:-1]), dim=-1)
        ret_boxes[:n] = torch.where(valid[:, None], rows, torch.zeros_like(rows))
        if bool(valid.any()):
            cls_idx = torch.stack((torch.zeros_like(inds[:n]), (gt_boxes[:, -1].long() - 1).clamp(min=0)), dim=-1)
            centernet_utils.draw_gaussians(heatmap[None], cls_idx[None], center_int.long()[None], radius[None], valid[None],
                                           max_radius=int(radius[valid].max()))
        return heatmap, ret_boxes, inds, mask, ret_boxes_src

    @torch.no_grad()
    def assign_targets(self, gt_boxes, feature_map_size=None, **kwargs):
        """gt_boxes (B, M, 7 + E + 1), global class (1-based, 0 = padding) last; feature_map_size (H, W) -> the reference's
        dict of per-head lists: heatmaps (B, C_head, H, W), target_boxes (B, N, 8 + E), inds (B, N), masks (B, N),
        target_boxes_src (B, N, 7 + E + 1) and an empty heatmap_masks.

        One deliberate difference: the reference rewrites the class column of the CALLER's gt_boxes while it collects a
        head's boxes (center_head.py:200-201 writes through a view), so that with interleaved class lists, e.g.
        [['Car', 'Cyclist'], ['Pedestrian']], a later head adopts boxes an earlier head relabelled.  Here gt_boxes is
        left untouched and every head is assigned from the original classes."""
        H, W = int(feature_map_size[0]), int(feature_map_size[1])
        cfg = _get(self.model_cfg, 'TARGET_ASSIGNER_CONFIG')
        stride, nmax = _get(cfg, 'FEATURE_MAP_STRIDE'), int(_get(cfg, 'NUM_MAX_OBJS'))
        overlap, min_radius = _get(cfg, 'GAUSSIAN_OVERLAP'), int(_get(cfg, 'MIN_RADIUS'))
        ret = {'heatmaps': [], 'target_boxes': [], 'inds': [], 'masks': [], 'heatmap_masks': [], 'target_boxes_src': []}
        for idx, names in enumerate(self.class_names_each_head):
            table = self._local_of(idx)
            if gt_boxes.is_cuda and self.use_fused:
                from .. import center_head_ops
                outs = center_head_ops.center_targets(
                    gt_boxes, table, len(names), H, W, self.point_cloud_range[0], self.point_cloud_range[1], self.voxel_size[0],
                    self.voxel_size[1], stride, nmax, overlap, min_radius)
            else:
                table_t = torch.tensor(table, dtype=torch.int64, device=gt_boxes.device)
                per_sample = []
                for b in range(gt_boxes.shape[0]):
                    cur = gt_boxes[b].float()
                    local = table_t[cur[:, -1].long().clamp(0, len(self.class_names))]
                    mine = cur[local > 0].clone()                    # (a copy: the caller's boxes keep their classes)
                    mine[:, -1] = local[local > 0].to(mine.dtype)
                    per_sample.append(self.assign_target_of_single_head(
                        num_classes=len(names), gt_boxes=mine, feature_map_size=(W, H), feature_map_stride=stride,
                        num_max_objs=nmax, gaussian_overlap=overlap, min_radius=min_radius))
                outs = [torch.stack(x, dim=0) for x in zip(*per_sample)]
            for key, val in zip(('heatmaps', 'target_boxes', 'inds', 'masks', 'target_boxes_src'), outs):
                ret[key].append(val)
        return ret

    # ---- losses ----------------------------------------------------------------------------------------------------
    def sigmoid(self, x):
        return torch.clamp(x.sigmoid(), min=1e-4, max=1 - 1e-4)

    def get_loss(self):
        """-> (loss, tb_dict): per head the penalty-reduced focal loss on clamp(sigmoid(hm)) times cls_weight plus the L1
        regression loss times code_weights and loc_weight; tb_dict holds detached device tensors under the reference's keys
        (hm_loss_head_%d, loc_loss_head_%d, rpn_loss): no .item(), no host read."""
        pred_dicts, target_dicts = self.forward_ret_dict['pred_dicts'], self.forward_ret_dict['target_dicts']
        weights = _get(_get(self.model_cfg, 'LOSS_CONFIG'), 'LOSS_WEIGHTS')
        cls_weight, loc_weight, code_weights = _get(weights, 'cls_weight'), _get(weights, 'loc_weight'), list(_get(weights, 'code_weights'))
        tb_dict, loss = {}, 0
        for idx, pred_dict in enumerate(pred_dicts):
            logits, heatmap = pred_dict['hm'], target_dicts['heatmaps'][idx]
            maps = [pred_dict[name] for name in self.head_order]
            fused = self.use_fused and logits.is_cuda and all(t.dtype in (torch.float32, torch.bfloat16) for t in [logits] + maps)
            if fused:
                from .. import center_head_ops, heatmap_loss
                hm_loss = heatmap_loss.heatmap_focal_loss(logits, heatmap.float().contiguous(), cls_weight)
                loc_loss, _ = center_head_ops.center_reg_loss(maps, target_dicts['inds'][idx], target_dicts['masks'][idx],
                                                              target_dicts['target_boxes'][idx], code_weights, loc_weight)
            else:
                hm_loss = self.hm_loss_func(self.sigmoid(logits.float()), heatmap) * cls_weight
                reg_loss = self.reg_loss_func(torch.cat(maps, dim=1).float(), target_dicts['masks'][idx], target_dicts['inds'][idx],
                                              target_dicts['target_boxes'][idx])
                loc_loss = (reg_loss * reg_loss.new_tensor(code_weights)).sum() * loc_weight
            loss = loss + hm_loss + loc_loss
            tb_dict['hm_loss_head_%d' % idx] = hm_loss.detach()
            tb_dict['loc_loss_head_%d' % idx] = loc_loss.detach()
        tb_dict['rpn_loss'] = loss.detach()
        return loss, tb_dict

    # ---- boxes -----------------------------------------------------------------------------------------------------
    def _decode_padded(self, idx, pred_dict, post_cfg):
        """one head's maps -> pdm_center_decode's padded output (labels global, 1-based)"""
        from .. import center_head_ops
        return center_head_ops.center_decode(
            pred_dict['hm'], pred_dict['center'], pred_dict['center_z'], pred_dict['dim'], pred_dict['rot'],
            pred_dict['vel'] if 'vel' in self.head_order else None, int(_get(post_cfg, 'MAX_OBJ_PER_SAMPLE')), _get(post_cfg, 'SCORE_THRESH'),
            list(_get(post_cfg, 'POST_CENTER_LIMIT_RANGE')), self.point_cloud_range[0], self.point_cloud_range[1], self.voxel_size[0],
            self.voxel_size[1], self.feature_map_stride, self.class_id_mapping_each_head[idx].tolist())

    def _batched_reason(self, post_cfg):
        from .. import post_process
        nms_cfg = _get(post_cfg, 'NMS_CONFIG')
        thresh = _get(post_cfg, 'SCORE_THRESH')
        if thresh is None or not thresh > 0:
            return 'SCORE_THRESH is not positive (padding rows carry the score 0)'
        if int(_get(nms_cfg, 'NMS_PRE_MAXSIZE')) > post_process.MAX_PRE:
            return f'NMS_PRE_MAXSIZE > {post_process.MAX_PRE}'
        if float(_get(nms_cfg, 'NMS_THRESH')) < 0:
            return 'NMS_THRESH < 0'
        return None

    def generate_predicted_boxes(self, batch_size, pred_dicts):
        """-> the reference's list of per-sample dicts pred_boxes (n, 7 | 9), pred_scores (n), pred_labels (n) (global,
        1-based): every head's K best candidates decoded, class-agnostic NMS per head and sample, heads concatenated in
        head order (center_head.py:297-365).

        Default: the decode of a head is one call for the batch (pdm_center_decode; its counts are read once per head),
        then the reference's per-sample NMS loop.  POST_PROCESSING.BATCHED: the padded decode output of every head goes
        through pdm_post_process (its score row holds the score in the label's column and zeros elsewhere), and ONE
        device-to-host read serves the whole batch and all heads."""
        post_cfg = _get(self.model_cfg, 'POST_PROCESSING')
        nms_cfg = _get(post_cfg, 'NMS_CONFIG')
        on_gpu = self.use_fused and pred_dicts[0]['hm'].is_cuda
        if on_gpu and _get(post_cfg, 'BATCHED', False):
            from .. import post_process
            reason = self._batched_reason(post_cfg)
            if reason is None:
                return self._generate_batched(batch_size, pred_dicts, post_cfg)
            post_process.warn_once(reason)
        ret = [{'pred_boxes': [], 'pred_scores': [], 'pred_labels': []} for _ in range(batch_size)]
        for idx, pred_dict in enumerate(pred_dicts):
            if on_gpu:
                boxes, scores, labels, count = self._decode_padded(idx, pred_dict, post_cfg)
                counts = count.tolist()
                finals = [{'pred_boxes': boxes[k, :counts[k]], 'pred_scores': scores[k, :counts[k]], 'pred_labels': labels[k, :counts[k]] - 1}
                          for k in range(batch_size)]
            else:
                finals = centernet_utils.decode_bbox_from_heatmap(
                    heatmap=pred_dict['hm'].float().sigmoid(), rot_cos=pred_dict['rot'][:, 0:1].float(), rot_sin=pred_dict['rot'][:, 1:2].float(),
                    center=pred_dict['center'].float(), center_z=pred_dict['center_z'].float(), dim=pred_dict['dim'].float().exp(),
                    vel=pred_dict['vel'].float() if 'vel' in self.head_order else None, point_cloud_range=self.point_cloud_range,
                    voxel_size=self.voxel_size, feature_map_stride=self.feature_map_stride, K=int(_get(post_cfg, 'MAX_OBJ_PER_SAMPLE')),
                    score_thresh=_get(post_cfg, 'SCORE_THRESH'), post_center_limit_range=list(_get(post_cfg, 'POST_CENTER_LIMIT_RANGE')))
                mapping = self.class_id_mapping_each_head[idx].to(pred_dict['hm'].device)
                for final in finals:
                    final['pred_labels'] = mapping[final['pred_labels'].long()]
            for k, final in enumerate(finals):
                selected, selected_scores = iou3d_nms_utils.class_agnostic_nms(
                    box_scores=final['pred_scores'], box_preds=final['pred_boxes'], nms_config=nms_cfg, score_thresh=None)
                ret[k]['pred_boxes'].append(final['pred_boxes'][selected])
                ret[k]['pred_scores'].append(selected_scores)
                ret[k]['pred_labels'].append(final['pred_labels'][selected])
        for k in range(batch_size):
            ret[k]['pred_boxes'] = torch.cat(ret[k]['pred_boxes'], dim=0)
            ret[k]['pred_scores'] = torch.cat(ret[k]['pred_scores'], dim=0)
            ret[k]['pred_labels'] = torch.cat(ret[k]['pred_labels'], dim=0) + 1
        return ret

    def _generate_batched(self, batch_size, pred_dicts, post_cfg):
        from .. import post_process
        nms_only = {'NMS_CONFIG': _get(post_cfg, 'NMS_CONFIG'), 'SCORE_THRESH': _get(post_cfg, 'SCORE_THRESH')}
        per_head = []
        for idx, pred_dict in enumerate(pred_dicts):
            boxes, scores, labels, _ = self._decode_padded(idx, pred_dict, post_cfg)
            B, K, D = boxes.shape
            cls = torch.zeros((B, K, self.num_class), dtype=torch.float32, device=boxes.device)
            cls.scatter_(2, (labels - 1).clamp_(min=0).unsqueeze(2), scores.unsqueeze(2))
            out = post_process.post_process_padded({'batch_size': B, 'batch_cls_preds': cls, 'batch_box_preds': boxes,
                                                    'cls_preds_normalized': True}, nms_only, self.num_class)
            rows = out['rows'].clamp(min=0)
            per_head.append((boxes.gather(1, rows.unsqueeze(2).expand(-1, -1, D)), out['scores'], out['labels'], out['count']))
        counts = torch.stack([h[3] for h in per_head], dim=0).cpu().tolist()      # the one device-to-host read
        ret = []
        for k in range(batch_size):
            ret.append({'pred_boxes': torch.cat([h[0][k, :counts[i][k]] for i, h in enumerate(per_head)], dim=0),
                        'pred_scores': torch.cat([h[1][k, :counts[i][k]] for i, h in enumerate(per_head)], dim=0),
                        'pred_labels': torch.cat([h[2][k, :counts[i][k]] for i, h in enumerate(per_head)], dim=0)})
        return ret

    @staticmethod
    def reorder_rois_for_refining(batch_size, pred_dicts):
        """per-sample dicts -> rois (B, R, 7 | 9), roi_scores (B, R), roi_labels (B, R) zero-padded to the longest
        sample (at least one row)"""
        num_max_rois = max(1, max(len(d['pred_boxes']) for d in pred_dicts))
        pred_boxes = pred_dicts[0]['pred_boxes']
        rois = pred_boxes.new_zeros((batch_size, num_max_rois, pred_boxes.shape[-1]))
        roi_scores = pred_boxes.new_zeros((batch_size, num_max_rois))
        roi_labels = pred_boxes.new_zeros((batch_size, num_max_rois)).long()
        for b in range(batch_size):
            n = len(pred_dicts[b]['pred_boxes'])
            rois[b, :n] = pred_dicts[b]['pred_boxes']
            roi_scores[b, :n] = pred_dicts[b]['pred_scores']
            roi_labels[b, :n] = pred_dicts[b]['pred_labels']
        return rois, roi_scores, roi_labels

    def forward(self, data_dict):
        x = data_dict['spatial_features_2d'] if 'spatial_features_2d' in data_dict else data_dict['spatial_features']
        if x.dim() == 4 and not x.is_contiguous() and x.permute(0, 2, 3, 1).is_contiguous():
            x = x.contiguous(memory_format=torch.channels_last)   # the neck's grid is channels-last storage: no copy
        shared = self.shared_conv(x)
        pred_dicts = [head(shared) for head in self.heads_list]
        if self.training:
            self.forward_ret_dict['target_dicts'] = self.assign_targets(
                data_dict['gt_boxes'], feature_map_size=x.size()[2:],
                feature_map_stride=data_dict.get('spatial_features_2d_strides', None))
        self.forward_ret_dict['pred_dicts'] = pred_dicts
        if not self.training or self.predict_boxes_when_training:
            with torch.no_grad():
                boxes = self.generate_predicted_boxes(data_dict['batch_size'], pred_dicts)
            if self.predict_boxes_when_training:
                rois, roi_scores, roi_labels = self.reorder_rois_for_refining(data_dict['batch_size'], boxes)
                data_dict['rois'] = rois
                data_dict['roi_scores'] = roi_scores
                data_dict['roi_labels'] = roi_labels
                data_dict['has_class_labels'] = True
            else:
                data_dict['final_box_dicts'] = boxes
        return data_dict

"""Part-A2's second stage: behaviour, constructor signature, config keys and state_dict keys (conv_part, conv_rpn,
shared_fc_layer, cls_layers, reg_layers, the post_act_block indice keys) of the reference's pcdet/models/roi_heads/partA2_head.py
(PartA2FCHead), restated, in eval mode.

Per RoI an S x S x S grid of cells; per cell the average of the part features (intra-object part location + foreground score)
and the maximum of the UNet's point features over the cell's first MAX_POINTS_PER_VOXEL - 1 points; the active cells of all
RoIs as one sparse tensor through two submanifold stacks; its dense (R, 128 S^3) form through the shared FC stack.

Two paths, `ROI_AWARE_POOL.FUSED` (default on):
  * fused: roiaware_pool_sparse pools the whole batch straight to the sparse rows (ONE host read: the row count);
    conv_part / conv_rpn run on those rows sharing one indice_dict; sparse_fc applies shared_fc_layer[0:3] (Conv1d, BatchNorm1d,
    ReLU folded) to the rows where they lie, with neither the torch.cat nor the dense tensor.  Point rows must be batch-major
    (UNetV2's are).
  * composed: the reference's formulation on this tree's operators: per-sample RoIAwarePool3d 'avg' and 'max', nonzero, gather,
    the four convolutions, dense(), Conv1d.  The on-device checker of the fused path, and the path for what it refuses: fewer
    than three active cells (the reference's fake_sparse_idx case), point lists past the pooling's capacity, a grid above 4096
    cells, widths outside the operators' multiples.  `last_path` tells which ran.

Training raises NotImplementedError: proposal targets for this head and the gradients of the two operators are not built.
"""
import torch
import torch.nn as nn

from .. import sparse_conv_ops, spconv
from ..pv_rcnn_ops import sample_counts
from ..roiaware_pool3d import roiaware_pool3d_utils
from .roi_head_template import RoIHeadTemplate, _get


class PartA2FCHead(RoIHeadTemplate):
    def __init__(self, input_channels, model_cfg, num_class=1, **kwargs):
        super().__init__(num_class=num_class, model_cfg=model_cfg)
        self.pool_cfg = _get(model_cfg, 'ROI_AWARE_POOL')
        self.SA_modules = nn.ModuleList()
        block = self.post_act_block
        c0 = _get(self.pool_cfg, 'NUM_FEATURES') // 2
        self.conv_part = spconv.SparseSequential(block(4, 64, 3, padding=1, indice_key='rcnn_subm1'),
                                                 block(64, c0, 3, padding=1, indice_key='rcnn_subm1_1'))
        self.conv_rpn = spconv.SparseSequential(block(input_channels, 64, 3, padding=1, indice_key='rcnn_subm2'),
                                                block(64, c0, 3, padding=1, indice_key='rcnn_subm1_2'))
        pool_size = int(_get(self.pool_cfg, 'POOL_SIZE'))
        pre_channel = _get(self.pool_cfg, 'NUM_FEATURES') * pool_size ** 3
        widths, drop = list(_get(model_cfg, 'SHARED_FC')), _get(model_cfg, 'DP_RATIO')
        shared = []
        for k, width in enumerate(widths):
            shared += [nn.Conv1d(pre_channel, width, kernel_size=1, bias=False), nn.BatchNorm1d(width), nn.ReLU()]
            pre_channel = width
            if k != len(widths) - 1 and drop > 0:       # (holds no parameter but shifts the children behind it: the reference's keys)
                shared.append(nn.Dropout(drop))
        self.shared_fc_layer = nn.Sequential(*shared)
        self.cls_layers = self.make_fc_layers(input_channels=pre_channel, output_channels=self.num_class, fc_list=_get(model_cfg, 'CLS_FC'))
        self.reg_layers = self.make_fc_layers(input_channels=pre_channel, output_channels=self.box_coder.code_size * self.num_class,
                                              fc_list=_get(model_cfg, 'REG_FC'))
        self.roiaware_pool3d_layer = roiaware_pool3d_utils.RoIAwarePool3d(out_size=pool_size,
                                                                          max_pts_each_voxel=_get(self.pool_cfg, 'MAX_POINTS_PER_VOXEL'))
        self.pool_size = pool_size
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
        nn.init.normal_(self.reg_layers[-1].weight, mean=0, std=0.001)

    @staticmethod
    def post_act_block(in_channels, out_channels, kernel_size, indice_key, stride=1, padding=0, conv_type='subm'):
        if conv_type == 'subm':
            conv = spconv.SubMConv3d(in_channels, out_channels, kernel_size, bias=False, indice_key=indice_key)
        elif conv_type == 'spconv':
            conv = spconv.SparseConv3d(in_channels, out_channels, kernel_size, stride=stride, padding=padding, bias=False, indice_key=indice_key)
        elif conv_type == 'inverseconv':
            conv = spconv.SparseInverseConv3d(in_channels, out_channels, kernel_size, indice_key=indice_key, bias=False)
        else:
            raise NotImplementedError(conv_type)
        return spconv.SparseSequential(conv, nn.BatchNorm1d(out_channels, eps=1e-3, momentum=0.01), nn.ReLU())

    # ------------------------------------------------------------------ pooling

    def _point_inputs(self, batch_dict):
        """-> batch_idx (P,), xyz (P, 3), part_features (P, 4), rpn features (P, C): the part location (or, with DISABLE_PART, the
        coordinates) and the foreground score, the location zeroed where the score is below SEG_MASK_SCORE_THRESH"""
        coords = batch_dict['point_coords']
        xyz = coords[:, 1:4]
        lead = xyz if _get(self.model_cfg, 'DISABLE_PART', False) else batch_dict['point_part_offset']
        part = torch.cat((lead, batch_dict['point_cls_scores'].view(-1, 1).detach()), dim=1)
        part[part[:, -1] < _get(self.model_cfg, 'SEG_MASK_SCORE_THRESH'), 0:3] = 0
        return coords[:, 0], xyz, part, batch_dict['point_features']

    def roiaware_pool(self, batch_dict):
        """the reference's per-sample pooling -> (B N, S, S, S, 4) averages and (B N, S, S, S, C) maxima"""
        batch_idx, xyz, part, rpn = self._point_inputs(batch_dict)
        rois = batch_dict['rois']
        pooled_part, pooled_rpn = [], []
        for b in range(batch_dict['batch_size']):
            mask = batch_idx == b
            cur_roi = rois[b][:, 0:7].contiguous()
            pooled_part.append(self.roiaware_pool3d_layer(cur_roi, xyz[mask], part[mask], pool_method='avg'))
            pooled_rpn.append(self.roiaware_pool3d_layer(cur_roi, xyz[mask], rpn[mask], pool_method='max'))
        return torch.cat(pooled_part, dim=0), torch.cat(pooled_rpn, dim=0)

    @staticmethod
    def fake_sparse_idx(sparse_idx, batch_size_rcnn):
        """fewer than three active cells: the first cell of every RoI stands in (the reference's rule)"""
        zeros = sparse_idx.new_zeros((batch_size_rcnn, 3))
        return torch.cat((torch.arange(batch_size_rcnn).type_as(sparse_idx).view(-1, 1), zeros), dim=1)

    def _fused_applies(self, batch_dict):
        if not _get(self.pool_cfg, 'FUSED', True):
            return False
        feats = batch_dict['point_features']
        c0 = _get(self.pool_cfg, 'NUM_FEATURES') // 2
        first = self.shared_fc_layer[0]
        return (feats.is_cuda and feats.dtype == torch.float32 and not torch.is_grad_enabled() and self.pool_size ** 3 <= 4096
                and c0 % 4 == 0 and (2 * c0) % 16 == 0 and 2 * c0 <= 512 and first.out_channels % 16 == 0 and first.out_channels <= 1024
                and isinstance(self.shared_fc_layer[1], nn.BatchNorm1d) and not self.shared_fc_layer[1].training)

    def _packed_fc(self):
        """shared_fc_layer[0] repacked cell-major and shared_fc_layer[1] folded, once per version of their tensors"""
        conv, bn = self.shared_fc_layer[0], self.shared_fc_layer[1]
        sources = [conv.weight, bn.weight, bn.bias, bn.running_mean, bn.running_var]
        key = tuple((t.data_ptr(), t._version) for t in sources)
        if self._fc_cache is None or self._fc_cache[0] != key:
            with torch.no_grad():
                scale, shift = spconv.fold_norm(bn, None, conv.out_channels, conv.weight)
                self._fc_cache = (key, (sparse_conv_ops.pack_fc_weight(conv.weight, self.pool_size ** 3), scale, shift))
        return self._fc_cache[1]

    def _shared_fused(self, batch_dict):
        """-> (R, SHARED_FC[0], 1) behind shared_fc_layer[0:3], or None where the fused path does not apply"""
        batch_idx, xyz, part, rpn = self._point_inputs(batch_dict)
        rois = batch_dict['rois'][:, :, 0:7].contiguous()
        B, R, S = rois.shape[0], rois.shape[0] * rois.shape[1], self.pool_size
        try:
            coords, part_rows, rpn_rows = roiaware_pool3d_utils.roiaware_pool_sparse(
                rois, xyz, sample_counts(batch_idx, B), part, rpn, S, _get(self.pool_cfg, 'MAX_POINTS_PER_VOXEL'))
        except roiaware_pool3d_utils.PointListOverflow:        # the boxes list more points than the pooling's workspace takes
            return None
        if coords.shape[0] < 3:
            return None
        indice_dict = {}
        x_part = self.conv_part(spconv.SparseConvTensor(part_rows, coords, (S, S, S), R, indice_dict))
        x_rpn = self.conv_rpn(spconv.SparseConvTensor(rpn_rows, coords, (S, S, S), R, indice_dict))
        wpack, scale, shift = self._packed_fc()
        relu = isinstance(self.shared_fc_layer[2], nn.ReLU)
        out = sparse_conv_ops.sparse_fc(coords, x_rpn.features, x_part.features, R, (S, S, S), wpack, self.shared_fc_layer[0].out_channels,
                                        scale, shift, relu)
        return out.unsqueeze(-1), (3 if relu else 2)

    def _shared_composed(self, batch_dict):
        pooled_part, pooled_rpn = self.roiaware_pool(batch_dict)
        R = pooled_part.shape[0]
        sparse_shape = pooled_part.shape[1:4]
        sparse_idx = pooled_part.sum(dim=-1).nonzero()
        if sparse_idx.shape[0] < 3:
            sparse_idx = self.fake_sparse_idx(sparse_idx, R)
        i = sparse_idx
        part_rows, rpn_rows = pooled_part[i[:, 0], i[:, 1], i[:, 2], i[:, 3]], pooled_rpn[i[:, 0], i[:, 1], i[:, 2], i[:, 3]]
        coords = sparse_idx.int().contiguous()
        x_part = self.conv_part(spconv.SparseConvTensor(part_rows, coords, sparse_shape, R))
        x_rpn = self.conv_rpn(spconv.SparseConvTensor(rpn_rows, coords, sparse_shape, R))
        merged = torch.cat((x_rpn.features, x_part.features), dim=1)
        return spconv.SparseConvTensor(merged, coords, sparse_shape, R).dense().view(R, -1, 1), 0

    # ------------------------------------------------------------------ forward

    def forward(self, batch_dict):
        """proposals (unless rois are given) -> rcnn_cls (R, num_class), rcnn_reg (R, code_size), batch_cls_preds /
        batch_box_preds with cls_preds_normalized = False"""
        if self.training:
            raise NotImplementedError('PartA2FCHead runs in eval mode only: proposal targets for this head and the gradients of '
                                      'pdm_roiaware_pool_sparse and pdm_sparse_fc are not built')
        self.proposal_layer(batch_dict, nms_config=_get(self.model_cfg, 'NMS_CONFIG')['TEST'])
        done = self._shared_fused(batch_dict) if self._fused_applies(batch_dict) else None
        self.last_path = 'fused' if done is not None else 'composed'
        shared, first = done if done is not None else self._shared_composed(batch_dict)
        for layer in list(self.shared_fc_layer)[first:]:
            shared = layer(shared)
        rcnn_cls = self.cls_layers(shared).transpose(1, 2).contiguous().squeeze(dim=1)
        rcnn_reg = self.reg_layers(shared).transpose(1, 2).contiguous().squeeze(dim=1)
        cls, boxes = self.generate_predicted_boxes(batch_size=batch_dict['batch_size'], rois=batch_dict['rois'], cls_preds=rcnn_cls,
                                                   box_preds=rcnn_reg)
        batch_dict.update(rcnn_cls=rcnn_cls, rcnn_reg=rcnn_reg, batch_cls_preds=cls, batch_box_preds=boxes, cls_preds_normalized=False)
        return batch_dict

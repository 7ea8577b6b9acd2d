"""Voxel R-CNN's second stage: behaviour, constructor signature, config keys and state_dict keys of the reference's
pcdet/models/roi_heads/voxelrcnn_head.py, restated.

Per RoI a G x G x G lattice of grid points; per grid point and per source level of the voxel backbone (ROI_GRID_POOL.
FEATURES_SOURCE) the voxels of a window around the point's cell, within POOL_RADIUS, the first NSAMPLE of them, pooled by
NeighborVoxelSAModuleMSG; the levels' columns side by side -> shared_fc_layer over the flattened (G^3 x channels) row ->
cls_fc_layers / cls_pred_layer and reg_fc_layers / reg_pred_layer.

roi_grid_pool (`use_fused_pool`, default on): per level ONE site index (sparse_conv_ops.site_index: bitmap + prefixes +
row_of_rank, 1 bit a cell instead of the 4 bytes a cell of the reference's dense table), per scale one mlps_in contraction
over the level's rows and one launch of pdm_roi_grid_pool writing its columns of the (B n G^3, sum C2) output: no torch.cat,
no host read, graph-capturable.  A level whose module the fused operator refuses (avg_pool, other widths) and
use_fused_pool = False take the reference's formulation on VoxelQueryAndGrouping, the checker of the fused operator.

Training (TARGET_CONFIG with the sampler's settings): proposals under NMS_CONFIG.TRAIN, proposal targets, the sampled rois
pooled under autograd, per level by NeighborVoxelSAModuleMSG.forward_fused_train (csrc/roi_grid_train.hip) where
it applies and by the composed formulation otherwise, the FC stacks, forward_ret_dict for RoIHeadTemplate.get_loss.  On the
device only: off it the RoI-grid pooling has no gradient.
"""
import torch
import torch.nn as nn

from .. import sparse_conv_ops
from ..pointnet2_stack import voxel_pool_modules as voxelpool_stack_modules
from ..utils import common_utils
from .roi_head_template import RoIHeadTemplate, _get


class VoxelRCNNHead(RoIHeadTemplate):
    def __init__(self, backbone_channels, model_cfg, point_cloud_range, voxel_size, num_class=1, **kwargs):
        super().__init__(num_class=num_class, model_cfg=model_cfg)
        self.pool_cfg = _get(model_cfg, 'ROI_GRID_POOL')
        layer_cfg = _get(self.pool_cfg, 'POOL_LAYERS')
        self.point_cloud_range = [float(v) for v in point_cloud_range]
        self.voxel_size = [float(v) for v in voxel_size]
        self.use_fused_pool = True

        c_out = 0
        self.roi_grid_pool_layers = nn.ModuleList()
        for src_name in _get(self.pool_cfg, 'FEATURES_SOURCE'):
            cfg = _get(layer_cfg, src_name)
            mlps = [[backbone_channels[src_name]] + list(spec) for spec in _get(cfg, 'MLPS')]      # (the reference edits MLPS in place)
            self.roi_grid_pool_layers.append(voxelpool_stack_modules.NeighborVoxelSAModuleMSG(
                query_ranges=_get(cfg, 'QUERY_RANGES'), nsamples=_get(cfg, 'NSAMPLE'), radii=_get(cfg, 'POOL_RADIUS'), mlps=mlps,
                pool_method=_get(cfg, 'POOL_METHOD')))
            c_out += sum(x[-1] for x in mlps)
        self.num_pooled_channels = c_out

        grid_size = int(_get(self.pool_cfg, 'GRID_SIZE'))
        drop = _get(model_cfg, 'DP_RATIO')

        def fc_stack(widths, pre_channel):
            """[Linear(no bias), BatchNorm1d, ReLU] per width, a Dropout behind every block but the last when DP_RATIO > 0 (it
            holds no parameter but shifts the indices of the children behind it: the reference's keys)"""
            layers = []
            for k, width in enumerate(widths):
                layers += [nn.Linear(pre_channel, width, bias=False), nn.BatchNorm1d(width), nn.ReLU()]
                pre_channel = width
                if k != len(widths) - 1 and drop > 0:
                    layers.append(nn.Dropout(drop))
            return nn.Sequential(*layers), pre_channel

        self.shared_fc_layer, shared = fc_stack(_get(model_cfg, 'SHARED_FC'), grid_size ** 3 * c_out)
        self.cls_fc_layers, width = fc_stack(_get(model_cfg, 'CLS_FC'), shared)
        self.cls_pred_layer = nn.Linear(width, self.num_class, bias=True)
        # (the reference feeds reg_fc_layers from the LAST cls width, its `pre_channel` running on: kept, or the keys' shapes differ)
        self.reg_fc_layers, width = fc_stack(_get(model_cfg, 'REG_FC'), width)
        self.reg_pred_layer = nn.Linear(width, self.box_coder.code_size * self.num_class, bias=True)
        self.init_weights()

    def init_weights(self):
        for stack in (self.shared_fc_layer, self.cls_fc_layers, self.reg_fc_layers):
            for m in stack.modules():
                if isinstance(m, nn.Linear):
                    nn.init.xavier_normal_(m.weight)
                    if m.bias is not None:
                        nn.init.constant_(m.bias, 0)
        nn.init.normal_(self.cls_pred_layer.weight, 0, 0.01)
        nn.init.constant_(self.cls_pred_layer.bias, 0)
        nn.init.normal_(self.reg_pred_layer.weight, mean=0, std=0.001)
        nn.init.constant_(self.reg_pred_layer.bias, 0)

    # ------------------------------------------------------------------ pooling

    def _level(self, batch_dict, src_name):
        key = 'multi_scale_3d_features_post' if batch_dict.get('with_voxel_feature_transform', False) else 'multi_scale_3d_features'
        return batch_dict[key][src_name], int(batch_dict['multi_scale_3d_strides'][src_name])

    def roi_grid_pool(self, batch_dict):
        """batch_size, rois (B, n, 7 + C), multi_scale_3d_features / multi_scale_3d_strides -> (B n, G^3, sum of the levels' C2);
        in training mode under autograd in the levels' features and the pool layers' parameters (the rois detached)"""
        if self.training:
            return self._roi_grid_pool_train(batch_dict)
        with torch.no_grad():
            return self._roi_grid_pool_eval(batch_dict)

    def _roi_grid_pool_train(self, batch_dict):
        rois = batch_dict['rois'].detach().float().contiguous()
        B, n = rois.shape[0], rois.shape[1]
        G = int(_get(self.pool_cfg, 'GRID_SIZE'))
        composed_inputs = None
        pooled = []
        for k, src_name in enumerate(_get(self.pool_cfg, 'FEATURES_SOURCE')):
            layer = self.roi_grid_pool_layers[k]
            sp, stride = self._level(batch_dict, src_name)
            if self.use_fused_pool and rois.is_cuda and layer.fused_train_supported(G):
                index = sparse_conv_ops.site_index(sp.indices, B, sp.spatial_shape)
                pooled.append(layer.forward_fused_train(rois, G, sp.features, index, stride, self.voxel_size, self.point_cloud_range))
                continue
            if composed_inputs is None:
                with torch.no_grad():
                    composed_inputs = self._grid_points_and_cells(rois, G)
            pooled.append(self._pool_level_composed(layer, sp, stride, B, *composed_inputs))
        return torch.cat(pooled, dim=1).view(B * n, G ** 3, self.num_pooled_channels)

    def _roi_grid_pool_eval(self, batch_dict):
        rois = batch_dict['rois'].float().contiguous()
        B, n = rois.shape[0], rois.shape[1]
        G = int(_get(self.pool_cfg, 'GRID_SIZE'))
        sources = list(_get(self.pool_cfg, 'FEATURES_SOURCE'))
        fused = [self.use_fused_pool and rois.is_cuda and layer.fused_supported(G) for layer in self.roi_grid_pool_layers]
        out = torch.empty((B * n * G ** 3, self.num_pooled_channels), dtype=torch.float32, device=rois.device)
        composed_inputs = None
        at = 0
        for k, src_name in enumerate(sources):
            layer = self.roi_grid_pool_layers[k]
            sp, stride = self._level(batch_dict, src_name)
            if fused[k]:
                index = sparse_conv_ops.site_index(sp.indices, B, sp.spatial_shape)
                at = layer.forward_fused(rois, G, sp.features, index, stride, self.voxel_size, self.point_cloud_range, out, at)
                continue
            if composed_inputs is None:
                composed_inputs = self._grid_points_and_cells(rois, G)
            pooled = self._pool_level_composed(layer, sp, stride, B, *composed_inputs)
            out[:, at:at + pooled.shape[1]] = pooled
            at += pooled.shape[1]
        return out.view(B * n, G ** 3, self.num_pooled_channels)

    def _grid_points_and_cells(self, rois, grid_size):
        """-> roi_grid_xyz (B, n G^3, 3) and the base-grid cells of the grid points as floats (B, n G^3, 3) (x, y, z)"""
        B = rois.shape[0]
        xyz, _ = self.get_global_grid_points_of_roi(rois, grid_size=grid_size)
        xyz = xyz.view(B, -1, 3)
        r0 = xyz.new_tensor(self.point_cloud_range[0:3])
        vs = xyz.new_tensor(self.voxel_size)
        return xyz, torch.floor((xyz - r0) / vs)

    def _pool_level_composed(self, layer, sp, stride, batch_size, roi_grid_xyz, roi_grid_coords):
        """the reference's formulation of one level (ref :145-187): voxel centres, the dense voxel -> row table, the level's
        cells, NeighborVoxelSAModuleMSG.forward.  Reads the per-sample row counts on the host."""
        coords = sp.indices
        xyz = common_utils.get_voxel_centers(coords[:, 1:4], downsample_times=stride, voxel_size=self.voxel_size,
                                             point_cloud_range=self.point_cloud_range)
        xyz_batch_cnt = torch.bincount(coords[:, 0].long(), minlength=batch_size)[:batch_size].int()
        table = common_utils.generate_voxel2pinds(sp)
        m = roi_grid_xyz.shape[1]
        batch_idx = torch.arange(batch_size, device=coords.device, dtype=roi_grid_coords.dtype).view(-1, 1, 1).expand(-1, m, 1)
        cur = torch.cat([batch_idx, torch.floor(roi_grid_coords / stride)], dim=-1).int()
        grid_cnt = torch.full((batch_size,), m, dtype=torch.int32, device=coords.device)
        return layer(xyz=xyz.contiguous(), xyz_batch_cnt=xyz_batch_cnt, new_xyz=roi_grid_xyz.contiguous().view(-1, 3),
                     new_xyz_batch_cnt=grid_cnt, new_coords=cur.contiguous().view(-1, 4), features=sp.features.contiguous(),
                     voxel2point_indices=table)

    def get_global_grid_points_of_roi(self, rois, grid_size):
        rois = rois.view(-1, rois.shape[-1])
        local = self.get_dense_grid_points(rois, rois.shape[0], grid_size)
        points = common_utils.rotate_points_along_z(local.clone(), rois[:, 6])
        points = points + rois[:, 0:3].unsqueeze(dim=1)
        return points, local

    @staticmethod
    def get_dense_grid_points(rois, batch_size_rcnn, grid_size):
        """(R, G^3, 3): (i + 0.5) / G size - size / 2 per axis, the lattice in nonzero()'s order (x index slowest, z fastest)"""
        dense_idx = rois.new_ones((grid_size, grid_size, grid_size)).nonzero()
        dense_idx = dense_idx.repeat(batch_size_rcnn, 1, 1).float()
        size = rois.view(batch_size_rcnn, -1)[:, 3:6]
        return (dense_idx + 0.5) / grid_size * size.unsqueeze(dim=1) - (size.unsqueeze(dim=1) / 2)

    # ------------------------------------------------------------------ forward

    def forward(self, batch_dict):
        """(ref :217-262) proposals (unless rois are given) -> pooled grid features -> rcnn_cls (R, num_class), rcnn_reg
        (R, code_size).  Eval: batch_cls_preds / batch_box_preds with cls_preds_normalized = False.  Training: the proposals go
        through assign_targets first, the sampled rois are pooled, and forward_ret_dict holds the targets with rcnn_cls and
        rcnn_reg for get_loss."""
        if self.training:
            levels = batch_dict.get('multi_scale_3d_features', None) or {}
            tensors = list(batch_dict.values()) + [getattr(sp, 'features', None) for sp in levels.values()]
            if not any(torch.is_tensor(v) and v.is_cuda for v in tensors):
                raise NotImplementedError('VoxelRCNNHead training on CPU tensors: off the device the RoI-grid pooling has no gradient yet')
            self._require_training_half(type(self).__name__)
        self.proposal_layer(batch_dict, nms_config=_get(self.model_cfg, 'NMS_CONFIG')['TRAIN' if self.training else 'TEST'])
        if self.training:
            targets_dict = self.assign_targets(batch_dict)
            batch_dict['rois'] = targets_dict['rois']
            batch_dict['roi_labels'] = targets_dict['roi_labels']
        pooled = self.roi_grid_pool(batch_dict)
        shared = self.shared_fc_layer(pooled.view(pooled.size(0), -1))
        rcnn_cls = self.cls_pred_layer(self.cls_fc_layers(shared))
        rcnn_reg = self.reg_pred_layer(self.reg_fc_layers(shared))
        if self.training:
            targets_dict['rcnn_cls'] = rcnn_cls
            targets_dict['rcnn_reg'] = rcnn_reg
            self.forward_ret_dict = targets_dict
            return batch_dict
        cls, boxes = self.generate_predicted_boxes(batch_size=batch_dict['batch_size'], rois=batch_dict['rois'], cls_preds=rcnn_cls,
                                                   box_preds=rcnn_reg)
        batch_dict.update(rcnn_cls=rcnn_cls, rcnn_reg=rcnn_reg, batch_cls_preds=cls, batch_box_preds=boxes, cls_preds_normalized=False)
        return batch_dict

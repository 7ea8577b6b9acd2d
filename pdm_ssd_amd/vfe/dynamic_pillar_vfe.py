"""DynamicPillarVFE and PFNLayerV2 of the reference's pcdet/models/backbones_3d/vfe/dynamic_pillar_vfe.py on the device
operators of pillar_ops: same constructor signatures, config keys (USE_NORM, WITH_DISTANCE, USE_ABSLOTE_XYZ, NUM_FILTERS)
and state_dict keys (pfn_layers.{i}.linear.weight, pfn_layers.{i}.norm.*), no torch_scatter, no torch.unique, no
boolean-mask indexing.

forward makes ONE host read per batch, the {kept rows, pillars} pair inside pillar_ops.assign, in eval and in training.
An encoder with a single PFN layer in eval mode runs the fused operator (features -> linear -> folded BatchNorm -> ReLU ->
max per pillar in one launch); every other case runs assign, features and segment_max around nn.Linear / nn.BatchNorm1d.
"""
import torch
import torch.nn as nn

from .. import pillar_ops
from ..config import cfg_get as _get
from .vfe_template import VFETemplate

CELL_TABLE_KEY = 'pillar_cell_table'      # batch_dict key under which forward leaves the (B nx ny) cell table


class PFNLayerV2(nn.Module):
    def __init__(self, in_channels, out_channels, use_norm=True, last_layer=False):
        super().__init__()
        self.last_vfe = last_layer
        self.use_norm = use_norm
        if not self.last_vfe:
            out_channels = out_channels // 2
        if self.use_norm:
            self.linear = nn.Linear(in_channels, out_channels, bias=False)
            self.norm = nn.BatchNorm1d(out_channels, eps=1e-3, momentum=0.01)
        else:
            self.linear = nn.Linear(in_channels, out_channels, bias=True)
        self.relu = nn.ReLU()

    def forward(self, inputs, pillars):
        """inputs (N', C_in), pillars = pillar_ops.assign's result (the reference passes unq_inv alone) -> x_max (P, C_out)
        for the last layer, else [x, x_max[unq_inv]] (N', 2 C_out)"""
        x = self.linear(inputs)
        x = self.norm(x) if self.use_norm else x
        x = self.relu(x)
        x_max = pillar_ops.segment_max(x, pillars)[0]
        if self.last_vfe:
            return x_max
        return torch.cat([x, x_max.index_select(0, pillars.unq_inv)], dim=1)

    def folded(self):
        """(weight (K, C_in), scale (K), shift (K)) of the layer in eval mode: y = relu((W x) * scale + shift); device
        arithmetic only"""
        w = self.linear.weight
        if not self.use_norm:
            return w, torch.ones_like(self.linear.bias), self.linear.bias
        scale = self.norm.weight * torch.rsqrt(self.norm.running_var + self.norm.eps)
        return w, scale, self.norm.bias - self.norm.running_mean * scale


class DynamicPillarVFE(VFETemplate):
    def __init__(self, model_cfg, num_point_features, voxel_size, grid_size, point_cloud_range, **kwargs):
        super().__init__(model_cfg=model_cfg)
        self.use_norm = _get(model_cfg, 'USE_NORM')
        self.with_distance = _get(model_cfg, 'WITH_DISTANCE')
        self.use_absolute_xyz = _get(model_cfg, 'USE_ABSLOTE_XYZ')
        self.num_raw_point_features = num_point_features
        num_point_features += 6 if self.use_absolute_xyz else 3
        if self.with_distance:
            num_point_features += 1
        self.num_filters = _get(model_cfg, 'NUM_FILTERS')
        assert len(self.num_filters) > 0
        num_filters = [num_point_features] + list(self.num_filters)
        pfn_layers = []
        for i in range(len(num_filters) - 1):
            pfn_layers.append(PFNLayerV2(num_filters[i], num_filters[i + 1], self.use_norm, last_layer=(i >= len(num_filters) - 2)))
        self.pfn_layers = nn.ModuleList(pfn_layers)
        self.voxel_size = [float(v) for v in voxel_size]
        self.grid_size = [int(v) for v in grid_size]
        self.point_cloud_range = [float(v) for v in point_cloud_range]
        assert self.grid_size[2] == 1, 'a pillar grid has nz = 1'
        self.geometry = pillar_ops.geometry(self.point_cloud_range, self.voxel_size)

    def get_output_feature_dim(self):
        return self.num_filters[-1]

    def forward(self, batch_dict, **kwargs):
        """batch_dict['points'] (N, 1 + C) rows (batch_idx, x, y, z, ...) in any order, batch_dict['batch_size'] ->
        voxel_features = pillar_features (P, NUM_FILTERS[-1]), voxel_coords (P, 4) int32 (b, 0, cy, cx) in torch.unique's
        order of the reference, and the cell table under CELL_TABLE_KEY for PointPillarScatter.  One host read."""
        points = batch_dict['points']
        assert points.shape[1] == 1 + self.num_raw_point_features, tuple(points.shape)
        pillars = pillar_ops.assign(points, batch_dict['batch_size'], self.point_cloud_range, self.voxel_size, self.grid_size)
        fused = (not self.training and len(self.pfn_layers) == 1
                 and self.pfn_layers[0].linear.in_features <= pillar_ops.MAX_FUSED_FEATURES)
        if fused:
            features = pillar_ops.fused_pfn(points, pillars, self.geometry, *self.pfn_layers[0].folded(),
                                            use_absolute_xyz=self.use_absolute_xyz, with_distance=self.with_distance)
        else:
            features = pillar_ops.features(points, pillars, self.geometry, self.use_absolute_xyz, self.with_distance)
            for pfn in self.pfn_layers:
                features = pfn(features, pillars)
        batch_dict['voxel_features'] = batch_dict['pillar_features'] = features
        batch_dict['voxel_coords'] = pillars.voxel_coords
        batch_dict[CELL_TABLE_KEY] = pillars.cell_table
        return batch_dict

"""PFNLayer and PillarVFE of the reference's pcdet/models/backbones_3d/vfe/pillar_vfe.py: same constructor signatures, config
keys (USE_NORM, WITH_DISTANCE, USE_ABSLOTE_XYZ, NUM_FILTERS) and state_dict keys (pfn_layers.{i}.linear.weight,
pfn_layers.{i}.norm.*), so a PointPillars checkpoint trained on hard voxels loads and computes what it was trained on.
Registered as `HardPillarVFE` (vfe/__init__.py says why).

forward takes either contract:
  * batch_dict already holds `voxels`, `voxel_num_points` and `voxel_coords` (the reference's): they are used as given and
    the reference's formulation runs in torch on the device, no host read;
  * otherwise batch_dict['points'] is voxelized on the device (hard_voxel_ops.voxelize, ONE host read) with
    MAX_POINTS_PER_VOXEL and MAX_NUMBER_OF_VOXELS from this module's own config.  One PFN layer in eval mode with at most
    16 input columns runs the fused operator (no (M, T, F) or (M, T, K) tensor); every other case (training, several
    layers, wider inputs) materialises `voxels` and runs the reference's formulation under autograd, where the BatchNorm's
    batch statistics include the zero-masked padding rows, as in the reference.

Two deliberate differences from the reference: pillar_features is (M, K) for every M (`squeeze(1)`; the reference's bare
`squeeze()` returns (K,) at M = 1), and the linear layer is not split into parts of 50 000 voxels.
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import hard_voxel_ops
from ..config import cfg_get as _get
from .mean_vfe import has_voxels, voxelizer_caps
from .vfe_template import VFETemplate


def pinned_norm(xyz):
    """|xyz| over the last axis, keepdim, as sqrt(fma(z, z, fma(y, y, x * x))) in fp32: the rounding sequence of torch.norm's
    CPU kernel on three elements, which the reference's fixtures record and the fused operator pins (pl_derived).  The
    device's torch.norm rounds otherwise by an ulp.  Each step is taken in double and rounded to fp32 once: a product of two
    fp32 values is exact in double, and a double square root rounded to fp32 is the correctly rounded fp32 one."""
    x, y, z = (xyz[..., i].double() for i in range(3))
    acc = (x * x).float().double()
    acc = (y * y + acc).float().double()
    acc = (z * z + acc).float().double()
    return torch.sqrt(acc).to(xyz.dtype).unsqueeze(-1)


class PFNLayer(nn.Module):
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

    def forward(self, inputs):
        """inputs (M, T, C_in) -> (M, 1, C_out) for the last layer, else [x, max over T repeated] (M, T, 2 C_out)"""
        x = self.linear(inputs)
        x = self.norm(x.permute(0, 2, 1)).permute(0, 2, 1) if self.use_norm else x
        x = F.relu(x)
        x_max = torch.max(x, dim=1, keepdim=True)[0]
        if self.last_vfe:
            return x_max
        return torch.cat([x, x_max.repeat(1, inputs.shape[1], 1)], dim=2)

    def folded(self):
        """(weight (K, C_in), scale (K), shift (K)) of the layer in eval mode: y = relu((W x) * scale + shift); device
        arithmetic only"""
        w = self.linear.weight
        if not self.use_norm:
            return w, torch.ones_like(self.linear.bias), self.linear.bias
        scale = self.norm.weight * torch.rsqrt(self.norm.running_var + self.norm.eps)
        return w, scale, self.norm.bias - self.norm.running_mean * scale


class PillarVFE(VFETemplate):
    def __init__(self, model_cfg, num_point_features, voxel_size, point_cloud_range, grid_size=None, **kwargs):
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
            pfn_layers.append(PFNLayer(num_filters[i], num_filters[i + 1], self.use_norm, last_layer=(i >= len(num_filters) - 2)))
        self.pfn_layers = nn.ModuleList(pfn_layers)
        self.voxel_size = [float(v) for v in voxel_size]
        self.point_cloud_range = [float(v) for v in point_cloud_range]
        self.grid_size = None if grid_size is None else [int(v) for v in grid_size]
        self.geometry = hard_voxel_ops.geometry(self.point_cloud_range, self.voxel_size)

    def get_output_feature_dim(self):
        return self.num_filters[-1]

    def features_of(self, voxels, voxel_num_points, coords):
        """the (M, T, F) rows the first PFN layer receives, in the reference's formulation: the mean is the sum over all T
        slots (padding is zero) divided by the count, the cell centre is float(cell) * voxel + offset with the product and the
        sum rounded separately, and padding rows are masked to zero AFTER the columns are built"""
        g = self.geometry
        xyz = voxels[:, :, :3]
        mean = xyz.sum(dim=1, keepdim=True) / voxel_num_points.type_as(voxels).view(-1, 1, 1)
        cell = coords[:, [3, 2, 1]].to(voxels.dtype)                               # (cx, cy, cz)
        centre = torch.stack([cell[:, 0] * g.vx + g.x_offset, cell[:, 1] * g.vy + g.y_offset, cell[:, 2] * g.vz + g.z_offset], dim=1)
        columns = [voxels if self.use_absolute_xyz else voxels[..., 3:], xyz - mean, xyz - centre[:, None, :]]
        if self.with_distance:
            columns.append(pinned_norm(xyz))
        real = torch.arange(voxels.shape[1], device=voxels.device)[None, :] < voxel_num_points[:, None]
        return torch.cat(columns, dim=-1) * real[:, :, None].type_as(voxels)

    def composed(self, voxels, voxel_num_points, coords):
        """the reference's formulation on the padded tensor -> (M, K)"""
        features = self.features_of(voxels, voxel_num_points, coords)
        for pfn in self.pfn_layers:
            features = pfn(features)
        return features.squeeze(1)

    def forward(self, batch_dict, **kwargs):
        """-> pillar_features = voxel_features (M, NUM_FILTERS[-1]), voxel_coords (M, 4) int32 (b, cz, cy, cx),
        voxel_num_points (M)"""
        batch_dict.pop('pillar_cell_table', None)       # a dynamic encoder's table would not describe these voxels
        if has_voxels(batch_dict):
            features = self.composed(batch_dict['voxels'], batch_dict['voxel_num_points'], batch_dict['voxel_coords'])
            batch_dict['voxel_features'] = batch_dict['pillar_features'] = features
            return batch_dict
        T, max_voxels = voxelizer_caps(self.model_cfg, self.training, 'PillarVFE')
        assert self.grid_size is not None, 'PillarVFE: voxelizing needs grid_size'
        points = batch_dict['points']
        assert points.shape[1] == 1 + self.num_raw_point_features, tuple(points.shape)
        fused = (not self.training and len(self.pfn_layers) == 1
                 and self.pfn_layers[0].linear.in_features <= hard_voxel_ops.MAX_FUSED_FEATURES)
        hv = hard_voxel_ops.voxelize(points, batch_dict['batch_size'], self.point_cloud_range, self.voxel_size, self.grid_size, T, max_voxels,
                                     materialize=not fused)
        if fused:
            features = hard_voxel_ops.fused_pfn(points, hv, self.geometry, *self.pfn_layers[0].folded(),
                                                use_absolute_xyz=self.use_absolute_xyz, with_distance=self.with_distance)
        else:
            features = self.composed(hv.voxels, hv.voxel_num_points, hv.voxel_coords)
        batch_dict['voxel_features'] = batch_dict['pillar_features'] = features
        batch_dict['voxel_coords'] = hv.voxel_coords
        batch_dict['voxel_num_points'] = hv.voxel_num_points
        return batch_dict

"""DynamicMeanVFE of the reference's pcdet/models/backbones_3d/vfe/dynamic_mean_vfe.py on sparse_conv_ops.voxel_assign: same
constructor signature and outputs, no torch_scatter, no torch.unique, no boolean-mask indexing.  It has no parameters.

forward makes ONE host read per batch, the {kept rows, voxels} pair inside voxel_assign.  voxel_features (P, C) is the mean of
every point column over the voxel, voxel_coords (P, 4) int32 (b, cz, cy, cx) in torch.unique's order of the reference's
merge_coords (x-major, z innermost).
"""
import torch

from .. import sparse_conv_ops
from .vfe_template import VFETemplate


class DynamicMeanVFE(VFETemplate):
    def __init__(self, model_cfg, num_point_features, voxel_size, grid_size, point_cloud_range, **kwargs):
        super().__init__(model_cfg=model_cfg)
        self.num_point_features = num_point_features
        self.voxel_size = [float(v) for v in voxel_size]
        self.grid_size = [int(v) for v in grid_size]
        self.point_cloud_range = [float(v) for v in point_cloud_range]

    def get_output_feature_dim(self):
        return self.num_point_features

    @torch.no_grad()
    def forward(self, batch_dict, **kwargs):
        points = batch_dict['points']
        assert points.shape[1] == 1 + self.num_point_features, tuple(points.shape)
        voxels = sparse_conv_ops.voxel_assign(points, batch_dict['batch_size'], self.point_cloud_range, self.voxel_size, self.grid_size)
        batch_dict['voxel_features'] = voxels.voxel_mean
        batch_dict['voxel_coords'] = voxels.voxel_coords
        return batch_dict

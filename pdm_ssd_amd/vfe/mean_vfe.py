"""MeanVFE of the reference's pcdet/models/backbones_3d/vfe/mean_vfe.py: the mean of every point column over a hard voxel's
kept points.  It has no parameters.  Registered as `HardMeanVFE` (vfe/__init__.py says why).

forward takes either contract:
  * batch_dict already holds `voxels`, `voxel_num_points` and `voxel_coords` (the reference's: its dataset voxelized on the
    CPU): they are used as given, with the reference's formulation in torch on the device, no host read;
  * otherwise batch_dict['points'] is voxelized on the device (hard_voxel_ops.voxelize, ONE host read) with
    MAX_POINTS_PER_VOXEL and MAX_NUMBER_OF_VOXELS from this module's own config, where the reference keeps them in the
    dataset's `transform_points_to_voxels` step, and the mean is taken from the slots without the padded tensor.
"""
import torch

from .. import hard_voxel_ops
from ..config import cfg_get as _get
from .vfe_template import VFETemplate


def voxelizer_caps(model_cfg, training, who):
    """(MAX_POINTS_PER_VOXEL, MAX_NUMBER_OF_VOXELS for this mode) of a hard-voxel encoder's config; MAX_NUMBER_OF_VOXELS is an
    int or {'train': ..., 'test': ...}.  A missing key is a ValueError that names it."""
    caps = []
    for key in ('MAX_POINTS_PER_VOXEL', 'MAX_NUMBER_OF_VOXELS'):
        value = _get(model_cfg, key, None)
        if value is None:
            raise ValueError(f"{who}: batch_dict holds no `voxels` and the config has no {key}: the voxelizer's sizes live in this "
                             "module's config (the reference keeps them in the dataset's transform_points_to_voxels step)")
        caps.append(value)
    max_voxels = caps[1]
    if not isinstance(max_voxels, int):
        mode = 'train' if training else 'test'
        max_voxels = _get(max_voxels, mode, None)
        if max_voxels is None:
            raise ValueError(f"{who}: MAX_NUMBER_OF_VOXELS has no '{mode}' entry")
    return int(caps[0]), int(max_voxels)


def has_voxels(batch_dict):
    return all(batch_dict.get(k, None) is not None for k in ('voxels', 'voxel_num_points', 'voxel_coords'))


class MeanVFE(VFETemplate):
    def __init__(self, model_cfg, num_point_features, voxel_size=None, grid_size=None, point_cloud_range=None, **kwargs):
        super().__init__(model_cfg=model_cfg)
        self.num_point_features = num_point_features
        self.voxel_size = None if voxel_size is None else [float(v) for v in voxel_size]
        self.grid_size = None if grid_size is None else [int(v) for v in grid_size]
        self.point_cloud_range = None if point_cloud_range is None else [float(v) for v in point_cloud_range]

    def get_output_feature_dim(self):
        return self.num_point_features

    @torch.no_grad()
    def forward(self, batch_dict, **kwargs):
        """-> voxel_features (M, C), voxel_coords (M, 4) int32 (b, cz, cy, cx), voxel_num_points (M)"""
        if has_voxels(batch_dict):
            voxels, num = batch_dict['voxels'], batch_dict['voxel_num_points']
            normalizer = torch.clamp_min(num.view(-1, 1), min=1.0).type_as(voxels)
            batch_dict['voxel_features'] = (voxels.sum(dim=1, keepdim=False) / normalizer).contiguous()
            return batch_dict
        T, max_voxels = voxelizer_caps(self.model_cfg, self.training, 'MeanVFE')
        assert self.grid_size is not None, 'MeanVFE: voxelizing needs voxel_size, grid_size and point_cloud_range'
        points = batch_dict['points']
        assert points.shape[1] == 1 + self.num_point_features, tuple(points.shape)
        hv = hard_voxel_ops.voxelize(points, batch_dict['batch_size'], self.point_cloud_range, self.voxel_size, self.grid_size, T, max_voxels)
        batch_dict['voxel_features'] = hard_voxel_ops.voxel_mean(points, hv)
        batch_dict['voxel_coords'] = hv.voxel_coords
        batch_dict['voxel_num_points'] = hv.voxel_num_points
        return batch_dict

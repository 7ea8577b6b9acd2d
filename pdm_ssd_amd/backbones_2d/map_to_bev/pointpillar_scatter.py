"""PointPillarScatter of the reference's pcdet/models/backbones_2d/map_to_bev/pointpillar_scatter.py on
pillar_ops.scatter: one launch writes the whole (B, C, ny, nx) canvas, zeros included, instead of a memset and a Python
loop over the samples; no host read.

One deliberate difference: the batch size is batch_dict['batch_size'].  The reference reads coords[:, 0].max().item() + 1,
a host synchronisation that also shrinks the batch when the last sample owns no pillar.

PointPillarScatter3d is the scatter behind DSVT: INPUT_SHAPE (nx, ny, nz) comes from the config, and NUM_BEV_FEATURES // nz
channels a voxel are folded with z into the channel axis.  With nz = 1 on the GPU it is the launch above on a cell table
built from the coordinates it is given (a multi-stage DSVT has pooled the VFE's voxels away); with nz > 1, and on the CPU, it
is the reference's formulation in torch operators, all samples in one indexed assignment.
"""
import torch
import torch.nn as nn

from ... import pillar_ops
from ...config import cfg_get as _get

CELL_TABLE_KEY = 'pillar_cell_table'


class PointPillarScatter(nn.Module):
    def __init__(self, model_cfg, grid_size, **kwargs):
        super().__init__()
        self.model_cfg = model_cfg
        self.num_bev_features = _get(model_cfg, 'NUM_BEV_FEATURES')
        self.nx, self.ny, self.nz = (int(v) for v in grid_size)
        assert self.nz == 1

    def forward(self, batch_dict, **kwargs):
        """pillar_features (P, C), voxel_coords (P, 4) (b, 0, cy, cx) -> spatial_features (B, C, ny, nx).  The cell table
        is the VFE's when it left one (CELL_TABLE_KEY), else it is built from voxel_coords on the device."""
        pillar_features, coords = batch_dict['pillar_features'], batch_dict['voxel_coords']
        assert pillar_features.shape[1] == self.num_bev_features, tuple(pillar_features.shape)
        batch_size, grid = int(batch_dict['batch_size']), (self.nx, self.ny, self.nz)
        table = batch_dict.get(CELL_TABLE_KEY, None)
        if table is None:
            table = pillar_ops.cell_table_from_coords(coords, batch_size, grid)
        batch_dict['spatial_features'] = pillar_ops.scatter(pillar_features.float(), table, coords.int(), batch_size, grid)
        return batch_dict


class PointPillarScatter3d(nn.Module):
    def __init__(self, model_cfg, grid_size, **kwargs):
        super().__init__()
        self.model_cfg = model_cfg
        self.nx, self.ny, self.nz = (int(v) for v in _get(model_cfg, 'INPUT_SHAPE'))
        self.num_bev_features = _get(model_cfg, 'NUM_BEV_FEATURES')
        self.num_bev_features_before_compression = self.num_bev_features // self.nz

    def forward(self, batch_dict, **kwargs):
        """pillar_features (P, C), voxel_coords (P, 4) (b, z, y, x) -> spatial_features (B, C nz, ny, nx), channel c nz + z"""
        pillar_features, coords = batch_dict['pillar_features'], batch_dict['voxel_coords']
        C, batch_size = self.num_bev_features_before_compression, int(batch_dict['batch_size'])
        assert pillar_features.shape[1] == C, tuple(pillar_features.shape)
        if self.nz == 1 and pillar_features.is_cuda:
            grid = (self.nx, self.ny, 1)
            table = pillar_ops.cell_table_from_coords(coords, batch_size, grid)
            batch_dict['spatial_features'] = pillar_ops.scatter(pillar_features.float(), table, coords.int(), batch_size, grid)
            return batch_dict
        c = coords.long()
        canvas = pillar_features.new_zeros((batch_size, C, self.nz * self.ny * self.nx))
        canvas[c[:, 0], :, (c[:, 1] * self.ny + c[:, 2]) * self.nx + c[:, 3]] = pillar_features
        batch_dict['spatial_features'] = canvas.view(batch_size, C * self.nz, self.ny, self.nx)
        return batch_dict

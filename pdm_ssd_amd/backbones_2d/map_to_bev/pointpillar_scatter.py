"""PointPillarScatter of the reference's pcdet/models/backbones_2d/map_to_bev/pointpillar_scatter.py on
pillar_ops.scatter: one launch writes the whole (B, C, ny, nx) canvas, zeros included, instead of a memset and a Python
loop over the samples; no host read.

One deliberate difference: the batch size is batch_dict['batch_size'].  The reference reads coords[:, 0].max().item() + 1,
a host synchronisation that also shrinks the batch when the last sample owns no pillar.
"""
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

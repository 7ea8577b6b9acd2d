"""DynamicPillarVFESimple2D of the reference's pcdet/models/backbones_3d/vfe/dynamic_pillar_vfe.py on the device operators of
pillar_ops: the pillar encoder in front of the sparse 2-D backbones (PillarNet).  Same constructor signature, config keys
(USE_NORM, WITH_DISTANCE, USE_ABSLOTE_XYZ, NUM_FILTERS) and state_dict keys (pfn_layers.{i}.linear.weight, pfn_layers.{i}.norm.*)
as the reference's; PFNLayerV2 is DynamicPillarVFE's.

The cell rule (x and y tested, z not) and the pillar order b nx ny + cx ny + cy are DynamicPillarVFE's, so pdm_pillar_assign
serves as it is.  The features differ: [f_center (x, y from the cell centre, z - z_offset) | points[:, 1:] or points[:, 4:] |
|xyz| when WITH_DISTANCE], no cluster term.  The outputs are pillar_features (P, NUM_FILTERS[-1]) and pillar_coords (P, 3) int32
(b, y, x), the rows a 2-D SparseConvTensor takes.

One host read per batch (pillar_ops.assign), in eval and in training.  A single PFN layer in eval mode runs
pdm_pillar_fused_pfn unchanged: that kernel's columns are [raw | f_cluster | f_center | |xyz|], so the layer's weight columns are
permuted into that order with zeros on the three cluster columns; a zero weight leaves the value of the kernel's fma chain
unchanged (the pillar means are finite whenever the points are).  Every other case runs pdm_pillar_features, drops the cluster
columns and reorders by one index_select, then nn.Linear / nn.BatchNorm1d and pdm_pillar_segment_max, as DynamicPillarVFE does.
"""
import torch
import torch.nn as nn

from .. import pillar_ops
from ..config import cfg_get as _get
from .dynamic_pillar_vfe import PFNLayerV2
from .vfe_template import VFETemplate


class DynamicPillarVFESimple2D(VFETemplate):
    def __init__(self, model_cfg, num_point_features, voxel_size, grid_size, point_cloud_range, **kwargs):
        super().__init__(model_cfg=model_cfg)
        self.use_norm = _get(model_cfg, 'USE_NORM')
        self.with_distance = _get(model_cfg, 'WITH_DISTANCE')
        self.use_absolute_xyz = _get(model_cfg, 'USE_ABSLOTE_XYZ')
        self.num_raw_point_features = num_point_features
        if self.use_absolute_xyz:
            num_point_features += 3
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
        # column c of this encoder's features is column kernel_columns[c] of pdm_pillar_features: [raw | cluster | center | dist]
        nraw = self.num_raw_point_features if self.use_absolute_xyz else self.num_raw_point_features - 3
        self.kernel_columns = [nraw + 3, nraw + 4, nraw + 5] + list(range(nraw)) + ([nraw + 6] if self.with_distance else [])
        self.num_kernel_columns = nraw + 6 + (1 if self.with_distance else 0)
        self.register_buffer('column_index', torch.tensor(self.kernel_columns, dtype=torch.long), persistent=False)
        self._cache = None

    def get_output_feature_dim(self):
        return self.num_filters[-1]

    def _fused_weight(self):
        """the single layer's folded (weight, scale, shift) with the weight's columns in the kernel's order and zeros on the
        cluster columns, made once per version of the layer's tensors"""
        layer = self.pfn_layers[0]
        sources = [layer.linear.weight, layer.linear.bias] + ([layer.norm.weight, layer.norm.bias, layer.norm.running_mean,
                                                               layer.norm.running_var] if self.use_norm else [])
        key = tuple((t.data_ptr(), t._version) for t in sources if t is not None)
        if self._cache is None or self._cache[0] != key:
            with torch.no_grad():
                w, scale, shift = layer.folded()
                wk = torch.zeros((w.shape[0], self.num_kernel_columns), dtype=w.dtype, device=w.device)
                wk[:, self.kernel_columns] = w
                self._cache = (key, (wk, scale.contiguous(), shift.contiguous()))
        return self._cache[1]

    def forward(self, batch_dict, **kwargs):
        """batch_dict['points'] (N, 1 + C) rows (batch_idx, x, y, z, ...) in any order, batch_dict['batch_size'] ->
        pillar_features (P, NUM_FILTERS[-1]) and pillar_coords (P, 3) int32 (b, cy, cx), in torch.unique's order of the
        reference's merged key.  One host read."""
        points = batch_dict['points']
        assert points.shape[1] == 1 + self.num_raw_point_features, tuple(points.shape)
        pillars = pillar_ops.assign(points, batch_dict['batch_size'], self.point_cloud_range, self.voxel_size, self.grid_size)
        fused = (not self.training and len(self.pfn_layers) == 1 and self.num_kernel_columns <= pillar_ops.MAX_FUSED_FEATURES)
        if fused:
            features = pillar_ops.fused_pfn(points, pillars, self.geometry, *self._fused_weight(),
                                            use_absolute_xyz=self.use_absolute_xyz, with_distance=self.with_distance)
        else:
            features = pillar_ops.features(points, pillars, self.geometry, self.use_absolute_xyz, self.with_distance)
            features = features.index_select(1, self.column_index)
            for pfn in self.pfn_layers:
                features = pfn(features, pillars)
        batch_dict['pillar_features'] = features
        batch_dict['pillar_coords'] = pillars.voxel_coords[:, [0, 2, 3]].contiguous()
        return batch_dict

"""NeighborVoxelSAModuleMSG of the reference's pcdet/ops/pointnet2/pointnet2_stack/voxel_pool_modules.py: the same
constructor, `forward` signature and state_dict keys (groupers, mlps_in, mlps_pos, mlps_out).

Two paths compute the same thing:
  * forward(): the reference's own formulation on the operators this package already has (VoxelQueryAndGrouping over a dense
    voxel -> row table, two grouped tensors, Conv2d + BatchNorm2d on the offsets, ReLU, pooling, the output layer).  It is the
    on-device checker of the fused operator and the path for what that operator refuses (avg_pool, other widths, training).
  * forward_fused(): one contraction for mlps_in over the level's rows and ONE launch of pdm_roi_grid_pool per scale
    (csrc/roi_grid_pool.hip), which writes straight into its columns of the caller's output rows.  Eval mode
    only; no host read.  The folded and packed weights are cached per parameter version.
"""
from typing import List

import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import sparse_conv_ops
from . import voxel_query_utils

FUSED_WIDTHS = (16, 32, 64)
FUSED_MAX_RANGE, FUSED_MAX_NSAMPLE, FUSED_MAX_GRID = 4, 32, 8


def _fold(norm):
    """eval BatchNorm -> (scale, shift) of one multiply-add per channel"""
    scale = norm.weight * torch.rsqrt(norm.running_var + norm.eps)
    return scale, norm.bias - norm.running_mean * scale


class NeighborVoxelSAModuleMSG(nn.Module):

    def __init__(self, *, query_ranges: List[List[int]], radii: List[float], nsamples: List[int], mlps: List[List[int]],
                 use_xyz: bool = True, pool_method='max_pool'):
        """query_ranges: per scale the (z, y, x) half-widths of the voxel window; radii, nsamples: per scale; mlps: per scale
        [C_in, C1, C2]; pool_method: max_pool / avg_pool"""
        super().__init__()
        assert len(query_ranges) == len(nsamples) == len(mlps)
        self.groupers = nn.ModuleList()
        self.mlps_in = nn.ModuleList()
        self.mlps_pos = nn.ModuleList()
        self.mlps_out = nn.ModuleList()
        for i in range(len(query_ranges)):
            self.groupers.append(voxel_query_utils.VoxelQueryAndGrouping(query_ranges[i], radii[i], nsamples[i]))
            spec = mlps[i]
            self.mlps_in.append(nn.Sequential(nn.Conv1d(spec[0], spec[1], kernel_size=1, bias=False), nn.BatchNorm1d(spec[1])))
            self.mlps_pos.append(nn.Sequential(nn.Conv2d(3, spec[1], kernel_size=1, bias=False), nn.BatchNorm2d(spec[1])))
            self.mlps_out.append(nn.Sequential(nn.Conv1d(spec[1], spec[2], kernel_size=1, bias=False), nn.BatchNorm1d(spec[2]), nn.ReLU()))
        self.relu = nn.ReLU()
        self.pool_method = pool_method
        self._cache = {}        # scale -> (parameter versions, folded and packed tensors)
        self.init_weights()

    def init_weights(self):
        for m in self.modules():
            if isinstance(m, (nn.Conv2d, nn.Conv1d)):
                nn.init.kaiming_normal_(m.weight)
                if m.bias is not None:
                    nn.init.constant_(m.bias, 0)
            if isinstance(m, (nn.BatchNorm2d, nn.BatchNorm1d)):
                nn.init.constant_(m.weight, 1.0)
                nn.init.constant_(m.bias, 0)

    def out_channels(self):
        return [m[0].out_channels for m in self.mlps_out]

    # ------------------------------------------------------------------ the composed formulation

    def forward(self, xyz, xyz_batch_cnt, new_xyz, new_xyz_batch_cnt, new_coords, features, voxel2point_indices):
        """xyz (N1 + N2 ..., 3) voxel centres, xyz_batch_cnt (B), new_xyz (M1 + M2 ..., 3) grid points, new_xyz_batch_cnt (B),
        new_coords (M1 + M2 ..., 4) [batch_idx, x, y, z] cells of the grid points, features (N1 + N2 ..., C),
        voxel2point_indices (B, Z, Y, X) -> (M1 + M2 ..., sum of the scales' C2)"""
        new_coords = new_coords[:, [0, 3, 2, 1]].contiguous()       # -> [batch_idx, z, y, x]
        new_features_list = []
        for k in range(len(self.groupers)):
            features_in = self.mlps_in[k](features.permute(1, 0).unsqueeze(0))
            features_in = features_in.permute(0, 2, 1).contiguous()
            features_in = features_in.view(-1, features_in.shape[-1])
            grouped_features, grouped_xyz, empty_ball_mask = self.groupers[k](
                new_coords, xyz, xyz_batch_cnt, new_xyz, new_xyz_batch_cnt, features_in, voxel2point_indices)
            empty = empty_ball_mask.view(-1, 1, 1)      # (masked_fill: a boolean-mask assignment would read the mask's count back)
            grouped_features = grouped_features.masked_fill(empty, 0)
            grouped_features = grouped_features.permute(1, 0, 2).unsqueeze(dim=0)       # (1, C, M, nsample)
            grouped_xyz = (grouped_xyz - new_xyz.unsqueeze(-1)).masked_fill(empty, 0)
            grouped_xyz = grouped_xyz.permute(1, 0, 2).unsqueeze(0)                     # (1, 3, M, nsample)
            position_features = self.mlps_pos[k](grouped_xyz)
            new_features = self.relu(grouped_features + position_features)
            if self.pool_method == 'max_pool':
                new_features = F.max_pool2d(new_features, kernel_size=[1, new_features.size(3)]).squeeze(dim=-1)
            elif self.pool_method == 'avg_pool':
                new_features = F.avg_pool2d(new_features, kernel_size=[1, new_features.size(3)]).squeeze(dim=-1)
            else:
                raise NotImplementedError
            new_features = self.mlps_out[k](new_features)
            new_features_list.append(new_features.squeeze(dim=0).permute(1, 0))
        return torch.cat(new_features_list, dim=1)

    # ------------------------------------------------------------------ the fused operator

    def fused_supported(self, grid_size):
        """whether pdm_roi_grid_pool (and the mlps_in contraction) serves every scale of this module"""
        if self.training or self.pool_method != 'max_pool' or not 1 <= int(grid_size) <= FUSED_MAX_GRID:
            return False
        for k, g in enumerate(self.groupers):
            cin, c1, c2 = self.mlps_in[k][0].in_channels, self.mlps_in[k][0].out_channels, self.mlps_out[k][0].out_channels
            if cin not in sparse_conv_ops.CIN_SUPPORTED or c1 not in FUSED_WIDTHS or c2 not in FUSED_WIDTHS:
                return False
            if len(g.max_range) != 3 or any(not 0 <= int(r) <= FUSED_MAX_RANGE for r in g.max_range):
                return False
            if not 1 <= int(g.nsample) <= FUSED_MAX_NSAMPLE or not float(g.radius) >= 0:
                return False
        return True

    def _folded(self, k):
        """the scale's folded and packed tensors, made once per version of its parameters and buffers (as
        spconv.SparseConvolution._cached keys its packs)"""
        mods = (self.mlps_in[k], self.mlps_pos[k], self.mlps_out[k])
        sources = [t for m in mods for t in (m[0].weight, m[1].weight, m[1].bias, m[1].running_mean, m[1].running_var)]
        key = tuple((t.data_ptr(), t._version) for t in sources)
        hit = self._cache.get(k)
        if hit is None or hit[0] != key:
            with torch.no_grad():
                w_in, w_pos, w_out = (m[0].weight.detach().float() for m in mods)
                c1, cin = w_in.shape[0], w_in.shape[1]
                f = {'w_in': sparse_conv_ops.pack_weight(w_in.reshape(c1, 1, 1, 1, cin)),
                     'w_pos': w_pos.reshape(c1, 3).contiguous(),
                     'w_out': sparse_conv_ops.pack_weight(w_out.reshape(w_out.shape[0], 1, 1, 1, c1))}
                for name, m in zip(('in', 'pos', 'out'), mods):
                    f['scale_' + name], f['shift_' + name] = (t.float().contiguous() for t in _fold(m[1]))
            hit = (key, f)
            self._cache[k] = hit
        return hit[1]

    @torch.no_grad()
    def forward_fused(self, rois, grid_size, features, index, stride, voxel_size, point_cloud_range, out, out_offset=0):
        """rois (B, n, 7 + ...), the level's features (P, C) and its sparse_conv_ops.site_index -> this module's columns
        [out_offset, out_offset + sum of C2) of out (B n G^3, row stride); returns the offset behind them."""
        assert self.fused_supported(grid_size), 'forward_fused: a configuration the fused operator refuses; use forward()'
        features = features.float().contiguous()
        P = features.shape[0]
        rows = torch.arange(P, dtype=torch.int32, device=features.device).view(P, 1)       # kvol = 1: every row reads itself
        for k, g in enumerate(self.groupers):
            f = self._folded(k)
            cin, c1, c2 = self.mlps_in[k][0].in_channels, self.mlps_in[k][0].out_channels, self.mlps_out[k][0].out_channels
            features_in = sparse_conv_ops.sparse_conv(features, rows, f['w_in'], cin, c1, f['scale_in'], f['shift_in'])
            sparse_conv_ops.roi_grid_pool(rois, grid_size, index, stride, voxel_size, point_cloud_range, features_in, f['w_pos'],
                                          f['scale_pos'], f['shift_pos'], g.max_range, g.radius, g.nsample, f['w_out'], f['scale_out'],
                                          f['shift_out'], c2, out=out, out_offset=out_offset)
            out_offset += c2
        return out_offset

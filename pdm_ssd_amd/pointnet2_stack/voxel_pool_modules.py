"""NeighborVoxelSAModuleMSG of the reference's pcdet/ops/pointnet2/pointnet2_stack/voxel_pool_modules.py: the same
constructor, `forward` signature and state_dict keys (groupers, mlps_in, mlps_pos, mlps_out).

Two paths compute the same thing:
  * forward(): the reference's own formulation on the operators this package already has (VoxelQueryAndGrouping over a dense
    voxel -> row table, two grouped tensors, Conv2d + BatchNorm2d on the offsets, ReLU, pooling, the output layer).  It is the
    on-device checker of the fused operators and the path for what they refuse (avg_pool, other widths).
  * forward_fused(): one contraction for mlps_in over the level's rows and ONE launch of pdm_roi_grid_pool per scale
    (csrc/roi_grid_pool.hip), which writes straight into its columns of the caller's output rows.  The eval
    form; no host read.  The folded and packed weights are cached per parameter version.
  * forward_fused_train(): the training form (csrc/roi_grid_train.hip).  mlps_in and mlps_out are the modules
    themselves (batch statistics over the level's rows and over the pooled rows); per scale one query that keeps the groups
    and the moments of the padded offsets, the position BatchNorm's batch statistics from those moments under autograd, and
    the autograd node RoIGridPoolFunction.  No dense table, no grouped tensor, no host read.
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

    def _within_fused_limits(self, grid_size):
        """the configurations the fused operators serve, eval and training form alike"""
        if self.pool_method != 'max_pool' or not 1 <= int(grid_size) <= FUSED_MAX_GRID:
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

    def fused_supported(self, grid_size):
        """whether pdm_roi_grid_pool (and the mlps_in contraction) serves every scale of this module: eval mode only"""
        return not self.training and self._within_fused_limits(grid_size)

    def fused_train_supported(self, grid_size):
        """whether forward_fused_train serves every scale of this module: fused_supported()'s limits, in training mode"""
        return self.training and self._within_fused_limits(grid_size)

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

    # ------------------------------------------------------------------ the fused operator, training

    @staticmethod
    def _position_norm(conv, norm, moments, num_slots):
        """Training-mode BatchNorm2d behind Conv2d(3 -> C1) over the padded (1, 3, M, nsample) offsets, from the nine moments of
        those offsets: the layer is linear, so mean_c = W[c] . mean and var_c = W[c]^T Cov W[c].  The moments are float64
        constants, the weight is under autograd, so the gradient runs through the statistics as BatchNorm's own backward does.
        Updates the running statistics as nn.BatchNorm2d would (unbiased variance, momentum None = cumulative average).
        -> (scale_p, shift_p) fp32 with position term = dot(W[c], d) scale_p[c] + shift_p[c]."""
        w = conv.weight.reshape(conv.out_channels, 3)
        n = float(num_slots)
        m = moments / n                                                     # (9) float64, no gradient
        mean3 = m[0:3]
        second = torch.stack([m[3], m[4], m[5], m[4], m[6], m[7], m[5], m[7], m[8]]).view(3, 3)
        cov = second - mean3.view(3, 1) * mean3.view(1, 3)
        wd = w.double()
        mean = (wd @ mean3).to(w.dtype)
        var = ((wd @ cov) * wd).sum(1).clamp_min(0).to(w.dtype)
        if norm.track_running_stats and norm.running_mean is not None:
            with torch.no_grad():
                norm.num_batches_tracked += 1
                factor = 1.0 / norm.num_batches_tracked.to(torch.float64) if norm.momentum is None else norm.momentum
                unbiased = var.detach() * (n / max(n - 1.0, 1.0))
                norm.running_mean += (mean.detach() - norm.running_mean) * factor
                norm.running_var += (unbiased - norm.running_var) * factor
        scale = torch.rsqrt(var + norm.eps)
        if norm.weight is not None:
            scale = scale * norm.weight
        shift = -mean * scale
        if norm.bias is not None:
            shift = shift + norm.bias
        return scale, shift

    def forward_fused_train(self, rois, grid_size, features, index, stride, voxel_size, point_cloud_range):
        """rois (B, n, 7 + ...), detached as the reference's (its targets come from no_grad); the level's features (P, C) and its
        sparse_conv_ops.site_index -> (B n G^3, sum of C2) under autograd in the features and in every parameter of the module."""
        assert self.fused_train_supported(grid_size), 'forward_fused_train: a configuration the fused operator refuses; use forward()'
        if features.is_cuda and torch.cuda.is_current_stream_capturing():
            # The three operators are captured and replayed bit for bit on their own (tests); a capture of this method with
            # its backward (torch's training BatchNorm, the autograd thread calling pdm_roi_grid_pool_grad) has ended in a
            # fault of the process at the end of the capture and is refused until its cause is known.
            raise RuntimeError('forward_fused_train cannot be captured in a graph: capture the operators of sparse_conv_ops '
                               '(roi_grid_query, roi_grid_pool_train, roi_grid_pool_grad), or run the training step eagerly')
        features = features.float()
        out = []
        for k, g in enumerate(self.groupers):
            features_in = self.mlps_in[k](features.permute(1, 0).unsqueeze(0)).squeeze(0).permute(1, 0).contiguous()      # (P, C1)
            groups = sparse_conv_ops.roi_grid_query(rois, grid_size, index, stride, voxel_size, point_cloud_range, g.max_range, g.radius, g.nsample)
            conv, norm = self.mlps_pos[k][0], self.mlps_pos[k][1]
            scale_p, shift_p = self._position_norm(conv, norm, groups.moments, groups.rows.shape[0] * groups.rows.shape[1])
            pooled, _ = sparse_conv_ops.RoIGridPoolFunction.apply(features_in, conv.weight.reshape(conv.out_channels, 3), scale_p, shift_p,
                                                                  groups.rows, groups.offsets)
            new_features = self.mlps_out[k](pooled.permute(1, 0).unsqueeze(0))                                            # (1, C2, M)
            out.append(new_features.squeeze(0).permute(1, 0))
        return torch.cat(out, dim=1)

"""RoI point pooling on MI355X with the names, argument order, dtypes and zero fill of
/root/reference/pcdet/ops/roipoint_pool3d/roipoint_pool3d_utils.py.  The work is one launch of pdm_roipoint_pool3d
(csrc/roi_pool.hip); there is no CPU or PyTorch fallback.
"""
import torch
import torch.nn as nn
from torch.autograd import Function

from .. import _native


def _extra_width(pool_extra_width):
    """A scalar means the same width on all three sizes (the reference's scalar default, 1.0, fails in its own
    enlarge_box3d, which indexes a 3-sequence)."""
    if isinstance(pool_extra_width, (int, float)):
        return [float(pool_extra_width)] * 3
    ew = [float(w) for w in pool_extra_width]
    assert len(ew) == 3
    return ew


def _check(points, point_features, boxes3d):
    assert points.dim() == 3 and points.shape[2] == 3
    assert boxes3d.dim() == 3 and boxes3d.shape[0] == points.shape[0] and boxes3d.shape[2] >= 7
    assert point_features.dim() == 3 and point_features.shape[:2] == points.shape[:2]
    if not (points.is_cuda and point_features.is_cuda and boxes3d.is_cuda):
        raise ValueError("RoIPointPool3d needs CUDA/HIP tensors: pdm_ssd_amd has no CPU fallback")


class RoIPointPool3d(nn.Module):
    def __init__(self, num_sampled_points=512, pool_extra_width=1.0):
        super().__init__()
        self.num_sampled_points = num_sampled_points
        self.pool_extra_width = pool_extra_width

    def forward(self, points, point_features, boxes3d):
        """points (B, N, 3), point_features (B, N, C), boxes3d (B, M, 7) [x, y, z, dx, dy, dz, heading] ->
        pooled_features (B, M, num_sampled_points, 3 + C), pooled_empty_flag (B, M) int32."""
        return RoIPointPool3dFunction.apply(points, point_features, boxes3d, self.pool_extra_width, self.num_sampled_points)


class RoIPointPool3dFunction(Function):
    @staticmethod
    def forward(ctx, points, point_features, boxes3d, pool_extra_width, num_sampled_points=512):
        _check(points, point_features, boxes3d)
        assert boxes3d.shape[2] == 7
        B, N, M, C, S = points.shape[0], points.shape[1], boxes3d.shape[1], point_features.shape[2], int(num_sampled_points)
        # box_utils.enlarge_box3d: one fp32 add per size
        enlarged = boxes3d.float().contiguous().clone(memory_format=torch.contiguous_format)
        enlarged[:, :, 3:6] += boxes3d.new_tensor(_extra_width(pool_extra_width), dtype=torch.float32)
        points, point_features = points.float().contiguous(), point_features.float().contiguous()
        # zero-filled by the caller, as the reference's: the kernel leaves the rows of an empty box alone
        pooled_features = torch.zeros((B, M, S, 3 + C), dtype=torch.float32, device=points.device)
        pooled_empty_flag = torch.zeros((B, M), dtype=torch.int32, device=points.device)
        if N == 0:      # no point to test: every box is empty (the entry point writes nothing for a zero size)
            pooled_empty_flag.fill_(1)
        _native.call("pdm_roipoint_pool3d", _native.stream(points), B, N, M, C, S, points.data_ptr(), enlarged.data_ptr(),
                     point_features.data_ptr(), pooled_features.data_ptr(), pooled_empty_flag.data_ptr())
        ctx.mark_non_differentiable(pooled_empty_flag)
        return pooled_features, pooled_empty_flag

    @staticmethod
    def backward(ctx, grad_out, grad_flag=None):
        raise NotImplementedError


@torch.no_grad()
def roipoint_pool3d_canonical(points, point_features, rois, pool_extra_width, num_sampled_points):
    """RoIPointPool3d and the PointRCNN head's canonical transformation (pointrcnn_head.py:116-129) as ONE launch of
    pdm_roipoint_pool3d_canonical: rois (B, M, 7 + C') un-enlarged -> (pooled_features (B, M, S, 3 + C) with the
    coordinates in each RoI's frame and zeros for an empty RoI, pooled_empty_flag (B, M) int32).  Not differentiable."""
    _check(points, point_features, rois)
    ew = _extra_width(pool_extra_width)
    B, N, M, C = points.shape[0], points.shape[1], rois.shape[1], point_features.shape[2]
    points, point_features, rois = points.float().contiguous(), point_features.float().contiguous(), rois.float().contiguous()
    pooled = torch.empty((B, M, int(num_sampled_points), 3 + C), dtype=torch.float32, device=points.device)
    flag = torch.empty((B, M), dtype=torch.int32, device=points.device)
    if N == 0:          # nothing to test: every RoI is empty (the entry point writes nothing for a zero size)
        pooled.zero_()
        flag.fill_(1)
    _native.call("pdm_roipoint_pool3d_canonical", _native.stream(points), B, N, M, C, int(num_sampled_points), points.data_ptr(),
                 rois.data_ptr(), rois.shape[2], ew[0], ew[1], ew[2], point_features.data_ptr(), pooled.data_ptr(), flag.data_ptr())
    return pooled, flag

"""RoI-aware pooling on MI355X with the names, argument order, dtypes and zero fill of
/root/reference/pcdet/ops/roiaware_pool3d/roiaware_pool3d_utils.py.  Forward and backward are one launch each
(pdm_roiaware_pool3d_forward / _backward, csrc/roi_pool.hip); there is no CPU or PyTorch fallback.  Unlike the reference's
atomicAdd, the backward is deterministic; it gathers per point, so the function keeps rois and pts for it.
"""
import torch
import torch.nn as nn
from torch.autograd import Function

from .. import _native
from ..iou3d_nms.iou3d_nms_utils import points_in_boxes_gpu  # noqa: F401  (lives there; the reference exports it from here)


def _out_size(out_size):
    """an int (a cube) or three ints -> (out_x, out_y, out_z)"""
    dims = (out_size,) * 3 if isinstance(out_size, int) else tuple(out_size)
    assert len(dims) == 3 and all(isinstance(d, int) for d in dims), out_size
    return dims


class RoIAwarePool3d(nn.Module):
    def __init__(self, out_size, max_pts_each_voxel=128):
        super().__init__()
        self.out_size = out_size
        self.max_pts_each_voxel = max_pts_each_voxel

    def forward(self, rois, pts, pts_feature, pool_method='max'):
        assert pool_method in ['max', 'avg']
        return RoIAwarePool3dFunction.apply(rois, pts, pts_feature, self.out_size, self.max_pts_each_voxel, pool_method)


class RoIAwarePool3dFunction(Function):
    @staticmethod
    def forward(ctx, rois, pts, pts_feature, out_size, max_pts_each_voxel, pool_method):
        """rois (N, 7), pts (npoints, 3), pts_feature (npoints, C) -> pooled_features (N, out_x, out_y, out_z, C)."""
        assert rois.shape[1] == 7 and pts.shape[1] == 3
        if not (rois.is_cuda and pts.is_cuda and pts_feature.is_cuda):
            raise ValueError("RoIAwarePool3d needs CUDA/HIP tensors: pdm_ssd_amd has no CPU fallback")
        out_x, out_y, out_z = _out_size(out_size)
        rois, pts, feats = rois.float().contiguous(), pts.float().contiguous(), pts_feature.float().contiguous()
        num_rois, num_channels, num_pts = rois.shape[0], feats.shape[-1], pts.shape[0]
        pooled_features = feats.new_zeros((num_rois, out_x, out_y, out_z, num_channels))
        # both fully written by the kernel (argmax in max mode only; it is not read in avg mode)
        argmax = torch.empty((num_rois, out_x, out_y, out_z, num_channels), dtype=torch.int32, device=feats.device)
        pts_idx_of_voxels = torch.empty((num_rois, out_x, out_y, out_z, max_pts_each_voxel), dtype=torch.int32, device=feats.device)
        pool_method = {'max': 0, 'avg': 1}[pool_method]
        nbytes = _native.lib().pdm_roiaware_pool3d_workspace_bytes(num_rois, out_x, out_y, out_z)
        ws = torch.empty(max(nbytes, 8), dtype=torch.uint8, device=feats.device)
        _native.call("pdm_roiaware_pool3d_forward", _native.stream(feats), num_rois, num_pts, num_channels, int(max_pts_each_voxel), out_x,
                     out_y, out_z, rois.data_ptr(), pts.data_ptr(), feats.data_ptr(), pool_method, ws.data_ptr(), nbytes,
                     pts_idx_of_voxels.data_ptr(), argmax.data_ptr(), pooled_features.data_ptr())
        ctx.roiaware_pool3d_for_backward = (pts_idx_of_voxels, argmax, pool_method, num_pts, num_channels, rois, pts,
                                            (out_x, out_y, out_z), int(max_pts_each_voxel))
        return pooled_features

    @staticmethod
    def backward(ctx, grad_out):
        """grad_out (N, out_x, out_y, out_z, C) -> gradient of pts_feature only, (npoints, C)."""
        pts_idx_of_voxels, argmax, pool_method, num_pts, num_channels, rois, pts, out, max_pts = ctx.roiaware_pool3d_for_backward
        grad_out = grad_out.float().contiguous()
        grad_in = torch.empty((num_pts, num_channels), dtype=torch.float32, device=grad_out.device)   # fully written
        _native.call("pdm_roiaware_pool3d_backward", _native.stream(grad_out), rois.shape[0], num_pts, num_channels, max_pts, out[0], out[1],
                     out[2], rois.data_ptr(), pts.data_ptr(), pts_idx_of_voxels.data_ptr(), argmax.data_ptr(), grad_out.data_ptr(),
                     pool_method, grad_in.data_ptr())
        return None, None, grad_in, None, None, None

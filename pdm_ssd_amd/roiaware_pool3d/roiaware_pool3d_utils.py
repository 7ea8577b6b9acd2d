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


class PointListOverflow(RuntimeError):
    """roiaware_pool_sparse: the boxes list more (box, point) pairs than its workspace was sized for"""


def sparse_list_capacity(num_rois, num_points, cells, max_pts_each_voxel):
    """ints of roiaware_pool_sparse's point-list workspace: every listed (box, point) pair takes one.  No more than the
    composed form's (boxes, cells, max_pts - 1) lists, and no more than 4 pairs a point plus 256 a box, which only boxes piled on
    one another exceed (the operator then raises and the caller takes the composed form)."""
    return max(min(num_rois * cells * (int(max_pts_each_voxel) - 1), 4 * num_points + 256 * num_rois), 1)


@torch.no_grad()
def roiaware_pool_sparse(rois, points, point_counts, part_features, rpn_features, out_size, max_pts_each_voxel=128, list_capacity=None):
    """The head's two RoI-aware poolings for the whole batch, straight to sparse rows (pdm_roiaware_pool_sparse_index / _emit,
    csrc/roiaware_sparse.hip): rois (B, N, 7), points (P, 3) batch-major, point_counts (B) int32 rows per sample (a
    device tensor: it is not read here), part_features (P, 4), rpn_features (P, C) ->
      coords (Q, 4) int32 (roi, x, y, z), ascending in ((roi Sx + x) Sy + y) Sz + z: the order pooled.sum(-1).nonzero() gives
      part (Q, 4) the 'avg' pooling, rpn (Q, C) the 'max' pooling
    of the ACTIVE cells: those whose averaged part channels, added in fp32 in ascending channel order, are non-zero.  Bit-equal
    to RoIAwarePool3d 'avg' / 'max' per sample, cat, sum(-1) != 0, nonzero and a gather.  ONE host read ({Q, overflow}, counted in
    sparse_conv_ops.HOST_READS); none and no launch without boxes or points.  Raises PointListOverflow (a RuntimeError) when the point lists do not
    fit list_capacity (default sparse_list_capacity)."""
    from .. import sparse_conv_ops
    assert rois.is_cuda and rois.dim() == 3 and rois.shape[2] == 7, 'rois: (B, N, 7) on the GPU'
    assert points.dim() == 2 and points.shape[1] == 3 and part_features.shape == (points.shape[0], 4), (tuple(points.shape), tuple(part_features.shape))
    assert rpn_features.dim() == 2 and rpn_features.shape[0] == points.shape[0] and rpn_features.shape[1] >= 1, tuple(rpn_features.shape)
    assert point_counts.is_cuda and point_counts.dtype == torch.int32 and point_counts.shape == (rois.shape[0],), 'point_counts: int32 (B) on the GPU'
    ox, oy, oz = _out_size(out_size)
    rois, points, part, rpn = (t.float().contiguous() for t in (rois, points, part_features, rpn_features))
    point_counts = point_counts.contiguous()
    (B, N), P, C, dev = rois.shape[:2], points.shape[0], rpn.shape[1], rois.device
    empty = (torch.empty((0, 4), dtype=torch.int32, device=dev), torch.empty((0, 4), dtype=torch.float32, device=dev),
             torch.empty((0, C), dtype=torch.float32, device=dev))
    if B * N == 0 or P == 0:
        return empty
    L = sparse_list_capacity(B * N, P, ox * oy * oz, max_pts_each_voxel) if list_capacity is None else int(list_capacity)
    nbytes = _native.lib().pdm_roiaware_pool_sparse_workspace_bytes(B, N, ox, oy, oz, L)
    ws = torch.empty(max(nbytes, 8), dtype=torch.uint8, device=dev)
    record = torch.empty(2, dtype=torch.int32, device=dev)
    _native.call("pdm_roiaware_pool_sparse_index", _native.stream(dev), B, N, P, int(max_pts_each_voxel), ox, oy, oz, rois.data_ptr(),
                 points.data_ptr(), point_counts.data_ptr(), part.data_ptr(), L, record.data_ptr(), ws.data_ptr(), nbytes)
    sparse_conv_ops.HOST_READS += 1
    Q, overflow = (int(v) for v in record.cpu().tolist())
    if overflow:
        raise PointListOverflow(f'roiaware_pool_sparse: the boxes list more than list_capacity = {L} (box, point) pairs; use the composed '
                           f'RoIAwarePool3d formulation or pass a larger list_capacity')
    if Q == 0:
        return empty
    coords = torch.empty((Q, 4), dtype=torch.int32, device=dev)
    out_part = torch.empty((Q, 4), dtype=torch.float32, device=dev)
    out_rpn = torch.empty((Q, C), dtype=torch.float32, device=dev)
    _native.call("pdm_roiaware_pool_sparse_emit", _native.stream(dev), B, N, P, C, ox, oy, oz, part.data_ptr(), rpn.data_ptr(), L, Q,
                 ws.data_ptr(), nbytes, coords.data_ptr(), out_part.data_ptr(), out_rpn.data_ptr())
    return coords, out_part, out_rpn


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

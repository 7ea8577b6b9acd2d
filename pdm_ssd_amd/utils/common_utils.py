"""Geometry helpers of the RoI heads (behaviour of /root/reference/pcdet/utils/common_utils.py)."""
import numpy as np
import torch


def rotate_points_along_z(points, angle):
    """points (B, N, 3 + C), angle (B) in radians about z, turning x towards y -> a new tensor with the first two columns
    turned per batch row and every other column kept.  Behaviour of the reference's function of this name (:35-57):
    x' = x cos a - y sin a, y' = x sin a + y cos a, here as element-wise operations instead of a matrix product."""
    c = torch.cos(angle).float().view(-1, 1)
    s = torch.sin(angle).float().view(-1, 1)
    x, y = points[:, :, 0], points[:, :, 1]
    out = points.clone()
    out[:, :, 0] = x * c - y * s
    out[:, :, 1] = x * s + y * c
    return out


def get_voxel_centers(voxel_coords, downsample_times, voxel_size, point_cloud_range):
    """voxel_coords (N, 3) (z, y, x) of a level at stride downsample_times -> (N, 3) fp32 centres (x, y, z):
    (float(c) + 0.5) * (float(voxel_size) * downsample_times) + range minimum, three fp32 roundings (the reference's function
    of this name; the RoI-grid pooling kernel forms the same bits from the cell it visits)."""
    assert voxel_coords.shape[1] == 3
    # the constants stay python numbers holding fp32 values (the product rounded in fp32 as the tensor form rounds it): no index
    # or constant tensor is uploaded, so nothing here makes the host wait for the stream
    size = [float(np.float32(v) * np.float32(downsample_times)) for v in voxel_size]
    low = [float(np.float32(v)) for v in point_cloud_range[0:3]]
    cols = [(voxel_coords[:, 2 - k].float() + 0.5) * size[k] + low[k] for k in range(3)]
    return torch.stack(cols, dim=1)


def generate_voxel2pinds(sparse_tensor):
    """A sparse tensor's rows -> the dense (B, D, H, W) int32 table of the row at every cell, -1 where none (the reference's
    function of this name): 4 bytes a cell, what the composed RoI-grid pooling reads and the fused operator does without."""
    indices = sparse_tensor.indices.long()
    table = torch.full([sparse_tensor.batch_size] + list(sparse_tensor.spatial_shape), -1, dtype=torch.int32, device=indices.device)
    table[indices[:, 0], indices[:, 1], indices[:, 2], indices[:, 3]] = torch.arange(indices.shape[0], device=indices.device, dtype=torch.int32)
    return table


def limit_period(val, offset=0.5, period=np.pi):
    """val folded into [-offset * period, (1 - offset) * period) (the reference's common_utils.limit_period on tensors)"""
    turns = torch.floor(val / period + offset)
    return val - turns * period

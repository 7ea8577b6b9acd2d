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


def limit_period(val, offset=0.5, period=np.pi):
    """val folded into [-offset * period, (1 - offset) * period) (the reference's common_utils.limit_period on tensors)"""
    turns = torch.floor(val / period + offset)
    return val - turns * period

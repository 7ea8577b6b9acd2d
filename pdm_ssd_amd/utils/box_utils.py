"""Box helpers of the heads (boxes are rows [x, y, z, dx, dy, dz, heading, ...], centre-based)."""
import numpy as np
import torch

from .common_utils import limit_period, rotate_points_along_z


def enlarge_box3d(boxes3d, extra_width=(0, 0, 0)):
    """/root/reference/pcdet/utils/box_utils.py:187-201 — a copy of the boxes with `extra_width` added to the three
    sizes (the ring between a box and its enlarged twin is the head's 'ignore' zone)."""
    large = boxes3d.clone()
    # python scalars, one in-place add per size: a tensor made from the list would be a pageable host-to-device copy in
    # the middle of every training step, and that copy blocks the host until the stream has drained (5 ms per step at the
    # bench shape: the host could not issue the losses and the backward ahead of the device)
    for k in range(3):
        if float(extra_width[k]) != 0.0:
            large[:, 3 + k] += float(extra_width[k])
    return large


def boxes_to_corners_3d(boxes3d):
    """/root/reference/pcdet/utils/box_utils.py:28-53 — boxes (N, 7) -> corners (N, 8, 3): the four corners of the bottom
    face (x, y signs + +, + -, - -, - +), then those of the top face in the same order; each is half the size times its
    signs, turned by the heading about z, moved to the centre."""
    signs = boxes3d.new_tensor([[1, 1, -1], [1, -1, -1], [-1, -1, -1], [-1, 1, -1],
                                [1, 1, 1], [1, -1, 1], [-1, -1, 1], [-1, 1, 1]]) / 2
    corners = boxes3d[:, None, 3:6] * signs[None, :, :]
    corners = rotate_points_along_z(corners, boxes3d[:, 6])
    return corners + boxes3d[:, None, 0:3]


def _area(boxes):
    return (boxes[:, 2] - boxes[:, 0]) * (boxes[:, 3] - boxes[:, 1])


def boxes_iou_normal(boxes_a, boxes_b):
    """boxes_a (N, 4), boxes_b (M, 4) as [x1, y1, x2, y2] -> (N, M) IoU of axis-aligned boxes: the overlap along each axis
    clamped at 0, their product over (area_a + area_b) - product, the union clamped to >= 1e-6 (the reference's
    box_utils.boxes_iou_normal; csrc/anchor_head.hip follows this operation order)."""
    assert boxes_a.shape[1] == 4 and boxes_b.shape[1] == 4
    low = torch.max(boxes_a[:, None, :2], boxes_b[None, :, :2])
    high = torch.min(boxes_a[:, None, 2:], boxes_b[None, :, 2:])
    side = (high - low).clamp(min=0)
    inter = side[..., 0] * side[..., 1]
    union = (_area(boxes_a)[:, None] + _area(boxes_b)[None, :] - inter).clamp(min=1e-6)
    return inter / union


def boxes3d_lidar_to_aligned_bev_boxes(boxes3d):
    """boxes3d (N, 7 + C) -> (N, 4) [x1, y1, x2, y2]: the box turned to the nearer axis, i.e. its extents swapped unless
    |limit_period(heading, 0.5, pi)| < pi / 4."""
    upright = limit_period(boxes3d[:, 6], offset=0.5, period=np.pi).abs() < np.pi / 4
    half = torch.where(upright[:, None], boxes3d[:, 3:5], boxes3d[:, 3:5].flip(1)) / 2
    centre = boxes3d[:, :2]
    return torch.cat((centre - half, centre + half), dim=1)


def boxes3d_nearest_bev_iou(boxes_a, boxes_b):
    """boxes_a (N, 7), boxes_b (M, 7) -> (N, M): IoU of the nearest axis-aligned BEV boxes."""
    return boxes_iou_normal(boxes3d_lidar_to_aligned_bev_boxes(boxes_a), boxes3d_lidar_to_aligned_bev_boxes(boxes_b))

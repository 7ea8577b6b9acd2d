"""Box helpers of the heads (boxes are rows [x, y, z, dx, dy, dz, heading, ...], centre-based)."""
import torch

from .common_utils import rotate_points_along_z


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

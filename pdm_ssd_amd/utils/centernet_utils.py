"""Gaussian heat-map targets for the BEV head, on the device.

gaussian_radius: the three-root rule of /root/reference/pcdet/models/model_utils/centernet_utils.py:9-35.
draw_gaussians: what the reference does box by box on the host (gaussian2D + draw_gaussian_to_heatmap, :38-70, called
from dense_heads/center_head.py:100-160) — a (2r+1)^2 window of exp(-(dx^2+dy^2)/(2 sigma^2)), sigma = (2r+1)/6,
entries below eps * max zeroed, max-merged into the map — as ONE batched scatter-max over all boxes.
"""
import torch


def gaussian_radius(height, width, min_overlap=0.5):
    a1 = 1
    b1 = (height + width)
    c1 = width * height * (1 - min_overlap) / (1 + min_overlap)
    r1 = (b1 + (b1 ** 2 - 4 * a1 * c1).sqrt()) / 2
    a2 = 4
    b2 = 2 * (height + width)
    c2 = (1 - min_overlap) * width * height
    r2 = (b2 + (b2 ** 2 - 4 * a2 * c2).sqrt()) / 2
    a3 = 4 * min_overlap
    b3 = -2 * min_overlap * (height + width)
    c3 = (min_overlap - 1) * width * height
    r3 = (b3 + (b3 ** 2 - 4 * a3 * c3).sqrt()) / 2
    return torch.min(torch.min(r1, r2), r3)


def draw_gaussians(heatmap, cls_idx, centers_int, radius, valid, max_radius=8):
    """heatmap (B, C, H, W) zero-initialised, updated in place; per box: batch index / class channel in `cls_idx`
    (B, M, 2) long, integer centre cell (B, M, 2) = (x, y), integer radius (B, M), valid (B, M) bool.
    The batched window is (2 max_radius + 1)^2 cells: a box of radius <= max_radius gets exactly the reference's window;
    a larger one keeps the reference's sigma = (2 r + 1) / 6 (from the UNCLAMPED radius) and loses only the part of its
    window beyond max_radius cells — pass max_radius >= the largest radius (PDMHeatmapHead derives it from MAX_RADIUS
    in the target config) for exact targets."""
    B, C, H, W = heatmap.shape
    dev = heatmap.device
    k = torch.arange(-max_radius, max_radius + 1, device=dev)
    dy, dx = torch.meshgrid(k, k, indexing="ij")                                     # (K, K)
    r_true = radius.clamp(min=0).float()[..., None, None]                            # (B, M, 1, 1)
    r = r_true.clamp(max=max_radius)
    sigma = (2 * r_true + 1) / 6
    g = torch.exp(-(dx * dx + dy * dy).float() / (2 * sigma * sigma))                # (B, M, K, K)
    inside = (dx.abs() <= r) & (dy.abs() <= r)
    g = torch.where(g < torch.finfo(torch.float32).eps, torch.zeros_like(g), g)       # h[h < eps * h.max()] = 0, max = 1
    x = centers_int[..., 0, None, None] + dx
    y = centers_int[..., 1, None, None] + dy
    ok = inside & valid[..., None, None] & (x >= 0) & (x < W) & (y >= 0) & (y < H)
    flat = ((cls_idx[..., 0, None, None] * C + cls_idx[..., 1, None, None]) * H + y) * W + x
    # entries outside the window / map / padding boxes carry the value 0 (a no-op under max on a non-negative map); they
    # are sent to addresses of their own — all of them on element 0 made the scatter's atomics queue up (1.2 ms)
    spread = torch.arange(flat.numel(), device=dev).view_as(flat) % heatmap.numel()
    flat = torch.where(ok, flat, spread)
    vals = torch.where(ok, g, torch.zeros_like(g))
    heatmap.view(-1).scatter_reduce_(0, flat.reshape(-1), vals.reshape(-1), reduce="amax", include_self=True)
    return heatmap


def _gather_feat(feat, ind):
    """feat (B, N, D), ind (B, K) -> (B, K, D): row ind[b, k] of sample b."""
    return feat.gather(1, ind.unsqueeze(2).expand(ind.size(0), ind.size(1), feat.size(2)))


def _transpose_and_gather_feat(feat, ind):
    """feat (B, D, H, W), ind (B, K) flat cells y * W + x -> (B, K, D): the channels at those cells."""
    B, D = feat.size(0), feat.size(1)
    return _gather_feat(feat.permute(0, 2, 3, 1).reshape(B, -1, D), ind)


def _topk(scores, K=40):
    """scores (B, C, H, W) -> the K best over (class, y, x) per sample in two stages, as the reference's
    centernet_utils.py:155-170: the K best cells of every class, then the K best of those C * K.  Returns score (B, K),
    flat cell y * W + x (B, K), class (B, K) int32, y and x (B, K) as floats.  K > H * W is torch.topk's error.
    Equal scores fall in whatever order torch.topk leaves them; the fused operator (center_head_ops.center_decode) takes
    the lower flat index c * H * W + y * W + x."""
    B, C, H, W = scores.size()
    per_class_score, per_class_cell = torch.topk(scores.flatten(2, 3), K)            # (B, C, K)
    best_score, best = torch.topk(per_class_score.view(B, -1), K)                       # (B, K) into (C * K)
    classes = (best // K).int()
    cells = per_class_cell.view(B, -1).gather(1, best)
    ys = (cells // W).float()
    xs = (cells % W).int().float()
    return best_score, cells, classes, ys, xs


def decode_bbox_from_heatmap(heatmap, rot_cos, rot_sin, center, center_z, dim, point_cloud_range=None, voxel_size=None,
                             feature_map_stride=None, vel=None, iou=None, K=100, circle_nms=False, score_thresh=None,
                             post_center_limit_range=None):
    """The torch formulation of the heat-map decode (the reference's centernet_utils.py:173-241): heatmap (B, C, H, W)
    scores, the regression maps with dim already exponentiated -> a list of per-sample dicts pred_boxes (n, 7 | 9),
    pred_scores (n), pred_labels (n) int32 (the head's 0-based class), the K best candidates that lie within
    post_center_limit_range (inclusive) and above score_thresh (strict), in rank order.  circle_nms is unsupported, as
    in the reference; an iou map is not part of this build."""
    assert not circle_nms, 'circle_nms: not checked in the reference (centernet_utils.py:178-180), not supported here'
    assert iou is None, 'an iou head is out of scope'
    assert post_center_limit_range is not None
    B = heatmap.size(0)
    scores, cells, classes, ys, xs = _topk(heatmap, K=K)
    center = _transpose_and_gather_feat(center, cells)
    angle = torch.atan2(_transpose_and_gather_feat(rot_sin, cells), _transpose_and_gather_feat(rot_cos, cells))
    xs = (xs.view(B, K, 1) + center[:, :, 0:1]) * feature_map_stride * voxel_size[0] + point_cloud_range[0]
    ys = (ys.view(B, K, 1) + center[:, :, 1:2]) * feature_map_stride * voxel_size[1] + point_cloud_range[1]
    parts = [xs, ys, _transpose_and_gather_feat(center_z, cells), _transpose_and_gather_feat(dim, cells), angle]
    if vel is not None:
        parts.append(_transpose_and_gather_feat(vel, cells))
    boxes = torch.cat(parts, dim=-1)
    limit = torch.as_tensor(post_center_limit_range, dtype=boxes.dtype, device=boxes.device)
    keep = (boxes[..., :3] >= limit[:3]).all(2) & (boxes[..., :3] <= limit[3:]).all(2)
    if score_thresh is not None:
        keep &= scores > score_thresh
    return [{'pred_boxes': boxes[b, keep[b]], 'pred_scores': scores[b, keep[b]], 'pred_labels': classes[b, keep[b]]}
            for b in range(B)]

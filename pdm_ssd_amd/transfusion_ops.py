"""TransFusionHead's two device operators (csrc/transfusion.hip): the query initialisation from the dense heat-map and the
query-wise box decode, each one launch chain for the whole batch with no host read, safe to capture in a
torch.cuda.graph after one warm-up call.

Their torch formulations (proposals_torch, decode_torch) stay next to them: the CPU path, and what the tests compare with.

The head's training half (csrc/tf_assign.hip) follows below: lsap (a batched linear-sum assignment), assign (the Hungarian
assigner's costs, matching and targets for the batch) and loss (the three losses with their gradients behind one autograd
node), next to lsap_host (the same solver in numpy), assign_torch and loss_torch (the reference's per-sample formulation).
"""
import ctypes

import numpy as np
import torch

from . import _native

MAX_P = 16384          # queries per sample the selection holds in LDS
EXEMPT = {'nuScenes': (8, 9), 'Waymo': (1, 2)}      # classes without the local-maximum filter (pedestrian-sized objects)


def exempt_classes(dataset_name, num_class):
    ex = EXEMPT.get(dataset_name, ())
    if any(c >= num_class for c in ex):
        raise ValueError(f'DATASET {dataset_name} exempts classes {ex} from the local-maximum filter: needs more than {num_class} classes')
    return list(ex)


def _check_proposals(C, H, W, P, nms_kernel_size):
    if nms_kernel_size < 1 or nms_kernel_size % 2 == 0:
        raise ValueError(f'NMS_KERNEL_SIZE = {nms_kernel_size} must be odd')
    if not 1 <= P <= min(C * H * W, MAX_P):
        raise ValueError(f'NUM_PROPOSALS = {P} out of range (1 .. {min(C * H * W, MAX_P)})')


@torch.no_grad()
def proposals_torch(logits, num_proposals, nms_kernel_size, exempt, y_size):
    """the operator's contract by torch operators on any device; ties by lower flat index (a stable sort)"""
    B, C, H, W = logits.shape
    P, k = int(num_proposals), int(nms_kernel_size)
    _check_proposals(C, H, W, P, k)
    s = logits.detach().float().sigmoid()
    pad = k // 2
    keep = torch.zeros_like(s, dtype=torch.bool)
    if H > 2 * pad and W > 2 * pad:
        inner = torch.nn.functional.max_pool2d(s, kernel_size=k, stride=1, padding=0)
        keep[:, :, pad:H - pad, pad:W - pad] = s[:, :, pad:H - pad, pad:W - pad] == inner
    for c in exempt:
        keep[:, c] = True
    masked = (s * keep).reshape(B, C, H * W)
    order = torch.sort(masked.reshape(B, -1), dim=-1, descending=True, stable=True).indices[:, :P]
    cls, index = order // (H * W), order % (H * W)
    qhs = masked.gather(2, index[:, None, :].expand(-1, C, -1))
    pos = torch.stack((index % y_size, index // y_size), dim=-1).float() + 0.5
    return index, cls, qhs, pos


@torch.no_grad()
def proposals(logits, num_proposals, nms_kernel_size, exempt, y_size):
    """logits (B, C, H, W) fp32 on the GPU -> index (B, P) int64 (the cell y * W + x), cls (B, P) int64,
    query_heatmap_score (B, C, P), query_pos (B, P, 2) = (index % y_size + 0.5, index // y_size + 0.5) (pdm_tf_proposals):
    s = sigmoid(logit) survives where it equals the maximum of its k x k window and the window lies inside the map, and
    everywhere for a class in `exempt`; others score 0; per sample the P highest over (class, y, x), ties by lower index."""
    B, C, H, W = logits.shape
    P, k = int(num_proposals), int(nms_kernel_size)
    _check_proposals(C, H, W, P, k)
    assert logits.is_cuda and logits.dtype == torch.float32
    x = logits.detach().contiguous()
    dev = x.device
    nbytes = _native.lib().pdm_tf_proposals_workspace_bytes(B, C, H, W, P)
    ws = torch.empty(max(nbytes, 8), dtype=torch.uint8, device=dev)
    index = torch.empty((B, P), dtype=torch.int64, device=dev)
    cls = torch.empty((B, P), dtype=torch.int64, device=dev)
    qhs = torch.empty((B, C, P), dtype=torch.float32, device=dev)
    pos = torch.empty((B, P, 2), dtype=torch.float32, device=dev)
    _native.call("pdm_tf_proposals", _native.stream(dev), B, C, H, W, x.data_ptr(), k, len(exempt), _native.host_array(ctypes.c_int, exempt),
                 P, int(y_size), index.data_ptr(), cls.data_ptr(), qhs.data_ptr(), pos.data_ptr(), ws.data_ptr(), nbytes)
    return index, cls, qhs, pos


def _check_decode(score_thresh, limit_range):
    if score_thresh is None or not float(score_thresh) >= 0:
        raise ValueError(f'SCORE_THRESH = {score_thresh} must be non-negative (a query of score 0 has no defined class)')
    assert len(limit_range) == 6


@torch.no_grad()
def decode_torch(heatmap, center, height, dim, rot, vel, cls, query_heatmap_score, score_thresh, limit_range, x0, y0, vx, vy, stride):
    """the operator's contract by torch operators on any device -> the padded (boxes, scores, labels, count)"""
    _check_decode(score_thresh, limit_range)
    B, C, P = heatmap.shape
    at = cls[:, None, :]
    score = (heatmap.float().sigmoid().gather(1, at) * query_heatmap_score.gather(1, at))[:, 0]
    x = center[:, 0].float() * stride * vx + x0
    y = center[:, 1].float() * stride * vy + y0
    cols = [x, y, height[:, 0].float(), *dim.float().exp().unbind(1), torch.atan2(rot[:, 0].float(), rot[:, 1].float())]
    if vel is not None:
        cols += list(vel.float().unbind(1))
    raw = torch.stack(cols, dim=-1)
    lim = raw.new_tensor(limit_range)
    keep = (score > score_thresh) & (raw[..., :3] >= lim[:3]).all(-1) & (raw[..., :3] <= lim[3:]).all(-1)
    order = torch.sort((~keep).to(torch.int8), dim=1, stable=True).indices            # survivors first, in query order
    kept = keep.gather(1, order)
    boxes = raw.gather(1, order[..., None].expand_as(raw)) * kept[..., None]
    scores = score.gather(1, order) * kept
    labels = (cls.gather(1, order) + 1) * kept
    return boxes, scores, labels, keep.sum(1).to(torch.int32)


@torch.no_grad()
def decode(heatmap, center, height, dim, rot, vel, cls, query_heatmap_score, score_thresh, limit_range, x0, y0, vx, vy, stride):
    """The prediction head's outputs, (B, c, P) fp32 on the GPU: heatmap logits (C), center (2, the query position added),
    height (1), dim (3, before exp), rot (2: [sin, cos]), vel (2) or None; cls (B, P) int64; query_heatmap_score (B, C, P)
    -> boxes (B, P, 7 | 9), scores (B, P), labels (B, P) int64 (1-based), count (B) int32 (pdm_tf_decode): a query of class c
    scores sigmoid(heatmap[c]) * query_heatmap_score[c]; kept iff score > score_thresh (strict) and the centre lies within
    limit_range (inclusive); survivors compacted in query order, padding rows zero."""
    _check_decode(score_thresh, limit_range)
    B, C, P = heatmap.shape
    maps = [heatmap, center, height, dim, rot] + ([vel] if vel is not None else [])
    for t, ch in zip(maps, (C, 2, 1, 3, 2, 2)):
        assert t.is_cuda and t.shape == (B, ch, P), (tuple(t.shape), (B, ch, P))
    maps = [t.detach().float().contiguous() for t in maps]
    cls = cls.contiguous()
    qhs = query_heatmap_score.detach().float().contiguous()
    assert cls.shape == (B, P) and cls.dtype == torch.int64 and qhs.shape == (B, C, P)
    dev, E = heatmap.device, 2 if vel is not None else 0
    boxes = torch.empty((B, P, 7 + E), dtype=torch.float32, device=dev)
    scores = torch.empty((B, P), dtype=torch.float32, device=dev)
    labels = torch.empty((B, P), dtype=torch.int64, device=dev)
    count = torch.empty((B,), dtype=torch.int32, device=dev)
    _native.call("pdm_tf_decode", _native.stream(dev), B, C, P, *[t.data_ptr() for t in maps[:5]], maps[5].data_ptr() if E else None,
                 cls.data_ptr(), qhs.data_ptr(), float(score_thresh), _native.host_array(ctypes.c_float, limit_range), float(x0),
                 float(y0), float(vx), float(vy), float(stride), boxes.data_ptr(), scores.data_ptr(), labels.data_ptr(), count.data_ptr())
    return boxes, scores, labels, count


# ---- training: linear-sum assignment, the Hungarian assigner's targets, the three losses (csrc/tf_assign.hip) -----------------
LSAP_MAX = 1024        # rows and columns of one sample the solver holds in LDS; a larger matrix is refused, never truncated
FLT_MAX = float(np.finfo(np.float32).max)
HEAD_ORDER = ('center', 'height', 'dim', 'rot', 'vel')      # the order of the box code [x y | z | log dims | sin cos | vx vy]


def _check_lsap(P, G):
    if not (1 <= P <= LSAP_MAX and 0 <= G <= LSAP_MAX):
        raise ValueError(f'lsap: a {P} x {G} cost matrix is out of range (1 <= P <= {LSAP_MAX}, 0 <= G <= {LSAP_MAX})')


def lsap_host(cost):
    """cost (P, G) -> gt_of_row (P) int32, row_of_gt (G) int32: the matching of size min(P, G) of least total cost, -1 = unmatched.
    The solver of pdm_lsap in numpy, step for step: shortest augmenting paths (Jonker-Volgenant as Crouse states it, the algorithm
    of scipy.optimize.linear_sum_assignment) over the smaller side's rows, duals and path lengths in float64, ties by the
    lower column index, every loop counted (min(P, G) augmentations of at most max(P, G) steps).  A cost that is not finite
    is read as FLT_MAX, where scipy raises.  Equal to scipy wherever the optimum is unique."""
    c = np.asarray(cost, dtype=np.float32)
    P, G = c.shape
    _check_lsap(P, G)
    gt_of_row, row_of_gt = np.full(P, -1, dtype=np.int32), np.full(G, -1, dtype=np.int32)
    if G == 0:
        return gt_of_row, row_of_gt
    c = np.where(np.isfinite(c), c, np.float32(FLT_MAX)).astype(np.float64)
    tr = G < P
    if tr:
        c = c.T
    nr, nc = c.shape
    u, v = np.zeros(nr), np.zeros(nc)
    col4row, row4col = np.full(nr, -1, dtype=np.int64), np.full(nc, -1, dtype=np.int64)
    for cur in range(nr):
        sh, path = np.full(nc, np.inf), np.full(nc, -1, dtype=np.int64)
        sc, sr = np.zeros(nc, dtype=bool), np.zeros(nr, dtype=bool)
        min_val, i, sink = 0.0, cur, -1
        for _ in range(nc):                                            # a step retires one column
            sr[i] = True
            r = ((min_val + c[i]) - u[i]) - v
            better = ~sc & (r < sh)
            path[better] = i
            sh[better] = r[better]
            masked = np.where(sc, np.inf, sh)
            j = int(np.argmin(masked))                                 # the first minimum: the lower index
            min_val = masked[j]
            sc[j] = True
            if row4col[j] < 0:
                sink = j
                break
            i = row4col[j]
        assert sink >= 0
        sr[cur] = False
        u[cur] += min_val
        u[sr] += min_val - sh[col4row[sr]]
        v[sc] -= min_val - sh[sc]
        j = sink
        for _ in range(nr):                                            # the path back to `cur`
            i = path[j]
            row4col[j] = i
            col4row[i], j = j, col4row[i]
            if i == cur:
                break
    rows, cols = (col4row, np.arange(nr)) if tr else (np.arange(nr), col4row)
    gt_of_row[rows] = cols
    row_of_gt[cols] = rows
    return gt_of_row, row_of_gt


@torch.no_grad()
def lsap(cost, num_gt):
    """cost (B, P, Gmax) fp32 on the GPU (rows contiguous), num_gt (B) int32 on the GPU, read there -> gt_of_row (B, P) int32,
    row_of_gt (B, Gmax) int32 (pdm_lsap): per sample lsap_host of the leading P x num_gt[b] block, one workgroup per sample."""
    assert cost.dim() == 3
    B, P, G = cost.shape
    _check_lsap(P, G)                                                  # before anything touches a device
    assert cost.is_cuda and cost.dtype == torch.float32 and num_gt.is_cuda and num_gt.dtype == torch.int32 and num_gt.shape == (B,)
    if G and (cost.stride(2) != 1 or cost.stride(1) < G or cost.stride(0) != P * cost.stride(1)):
        cost = cost.contiguous()
    dev = cost.device
    gt_of_row = torch.empty((B, P), dtype=torch.int32, device=dev)
    row_of_gt = torch.empty((B, G), dtype=torch.int32, device=dev)
    _native.call("pdm_lsap", _native.stream(dev), B, P, G, cost.data_ptr() if G else None, cost.stride(1) if G else 0,
                 num_gt.contiguous().data_ptr(), gt_of_row.data_ptr(), row_of_gt.data_ptr() if G else None)
    return gt_of_row, row_of_gt


def _cost_cfg(cls_cost, reg_cost, iou_cost):
    return [float(cls_cost.get('weight', 0.15)), float(cls_cost.get('alpha', 0.25)), float(cls_cost.get('gamma', 2.0)),
            float(cls_cost.get('eps', 1e-12)), float(reg_cost.get('weight', 0.25)), float(iou_cost.get('weight', 0.25))]


def _check_assign(heatmap, center, height, dim, rot, vel, gt_boxes):
    B, C, P = heatmap.shape
    E = 0 if vel is None else 2
    for t, ch in zip((center, height, dim, rot) + (() if vel is None else (vel,)), (2, 1, 3, 2, 2)):
        assert t.shape == (B, ch, P), (tuple(t.shape), (B, ch, P))
    if gt_boxes.dim() != 3 or gt_boxes.shape[0] != B or gt_boxes.shape[2] not in (8, 10) or gt_boxes.shape[2] - 8 < E:
        raise ValueError(f'gt_boxes (B, M, 8 | 10) with the 1-based class last (10 columns with a velocity map): {tuple(gt_boxes.shape)}')
    _check_lsap(P, gt_boxes.shape[1])
    return B, C, P, gt_boxes.shape[1], E


@torch.no_grad()
def assign(heatmap, center, height, dim, rot, vel, gt_boxes, cls_cost, reg_cost, iou_cost, point_cloud_range, voxel_size, stride,
           map_hw, gaussian_overlap, min_radius, num_classes):
    """The prediction head's maps as decode takes them, (B, c, P) fp32 on the GPU; gt_boxes (B, M, 8 | 10) with the 1-based
    class last and zero padding -> dict (pdm_tf_assign, no host read): labels (B, P) int64 (class - 1, num_classes = background),
    label_weights (B, P), bbox_targets / bbox_weights (B, P, 8 | 10), ious (B, P), assigned (B, P) int32 (index among the
    sample's valid boxes, dx > 0 and dy > 0, or -1), num_pos () int32, matched_ious (), heatmap (B, C, H, W)."""
    B, C, P, M, E = _check_assign(heatmap, center, height, dim, rot, vel, gt_boxes)
    H, W = int(map_hw[0]), int(map_hw[1])
    maps = [heatmap, center, height, dim, rot] + ([vel] if E else [])
    assert all(t.is_cuda for t in maps) and gt_boxes.is_cuda
    maps = [t.detach().float().contiguous() for t in maps]
    gt = gt_boxes.detach().float().contiguous()
    dev, code = heatmap.device, 8 + E
    out = {'labels': torch.empty((B, P), dtype=torch.int64, device=dev), 'label_weights': torch.empty((B, P), dtype=torch.float32, device=dev),
           'bbox_targets': torch.empty((B, P, code), dtype=torch.float32, device=dev),
           'bbox_weights': torch.empty((B, P, code), dtype=torch.float32, device=dev),
           'ious': torch.empty((B, P), dtype=torch.float32, device=dev), 'assigned': torch.empty((B, P), dtype=torch.int32, device=dev),
           'num_pos': torch.empty((), dtype=torch.int32, device=dev), 'matched_ious': torch.empty((), dtype=torch.float32, device=dev),
           'heatmap': torch.empty((B, C, H, W), dtype=torch.float32, device=dev)}
    nbytes = _native.lib().pdm_tf_assign_workspace_bytes(B, P, M)
    ws = torch.empty(max(nbytes, 8), dtype=torch.uint8, device=dev)
    _native.call("pdm_tf_assign", _native.stream(dev), B, C, P, M, gt.shape[2], H, W, *[t.data_ptr() for t in maps[:5]],
                 maps[5].data_ptr() if E else None, gt.data_ptr() if M else None, _native.host_array(ctypes.c_double, _cost_cfg(cls_cost, reg_cost, iou_cost)),
                 _native.host_array(ctypes.c_float, point_cloud_range), float(voxel_size[0]), float(voxel_size[1]), float(stride),
                 float(gaussian_overlap), int(min_radius), int(num_classes), out['labels'].data_ptr(), out['label_weights'].data_ptr(),
                 out['bbox_targets'].data_ptr(), out['bbox_weights'].data_ptr(), out['ious'].data_ptr(), out['assigned'].data_ptr(),
                 out['num_pos'].data_ptr(), out['matched_ious'].data_ptr(), out['heatmap'].data_ptr(), ws.data_ptr(), nbytes)
    return out


def _cross3(p1, p2, p0):
    return (p1[0] - p0[0]) * (p2[1] - p0[1]) - (p2[0] - p0[0]) * (p1[1] - p0[1])


def _corners_host(b):
    hx, hy, c, s = b[3] / 2, b[4] / 2, np.cos(b[6]), np.sin(b[6])
    return [(dx * c - dy * s + b[0], dx * s + dy * c + b[1]) for dx, dy in ((-hx, -hy), (hx, -hy), (hx, hy), (-hx, hy))]


def _inside_host(b, p, margin=1e-2):
    c, s = np.cos(-b[6]), np.sin(-b[6])
    rx, ry = (p[0] - b[0]) * c - (p[1] - b[1]) * s, (p[0] - b[0]) * s + (p[1] - b[1]) * c
    return abs(rx) < b[3] / 2 + margin and abs(ry) < b[4] / 2 + margin


def _segments_cross(p1, p0, q1, q0):
    if not (min(p0[0], p1[0]) <= max(q0[0], q1[0]) and min(q0[0], q1[0]) <= max(p0[0], p1[0]) and
            min(p0[1], p1[1]) <= max(q0[1], q1[1]) and min(q0[1], q1[1]) <= max(p0[1], p1[1])):
        return None
    s1, s2, s3, s4 = _cross3(q0, p1, p0), _cross3(p1, q1, p0), _cross3(p0, q1, q0), _cross3(q1, p1, q0)
    if not (s1 * s2 > 0 and s3 * s4 > 0):
        return None
    s5 = _cross3(q1, p1, p0)
    if abs(s5 - s1) > 1e-8:
        return (s5 * q0[0] - s1 * q1[0]) / (s5 - s1), (s5 * q0[1] - s1 * q1[1]) / (s5 - s1)
    a0, b0, c0 = p0[1] - p1[1], p1[0] - p0[0], p0[0] * p1[1] - p1[0] * p0[1]
    a1, b1, c1 = q0[1] - q1[1], q1[0] - q0[0], q0[0] * q1[1] - q1[0] * q0[1]
    d = a0 * b1 - a1 * b0
    return (b0 * c1 - b1 * c0) / d, (a1 * c0 - a0 * c1) / d


def overlap_bev_host(boxes_a, boxes_b):
    """(N, M) areas of intersection of the BEV footprints of boxes [x y z dx dy dz yaw ..], the algorithm of the library's
    box_overlap_bev (csrc/box_geometry.h; the reference's boxes_overlap_bev_gpu) in float64 on the host: the crossings of the
    edges and the corners of either box inside the other WITH ITS MARGIN OF 1e-2, ordered by angle about their mean, then
    the fan's area.  The margin is part of the contract: two boxes a centimetre apart overlap a little."""
    a, b = np.asarray(boxes_a, dtype=np.float64), np.asarray(boxes_b, dtype=np.float64)
    out = np.zeros((len(a), len(b)))
    ra, rb = 0.5 * np.hypot(a[:, 3], a[:, 4]), 0.5 * np.hypot(b[:, 3], b[:, 4])
    for i in range(len(a)):
        ca = _corners_host(a[i])
        for j in np.nonzero(np.hypot(a[i, 0] - b[:, 0], a[i, 1] - b[:, 1]) <= ra[i] + rb + 0.1)[0]:
            cb = _corners_host(b[j])
            pts = []
            for k in range(4):
                for m in range(4):
                    x = _segments_cross(ca[(k + 1) % 4], ca[k], cb[(m + 1) % 4], cb[m])
                    if x is not None:
                        pts.append(x)
            for k in range(4):
                if _inside_host(a[i], cb[k]):
                    pts.append(cb[k])
                if _inside_host(b[j], ca[k]):
                    pts.append(ca[k])
            if len(pts) < 3:
                continue
            pts = np.array(pts)
            centre = pts.mean(0)
            pts = pts[np.argsort(np.arctan2(pts[:, 1] - centre[1], pts[:, 0] - centre[0]), kind='stable')]
            u = pts[1:-1] - pts[0]
            w = pts[2:] - pts[0]
            out[i, j] = abs(float((u[:, 0] * w[:, 1] - u[:, 1] * w[:, 0]).sum())) / 2
    return out


def overlaps_torch(boxes1, boxes2):
    """the reference's hungarian_assigner.overlaps(): BEV overlap x height overlap over the union, z read as the box's BOTTOM"""
    if boxes1.is_cuda:
        from .iou3d_nms import iou3d_nms_utils
        bev = iou3d_nms_utils.boxes_overlap_bev(boxes1[:, :7], boxes2[:, :7])
    else:
        bev = torch.from_numpy(overlap_bev_host(boxes1.detach().numpy(), boxes2.detach().numpy())).to(boxes1.dtype)
    top = torch.min((boxes1[:, 2] + boxes1[:, 5]).view(-1, 1), (boxes2[:, 2] + boxes2[:, 5]).view(1, -1))
    bottom = torch.max(boxes1[:, 2].view(-1, 1), boxes2[:, 2].view(1, -1))
    o3 = bev * torch.clamp(top - bottom, min=0)
    v1, v2 = (boxes1[:, 3] * boxes1[:, 4] * boxes1[:, 5]).view(-1, 1), (boxes2[:, 3] * boxes2[:, 4] * boxes2[:, 5]).view(1, -1)
    return o3 / torch.clamp(v1 + v2 - o3, min=1e-8)


def cost_torch(boxes, gt_boxes, gt_labels, cls_pred, point_cloud_range, cls_cost, reg_cost, iou_cost):
    """boxes (P, 7 | 9), gt_boxes (G, 7 | 9), gt_labels (G) 0-based, cls_pred (C, P) logits -> cost (P, G), iou (P, G):
    HungarianAssigner3D's three weighted costs and their sum"""
    w, alpha, gamma, eps, rw, iw = _cost_cfg(cls_cost, reg_cost, iou_cost)
    s = cls_pred.t().sigmoid()
    neg = -(1 - s + eps).log() * (1 - alpha) * s.pow(gamma)
    pos = -(s + eps).log() * alpha * (1 - s).pow(gamma)
    cls = (pos[:, gt_labels] - neg[:, gt_labels]) * w
    start = boxes.new_tensor(point_cloud_range[0:2])
    extent = boxes.new_tensor(point_cloud_range[3:5]) - start
    reg = torch.cdist((boxes[:, :2] - start) / extent, (gt_boxes[:, :2] - start) / extent, p=1) * rw
    iou = overlaps_torch(boxes, gt_boxes)
    return cls + reg + (-iou) * iw, iou


def encode_bbox_torch(boxes, point_cloud_range, voxel_size, stride, code):
    t = boxes.new_zeros((boxes.shape[0], code))
    t[:, 0] = (boxes[:, 0] - point_cloud_range[0]) / (stride * voxel_size[0])
    t[:, 1] = (boxes[:, 1] - point_cloud_range[1]) / (stride * voxel_size[1])
    t[:, 3:6] = boxes[:, 3:6].log()
    t[:, 2] = boxes[:, 2]
    t[:, 6], t[:, 7] = torch.sin(boxes[:, 6]), torch.cos(boxes[:, 6])
    if code == 10:
        t[:, 8:10] = boxes[:, 7:9]
    return t


@torch.no_grad()
def assign_torch(heatmap, center, height, dim, rot, vel, gt_boxes, cls_cost, reg_cost, iou_cost, point_cloud_range, voxel_size, stride,
                 map_hw, gaussian_overlap, min_radius, num_classes, detail=None):
    """assign()'s contract in the reference's formulation on any device: sample by sample the unfiltered decode, the three cost
    matrices, lsap_host on the host, the targets, and the heat-map gaussians box by box.  detail: a list that receives
    (cost, gt_of_row, row_of_gt) per sample.  Differences from the reference, as in assign(): a sample without a valid box
    is all background (the reference fails on an undefined name), and a box whose centre cell lies outside the map draws
    nothing (the reference's slices then cut an arbitrary part of the window)."""
    from .utils import centernet_utils
    B, C, P, M, E = _check_assign(heatmap, center, height, dim, rot, vel, gt_boxes)
    H, W = int(map_hw[0]), int(map_hw[1])
    dev, code = heatmap.device, 8 + E
    f = lambda t: t.detach().float()
    x = f(center)[:, 0] * stride * voxel_size[0] + point_cloud_range[0]
    y = f(center)[:, 1] * stride * voxel_size[1] + point_cloud_range[1]
    cols = [x, y, f(height)[:, 0], *f(dim).exp().unbind(1), torch.atan2(f(rot)[:, 0], f(rot)[:, 1])] + (list(f(vel).unbind(1)) if E else [])
    boxes = torch.stack(cols, dim=-1)                                     # (B, P, 7 | 9)
    out = {'labels': torch.full((B, P), int(num_classes), dtype=torch.int64, device=dev), 'label_weights': torch.ones((B, P), device=dev),
           'bbox_targets': torch.zeros((B, P, code), device=dev), 'bbox_weights': torch.zeros((B, P, code), device=dev),
           'ious': torch.zeros((B, P), device=dev), 'assigned': torch.full((B, P), -1, dtype=torch.int32, device=dev),
           'heatmap': torch.zeros((B, C, H, W), device=dev)}
    num_pos, means = 0, []
    for b in range(B):
        g = f(gt_boxes[b])
        g = g[(g[:, 3] > 0) & (g[:, 4] > 0)]
        labels = g[:, -1].long() - 1
        G = g.shape[0]
        if G == 0:
            means.append(0.0)
            if detail is not None:
                detail.append((np.zeros((P, 0), np.float32), np.full(P, -1, np.int32), np.zeros(0, np.int32)))
            continue
        cost, iou = cost_torch(boxes[b], g[:, :7 + E], labels, f(heatmap[b]), point_cloud_range, cls_cost, reg_cost, iou_cost)
        gt_of_row, row_of_gt = lsap_host(cost.cpu().numpy())
        if detail is not None:
            detail.append((cost.cpu().numpy(), gt_of_row, row_of_gt))
        at = torch.from_numpy(gt_of_row).to(dev).long()
        pos = at >= 0
        out['assigned'][b] = at.int()
        out['labels'][b, pos] = labels[at[pos]]
        out['bbox_targets'][b, pos] = encode_bbox_torch(g[at[pos]], point_cloud_range, voxel_size, stride, code)
        out['bbox_weights'][b, pos] = 1.0
        out['ious'][b, pos] = iou[pos, at[pos]].clamp(0.0, 1.0)
        n = int(pos.sum())
        num_pos += n
        means.append(float(out['ious'][b, pos].sum() / max(n, 1)))
        for k in range(G):
            width, length = g[k, 3] / voxel_size[0] / stride, g[k, 4] / voxel_size[1] / stride
            radius = max(int(min_radius), int(centernet_utils.gaussian_radius(length.view(-1), width.view(-1), gaussian_overlap)[0]))
            cx = int((g[k, 0] - point_cloud_range[0]) / voxel_size[0] / stride)
            cy = int((g[k, 1] - point_cloud_range[1]) / voxel_size[1] / stride)
            c = int(labels[k])
            if not (0 <= cx < W and 0 <= cy < H and 0 <= c < C):
                continue
            sigma = (2 * radius + 1) / 6
            ys, xs = np.ogrid[-radius:radius + 1, -radius:radius + 1]
            window = np.exp(-(xs * xs + ys * ys) / (2 * sigma * sigma))
            window[window < np.finfo(window.dtype).eps * window.max()] = 0
            left, right, top, bottom = min(cx, radius), min(W - cx, radius + 1), min(cy, radius), min(H - cy, radius + 1)
            part = torch.from_numpy(window[radius - top:radius + bottom, radius - left:radius + right]).to(dev).float()
            view = out['heatmap'][b, c, cy - top:cy + bottom, cx - left:cx + right]
            torch.max(view, part, out=view)
    out['num_pos'] = torch.tensor(num_pos, dtype=torch.int32, device=dev)
    out['matched_ious'] = torch.tensor(float(np.mean(means)), dtype=torch.float32, device=dev)
    return out


def _pred_rows(center, height, dim, rot, vel):
    return torch.cat([center, height, dim, rot] + ([] if vel is None else [vel]), dim=1).permute(0, 2, 1)        # (B, P, 8 | 10)


def loss_torch(heatmap, center, height, dim, rot, vel, dense_heatmap, targets, code_weights, cls_weight, bbox_weight, hm_weight, alpha, gamma):
    """loss()'s contract in the reference's formulation under autograd on any device -> (loss_cls, loss_bbox, loss_heatmap), each
    already times its weight.  (dense_heatmap is left untouched: the reference's clip_sigmoid overwrites it with its sigmoid.)"""
    target = targets['heatmap']
    p = torch.clamp(dense_heatmap.sigmoid(), min=1e-4, max=1 - 1e-4)
    eps = 1e-12
    pos = -(p + eps).log() * (1 - p).pow(2.0) * target.eq(1)
    neg = -(1 - p + eps).log() * p.pow(2.0) * (1 - target).pow(4.0)
    loss_heatmap = (pos + neg).sum() / target.eq(1).float().sum().clamp(min=1)
    den = targets['num_pos'].to(heatmap.dtype).clamp(min=1)
    C = heatmap.shape[1]
    x = heatmap.permute(0, 2, 1)                                         # (B, P, C)
    t = torch.nn.functional.one_hot(targets['labels'], C + 1)[..., :C].to(x.dtype)
    s = torch.sigmoid(x)
    focal = (t * alpha + (1 - t) * (1 - alpha)) * torch.pow(t * (1.0 - s) + (1.0 - t) * s, gamma)
    bce = torch.clamp(x, min=0) - x * t + torch.log1p(torch.exp(-torch.abs(x)))
    loss_cls = (focal * bce * targets['label_weights'].to(x.dtype).unsqueeze(-1)).sum() / den
    preds = _pred_rows(center, height, dim, rot, vel)
    w = targets['bbox_weights'] * preds.new_tensor(list(code_weights)[:preds.shape[2]])
    loss_bbox = (torch.abs(preds - targets['bbox_targets']) * w).sum() / den
    return loss_cls * cls_weight, loss_bbox * bbox_weight, loss_heatmap * hm_weight


class _TransFusionLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, targets, scalars, code_weights, heatmap, center, height, dim, rot, vel, dense_heatmap):
        B, C, P = heatmap.shape
        H, W = dense_heatmap.shape[2:]
        E = 0 if vel is None else 2
        maps = [heatmap, center, height, dim, rot] + ([vel] if E else [])
        assert all(t.is_cuda and t.dtype == torch.float32 for t in maps) and dense_heatmap.is_cuda and dense_heatmap.dtype == torch.float32
        assert dense_heatmap.shape == targets['heatmap'].shape == (B, C, H, W) and len(code_weights) >= 8 + E
        maps = [t.detach().contiguous() for t in maps]
        dense = dense_heatmap.detach().contiguous()
        tg = {k: targets[k].contiguous() for k in ('labels', 'label_weights', 'bbox_targets', 'bbox_weights', 'num_pos', 'heatmap')}
        assert tg['labels'].dtype == torch.int64 and tg['num_pos'].dtype == torch.int32 and tg['bbox_targets'].shape == (B, P, 8 + E)
        dev = heatmap.device
        out = torch.empty(6, dtype=torch.float32, device=dev)
        grads = [torch.empty_like(t) for t in maps]
        g_dense = torch.empty_like(dense)
        nbytes = _native.lib().pdm_tf_loss_workspace_bytes(B, C, P, E, H, W)
        ws = torch.empty(max(nbytes, 8), dtype=torch.uint8, device=dev)
        cls_w, bbox_w, hm_w, alpha, gamma = scalars
        _native.call("pdm_tf_loss", _native.stream(dev), B, C, P, H, W, *[t.data_ptr() for t in maps[:5]], maps[5].data_ptr() if E else None,
                     dense.data_ptr(), tg['labels'].data_ptr(), tg['label_weights'].data_ptr(), tg['bbox_targets'].data_ptr(),
                     tg['bbox_weights'].data_ptr(), tg['num_pos'].data_ptr(), tg['heatmap'].data_ptr(),
                     _native.host_array(ctypes.c_float, code_weights[:8 + E]), cls_w, bbox_w, hm_w, alpha, gamma, out.data_ptr(),
                     *[g.data_ptr() for g in grads[:5]], grads[5].data_ptr() if E else None, g_dense.data_ptr(), ws.data_ptr(), nbytes)
        ctx.save_for_backward(out, g_dense, *grads)
        ctx.with_vel = bool(E)
        return out[0], out[1], out[2]

    @staticmethod
    def backward(ctx, g_cls, g_bbox, g_hm):
        out, g_dense, g_heatmap, *g_box = ctx.saved_tensors            # the gradients were formed in forward(): only scaled here
        box = [g * g_bbox for g in g_box] + ([] if ctx.with_vel else [None])
        return (None, None, None, g_heatmap * g_cls, *box, g_dense * (out[3] * g_hm))


def loss(heatmap, center, height, dim, rot, vel, dense_heatmap, targets, code_weights, cls_weight, bbox_weight, hm_weight, alpha, gamma):
    """The prediction head's maps (B, c, P) and dense_heatmap (B, C, H, W), fp32 on the GPU, with assign()'s targets ->
    (loss_cls, loss_bbox, loss_heatmap) 0-dim, each the reference's term times its weight, with its gradient on its maps
    (pdm_tf_loss): sigmoid focal loss against the one-hot of labels and L1 of [center height dim rot vel] against bbox_targets,
    both over max(num_pos, 1) read on the device; the penalty-reduced focal loss of clip_sigmoid(dense_heatmap) over
    max(#peaks, 1).  Sums are block partials folded in a fixed order: two runs give the same bits.  No host read."""
    scalars = tuple(float(v) for v in (cls_weight, bbox_weight, hm_weight, alpha, gamma))
    return _TransFusionLoss.apply(targets, scalars, tuple(float(v) for v in code_weights), heatmap, center, height, dim, rot, vel, dense_heatmap)

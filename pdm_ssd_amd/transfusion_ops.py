"""TransFusionHead's two device operators (csrc/transfusion.hip): the query initialisation from the dense heat-map and the
query-wise box decode, each one launch chain for the whole batch with no host read, safe to capture in a
torch.cuda.graph after one warm-up call.

Their torch formulations (proposals_torch, decode_torch) stay next to them: the CPU path, and what the tests compare with.
"""
import ctypes

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

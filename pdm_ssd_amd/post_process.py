"""Batched detector post-processing on the device (POST_PROCESSING.BATCHED): the whole batch's score threshold,
top-NMS_PRE_MAXSIZE selection, NMS, NMS_POST_MAXSIZE cut and recall counts in one native call (pdm_post_process,
post_process.hip) instead of Detector3DTemplate's per-sample loop with its host synchronisations.

Results equal the loop's bit for bit: candidates are ranked as pdm_topk_sampling ranks them (score descending, equal
scores by lower row), the NMS keep lists are those of pdm_nms, the sigmoid is torch's (applied here, not in the kernel),
and the recall IoU follows iou3d_nms_utils._iou3d_from_overlap operation for operation.
"""
import ctypes
import warnings

import torch

from . import _native

MAX_PRE = 16384   # candidates per segment the select kernel holds in LDS


def _get(cfg, key, default=None):
    return cfg.get(key, default) if isinstance(cfg, dict) else getattr(cfg, key, default)


def workspace_bytes(num_segments, pre_max, post_max):
    """Device workspace of one pdm_post_process call (segments = B, or B * C with MULTI_CLASSES_NMS)."""
    return int(_native.lib().pdm_post_process_workspace_bytes(num_segments, pre_max, post_max))


def _layout(batch_dict):
    """-> (probabilities (rows, C) fp32, boxes (rows, D) fp32, offsets (B + 1) int32, batch_index (rows) fp32 | None,
    the raw logits (rows, C)), all on the device, without a synchronisation."""
    B = int(batch_dict['batch_size'])
    cls, box = batch_dict['batch_cls_preds'], batch_dict['batch_box_preds']
    bi = batch_dict.get('batch_index', None)
    if bi is not None:
        assert box.dim() == 2
        bif = bi.float().contiguous()
        offsets = torch.searchsorted(bif, torch.arange(B + 1, dtype=torch.float32, device=bif.device)).int()
    else:
        assert box.dim() == 3
        n = box.shape[1]
        cls, box = cls.reshape(B * n, cls.shape[-1]), box.reshape(B * n, box.shape[-1])
        offsets = torch.arange(B + 1, dtype=torch.int32, device=box.device) * n
        bif = None
    probs = cls if batch_dict['cls_preds_normalized'] else torch.sigmoid(cls)
    return probs.float().contiguous(), box.float().contiguous(), offsets, bif, cls


def post_process_padded(batch_dict, post_cfg, num_class, gt_boxes=None, workspace=None):
    """batch_dict as Detector3DTemplate.post_processing reads it (one batch_cls_preds tensor; 2-D layout with a
    sample-major batch_index, or 3-D (B, N, .)) -> dict of device tensors, with no host synchronisation:
      rows (B, P) int64    selected row within the sample, -1 = padding (P = NMS_POST_MAXSIZE, times C in multi-class
                           mode, where a sample's survivors come class after class)
      boxes (B, P, 7), scores (B, P), labels (B, P) int64 (1 .. C), count (B) int32
      error (1) int32      non-zero: batch_index is not sample-major (the results are then meaningless)
      recall (1 + T) int64 [gt rows, recalled at each RECALL_THRESH_LIST entry] summed over the batch, or None
      offsets (B + 1) int32, the sample row ranges.
    After one warm-up call (which grants the select kernel its LDS) the call can be captured in a torch.cuda.graph.
    workspace: an optional uint8 device tensor of at least workspace_bytes(...) bytes (allocated here otherwise)."""
    nms_cfg = _get(post_cfg, 'NMS_CONFIG')
    multi = bool(_get(nms_cfg, 'MULTI_CLASSES_NMS', False))
    pre, post = int(_get(nms_cfg, 'NMS_PRE_MAXSIZE')), int(_get(nms_cfg, 'NMS_POST_MAXSIZE'))
    if pre > MAX_PRE:
        raise ValueError(f"batched post-processing holds at most {MAX_PRE} candidates per segment (NMS_PRE_MAXSIZE={pre})")
    normal = {'nms_gpu': 0, 'nms_normal_gpu': 1}[_get(nms_cfg, 'NMS_TYPE')]
    B = int(batch_dict['batch_size'])
    probs, boxes, offsets, bif, _ = _layout(batch_dict)
    C = probs.shape[1]
    assert C in [1, num_class]
    if multi:
        assert C == num_class, 'MULTI_CLASSES_NMS needs one score column per class'
    dev = boxes.device
    P = post * (C if multi else 1)
    S = B * (C if multi else 1)
    out = {'rows': torch.empty((B, P), dtype=torch.int64, device=dev),
           'boxes': torch.empty((B, P, 7), dtype=torch.float32, device=dev),
           'scores': torch.empty((B, P), dtype=torch.float32, device=dev),
           'labels': torch.empty((B, P), dtype=torch.int64, device=dev),
           'count': torch.empty((B,), dtype=torch.int32, device=dev),
           'error': torch.empty((1,), dtype=torch.int32, device=dev),
           'offsets': offsets, 'recall': None}
    thresholds = [float(t) for t in (_get(post_cfg, 'RECALL_THRESH_LIST', None) or [])]
    gt, G, gdim = None, 0, 7
    if gt_boxes is not None:
        gt = gt_boxes.float().contiguous()
        assert gt.dim() == 3 and gt.shape[0] == B and gt.shape[2] >= 7
        G, gdim = gt.shape[1], gt.shape[2]
        out['recall'] = torch.empty((1 + len(thresholds),), dtype=torch.int64, device=dev)
    nbytes = workspace_bytes(S, pre, post)
    if workspace is None:
        ws = torch.empty((max(nbytes, 256),), dtype=torch.uint8, device=dev)
    else:
        ws = workspace
        assert ws.dtype == torch.uint8 and ws.is_contiguous() and ws.numel() >= nbytes
    tarr = _native.host_array(ctypes.c_float, thresholds)
    score_thresh = _get(post_cfg, 'SCORE_THRESH', None)
    _native.call("pdm_post_process", _native.stream(dev), B, C, 1 if multi else 0, probs.shape[0],
                 probs.data_ptr(), probs.stride(0), boxes.data_ptr(), boxes.stride(0), offsets.data_ptr(),
                 bif.data_ptr() if bif is not None else None,
                 float('-inf') if score_thresh is None else float(score_thresh), pre, post,
                 float(_get(nms_cfg, 'NMS_THRESH')), normal, G, gdim, gt.data_ptr() if gt is not None else None,
                 len(thresholds), tarr, ws.data_ptr(), nbytes, out['rows'].data_ptr(),
                 out['boxes'].data_ptr(), out['scores'].data_ptr(), out['labels'].data_ptr(), out['count'].data_ptr(),
                 out['error'].data_ptr(), out['recall'].data_ptr() if out['recall'] is not None else None)
    return out


def batched_post_processing(batch_dict, post_cfg, num_class, gt_boxes=None):
    """-> (pred_dicts, recall_dict) in exactly the format of Detector3DTemplate.post_processing's loop, after ONE
    device-to-host read (counts, error flag and recall counts together); None if the device reports a batch_index
    that is not sample-major (the caller then runs the loop)."""
    nms_cfg = _get(post_cfg, 'NMS_CONFIG')
    multi = bool(_get(nms_cfg, 'MULTI_CLASSES_NMS', False))
    B = int(batch_dict['batch_size'])
    out = post_process_padded(batch_dict, post_cfg, num_class, gt_boxes=gt_boxes)
    glob = (out['rows'] + out['offsets'][:B].long().view(B, 1)).clamp_(min=0)           # global row of every output slot
    scores = out['scores']
    box_preds = batch_dict['batch_box_preds']
    box_preds = box_preds.reshape(-1, box_preds.shape[-1])
    if _get(post_cfg, 'OUTPUT_RAW_SCORE', False) and not multi:
        cls = batch_dict['batch_cls_preds']
        scores = torch.max(cls.reshape(-1, cls.shape[-1]), dim=-1)[0][glob]
    wide = box_preds.shape[1] != 7
    fetched = torch.cat([out['count'].long(), out['error'].long()] +
                        ([out['recall']] if out['recall'] is not None else [])).cpu()
    counts = fetched[:B].tolist()
    if int(fetched[B]) != 0:
        return None
    pred_dicts = []
    for b in range(B):
        n = counts[b]
        bx = box_preds[glob[b, :n]] if wide else out['boxes'][b, :n]
        pred_dicts.append({'pred_boxes': bx, 'pred_scores': scores[b, :n], 'pred_labels': out['labels'][b, :n]})
    recall_dict = {}
    if out['recall'] is not None:
        rec = fetched[B + 1:].tolist()
        recall_dict = {'gt': rec[0]}
        for i, t in enumerate(_get(post_cfg, 'RECALL_THRESH_LIST') or []):
            recall_dict['roi_%s' % str(t)] = 0
            recall_dict['rcnn_%s' % str(t)] = rec[1 + i]
    return pred_dicts, recall_dict


_warned = set()


def warn_once(reason):
    if reason not in _warned:
        _warned.add(reason)
        warnings.warn(f"POST_PROCESSING.BATCHED: {reason}; using the per-sample loop", RuntimeWarning, stacklevel=3)

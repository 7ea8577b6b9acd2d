"""KITTI object evaluation on the device: from the padded detections of post_process_padded to AP numbers
(bbox / BEV / 3D / AOS, easy / moderate / hard, AP_11 and AP_R40) without a per-frame host loop.

Semantics are those of the reference's kitti_object_eval_python/eval.py (clean_data, the three overlaps,
compute_statistics_jit, get_thresholds, eval_class, get_mAP / get_mAP_R40, get_official_eval_result) and of
kitti_dataset.generate_prediction_dicts for the conversion; the kernels are in csrc/kitti_eval.hip.  One evaluation is

    overlaps (one launch per metric) -> detection flags -> pass 1 -> READ true-positive scores -> thresholds (host, <= 41
    per combination) -> pass 2 + fold -> READ [tp, fp, fn, similarity] -> recall / precision / AP in numpy float64

so the number of launches and device-to-host reads does not depend on the number of frames.  The ground truth's ignore
flags are a vectorised numpy pass (the annotations arrive on the host); the detections' flags are computed on the device.
There is no CPU fallback: without the native library every call raises.
"""
import ctypes
import io

import numpy as np
import torch

from . import _native

CLASS_NAMES = ['car', 'pedestrian', 'cyclist', 'van', 'person_sitting', 'truck']   # clean_data's table, lower case
CLASS_TO_NAME = {0: 'Car', 1: 'Pedestrian', 2: 'Cyclist', 3: 'Van', 4: 'Person_sitting', 5: 'Truck'}
NAME_TO_CLASS = {v: k for k, v in CLASS_TO_NAME.items()}
DONTCARE, OTHER = 6, 7
MIN_HEIGHT = (40, 25, 25)
MAX_OCCLUSION = (0, 1, 2)
MAX_TRUNCATION = (0.15, 0.3, 0.5)
N_SAMPLE_PTS = 41
MAX_DT_PER_FRAME = 4096
METRIC_NAMES = ('bbox', 'bev', '3d')


def official_min_overlaps():
    """(2 overlap sets, 3 metrics, 6 classes), get_official_eval_result's table."""
    overlap_0_7 = np.array([[0.7, 0.5, 0.5, 0.7, 0.5, 0.7]] * 3)
    overlap_0_5 = np.array([[0.7, 0.5, 0.5, 0.7, 0.5, 0.5], [0.5, 0.25, 0.25, 0.5, 0.25, 0.5], [0.5, 0.25, 0.25, 0.5, 0.25, 0.5]])
    return np.stack([overlap_0_7, overlap_0_5], axis=0)


def _name_id(name):
    low = name.lower()
    if low in CLASS_NAMES:
        return CLASS_NAMES.index(low)
    return DONTCARE if name == 'DontCare' else OTHER


def name_ids(names):
    """class names -> the small integers the kernels compare: 0 .. 5 by lower-cased name, 6 'DontCare' (exact), 7 others."""
    names = np.asarray(names).astype(str).reshape(-1)
    if names.shape[0] == 0:
        return np.zeros((0,), dtype=np.int32)
    uniq, inverse = np.unique(names, return_inverse=True)
    return np.array([_name_id(str(u)) for u in uniq], dtype=np.int32)[inverse.reshape(-1)]


def gt_ignore_flags(names, bbox, occluded, truncated, classes, difficulties):
    """clean_data's ground-truth side for every (class, difficulty): (len(classes) * len(difficulties), NG) int8 with
    0 = counts, 1 = neutral (Van for Car, Person_sitting for Pedestrian, or too hard), -1 = another class."""
    names = np.asarray(names, dtype=np.int32)
    height = bbox[:, 3] - bbox[:, 1]
    out = np.empty((len(classes) * len(difficulties), names.shape[0]), dtype=np.int8)
    for ci, c in enumerate(classes):
        valid = np.where(names == c, 1, -1)
        if c == 1:
            valid = np.where(names == 4, 0, valid)
        elif c == 0:
            valid = np.where(names == 3, 0, valid)
        for di, d in enumerate(difficulties):
            ignore = (occluded > MAX_OCCLUSION[d]) | (truncated > MAX_TRUNCATION[d]) | (height <= MIN_HEIGHT[d])
            out[ci * len(difficulties) + di] = np.where((valid == 1) & ~ignore, 0, np.where((valid == 0) | (ignore & (valid == 1)), 1, -1))
    return out


def get_thresholds(scores, num_gt, num_sample_pts=N_SAMPLE_PTS):
    """The scores at which recall crosses each of num_sample_pts evenly spaced levels (eval.py get_thresholds).
    The reference walks all scores; its skip test ((i + 2) / num_gt - recall < recall - (i + 1) / num_gt, never for the
    last score) is monotone in the rank i, so the next kept rank is found by bisection with the same float expressions."""
    scores = np.sort(np.asarray(scores, dtype=np.float64))[::-1]
    n = scores.shape[0]
    current_recall = 0
    out = []

    def skipped(i):
        return i < n - 1 and ((i + 2) / num_gt - current_recall) < (current_recall - (i + 1) / num_gt)
    i = 0
    while i < n:
        lo, hi = i, n - 1          # the last score is never skipped
        while lo < hi:
            mid = (lo + hi) // 2
            if skipped(mid):
                lo = mid + 1
            else:
                hi = mid
        out.append(scores[lo])
        current_recall += 1 / (num_sample_pts - 1.0)
        i = lo + 1
    return out


def get_mAP(prec):
    sums = 0
    for i in range(0, prec.shape[-1], 4):
        sums = sums + prec[..., i]
    return sums / 11 * 100


def get_mAP_R40(prec):
    sums = 0
    for i in range(1, prec.shape[-1]):
        sums = sums + prec[..., i]
    return sums / 40 * 100


# ---- conversion -----------------------------------------------------------------------------------------------------

def boxes_to_camera(boxes, count, V2C, R0, P2, image_shape=None):
    """boxes (B, P, 7) lidar fp32, count (B) int32 and the per-sample calibration matrices, all on the device ->
    (cam (B, P, 7) [x, y, z, l, h, w, ry], img (B, P, 4) [x1, y1, x2, y2] clipped to image_shape (B, 2) [h, w],
    alpha (B, P)), fp32 as generate_prediction_dicts produces them.  One launch, no synchronisation."""
    assert boxes.dim() == 3 and boxes.shape[2] == 7 and boxes.dtype == torch.float32
    B, P = boxes.shape[:2]
    dev = boxes.device
    boxes = boxes.contiguous()
    count = count.to(torch.int32).contiguous()
    V2C, R0, P2 = (m.to(device=dev, dtype=torch.float32).contiguous() for m in (V2C, R0, P2))
    assert V2C.shape == (B, 3, 4) and R0.shape == (B, 3, 3) and P2.shape == (B, 3, 4) and count.shape == (B,)
    shp = None
    if image_shape is not None:
        shp = image_shape.to(device=dev, dtype=torch.int32).contiguous()
        assert shp.shape == (B, 2)
    cam = torch.empty((B, P, 7), dtype=torch.float32, device=dev)
    img = torch.empty((B, P, 4), dtype=torch.float32, device=dev)
    alpha = torch.empty((B, P), dtype=torch.float32, device=dev)
    _native.call("pdm_kitti_boxes_to_camera", _native.stream(dev), B, P, boxes.data_ptr(), count.data_ptr(),
                 V2C.data_ptr(), R0.data_ptr(), P2.data_ptr(), shp.data_ptr() if shp is not None else None, cam.data_ptr(),
                 img.data_ptr(), alpha.data_ptr())
    return cam, img, alpha


def stack_calib(calibs, device):
    """list of calibration objects (attributes V2C, R0, P2 as in calibration_kitti.Calibration) or dicts
    (Tr_velo2cam / V2C, R0, P2) -> {'V2C': (B, 3, 4), 'R0': (B, 3, 3), 'P2': (B, 3, 4)} on the device."""
    def field(c, *keys):
        for k in keys:
            if isinstance(c, dict) and k in c:
                return np.asarray(c[k], dtype=np.float32)
            if not isinstance(c, dict) and hasattr(c, k):
                return np.asarray(getattr(c, k), dtype=np.float32)
        raise KeyError(keys[0])
    return {'V2C': torch.from_numpy(np.stack([field(c, 'V2C', 'Tr_velo2cam') for c in calibs])).to(device),
            'R0': torch.from_numpy(np.stack([field(c, 'R0') for c in calibs])).to(device),
            'P2': torch.from_numpy(np.stack([field(c, 'P2') for c in calibs])).to(device)}


def empty_prediction(num_samples=0):
    """generate_prediction_dicts' template."""
    return {'name': np.zeros(num_samples), 'truncated': np.zeros(num_samples), 'occluded': np.zeros(num_samples),
            'alpha': np.zeros(num_samples), 'bbox': np.zeros([num_samples, 4]), 'dimensions': np.zeros([num_samples, 3]),
            'location': np.zeros([num_samples, 3]), 'rotation_y': np.zeros(num_samples), 'score': np.zeros(num_samples),
            'boxes_lidar': np.zeros([num_samples, 7])}


def prediction_dicts(class_names, boxes, scores, labels, count, cam, img, alpha, frame_ids=None):
    """host arrays of one padded batch -> the reference's list of per-frame annotation dicts."""
    names = np.array(class_names)
    out = []
    for b in range(boxes.shape[0]):
        n = int(count[b])
        d = empty_prediction(n)
        if n > 0:
            d['name'] = names[labels[b, :n] - 1]
            d['alpha'] = alpha[b, :n]
            d['bbox'] = img[b, :n]
            d['dimensions'] = cam[b, :n, 3:6]
            d['location'] = cam[b, :n, 0:3]
            d['rotation_y'] = cam[b, :n, 6]
            d['score'] = scores[b, :n]
            d['boxes_lidar'] = boxes[b, :n]
        if frame_ids is not None:
            d['frame_id'] = frame_ids[b]
        out.append(d)
    return out


# ---- the evaluator --------------------------------------------------------------------------------------------------

def _cat(annos, key, width=None, dtype=np.float64):
    parts = [np.asarray(a[key], dtype=dtype).reshape((-1,) if width is None else (-1, width)) for a in annos]
    if not parts:
        return np.zeros((0,) if width is None else (0, width), dtype=dtype)
    return np.concatenate(parts, 0)


def _pack_annos(annos, with_score):
    """list of annotation dicts -> concatenated float64 host arrays + per-frame counts."""
    counts = np.array([len(a['name']) for a in annos], dtype=np.int64)
    pack = {'count': counts,
            'name': name_ids(np.concatenate([np.asarray(a['name']).astype(str) for a in annos if len(a['name'])] + [np.zeros(0, dtype=str)])),
            'bbox': _cat(annos, 'bbox', 4), 'alpha': _cat(annos, 'alpha'),
            'cam': np.concatenate([_cat(annos, 'location', 3), _cat(annos, 'dimensions', 3), _cat(annos, 'rotation_y')[:, None]], 1)}
    if with_score:
        pack['score'] = _cat(annos, 'score')
    else:
        pack['occluded'] = _cat(annos, 'occluded')
        pack['truncated'] = _cat(annos, 'truncated')
    return pack


def _dt_to_device(pack, device):
    return {'count': pack['count'],
            'name': torch.from_numpy(pack['name']).to(device),
            'bbox': torch.from_numpy(np.ascontiguousarray(pack['bbox'])).to(device),
            'alpha': torch.from_numpy(np.ascontiguousarray(pack['alpha'])).to(device),
            'score': torch.from_numpy(np.ascontiguousarray(pack['score'])).to(device),
            'cam': torch.from_numpy(np.ascontiguousarray(pack['cam'])).to(device)}


def _ptr(t):
    return t.data_ptr() if t is not None and t.numel() > 0 else None


def _stage(stats, name, dev):
    """stage timing for tools (stats['stage_ms'] = {}): synchronises, so it is off unless asked for"""
    if stats is not None and 'stage_ms' in stats:
        import time
        torch.cuda.synchronize(dev)
        now = time.perf_counter()
        stats['stage_ms'][name] = stats['stage_ms'].get(name, 0.0) + (now - stats.get('_t', now)) * 1e3
        stats['_t'] = now


def workspace_bytes(num_frames, combinations):
    """Device workspace of pass 2 (the per-chunk partial sums)."""
    return int(_native.lib().pdm_kitti_eval_workspace_bytes(int(num_frames), int(combinations)))


def evaluate_device(gt, dt, classes, difficulties, metrics, min_overlaps, compute_aos=False, workspace=None, stats=None,
                    keep=None):
    """gt: host pack (_pack_annos), dt: device pack (count on the host), classes / difficulties / metrics: lists of ints,
    min_overlaps (K, 3, len(classes)).  -> {'recall', 'precision', 'orientation'}: (len(metrics), C, D, K, 41) float64.
    stats: optional dict, 'launches' and 'reads' are added up.  keep: optional dict that receives the intermediate
    results (overlaps, flags, thresholds, sums) for tests and tools."""
    F = int(gt['count'].shape[0])
    assert dt['count'].shape[0] == F, "ground truth and detections must cover the same frames"
    nM, nC, nD = len(metrics), len(classes), len(difficulties)
    min_overlaps = np.asarray(min_overlaps, dtype=np.float64)
    K = min_overlaps.shape[0]
    assert min_overlaps.shape == (K, 3, nC)
    ncombo = nM * nC * nD * K
    dev = dt['bbox'].device
    stream = _native.stream(dev)
    stats = stats if stats is not None else {}
    stats.setdefault('launches', 0)
    stats.setdefault('reads', 0)
    _stage(stats, 'start', dev)
    gcount, dcount = gt['count'].astype(np.int64), np.asarray(dt['count']).astype(np.int64)
    NG, ND = int(gcount.sum()), int(dcount.sum())
    max_dt = int(dcount.max()) if F else 0
    if max_dt > MAX_DT_PER_FRAME:
        raise ValueError(f"at most {MAX_DT_PER_FRAME} detections per frame ({max_dt} given)")
    offs = np.zeros((3, F + 1), dtype=np.int64)
    offs[0, 1:] = np.cumsum(gcount)
    offs[1, 1:] = np.cumsum(dcount)
    offs[2, 1:] = np.cumsum(gcount * dcount)
    NP = int(offs[2, F])
    if NP >= 2 ** 31 - 256:
        raise ValueError(f"{NP} (detection, ground truth) pairs exceed the kernels' 32-bit indexing")
    # ground-truth flags and the pass-1 slot table on the host (the annotations are host data)
    ign_gt = gt_ignore_flags(gt['name'], gt['bbox'], gt['occluded'], gt['truncated'], classes, difficulties)
    frame_of_gt = np.repeat(np.arange(F), gcount)
    valid = np.zeros((nC * nD, F), dtype=np.int64)
    for cd in range(nC * nD):
        valid[cd] = np.bincount(frame_of_gt[ign_gt[cd] == 0], minlength=F)[:F] if NG else 0
    total_valid = valid.sum(1)
    SV = int(total_valid.sum())
    cd_base = np.concatenate([[0], np.cumsum(total_valid)])
    slot_off = np.zeros((nC * nD, F + 1), dtype=np.int64)
    slot_off[:, 1:] = np.cumsum(valid, 1)
    slot_off += cd_base[:-1, None]
    mo = np.empty((nM, nC, nD, K), dtype=np.float64)
    for mi, m in enumerate(metrics):
        for c in range(nC):
            mo[mi, c, :, :] = min_overlaps[:, m, c][None, :]

    d_offs = torch.from_numpy(offs.astype(np.int32)).to(dev)
    d_slot = torch.from_numpy(slot_off.astype(np.int32)).to(dev)
    d_ign_gt = torch.from_numpy(ign_gt).to(dev)
    d_mo = torch.from_numpy(mo.reshape(-1)).to(dev)
    g_bbox = torch.from_numpy(np.ascontiguousarray(gt['bbox'])).to(dev)
    g_cam = torch.from_numpy(np.ascontiguousarray(gt['cam'])).to(dev)
    g_alpha = torch.from_numpy(np.ascontiguousarray(gt['alpha'])).to(dev)
    g_name = torch.from_numpy(np.ascontiguousarray(gt['name'])).to(dev)
    t_bbox, t_cam, t_alpha, t_score = (dt[k].to(torch.float64).contiguous() for k in ('bbox', 'cam', 'alpha', 'score'))
    t_name = dt['name'].to(torch.int32).contiguous()
    assert t_bbox.shape == (ND, 4) and t_cam.shape == (ND, 7) and t_score.shape == (ND,) and t_name.shape == (ND,)

    overlaps = torch.empty((nM, NP), dtype=torch.float64, device=dev)
    ign_dt = torch.empty((nC * nD, ND), dtype=torch.int8, device=dev)
    slab = torch.empty((nM * K, SV), dtype=torch.float64, device=dev)
    sums = torch.empty((ncombo, N_SAMPLE_PTS, 4), dtype=torch.int64, device=dev)
    nbytes = workspace_bytes(F, ncombo)
    if workspace is None:
        ws = torch.empty((max(nbytes, 256),), dtype=torch.uint8, device=dev)
    else:
        ws = workspace
        assert ws.dtype == torch.uint8 and ws.is_contiguous() and ws.numel() >= nbytes
    c_metrics, c_classes, c_diffs = (_native.host_array(ctypes.c_int, v) for v in (metrics, classes, difficulties))
    _stage(stats, 'host flags + upload', dev)
    off_g, off_d, off_o = d_offs[0].data_ptr(), d_offs[1].data_ptr(), d_offs[2].data_ptr()

    _native.call("pdm_kitti_eval_overlaps", stream, F, off_g, off_d, off_o, NP, nM, c_metrics,
                 _ptr(g_bbox), _ptr(t_bbox), _ptr(g_cam), _ptr(t_cam), _ptr(overlaps))
    stats['launches'] += nM if F and NP else 0
    _stage(stats, 'overlaps', dev)
    _native.call("pdm_kitti_eval_dt_flags", stream, ND, _ptr(t_bbox), _ptr(t_name), nC, c_classes, nD,
                 c_diffs, _ptr(ign_dt))
    stats['launches'] += 1 if ND else 0
    _stage(stats, 'detection flags', dev)
    _native.call("pdm_kitti_eval_pass1", stream, F, off_g, off_d, off_o, max_dt, nM, c_metrics, nC, nD, K,
                 _ptr(overlaps), NP, _ptr(d_ign_gt), NG, _ptr(ign_dt), ND, _ptr(t_score), d_mo.data_ptr(), d_slot.data_ptr(), SV,
                 _ptr(slab))
    stats['launches'] += 1 if F else 0
    tp_scores = slab.cpu().numpy().reshape(nM, K, SV)                       # read 1
    stats['reads'] += 1
    _stage(stats, 'pass 1 + read', dev)
    thresholds = np.zeros((ncombo, N_SAMPLE_PTS), dtype=np.float64)
    nthr = np.zeros((ncombo,), dtype=np.int32)
    for mi in range(nM):
        for cd in range(nC * nD):
            for k in range(K):
                s = tp_scores[mi, k, cd_base[cd]:cd_base[cd + 1]]
                th = get_thresholds(s[~np.isnan(s)], int(total_valid[cd]))
                t = (mi * nC * nD + cd) * K + k
                nthr[t] = len(th)
                thresholds[t, :len(th)] = th
    d_thr = torch.from_numpy(thresholds).to(dev)
    d_nthr = torch.from_numpy(nthr).to(dev)
    _stage(stats, 'thresholds (host)', dev)
    aos_mask = 0
    if compute_aos:
        aos_mask = (1 << nM) - 1 if compute_aos is True else int(compute_aos)
    _native.call("pdm_kitti_eval_pass2", stream, F, off_g, off_d, off_o, max_dt, nM, c_metrics, nC, nD, K,
                 _ptr(overlaps), NP, _ptr(d_ign_gt), NG, _ptr(ign_dt), ND, _ptr(t_score), _ptr(g_alpha), _ptr(t_alpha), _ptr(g_bbox),
                 _ptr(t_bbox), _ptr(g_name), d_mo.data_ptr(), d_thr.data_ptr(), d_nthr.data_ptr(), aos_mask, ws.data_ptr(), nbytes,
                 sums.data_ptr())
    stats['launches'] += 2
    h_sums = sums.cpu().numpy()                                             # read 2
    stats['reads'] += 1
    _stage(stats, 'pass 2 + fold + read', dev)
    pr = h_sums.astype(np.float64)
    pr[..., 3] = h_sums[..., 3].copy().view(np.float64)
    recall = np.zeros((ncombo, N_SAMPLE_PTS))
    precision = np.zeros((ncombo, N_SAMPLE_PTS))
    aos = np.zeros((ncombo, N_SAMPLE_PTS))
    with np.errstate(divide='ignore', invalid='ignore'):
        for t in range(ncombo):
            n = int(nthr[t])
            p = pr[t, :n]
            recall[t, :n] = p[:, 0] / (p[:, 0] + p[:, 2])
            precision[t, :n] = p[:, 0] / (p[:, 0] + p[:, 1])
            if (aos_mask >> (t // (nC * nD * K))) & 1:
                aos[t, :n] = p[:, 3] / (p[:, 0] + p[:, 1])
            for a in (recall, precision, aos):
                a[t, :n] = np.maximum.accumulate(a[t, ::-1])[::-1][:n]      # the running maximum from the right
    shape = (nM, nC, nD, K, N_SAMPLE_PTS)
    _stage(stats, 'curves (host)', dev)
    if keep is not None:
        keep.update({'overlaps': overlaps, 'offsets': offs, 'ign_gt': ign_gt, 'ign_dt': ign_dt, 'total_valid': total_valid,
                     'thresholds': thresholds.reshape(shape), 'num_thresholds': nthr.reshape(shape[:-1]),
                     'pr': pr.reshape(shape + (4,)), 'sums': h_sums.reshape(shape + (4,)), 'tp_scores': tp_scores,
                     'cd_base': cd_base, 'workspace': ws, 'workspace_bytes': nbytes})
    return {'recall': recall.reshape(shape), 'precision': precision.reshape(shape), 'orientation': aos.reshape(shape)}


def _device_of(device):
    if device is None:
        if not torch.cuda.is_available():
            raise _native.NativeLibraryError("kitti_eval needs a GPU: the evaluator has no CPU fallback")
        return torch.device('cuda', torch.cuda.current_device())
    return torch.device(device)


def eval_class(gt_annos, dt_annos, current_classes, difficultys, metric, min_overlaps, compute_aos=False, num_parts=100,
               device=None, stats=None):
    """eval.py's eval_class: -> {'recall', 'precision', 'orientation'}, each (class, difficulty, overlap set, 41).
    num_parts is accepted and ignored (overlaps are computed within frames only)."""
    assert len(gt_annos) == len(dt_annos)
    dev = _device_of(device)
    ret = evaluate_device(_pack_annos(gt_annos, False), _dt_to_device(_pack_annos(dt_annos, True), dev), list(current_classes),
                          list(difficultys), [int(metric)], min_overlaps, compute_aos=bool(compute_aos), stats=stats)
    return {k: v[0] for k, v in ret.items()}


def _classes_to_int(current_classes):
    if not isinstance(current_classes, (list, tuple)):
        current_classes = [current_classes]
    return [NAME_TO_CLASS[c] if isinstance(c, str) else int(c) for c in current_classes]


def format_result(current_classes, min_overlaps, maps, compute_aos):
    """get_official_eval_result's text and ret_dict from the eight mAP arrays (class, difficulty, overlap set)."""
    mAPbbox, mAPbev, mAP3d, mAPaos, mAPbbox_R40, mAPbev_R40, mAP3d_R40, mAPaos_R40 = maps
    out = io.StringIO()
    ret_dict = {}

    def line(text):
        print(text, file=out)

    def triple(tag, a, j, i, fmt):
        line(f"{tag}" + ", ".join(format(a[j, d, i], fmt) for d in range(3)))

    for j, curcls in enumerate(current_classes):
        name = CLASS_TO_NAME[curcls]
        for i in range(min_overlaps.shape[0]):
            line(f"{name} " + "AP@{:.2f}, {:.2f}, {:.2f}:".format(*min_overlaps[i, :, j]))
            triple("bbox AP:", mAPbbox, j, i, ".4f")
            triple("bev  AP:", mAPbev, j, i, ".4f")
            triple("3d   AP:", mAP3d, j, i, ".4f")
            if compute_aos:
                triple("aos  AP:", mAPaos, j, i, ".2f")
            line(f"{name} " + "AP_R40@{:.2f}, {:.2f}, {:.2f}:".format(*min_overlaps[i, :, j]))
            triple("bbox AP:", mAPbbox_R40, j, i, ".4f")
            triple("bev  AP:", mAPbev_R40, j, i, ".4f")
            triple("3d   AP:", mAP3d_R40, j, i, ".4f")
            if compute_aos:
                triple("aos  AP:", mAPaos_R40, j, i, ".2f")
                if i == 0:
                    for d, diff in enumerate(('easy', 'moderate', 'hard')):
                        ret_dict['%s_aos/%s_R40' % (name, diff)] = mAPaos_R40[j, d, 0]
            if i == 0:
                for key, arr in (('3d', mAP3d_R40), ('bev', mAPbev_R40), ('image', mAPbbox_R40)):
                    for d, diff in enumerate(('easy', 'moderate', 'hard')):
                        ret_dict['%s_%s/%s_R40' % (name, key, diff)] = arr[j, d, 0]
    return out.getvalue(), ret_dict


def _official(gt_pack, dt_dev, dt_first_alpha, current_classes, PR_detail_dict, stats=None, keep=None, workspace=None):
    classes = _classes_to_int(current_classes)
    min_overlaps = official_min_overlaps()[:, :, classes]
    compute_aos = dt_first_alpha is not None and dt_first_alpha != -10
    ret = evaluate_device(gt_pack, dt_dev, classes, [0, 1, 2], [0, 1, 2], min_overlaps, compute_aos=1 if compute_aos else 0,
                          stats=stats, keep=keep, workspace=workspace)
    prec, aos = ret['precision'], ret['orientation']
    maps = [get_mAP(prec[0]), get_mAP(prec[1]), get_mAP(prec[2]), get_mAP(aos[0]) if compute_aos else None,
            get_mAP_R40(prec[0]), get_mAP_R40(prec[1]), get_mAP_R40(prec[2]), get_mAP_R40(aos[0]) if compute_aos else None]
    if PR_detail_dict is not None:
        PR_detail_dict['bbox'] = prec[0]
        if compute_aos:
            PR_detail_dict['aos'] = aos[0]
        PR_detail_dict['bev'] = prec[1]
        PR_detail_dict['3d'] = prec[2]
    if keep is not None:
        keep['maps'] = maps
        keep['ret'] = ret
    return format_result(classes, min_overlaps, maps, compute_aos)


def get_official_eval_result(gt_annos, dt_annos, current_classes, PR_detail_dict=None, device=None, stats=None, keep=None):
    """eval.py's get_official_eval_result: -> (result text, ret_dict with the '<Class>_<3d|bev|image|aos>/<difficulty>_R40'
    keys).  AOS is reported when the first non-empty detection frame's first alpha is not -10."""
    assert len(gt_annos) == len(dt_annos)
    first_alpha = None
    for anno in dt_annos:
        if np.asarray(anno['alpha']).shape[0] != 0:
            first_alpha = float(np.asarray(anno['alpha'])[0])
            break
    dev = _device_of(device)
    return _official(_pack_annos(gt_annos, False), _dt_to_device(_pack_annos(dt_annos, True), dev), first_alpha, current_classes,
                     PR_detail_dict, stats=stats, keep=keep)


class KittiEvaluator:
    """Collects the converted detections of every eval batch on the device and scores them once at the end.

        ev = KittiEvaluator(class_names)
        for batch: ev.add_batch(post_process_padded(...), calib, image_shape, frame_ids)   # no synchronisation
        result_str, ret_dict = ev.evaluate(gt_annos)
    """

    def __init__(self, class_names):
        self.class_names = list(class_names)
        self._ids = name_ids(self.class_names)
        self._table = None
        self.batches = []
        self.frame_ids = []
        self.stats = {'launches': 0, 'reads': 0}

    def add_batch(self, padded, calib, image_shape=None, frame_ids=None):
        """padded: post_process_padded's dict (boxes (B, P, 7), scores, labels, count); calib: {'V2C', 'R0', 'P2'} device
        tensors (stack_calib builds them); image_shape (B, 2) [height, width] or None; frame_ids: B ids or None.
        After one warm-up call it can be captured in a torch.cuda.graph (a replay rewrites the captured batch's slots)."""
        boxes = padded['boxes']
        dev = boxes.device
        if self._table is None or self._table.device != dev:
            self._table = torch.from_numpy(self._ids).to(dev)
        cam, img, alpha = boxes_to_camera(boxes, padded['count'], calib['V2C'], calib['R0'], calib['P2'], image_shape)
        names = self._table[(padded['labels'] - 1).clamp(0, len(self.class_names) - 1)]
        self.batches.append({'boxes': boxes, 'scores': padded['scores'], 'labels': padded['labels'], 'count': padded['count'],
                             'cam': cam, 'img': img, 'alpha': alpha, 'name': names})
        B = boxes.shape[0]
        self.frame_ids.extend(list(frame_ids) if frame_ids is not None else [None] * B)
        self.stats['launches'] += 1
        return cam, img, alpha

    def reset(self):
        self.batches, self.frame_ids = [], []

    def _merged(self):
        """all batches as one padded set (F, P, .); batches with fewer slots are padded"""
        P = max(b['boxes'].shape[1] for b in self.batches)

        def pad(x):
            if x.shape[1] == P:
                return x
            shape = list(x.shape)
            shape[1] = P - x.shape[1]
            return torch.cat([x, x.new_zeros(shape)], 1)
        return {k: torch.cat([pad(b[k]) for b in self.batches], 0) if k != 'count' else torch.cat([b['count'] for b in self.batches], 0)
                for k in self.batches[0]}

    def _ragged(self):
        dev = self.batches[0]['boxes'].device
        m = self._merged()
        count = m['count'].cpu().numpy().astype(np.int64)          # the one read that tells the host the frame sizes
        self.stats['reads'] += 1
        P = m['boxes'].shape[1]
        rows = np.concatenate([f * P + np.arange(n) for f, n in enumerate(count)] + [np.zeros((0,), dtype=np.int64)]).astype(np.int64)
        idx = torch.from_numpy(rows).to(dev)

        def take(x):
            return x.reshape((-1,) + tuple(x.shape[2:])).index_select(0, idx)
        dt = {'count': count, 'name': take(m['name']), 'bbox': take(m['img']).double(), 'alpha': take(m['alpha']).double(),
              'score': take(m['scores']).double(), 'cam': take(m['cam']).double()}
        return dt, m

    def evaluate(self, gt_annos, PR_detail_dict=None, keep=None):
        """gt_annos: the frames' ground-truth annotation dicts in the order the batches were added (or, if every one
        carries a 'frame_id' and add_batch was given ids, in any order) -> (result text, ret_dict)."""
        F = len(self.frame_ids)
        assert len(gt_annos) == F, f"{len(gt_annos)} ground-truth frames for {F} detection frames"
        if F and all(isinstance(g, dict) and 'frame_id' in g for g in gt_annos) and all(f is not None for f in self.frame_ids):
            by_id = {g['frame_id']: g for g in gt_annos}
            gt_annos = [by_id[f] for f in self.frame_ids]
        gt = _pack_annos(gt_annos, False)
        if not self.batches:
            dt = _dt_to_device(_pack_annos([], True), _device_of(None))
            first_alpha = None
        else:
            dt, _ = self._ragged()
            # compute_aos as eval.py decides it: alpha is computed for every detection here, so it is valid whenever
            # there is a detection at all
            first_alpha = 0.0 if int(dt['count'].sum()) else None
        return _official(gt, dt, first_alpha, self.class_names, PR_detail_dict, stats=self.stats, keep=keep)

    def annos(self):
        """the reference-format annotation dicts (host numpy), one per frame, as generate_prediction_dicts returns them"""
        out = []
        k = 0
        for b in self.batches:
            h = {key: b[key].cpu().numpy() for key in ('boxes', 'scores', 'labels', 'count', 'cam', 'img', 'alpha')}
            B = h['boxes'].shape[0]
            out.extend(prediction_dicts(self.class_names, h['boxes'], h['scores'], h['labels'], h['count'], h['cam'], h['img'],
                                        h['alpha'], self.frame_ids[k:k + B]))
            k += B
        return out

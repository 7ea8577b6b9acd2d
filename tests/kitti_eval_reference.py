"""Plain numpy / Python restatement of the KITTI object evaluation for tests (no numba, no GPU): the conversion of lidar
detections to camera annotations, clean_data, the three overlaps (rotated intersection by clipping in float64),
the greedy matching of compute_statistics_jit (vectorised over the score thresholds only), get_thresholds, eval_class
and the official result text.  Written for clarity; pdm_ssd_amd.kitti_eval must agree with it."""
import math

import numpy as np

CLASS_NAMES = ['car', 'pedestrian', 'cyclist', 'van', 'person_sitting', 'truck']
CLASS_TO_NAME = {0: 'Car', 1: 'Pedestrian', 2: 'Cyclist', 3: 'Van', 4: 'Person_sitting', 5: 'Truck'}
MIN_HEIGHT = [40, 25, 25]
MAX_OCCLUSION = [0, 1, 2]
MAX_TRUNCATION = [0.15, 0.3, 0.5]
MIN_OVERLAPS = np.stack([np.array([[0.7, 0.5, 0.5, 0.7, 0.5, 0.7]] * 3),
                         np.array([[0.7, 0.5, 0.5, 0.7, 0.5, 0.5], [0.5, 0.25, 0.25, 0.5, 0.25, 0.5],
                                   [0.5, 0.25, 0.25, 0.5, 0.25, 0.5]])], 0)


# ---- conversion (float32, as the reference's numpy code runs it) ----------------------------------------------------

def boxes_to_camera(boxes, V2C, R0, P2, image_shape=None):
    """boxes (N, 7) lidar float32 -> cam (N, 7) [x, y, z, l, h, w, ry], img (N, 4), alpha (N), all float32."""
    boxes = np.asarray(boxes, dtype=np.float32)
    n = boxes.shape[0]
    xyz = boxes[:, 0:3].copy()
    xyz[:, 2] -= boxes[:, 5] / 2
    hom = np.hstack([xyz, np.ones((n, 1), dtype=np.float32)])
    loc = hom @ (V2C.T.astype(np.float32) @ R0.T.astype(np.float32))
    ry = (-boxes[:, 6] - np.float32(np.pi / 2)).astype(np.float32)
    l, w, h = boxes[:, 3], boxes[:, 4], boxes[:, 5]
    cam = np.concatenate([loc, l[:, None], h[:, None], w[:, None], ry[:, None]], 1).astype(np.float32)
    xs = np.stack([l / 2, l / 2, -l / 2, -l / 2] * 2, 1)
    zs = np.stack([w / 2, -w / 2, -w / 2, w / 2] * 2, 1)
    ys = np.concatenate([np.zeros((n, 4), np.float32), -np.repeat(h[:, None], 4, 1)], 1)
    c, s = np.cos(ry)[:, None], np.sin(ry)[:, None]
    px = loc[:, 0:1] + (xs * c + zs * s)
    py = loc[:, 1:2] + ys
    pz = loc[:, 2:3] + (-xs * s + zs * c)
    P2 = P2.astype(np.float32)
    u = (px * P2[0, 0] + py * P2[0, 1] + pz * P2[0, 2] + P2[0, 3]) / pz
    v = (px * P2[1, 0] + py * P2[1, 1] + pz * P2[1, 2] + P2[1, 3]) / pz
    img = np.stack([u.min(1), v.min(1), u.max(1), v.max(1)], 1).astype(np.float32)
    if image_shape is not None:
        img[:, [0, 2]] = np.clip(img[:, [0, 2]], 0, image_shape[1] - 1)
        img[:, [1, 3]] = np.clip(img[:, [1, 3]], 0, image_shape[0] - 1)
    alpha = (-np.arctan2(-boxes[:, 1], boxes[:, 0]) + ry).astype(np.float32)
    return cam, img, alpha


# ---- overlaps -------------------------------------------------------------------------------------------------------

def image_overlap(b, q):
    iw = min(b[2], q[2]) - max(b[0], q[0])
    if iw <= 0:
        return 0.0
    ih = min(b[3], q[3]) - max(b[1], q[1])
    if ih <= 0:
        return 0.0
    return iw * ih / ((b[2] - b[0]) * (b[3] - b[1]) + (q[2] - q[0]) * (q[3] - q[1]) - iw * ih)


def rotated_intersection(a, b):
    """area shared by two rectangles [x, y, dx, dy, angle] whose corners are turned by -angle, float64"""
    if math.hypot(a[0] - b[0], a[1] - b[1]) > 0.5 * (math.hypot(a[2], a[3]) + math.hypot(b[2], b[3])) + 1e-6:
        return 0.0
    cb, sb = math.cos(b[4]), math.sin(b[4])
    dx, dy = a[0] - b[0], a[1] - b[1]
    ox, oy = cb * dx - sb * dy, sb * dx + cb * dy
    t = b[4] - a[4]
    ct, st = math.cos(t), math.sin(t)
    poly = [(ct * x - st * y + ox, st * x + ct * y + oy)
            for x, y in ((-a[2] / 2, -a[3] / 2), (-a[2] / 2, a[3] / 2), (a[2] / 2, a[3] / 2), (a[2] / 2, -a[3] / 2))]
    for axis, sgn, lim in ((0, 1.0, b[2] / 2), (0, -1.0, b[2] / 2), (1, 1.0, b[3] / 2), (1, -1.0, b[3] / 2)):
        out = []
        for k in range(len(poly)):
            p, q = poly[k], poly[(k + 1) % len(poly)]
            c1, c2 = sgn * p[axis], sgn * q[axis]
            if c1 <= lim:
                out.append(p)
            if (c1 <= lim) != (c2 <= lim):
                u = (lim - c1) / (c2 - c1)
                out.append((p[0] + u * (q[0] - p[0]), p[1] + u * (q[1] - p[1])))
        poly = out
        if not poly:
            return 0.0
    if len(poly) < 3:
        return 0.0
    s2 = 0.0
    for k in range(1, len(poly) - 1):
        s2 += (poly[k][0] - poly[0][0]) * (poly[k + 1][1] - poly[0][1]) - (poly[k + 1][0] - poly[0][0]) * (poly[k][1] - poly[0][1])
    return abs(s2) / 2.0


def frame_overlaps(gt, dt, metric):
    """(ndt, ngt) float64 overlaps of one frame's annotation dicts"""
    ndt, ngt = len(dt['name']), len(gt['name'])
    out = np.zeros((ndt, ngt))
    for j in range(ndt):
        for i in range(ngt):
            if metric == 0:
                out[j, i] = image_overlap(np.asarray(dt['bbox'][j], np.float64), np.asarray(gt['bbox'][i], np.float64))
                continue
            b = [float(dt['location'][j][0]), float(dt['location'][j][2]), float(dt['dimensions'][j][0]), float(dt['dimensions'][j][2]),
                 float(dt['rotation_y'][j])]
            q = [float(gt['location'][i][0]), float(gt['location'][i][2]), float(gt['dimensions'][i][0]), float(gt['dimensions'][i][2]),
                 float(gt['rotation_y'][i])]
            inter = rotated_intersection(b, q)
            if metric == 1:
                out[j, i] = inter / (b[2] * b[3] + q[2] * q[3] - inter)
            elif inter > 0:
                by, bh, qy, qh = float(dt['location'][j][1]), float(dt['dimensions'][j][1]), float(gt['location'][i][1]), float(gt['dimensions'][i][1])
                iw = min(by, qy) - max(by - bh, qy - qh)
                if iw > 0:
                    inc = iw * inter
                    out[j, i] = inc / (b[2] * bh * b[3] + q[2] * qh * q[3] - inc)
    return out


# ---- clean_data -----------------------------------------------------------------------------------------------------

def clean_data(gt, dt, current_class, difficulty):
    """-> (number of valid ground truths, ignored_gt, ignored_dt, DontCare image boxes)"""
    cls = CLASS_NAMES[current_class]
    ignored_gt, ignored_dt, dc = [], [], []
    num_valid = 0
    for i in range(len(gt['name'])):
        name = str(gt['name'][i]).lower()
        height = gt['bbox'][i][3] - gt['bbox'][i][1]
        if name == cls:
            valid = 1
        elif (cls == 'pedestrian' and name == 'person_sitting') or (cls == 'car' and name == 'van'):
            valid = 0
        else:
            valid = -1
        ignore = bool(gt['occluded'][i] > MAX_OCCLUSION[difficulty] or gt['truncated'][i] > MAX_TRUNCATION[difficulty]
                      or height <= MIN_HEIGHT[difficulty])
        if valid == 1 and not ignore:
            ignored_gt.append(0)
            num_valid += 1
        elif valid == 0 or (ignore and valid == 1):
            ignored_gt.append(1)
        else:
            ignored_gt.append(-1)
        if str(gt['name'][i]) == 'DontCare':
            dc.append(np.asarray(gt['bbox'][i], np.float64))
    for j in range(len(dt['name'])):
        height = abs(float(dt['bbox'][j][3]) - float(dt['bbox'][j][1]))
        if height < MIN_HEIGHT[difficulty]:
            ignored_dt.append(1)
        elif str(dt['name'][j]).lower() == cls:
            ignored_dt.append(0)
        else:
            ignored_dt.append(-1)
    return num_valid, np.array(ignored_gt, np.int64), np.array(ignored_dt, np.int64), dc


# ---- statistics -----------------------------------------------------------------------------------------------------

def true_positive_scores(overlap, ign_gt, ign_dt, scores, min_overlap):
    """pass 1: every ground truth takes the best-scoring free detection that overlaps enough"""
    assigned = np.zeros(len(ign_dt), bool)
    out = []
    for i in range(len(ign_gt)):
        if ign_gt[i] == -1:
            continue
        det, best = -1, -10000000
        for j in range(len(ign_dt)):
            if ign_dt[j] == -1 or assigned[j]:
                continue
            if overlap[j, i] > min_overlap and scores[j] > best:
                det, best = j, scores[j]
        if det < 0:
            continue
        if not (ign_gt[i] == 1 or ign_dt[det] == 1):
            out.append(scores[det])
        assigned[det] = True
    return out


def statistics(overlap, ign_gt, ign_dt, scores, gt_alpha, dt_alpha, dt_bbox, dc_boxes, metric, min_overlap, thresholds, compute_aos):
    """pass 2 for all thresholds at once -> (T, 4) [tp, fp, fn, similarity]"""
    thresholds = np.asarray(thresholds, np.float64)
    T, ndt = thresholds.shape[0], len(ign_dt)
    scores = np.asarray(scores, np.float64)
    below = scores[None, :] < thresholds[:, None]
    assigned = np.zeros((T, ndt), bool)
    tp, fp, fn, sim = np.zeros(T, np.int64), np.zeros(T, np.int64), np.zeros(T, np.int64), np.zeros(T)
    rows = np.arange(T)
    for i in range(len(ign_gt)):
        if ign_gt[i] == -1:
            continue
        det = np.full(T, -1)
        max_ov = np.zeros(T)
        ign_pick = np.zeros(T, bool)
        for j in range(ndt):
            if ign_dt[j] == -1 or not overlap[j, i] > min_overlap:
                continue
            free = ~assigned[:, j] & ~below[:, j]
            if ign_dt[j] == 0:
                upd = free & ((overlap[j, i] > max_ov) | ign_pick)
                max_ov[upd] = overlap[j, i]
                det[upd] = j
                ign_pick[upd] = False
            else:
                upd = free & (det < 0)
                det[upd] = j
                ign_pick[upd] = True
        found = det >= 0
        if ign_gt[i] == 0:
            fn += ~found
        neutral = np.zeros(T, bool) if ndt == 0 else (ign_dt[np.maximum(det, 0)] == 1)
        is_tp = found & ~neutral & (ign_gt[i] != 1)
        tp += is_tp
        if compute_aos and ndt:
            delta = gt_alpha[i] - np.asarray(dt_alpha, np.float64)[np.maximum(det, 0)]
            sim += np.where(is_tp, (1.0 + np.cos(delta)) / 2.0, 0.0)
        assigned[rows[found], det[found]] = True
    counted = ~assigned & ~below & (np.asarray(ign_dt)[None, :] == 0)
    fp += counted.sum(1)
    if metric == 0:
        for q in dc_boxes:
            for j in range(ndt):
                if ign_dt[j] != 0:
                    continue
                b = np.asarray(dt_bbox[j], np.float64)
                iw = min(b[2], q[2]) - max(b[0], q[0])
                ih = min(b[3], q[3]) - max(b[1], q[1])
                o = iw * ih / ((b[2] - b[0]) * (b[3] - b[1])) if iw > 0 and ih > 0 else 0.0
                if o > min_overlap:
                    hit = ~assigned[:, j] & ~below[:, j]
                    assigned[hit, j] = True
                    fp -= hit
    return np.stack([tp, fp, fn, sim], 1)


def get_thresholds(scores, num_gt, num_sample_pts=41):
    scores = sorted((float(s) for s in scores), reverse=True)
    current_recall, out = 0, []
    for i, score in enumerate(scores):
        l_recall = (i + 1) / num_gt
        r_recall = (i + 2) / num_gt if i < len(scores) - 1 else l_recall
        if (r_recall - current_recall) < (current_recall - l_recall) and i < len(scores) - 1:
            continue
        out.append(score)
        current_recall += 1 / (num_sample_pts - 1.0)
    return out


def eval_class(gt_annos, dt_annos, current_classes, difficultys, metric, min_overlaps, compute_aos=False, overlaps=None,
               detail=None):
    """-> {'recall', 'precision', 'orientation'} (class, difficulty, overlap set, 41).  overlaps: per-frame (ndt, ngt)
    arrays to use instead of this module's own; detail: dict that receives flags / thresholds / pr per combination."""
    if overlaps is None:
        overlaps = [frame_overlaps(g, d, metric) for g, d in zip(gt_annos, dt_annos)]
    nC, nD, K = len(current_classes), len(difficultys), len(min_overlaps)
    precision, recall, aos = np.zeros([nC, nD, K, 41]), np.zeros([nC, nD, K, 41]), np.zeros([nC, nD, K, 41])
    for m, cls in enumerate(current_classes):
        for l, diff in enumerate(difficultys):
            cleaned = [clean_data(g, d, cls, diff) for g, d in zip(gt_annos, dt_annos)]
            total_valid = sum(c[0] for c in cleaned)
            if detail is not None:
                detail[('flags', m, l)] = (np.concatenate([c[1] for c in cleaned] + [np.zeros(0, np.int64)]),
                                           np.concatenate([c[2] for c in cleaned] + [np.zeros(0, np.int64)]), total_valid)
            for k, min_overlap in enumerate(min_overlaps[:, metric, m]):
                tps = []
                for f, (g, d) in enumerate(zip(gt_annos, dt_annos)):
                    tps += true_positive_scores(overlaps[f], cleaned[f][1], cleaned[f][2], d['score'], min_overlap)
                thresholds = np.array(get_thresholds(tps, total_valid))
                pr = np.zeros([len(thresholds), 4])
                for f, (g, d) in enumerate(zip(gt_annos, dt_annos)):
                    pr += statistics(overlaps[f], cleaned[f][1], cleaned[f][2], d['score'], np.asarray(g['alpha'], np.float64), d['alpha'],
                                     d['bbox'], cleaned[f][3], metric, min_overlap, thresholds, compute_aos)
                if detail is not None:
                    detail[('tp_scores', m, l, k)] = np.array(tps)
                    detail[('thresholds', m, l, k)] = thresholds
                    detail[('pr', m, l, k)] = pr
                n = len(thresholds)
                with np.errstate(divide='ignore', invalid='ignore'):
                    recall[m, l, k, :n] = pr[:, 0] / (pr[:, 0] + pr[:, 2])
                    precision[m, l, k, :n] = pr[:, 0] / (pr[:, 0] + pr[:, 1])
                    if compute_aos:
                        aos[m, l, k, :n] = pr[:, 3] / (pr[:, 0] + pr[:, 1])
                for i in range(n):
                    precision[m, l, k, i] = np.max(precision[m, l, k, i:])
                    recall[m, l, k, i] = np.max(recall[m, l, k, i:])
                    if compute_aos:
                        aos[m, l, k, i] = np.max(aos[m, l, k, i:])
    return {'recall': recall, 'precision': precision, 'orientation': aos}


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


def official_result(gt_annos, dt_annos, current_classes, overlaps=None, detail=None):
    """-> (text, ret_dict, maps, rets) with maps = the eight mAP arrays (bbox, bev, 3d, aos, then the R40 ones) and rets the
    three eval_class results.
    overlaps: {metric: per-frame arrays} to use instead of this module's own."""
    classes = [c if isinstance(c, int) else {v: k for k, v in CLASS_TO_NAME.items()}[c] for c in current_classes]
    min_overlaps = MIN_OVERLAPS[:, :, classes]
    compute_aos = False
    for anno in dt_annos:
        if len(anno['alpha']) != 0:
            compute_aos = bool(anno['alpha'][0] != -10)
            break
    rets = []
    for metric in range(3):
        sub = {} if detail is not None else None
        rets.append(eval_class(gt_annos, dt_annos, classes, [0, 1, 2], metric, min_overlaps, compute_aos and metric == 0,
                               None if overlaps is None else overlaps[metric], sub))
        if detail is not None:
            detail[metric] = sub
    maps = [get_mAP(rets[0]['precision']), get_mAP(rets[1]['precision']), get_mAP(rets[2]['precision']),
            get_mAP(rets[0]['orientation']) if compute_aos else None,
            get_mAP_R40(rets[0]['precision']), get_mAP_R40(rets[1]['precision']), get_mAP_R40(rets[2]['precision']),
            get_mAP_R40(rets[0]['orientation']) if compute_aos else None]
    text, ret_dict = '', {}
    rows = [('bbox', 0, '.4f'), ('bev ', 1, '.4f'), ('3d  ', 2, '.4f')] + ([('aos ', 3, '.2f')] if compute_aos else [])
    for j, cls in enumerate(classes):
        name = CLASS_TO_NAME[cls]
        for i in range(min_overlaps.shape[0]):
            for head, shift in (('AP', 0), ('AP_R40', 4)):
                text += '%s %s@%.2f, %.2f, %.2f:\n' % ((name, head) + tuple(min_overlaps[i, :, j]))
                for tag, idx, fmt in rows:
                    text += '%s AP:' % tag + ', '.join(format(maps[idx + shift][j, d, i], fmt) for d in range(3)) + '\n'
    for j, cls in enumerate(classes):
        name = CLASS_TO_NAME[cls]
        keys = ([('aos', 7)] if compute_aos else []) + [('3d', 6), ('bev', 5), ('image', 4)]
        for key, idx in keys:
            for d, diff in enumerate(('easy', 'moderate', 'hard')):
                ret_dict['%s_%s/%s_R40' % (name, key, diff)] = maps[idx][j, d, 0]
    return text, ret_dict, maps, rets


# ---- the committed fixture (tests/golden/ref_kitti_eval.npz) --------------------------------------------------------

def split_annos(count, **fields):
    """concatenated arrays + per-frame counts -> list of per-frame dicts"""
    out, k = [], 0
    for n in count:
        out.append({key: v[k:k + n] for key, v in fields.items()})
        k += n
    return out


def load_fixture(path):
    """-> (npz dict, gt annos, dt annos): the detections widened to float64, as the reference evaluated them"""
    z = dict(np.load(path))
    gts = split_annos(z['gt_count'], name=z['gt_name'], bbox=z['gt_bbox'], alpha=z['gt_alpha'], location=z['gt_location'],
                      dimensions=z['gt_dimensions'], rotation_y=z['gt_rotation_y'], occluded=z['gt_occluded'],
                      truncated=z['gt_truncated'])
    F, P = z['pred_scores'].shape
    live = np.arange(P)[None, :] < z['pred_count'][:, None]
    dts = split_annos(z['pred_count'], name=z['dt_name'], bbox=z['dt_bbox'].astype(np.float64), alpha=z['dt_alpha'].astype(np.float64),
                      location=z['dt_location'].astype(np.float64), dimensions=z['dt_dimensions'].astype(np.float64),
                      rotation_y=z['dt_rotation_y'].astype(np.float64), score=z['pred_scores'][live].astype(np.float64))
    return z, gts, dts


def fixture_overlaps(z):
    """{metric: per-frame (ndt, ngt) arrays} of the fixture"""
    out = {}
    for m, key in enumerate(('overlaps_bbox', 'overlaps_bev', 'overlaps_3d')):
        k, frames = 0, []
        for ng, nd in zip(z['gt_count'], z['pred_count']):
            frames.append(z[key][k:k + ng * nd].reshape(nd, ng))
            k += ng * nd
        out[m] = frames
    return out


# ---- seeded synthetic annotations beyond the fixture ----------------------------------------------------------------

_SIZES = {'Car': (3.9, 1.56, 1.6), 'Van': (5.0, 2.2, 1.9), 'Pedestrian': (0.8, 1.73, 0.6), 'Person_sitting': (0.8, 1.3, 0.6),
          'Cyclist': (1.76, 1.73, 0.6), 'DontCare': (1.0, 1.0, 1.0)}
_NAMES = ['Car', 'Pedestrian', 'Cyclist', 'Van', 'Person_sitting', 'DontCare']


def _draw_frame(rng, ngt, max_false=4):
    nm = rng.choice(_NAMES, ngt, p=[.3, .25, .25, .07, .05, .08])
    loc = np.stack([rng.uniform(-20, 20, ngt), rng.uniform(1, 2, ngt), rng.uniform(5, 60, ngt)], 1)
    dim = np.array([_SIZES[n] for n in nm]).reshape(ngt, 3) * rng.uniform(0.9, 1.1, (ngt, 3))
    ry = rng.uniform(-np.pi, np.pi, ngt)
    x1, y1 = rng.uniform(0, 1000, ngt), rng.uniform(0, 250, ngt)
    hgt = rng.choice([20., 30., 33., 50., 60., 90.], ngt, p=[.08, .12, .1, .3, .2, .2]) + rng.uniform(1, 4, ngt)
    bbox = np.stack([x1, y1, x1 + rng.uniform(20, 200, ngt), y1 + hgt], 1)
    gt = dict(name=nm.astype('<U16'), truncated=rng.choice([0, 0.2, 0.4, 0.6], ngt, p=[.6, .2, .15, .05]),
              occluded=rng.choice([0., 1., 2., 3.], ngt, p=[.55, .25, .15, .05]), alpha=rng.uniform(-3, 3, ngt), bbox=bbox,
              dimensions=dim, location=loc, rotation_y=ry)
    keep = (nm != 'DontCare') & (rng.random(ngt) < 0.8)
    k, nf = int(keep.sum()), int(rng.integers(1, max_false + 1))
    shown = np.where(nm[keep] == 'Van', 'Car', np.where(nm[keep] == 'Person_sitting', 'Pedestrian', nm[keep]))
    dn = np.concatenate([np.where(rng.random(k) < 0.9, shown, 'Car'), rng.choice(_NAMES[:3], nf)])
    sig = rng.choice([0.03, 0.12, 0.3], (k, 1))
    dl = np.concatenate([loc[keep] + rng.normal(0, 1, (k, 3)) * sig,
                         np.stack([rng.uniform(-20, 20, nf), rng.uniform(1, 2, nf), rng.uniform(5, 60, nf)], 1)])
    dd = np.concatenate([dim[keep] * rng.uniform(0.95, 1.05, (k, 3)), np.array([_SIZES[n] for n in dn[k:]]).reshape(nf, 3)])
    dr = np.concatenate([ry[keep] + rng.normal(0, 0.05, k), rng.uniform(-3, 3, nf)])
    # false detections: half of them inside a DontCare region when the frame has one
    dc = bbox[nm == 'DontCare']
    fx, fy = rng.uniform(0, 1000, nf), rng.uniform(0, 250, nf)
    fb = np.stack([fx, fy, fx + 60, fy + rng.choice([22., 45., 70.], nf)], 1)
    for i in range(nf):
        if len(dc) and rng.random() < 0.5:
            q = dc[int(rng.integers(0, len(dc)))]
            fb[i] = [q[0] + 1, q[1] + 1, q[0] + 0.6 * (q[2] - q[0]), q[1] + 0.9 * (q[3] - q[1])]
    db = np.concatenate([bbox[keep] + rng.normal(0, 1, (k, 4)) * rng.choice([1., 6., 15.], (k, 1)), fb])
    sc = np.round(np.concatenate([rng.uniform(0.3, 1, k), rng.uniform(0.05, 0.8, nf)]), 2)
    dt = dict(name=dn.astype('<U16'), alpha=np.concatenate([gt['alpha'][keep] + rng.normal(0, .1, k), rng.uniform(-3, 3, nf)]), bbox=db,
              dimensions=dd, location=dl, rotation_y=dr, score=sc)
    return gt, dt


def frame_is_robust(gt, dt, margin, overlaps=None):
    """no overlap within margin of 0.25 / 0.5 / 0.7 and no image-box height within margin of 25 / 40 (float64)"""
    for bb in (gt['bbox'], dt['bbox']):
        h = np.abs(bb[:, 3] - bb[:, 1])
        if len(h) and min(np.abs(h - 25).min(), np.abs(h - 40).min()) < margin:
            return False
    for metric in range(3):
        ov = frame_overlaps(gt, dt, metric) if overlaps is None else overlaps[metric]
        if ov.size and min(np.abs(ov - th).min() for th in (0.25, 0.5, 0.7)) < margin:
            return False
    return True


def synthetic_frames(seed, num_frames, margin=1e-3, gt_range=(4, 16), check=True):
    """-> (gt annos, dt annos): a seeded set in which no matching decision is fragile (frames are redrawn until
    frame_is_robust holds; check=False skips that, for timing runs on large sets)"""
    rng = np.random.default_rng(seed)
    gts, dts = [], []
    while len(gts) < num_frames:
        gt, dt = _draw_frame(rng, int(rng.integers(gt_range[0], gt_range[1])))
        if check and not frame_is_robust(gt, dt, margin):
            continue
        gts.append(gt)
        dts.append(dt)
    return gts, dts

#!/usr/bin/env python3
"""Generates tests/golden/ref_kitti_eval.npz (+ ref_kitti_eval.json, the result text and ret_dict) by running the
REFERENCE's own evaluator and conversion code on the CPU: kitti_object_eval_python/eval.py (get_official_eval_result and
everything under it), rotate_iou.py (devRotateIoUEval), pcdet/utils/box_utils.py (boxes3d_lidar_to_kitti_camera,
boxes3d_kitti_camera_to_imageboxes, boxes3d_kitti_camera_to_lidar) and calibration_kitti.Calibration, imported from where
they lie, nothing copied.  Only what this image lacks is replaced:
  - numba by a stand-in whose jit (bare and with arguments) returns the function, numba.cuda.jit likewise,
    cuda.local.array / cuda.shared.array -> np.zeros(shape, np.float32);
  - the host launcher rotate_iou_gpu_eval by a double loop that calls devRotateIoUEval per pair on float32 copies (pairs
    whose bounding circles are disjoint get the 0 the function would return);
  - roiaware_pool3d_utils and SharedArray (imported by box_utils / common_utils, never called here) by empty modules.
The evaluator's intermediate results are recorded by wrapping clean_data, get_thresholds and fused_compute_statistics.

The scene: 60 seeded synthetic frames in rect camera coordinates with a KITTI-like calibration; ground-truth image boxes
are the projections of the 3D boxes; detections are perturbed ground truths taken to the lidar frame and brought back by
the reference's conversion (then widened to float64, as annotations read from KITTI result files are), plus false
detections, some of them inside DontCare regions.  Frames are redrawn until no decision is fragile: every within-frame
overlap is at least M = 1e-3 from 0.25 / 0.5 / 0.7 and every image-box height at least M pixels from 25 and 40.  The
coverage conditions of the fixture are asserted at the end.  Run in the authoring container only (needs the reference
tree); the outputs are committed.
"""
import importlib.util
import json
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = '/root/reference'
EVAL_DIR = f'{REF}/pcdet/datasets/kitti/kitti_object_eval_python'
M = 1e-3
F = 60
P = 32
CLASS_NAMES = ['Car', 'Pedestrian', 'Cyclist']
SIZES = {'Car': (3.9, 1.56, 1.6), 'Van': (5.0, 2.2, 1.9), 'Pedestrian': (0.8, 1.73, 0.6), 'Person_sitting': (0.8, 1.3, 0.6),
         'Cyclist': (1.76, 1.73, 0.6)}   # l, h, w
IMAGE_SHAPE = np.array([375, 1242], dtype=np.int32)


def install_reference():
    nb = types.ModuleType('numba')

    def jit(*a, **k):
        if len(a) == 1 and callable(a[0]) and not k:
            return a[0]
        return lambda f: f
    nb.jit, nb.float32, nb.prange = jit, np.float32, range
    cu = types.ModuleType('numba.cuda')
    cu.jit = jit
    cu.local = types.SimpleNamespace(array=lambda shape, dtype=None: np.zeros(shape, np.float32))
    cu.shared = cu.local
    nb.cuda = cu
    sys.modules['numba'], sys.modules['numba.cuda'] = nb, cu

    def pkg(name, path=None):
        m = types.ModuleType(name)
        m.__path__ = [path] if path else []
        sys.modules[name] = m
        return m
    pkg('kev', EVAL_DIR)

    def load(name, path):
        spec = importlib.util.spec_from_file_location(name, path)
        m = importlib.util.module_from_spec(spec)
        sys.modules[name] = m
        spec.loader.exec_module(m)
        return m
    ri = load('kev.rotate_iou', f'{EVAL_DIR}/rotate_iou.py')

    def host_rotate_iou(boxes, query_boxes, criterion=-1, device_id=0):
        b, q = boxes.astype(np.float32), query_boxes.astype(np.float32)
        out = np.zeros((len(b), len(q)), np.float32)
        for i in range(len(b)):
            for j in range(len(q)):
                if np.hypot(b[i, 0] - q[j, 0], b[i, 1] - q[j, 1]) > 0.5 * (np.hypot(b[i, 2], b[i, 3]) + np.hypot(q[j, 2], q[j, 3])) + 0.01:
                    continue
                out[i, j] = ri.devRotateIoUEval(q[j].copy(), b[i].copy(), criterion)
        return out.astype(boxes.dtype)
    ri.rotate_iou_gpu_eval = host_rotate_iou
    ev = load('kev.eval', f'{EVAL_DIR}/eval.py')
    pkg('pcdet', f'{REF}/pcdet')
    pkg('pcdet.utils', f'{REF}/pcdet/utils')
    pkg('pcdet.ops', f'{REF}/pcdet/ops')
    roi = pkg('pcdet.ops.roiaware_pool3d')
    roi.roiaware_pool3d_utils = types.ModuleType('pcdet.ops.roiaware_pool3d.roiaware_pool3d_utils')
    sys.modules[roi.roiaware_pool3d_utils.__name__] = roi.roiaware_pool3d_utils
    sys.modules['SharedArray'] = types.ModuleType('SharedArray')
    from pcdet.utils import box_utils, calibration_kitti
    return ev, ri, box_utils, calibration_kitti


def make_calib(rng, calibration_kitti):
    P2 = np.array([[721.5377, 0, 609.5593, 44.85728], [0, 721.5377, 172.854, 0.2163791], [0, 0, 1, 0.002745884]], np.float32)
    P2[0, 2] += rng.uniform(-3, 3)
    P2[1, 2] += rng.uniform(-3, 3)
    a = rng.uniform(-0.01, 0.01, 3)
    R0 = np.array([[1, -a[2], a[1]], [a[2], 1, -a[0]], [-a[1], a[0], 1]], np.float32)
    V2C = np.array([[7.533745e-04, -9.999714e-01, -6.166020e-03, -4.069766e-03],
                    [1.480249e-02, 7.280733e-04, -9.998902e-01, -7.631618e-02],
                    [9.998621e-01, 7.523790e-04, 1.480755e-02, -2.717806e-01]], np.float32)
    V2C[:, 3] += rng.uniform(-0.02, 0.02, 3).astype(np.float32)
    d = {'P2': P2, 'R0': R0, 'Tr_velo2cam': V2C}
    return d, calibration_kitti.Calibration(d)


def draw_camera_box(rng, name, z_lo=6.0, z_hi=58.0):
    z = z_lo + (z_hi - z_lo) * rng.random() ** 1.7
    x = rng.uniform(-0.55, 0.55) * z
    l, h, w = np.array(SIZES[name]) * rng.uniform(0.9, 1.1, 3)
    return np.array([x, rng.uniform(1.4, 1.9), z, l, h, w, rng.uniform(-np.pi, np.pi)])


def draw_frame(rng, box_utils, calibration_kitti, ngt, with_dt=True, extras=True):
    """-> (gt anno, calib dict, lidar boxes (n, 7) f32, scores f32, labels int64)"""
    cd, calib = make_calib(rng, calibration_kitti)
    names = list(rng.choice(['Car', 'Pedestrian', 'Cyclist', 'Van', 'Person_sitting'], ngt, p=[.32, .25, .25, .1, .08])) if ngt else []
    cam = np.stack([draw_camera_box(rng, n) for n in names]) if ngt else np.zeros((0, 7))
    bbox = box_utils.boxes3d_kitti_camera_to_imageboxes(cam, calib, image_shape=IMAGE_SHAPE).astype(np.float64) if ngt else np.zeros((0, 4))
    occluded = rng.choice([0, 1, 2, 3], ngt, p=[.55, .25, .15, .05]).astype(np.float64)
    truncated = rng.choice([0, 0.2, 0.4, 0.6], ngt, p=[.6, .2, .15, .05])
    det_cam, det_label, det_score = [], [], []
    label_of = {'Car': 1, 'Pedestrian': 2, 'Cyclist': 3, 'Van': 1, 'Person_sitting': 2}
    for i in range(ngt):
        if not with_dt or rng.random() > 0.82:
            continue
        sig = rng.choice([0.02, 0.08, 0.25], p=[.45, .35, .2])
        b = cam[i].copy()
        b[:3] += rng.normal(0, 1, 3) * sig * np.array([1, 0.3, 1]) * min(1.0, cam[i, 5] / 1.2)   # smaller footprints move less
        b[3:6] *= rng.uniform(0.96, 1.04, 3)
        b[6] += rng.normal(0, 0.04)
        lab = label_of[names[i]] if rng.random() < 0.92 else int(rng.integers(1, 4))
        sc = np.round(rng.uniform(0.3, 1.0), 2)
        det_cam.append(b); det_label.append(lab); det_score.append(sc)
        r = rng.random()
        if extras and r < 0.10:      # a second detection with the SAME score, slightly moved
            b2 = b.copy(); b2[0] += 0.05
            det_cam.append(b2); det_label.append(lab); det_score.append(sc)
        elif extras and r < 0.20:    # an identical box (equal overlap in every metric) with a lower score
            det_cam.append(b.copy()); det_label.append(lab); det_score.append(np.round(sc - 0.1, 2))
    n_false = int(rng.integers(1, 5)) if with_dt else 0
    for _ in range(n_false):
        nm = CLASS_NAMES[int(rng.integers(0, 3))]
        det_cam.append(draw_camera_box(rng, nm)); det_label.append(label_of[nm]); det_score.append(np.round(rng.uniform(0.05, 0.8), 2))
    # DontCare regions around phantom objects that are detected but not annotated
    n_dc = int(rng.integers(0, 3)) if ngt else 0
    dc_boxes = []
    for _ in range(n_dc):
        nm = CLASS_NAMES[int(rng.integers(0, 3))]
        ph = draw_camera_box(rng, nm, 8.0, 30.0)
        bb = box_utils.boxes3d_kitti_camera_to_imageboxes(ph[None], calib, image_shape=IMAGE_SHAPE)[0].astype(np.float64)
        dc_boxes.append(bb + np.array([-6, -6, 6, 6]))
        if with_dt:
            det_cam.append(ph); det_label.append(label_of[nm]); det_score.append(np.round(rng.uniform(0.2, 0.9), 2))
    if n_dc:
        names += ['DontCare'] * n_dc
        cam = np.concatenate([cam, np.tile(np.array([-1000., -1000, -1000, -1, -1, -1, -10]), (n_dc, 1))])
        bbox = np.concatenate([bbox, np.stack(dc_boxes)])
        occluded = np.concatenate([occluded, -np.ones(n_dc)])
        truncated = np.concatenate([truncated, -np.ones(n_dc)])
    n = len(names)
    alpha = np.where(np.array(names) == 'DontCare', -10.0, -np.arctan2(cam[:, 0], cam[:, 2]) + cam[:, 6]) if n else np.zeros(0)
    gt = {'name': np.array(names, dtype='<U16') if n else np.zeros(0, dtype='<U16'), 'truncated': truncated, 'occluded': occluded,
          'alpha': alpha, 'bbox': bbox.reshape(n, 4), 'dimensions': cam[:, 3:6].reshape(n, 3), 'location': cam[:, 0:3].reshape(n, 3),
          'rotation_y': cam[:, 6].reshape(n)}
    if det_cam:
        order = rng.permutation(len(det_cam))[:P]
        lidar = box_utils.boxes3d_kitti_camera_to_lidar(np.stack(det_cam)[order], calib).astype(np.float32)
        return gt, cd, lidar, np.array(det_score, np.float32)[order], np.array(det_label, np.int64)[order]
    return gt, cd, np.zeros((0, 7), np.float32), np.zeros(0, np.float32), np.zeros(0, np.int64)


def reference_prediction(box_utils, calibration_kitti, cd, lidar, scores, labels):
    """kitti_dataset.generate_prediction_dicts' single-sample body on numpy inputs (its own lines call torch .cpu() only)."""
    n = scores.shape[0]
    d = {'name': np.zeros(n), 'truncated': np.zeros(n), 'occluded': np.zeros(n), 'alpha': np.zeros(n), 'bbox': np.zeros([n, 4]),
         'dimensions': np.zeros([n, 3]), 'location': np.zeros([n, 3]), 'rotation_y': np.zeros(n), 'score': np.zeros(n),
         'boxes_lidar': np.zeros([n, 7])}
    if n == 0:
        return d
    calib = calibration_kitti.Calibration(cd)
    cam = box_utils.boxes3d_lidar_to_kitti_camera(lidar, calib)
    img = box_utils.boxes3d_kitti_camera_to_imageboxes(cam, calib, image_shape=IMAGE_SHAPE)
    d['name'] = np.array(CLASS_NAMES)[labels - 1]
    d['alpha'] = -np.arctan2(-lidar[:, 1], lidar[:, 0]) + cam[:, 6]
    d['bbox'], d['dimensions'], d['location'], d['rotation_y'] = img, cam[:, 3:6], cam[:, 0:3], cam[:, 6]
    d['score'], d['boxes_lidar'] = scores, lidar
    return d


def widen(d):
    return {k: (v.astype(np.float64) if v.dtype.kind == 'f' else v) for k, v in d.items()}


def robust(ev, gt, dt):
    """no fragile decision in this frame"""
    for bb in (gt['bbox'], dt['bbox']):
        if len(bb):
            hgt = np.abs(bb[:, 3] - bb[:, 1])
            if (np.abs(hgt - 25) < M).any() or (np.abs(hgt - 40) < M).any():
                return False
    if len(gt['name']) == 0 or len(dt['name']) == 0:
        return True
    for metric in range(3):
        ov = ev.calculate_iou_partly([dt], [gt], metric, 100)[0][0]
        for th in (0.25, 0.5, 0.7):
            if (np.abs(ov - th) < M).any():
                return False
    return True


def run_reference(ev, gt_annos, dt_annos):
    rec = {'clean': [], 'thr': [], 'pr': []}
    orig = (ev.clean_data, ev.get_thresholds, ev.fused_compute_statistics)

    def clean_data(gt, dt, cls, diff):
        r = orig[0](gt, dt, cls, diff)
        rec['clean'].append((cls, diff, r[0], list(r[1]), list(r[2])))
        return r

    def get_thresholds(scores, num_gt, num_sample_pts=41):
        s = np.array(scores, dtype=np.float64).copy()
        r = orig[1](scores, num_gt, num_sample_pts)
        rec['thr'].append((s, int(num_gt), np.array(r, dtype=np.float64)))
        return r

    def fused(overlaps, pr, *a, **k):
        orig[2](overlaps, pr, *a, **k)
        rec['pr'].append(pr)      # one part only (F < num_parts), so pr is final after this call
    ev.clean_data, ev.get_thresholds, ev.fused_compute_statistics = clean_data, get_thresholds, fused
    try:
        detail = {}
        text, ret = ev.get_official_eval_result(gt_annos, dt_annos, CLASS_NAMES, PR_detail_dict=detail)
    finally:
        ev.clean_data, ev.get_thresholds, ev.fused_compute_statistics = orig
    return text, ret, detail, rec


def ev_min_overlaps():
    o7 = np.array([[0.7, 0.5, 0.5, 0.7, 0.5, 0.7]] * 3)
    o5 = np.array([[0.7, 0.5, 0.5, 0.7, 0.5, 0.5], [0.5, 0.25, 0.25, 0.5, 0.25, 0.5], [0.5, 0.25, 0.25, 0.5, 0.25, 0.5]])
    return np.stack([o7, o5], 0)[:, :, [0, 1, 2]]


def main():
    ev, ri, box_utils, calibration_kitti = install_reference()
    rng = np.random.default_rng(20261016)
    frames, redraws = [], 0
    while len(frames) < F:
        f = len(frames)
        ngt = 0 if f in (5, 13) else int(rng.integers(7, 16))
        with_dt = f not in (9, 13)
        gt, cd, lidar, scores, labels = draw_frame(rng, box_utils, calibration_kitti, ngt, with_dt)
        dt32 = reference_prediction(box_utils, calibration_kitti, cd, lidar, scores, labels)
        dt = widen(dt32)
        if not robust(ev, gt, dt):
            redraws += 1
            continue
        frames.append((gt, cd, lidar, scores, labels, dt32, dt))
    gts, dts = [fr[0] for fr in frames], [fr[6] for fr in frames]
    print('frames', F, 'redrawn', redraws, 'gt', sum(len(g['name']) for g in gts), 'dt', sum(len(d['name']) for d in dts))

    text, ret, detail, rec = run_reference(ev, gts, dts)
    # the eight mAP arrays and the curves, from eval_class itself
    mo = ev_min_overlaps()
    curves = [ev.eval_class(gts, dts, [0, 1, 2], [0, 1, 2], m, mo, compute_aos=(m == 0)) for m in range(3)]
    maps = {'mAP_bbox': ev.get_mAP(curves[0]['precision']), 'mAP_bev': ev.get_mAP(curves[1]['precision']),
            'mAP_3d': ev.get_mAP(curves[2]['precision']), 'mAP_aos': ev.get_mAP(curves[0]['orientation']),
            'mAP_bbox_R40': ev.get_mAP_R40(curves[0]['precision']), 'mAP_bev_R40': ev.get_mAP_R40(curves[1]['precision']),
            'mAP_3d_R40': ev.get_mAP_R40(curves[2]['precision']), 'mAP_aos_R40': ev.get_mAP_R40(curves[0]['orientation'])}
    assert np.array_equal(detail['bbox'], curves[0]['precision']) and np.array_equal(detail['3d'], curves[2]['precision'])
    overlaps = [ev.calculate_iou_partly(dts, gts, m, 100)[0] for m in range(3)]

    # ---- the recorded intermediates, in combination order (metric, class, difficulty, overlap set) ---------------
    assert len(rec['thr']) == 54 and len(rec['pr']) == 54 and len(rec['clean']) == 3 * 9 * F
    thresholds = np.zeros((54, 41)); nthr = np.zeros(54, np.int32); pr = np.zeros((54, 41, 4))
    tp_scores, tp_len, valid = [], [], np.zeros(54, np.int64)
    for t in range(54):
        s, num_gt, th = rec['thr'][t]
        nthr[t] = len(th); thresholds[t, :len(th)] = th; pr[t, :len(th)] = rec['pr'][t]
        tp_scores.append(np.sort(s)); tp_len.append(len(s)); valid[t] = num_gt
    ign_gt = np.zeros((9, sum(len(g['name']) for g in gts)), np.int8)
    ign_dt = np.zeros((9, sum(len(d['name']) for d in dts)), np.int8)
    for cdx in range(9):
        block = rec['clean'][cdx * F:(cdx + 1) * F]        # metric 0's calls: (class, difficulty) major, frames minor
        assert all(b[0] == cdx // 3 and b[1] == cdx % 3 for b in block)
        ign_gt[cdx] = np.concatenate([np.array(b[3], np.int8) for b in block])
        ign_dt[cdx] = np.concatenate([np.array(b[4], np.int8) for b in block])

    # ---- coverage conditions ---------------------------------------------------------------------------------------
    r40 = np.stack([maps['mAP_bbox_R40'], maps['mAP_bev_R40'], maps['mAP_3d_R40']])          # (metric, class, diff, k)
    for t in range(54):
        mi, c, d, k = t // 18, (t // 6) % 3, (t // 2) % 3, t % 2
        n = nthr[t]
        low = pr[t, n - 1]
        print('combination', t, (mi, c, d, k), 'thresholds', n, 'lowest', low[:3], 'AP_R40 %.2f' % r40[mi, c, d, k])
        assert n >= 10, (t, n)
        assert low[0] > 0 and low[1] > 0 and low[2] > 0, (t, low)
        assert 5 < r40[mi, c, d, k] < 95, (t, r40[mi, c, d, k])
    allnames = np.concatenate([g['name'] for g in gts])
    assert (allnames == 'Van').sum() > 3 and (allnames == 'Person_sitting').sum() > 3 and (allnames == 'DontCare').sum() > 3
    occ = np.concatenate([g['occluded'] for g in gts]); tru = np.concatenate([g['truncated'] for g in gts])
    hgt = np.concatenate([g['bbox'][:, 3] - g['bbox'][:, 1] for g in gts])
    real = ~np.isin(allnames, ['DontCare'])
    for d in range(3):
        o, tr, hh = occ > [0, 1, 2][d], tru > [0.15, 0.3, 0.5][d], hgt <= [40, 25, 25][d]
        assert (real & o & ~tr & ~hh).any() and (real & ~o & tr & ~hh).any() and (real & ~o & ~tr & hh).any(), d
    dth = np.concatenate([np.abs(d['bbox'][:, 3] - d['bbox'][:, 1]) for d in dts if len(d['name'])])
    assert (dth < 25).any() and ((dth >= 25) & (dth < 40)).any()
    assert (ign_gt == 1).any() and (ign_dt == 1).any()
    # neutral ground truths that take a detection: a Van under a Car detection, a Person_sitting under a Pedestrian one
    neutral_hit = {'Van': 0, 'Person_sitting': 0}
    for f, (g, d) in enumerate(zip(gts, dts)):
        for i, nm in enumerate(g['name']):
            if nm in neutral_hit and len(d['name']):
                want = 'Car' if nm == 'Van' else 'Pedestrian'
                neutral_hit[nm] += int(((overlaps[2][f][:, i] > 0.5) & (d['name'] == want)).any())
    assert neutral_hit['Van'] > 0 and neutral_hit['Person_sitting'] > 0, neutral_hit
    # equal scores on one ground truth, equal overlaps on one ground truth, scores equal to a threshold
    eq_score = eq_overlap = 0
    for f, d in enumerate(dts):
        for i in range(len(gts[f]['name'])):
            hit = np.nonzero(overlaps[2][f][:, i] > 0.25)[0] if len(d['name']) else []
            for a in hit:
                for b in hit:
                    if a < b:
                        eq_score += int(d['score'][a] == d['score'][b])
                        eq_overlap += int(overlaps[2][f][a, i] == overlaps[2][f][b, i] and overlaps[0][f][a, i] == overlaps[0][f][b, i])
    allscores = np.concatenate([d['score'] for d in dts])
    on_thr = sum(int((allscores == th).sum() > 1) for t in range(54) for th in thresholds[t, :nthr[t]])
    assert eq_score > 0 and eq_overlap > 0 and on_thr > 0, (eq_score, eq_overlap, on_thr)
    # DontCare regions remove false positives: without them fp changes
    stripped = []
    for g in gts:
        keep = g['name'] != 'DontCare'
        stripped.append({k: v[keep] for k, v in g.items()})
    _, _, _, rec2 = run_reference(ev, stripped, dts)
    changed = sum(int((rec2['pr'][t][:, 1] != rec['pr'][t][:, 1]).any()) for t in range(18)
                  if rec2['pr'][t].shape == rec['pr'][t].shape)
    assert changed > 0, 'DontCare boxes change no fp count'
    # margins, once more over the whole set
    closest = 1.0
    for m in range(3):
        a = np.concatenate([o.ravel() for o in overlaps[m]])
        for th in (0.25, 0.5, 0.7):
            closest = min(closest, float(np.abs(a - th).min()))
    assert closest >= M, closest
    print('thresholds per combination', nthr.min(), '..', nthr.max(), '| AP_R40', r40.min(), '..', r40.max(), '| closest overlap', closest,
          '| fp changed by DontCare in', changed, 'bbox combinations | pairs', sum(o.size for o in overlaps[0]))

    # ---- write -----------------------------------------------------------------------------------------------------
    def cat(annos, key, width=None):
        parts = [np.asarray(a[key], np.float64).reshape((-1,) if width is None else (-1, width)) for a in annos]
        return np.concatenate(parts, 0)
    cnt = np.zeros(F, np.int32)
    boxes = np.zeros((F, P, 7), np.float32); scores = np.zeros((F, P), np.float32); labels = np.ones((F, P), np.int64)
    for f, fr in enumerate(frames):
        n = len(fr[3]); cnt[f] = n
        boxes[f, :n], scores[f, :n], labels[f, :n] = fr[2], fr[3], fr[4]
    dt32 = [fr[5] for fr in frames]
    out = {
        'margin': np.float64(M), 'image_shape': np.tile(IMAGE_SHAPE, (F, 1)),
        'V2C': np.stack([fr[1]['Tr_velo2cam'] for fr in frames]), 'R0': np.stack([fr[1]['R0'] for fr in frames]),
        'P2': np.stack([fr[1]['P2'] for fr in frames]),
        'pred_boxes': boxes, 'pred_scores': scores, 'pred_labels': labels, 'pred_count': cnt,
        'gt_count': np.array([len(g['name']) for g in gts], np.int32), 'gt_name': np.concatenate([g['name'] for g in gts]),
        'gt_bbox': cat(gts, 'bbox', 4), 'gt_alpha': cat(gts, 'alpha'), 'gt_location': cat(gts, 'location', 3),
        'gt_dimensions': cat(gts, 'dimensions', 3), 'gt_rotation_y': cat(gts, 'rotation_y'), 'gt_occluded': cat(gts, 'occluded'),
        'gt_truncated': cat(gts, 'truncated'),
        # the reference's conversion, float32 as it returns it (the evaluation ran on these widened to float64)
        'dt_name': np.concatenate([d['name'] for d in dt32 if len(d['score'])]),
        'dt_bbox': np.concatenate([d['bbox'] for d in dt32 if len(d['score'])]).astype(np.float32),
        'dt_alpha': np.concatenate([d['alpha'] for d in dt32 if len(d['score'])]).astype(np.float32),
        'dt_location': np.concatenate([d['location'] for d in dt32 if len(d['score'])]).astype(np.float32),
        'dt_dimensions': np.concatenate([d['dimensions'] for d in dt32 if len(d['score'])]).astype(np.float32),
        'dt_rotation_y': np.concatenate([d['rotation_y'] for d in dt32 if len(d['score'])]).astype(np.float32),
        'overlaps_bbox': np.concatenate([o.ravel() for o in overlaps[0]]), 'overlaps_bev': np.concatenate([o.ravel() for o in overlaps[1]]),
        'overlaps_3d': np.concatenate([o.ravel() for o in overlaps[2]]),
        'ign_gt': ign_gt, 'ign_dt': ign_dt, 'valid_gt': valid, 'tp_scores': np.concatenate(tp_scores), 'tp_len': np.array(tp_len, np.int32),
        'thresholds': thresholds, 'num_thresholds': nthr, 'pr': pr,
        'precision': np.stack([c['precision'] for c in curves]), 'recall': np.stack([c['recall'] for c in curves]),
        'orientation': curves[0]['orientation'],
    }
    for d in dt32:
        if len(d['score']):
            assert d['bbox'].dtype == np.float32 and d['location'].dtype == np.float32 and d['alpha'].dtype == np.float32
    out.update(maps)
    np.savez_compressed(os.path.join(HERE, 'ref_kitti_eval.npz'), **out)
    with open(os.path.join(HERE, 'ref_kitti_eval.json'), 'w') as fh:
        json.dump({'result': text, 'ret_dict': {k: float(v) for k, v in ret.items()}}, fh, indent=1)
    print(text)
    print('wrote', os.path.getsize(os.path.join(HERE, 'ref_kitti_eval.npz')), 'bytes')


if __name__ == '__main__':
    main()

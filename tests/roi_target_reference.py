"""numpy restatement of pdm_proposal_targets (pdm_ssd_amd/csrc/roi_targets.hip): the ground-truth row rule, the per-RoI best
3-D IoU and its ground truth, the fg / hard bg / easy bg split, the count rules of subsample_rois / sample_bg_inds, the
written draw rule, the gather, both label types and the canonical ground truth.  IoUs come from the CPU oracle's
boxes_overlap_bev plus the height and volume arithmetic of iou3d_nms_utils._iou3d_from_overlap in fp32.  The checker of
the device operator (tests/test_roi_targets_gpu.py) and the source of the draw that tests/golden/gen_roi_target_fixtures.py
hands to the reference's own code.  KNOWN_FOLDS and KNOWN_COUNTS are hand-derived answers for the two rules that are
easiest to get wrong."""
import numpy as np

F = np.float32
M32 = 0xFFFFFFFF
PI, TWO_PI, HALF_PI, THREE_HALF_PI = F(np.pi), F(2 * np.pi), F(np.pi * 0.5), F(np.pi * 1.5)


def fmix32(h):
    h &= M32
    h ^= h >> 16
    h = (h * 0x85EBCA6B) & M32
    h ^= h >> 13
    h = (h * 0xC2B2AE35) & M32
    h ^= h >> 16
    return h


def draw_key(seed, step, b, s):
    return fmix32(fmix32((seed ^ (step * 0x85EBCA6B)) & M32) ^ ((b * 0x9E3779B1) & M32) ^ ((s * 0x7F4A7C15) & M32))


def feistel_perm(i, n, kp):
    w = 1
    while (1 << (2 * w)) < n:
        w += 1
    mask = (1 << w) - 1
    x = i
    while True:
        L, R = x >> w, x & mask
        for r in range(4):
            f = fmix32(kp ^ ((R * 0x9E3779B1) & M32) ^ (((r + 1) * 0x7F4A7C15) & M32)) & mask
            L, R = R, L ^ f
        x = (L << w) | R
        if x < n:
            return x


def draw_index(k, j, n):
    return (fmix32((k + j * 0x9E3779B1) & M32) * n) >> 32


def iou3d(rois, gt):
    """(R, 7), (K, 7) -> (R, K) fp32, the operation order of _iou3d_from_overlap"""
    from oracle import cpu_oracle as o
    rois, gt = np.ascontiguousarray(rois, dtype=F), np.ascontiguousarray(gt, dtype=F)
    ov = o.boxes_overlap_bev(rois, gt).astype(F)
    a_max, a_min = (rois[:, 2] + rois[:, 5] / F(2))[:, None], (rois[:, 2] - rois[:, 5] / F(2))[:, None]
    b_max, b_min = (gt[:, 2] + gt[:, 5] / F(2))[None, :], (gt[:, 2] - gt[:, 5] / F(2))[None, :]
    h = np.maximum(np.minimum(a_max, b_max) - np.maximum(a_min, b_min), F(0))
    o3 = ov * h
    vol_a, vol_b = (rois[:, 3] * rois[:, 4] * rois[:, 5])[:, None], (gt[:, 3] * gt[:, 4] * gt[:, 5])[None, :]
    return (o3 / np.maximum(vol_a + vol_b - o3, F(1e-6))).astype(F)


def live_rows(gt):
    """(M, 8) -> the rows up to the last one whose elements do not sum to 0; none left: one all-zero box"""
    k = gt.shape[0] - 1
    while k >= 0:
        s = F(0)
        for v in gt[k]:
            s = F(s + v)
        if s != 0:
            break
        k -= 1
    return gt[:k + 1] if k >= 0 else np.zeros((1, gt.shape[1]), dtype=F)


def assign(rois, labels, gt, by_class):
    """-> max_overlaps (R) fp32, gt_assignment (R): the best IoU over the ground truth of the RoI's label (or all of it), the
    LOWEST index on a tie; a label without ground truth: (0, 0)"""
    iou = iou3d(rois[:, 0:7], gt[:, 0:7])
    gcls = gt[:, 7].astype(np.int64)
    mo, ga = np.zeros(rois.shape[0], dtype=F), np.zeros(rois.shape[0], dtype=np.int64)
    for r in range(rois.shape[0]):
        cols = np.flatnonzero(gcls == labels[r]) if by_class else np.arange(gt.shape[0])
        if cols.size:
            k = int(np.argmax(iou[r, cols]))          # first maximum
            mo[r], ga[r] = iou[r, cols[k]], cols[k]
    return mo, ga


def counts(n_fg, n_hard, n_easy, per_image, fg_per_image, hard_ratio):
    """-> (fg slots, fg drawn with repetition?, hard bg slots, easy bg slots), or None when there is neither fg nor bg"""
    n_bg = n_hard + n_easy
    if n_fg > 0 and n_bg > 0:
        take_fg, rep = min(fg_per_image, n_fg), False
    elif n_fg > 0:
        take_fg, rep = per_image, True
    elif n_bg > 0:
        take_fg, rep = 0, False
    else:
        return None
    take_bg = per_image - take_fg if n_bg > 0 else 0
    if n_hard > 0 and n_easy > 0:
        take_hard = min(int(take_bg * hard_ratio), n_hard)
    else:
        take_hard = take_bg if n_hard > 0 else 0
    return take_fg, rep, take_hard, take_bg - take_hard


def py_mod(a, b):
    m = np.fmod(F(a), F(b)).astype(F)
    return F(m + b) if m != 0 and m < 0 else F(m)


def fold_heading(h):
    """relative heading (fp32) -> [-pi / 2, pi / 2] by the opposite-orientation rule"""
    h = py_mod(h, TWO_PI)
    if h > HALF_PI and h < THREE_HALF_PI:
        h = py_mod(F(h + PI), TWO_PI)
    if h > PI:
        h = F(h - TWO_PI)
    return F(min(max(h, -HALF_PI), HALF_PI))


def canonical(roi, g):
    """roi (7), g (8) -> (8): g relative to the RoI's centre, turned by minus the RoI's heading, heading folded"""
    ry = py_mod(roi[6], TWO_PI)
    x, y, z = F(g[0] - roi[0]), F(g[1] - roi[1]), F(g[2] - roi[2])
    c, s = np.cos(F(-ry)).astype(F), np.sin(F(-ry)).astype(F)
    out = np.array(g, dtype=F)
    out[0] = F(F(x * c) + F(y * F(-s)))
    out[1] = F(F(x * s) + F(y * c))
    out[2] = z
    out[6] = fold_heading(F(g[6] - ry))
    return out


def relative_heading(roi, g):
    """the heading before folding, in [0, 2 pi)"""
    return py_mod(F(g[6] - py_mod(roi[6], TWO_PI)), TWO_PI)


def proposal_targets(rois, scores, labels, gt_boxes, cfg, seed, step):
    """rois (B, R, 7), scores (B, R), labels (B, R), gt_boxes (B, M, 8), cfg the sampler's settings -> dict of numpy arrays
    keyed as the operator's outputs, plus per-sample 'sets' (fg, hard, easy index arrays), 'max_overlaps' (B, R) and
    'failed' (B) bool"""
    B, R = rois.shape[0], rois.shape[1]
    S = int(cfg['ROI_PER_IMAGE'])
    fg_per_image = int(np.round(cfg['FG_RATIO'] * S))
    reg_fg, cls_fg, cls_bg, bg_lo = F(cfg['REG_FG_THRESH']), F(cfg['CLS_FG_THRESH']), F(cfg['CLS_BG_THRESH']), F(cfg['CLS_BG_THRESH_LO'])
    ramp = F(cfg['CLS_FG_THRESH'] - cfg['CLS_BG_THRESH'])
    fg_t = min(reg_fg, cls_fg)
    as_cls = cfg['CLS_SCORE_TYPE'] == 'cls'
    out = {'rois': np.zeros((B, S, 7), F), 'roi_labels': np.zeros((B, S), np.int64), 'roi_scores': np.zeros((B, S), F),
           'gt_iou_of_rois': np.zeros((B, S), F), 'gt_of_rois_src': np.zeros((B, S, 8), F), 'gt_of_rois': np.zeros((B, S, 8), F),
           'reg_valid_mask': np.zeros((B, S), np.int64), 'rcnn_cls_labels': np.zeros((B, S), np.int64 if as_cls else F),
           'sampled_inds': np.zeros((B, S), np.int32), 'gt_assignment': np.zeros((B, S), np.int32),
           'max_overlaps': np.zeros((B, R), F), 'sets': [], 'failed': np.zeros(B, bool), 'counts': []}
    for b in range(B):
        gt = live_rows(np.asarray(gt_boxes[b], dtype=F))
        mo, ga = assign(np.asarray(rois[b], dtype=F), labels[b], gt, bool(cfg.get('SAMPLE_ROI_BY_EACH_CLASS', False)))
        out['max_overlaps'][b] = mo
        fg = np.flatnonzero(mo >= fg_t)
        easy = np.flatnonzero(mo < bg_lo)
        hard = np.flatnonzero((mo < reg_fg) & (mo >= bg_lo))
        out['sets'].append((fg, hard, easy))
        rule = counts(fg.size, hard.size, easy.size, S, fg_per_image, cfg['HARD_BG_RATIO'])
        out['counts'].append(rule)
        if rule is None:
            out['failed'][b] = True
            picked = np.zeros(S, dtype=np.int64)
        else:
            take_fg, rep, take_hard, take_easy = rule
            k = [draw_key(seed, step, b, p) for p in (1, 2, 3, 4)]
            picked = [fg[draw_index(k[1], j, fg.size)] if rep else fg[feistel_perm(j, fg.size, k[0])] for j in range(take_fg)]
            picked += [hard[draw_index(k[2], j, hard.size)] for j in range(take_hard)]
            picked += [easy[draw_index(k[3], j, easy.size)] for j in range(take_easy)]
            picked = np.array(picked, dtype=np.int64)
        iou = mo[picked]
        out['sampled_inds'][b], out['gt_assignment'][b] = picked, ga[picked]
        out['rois'][b], out['roi_labels'][b], out['roi_scores'][b] = rois[b][picked], labels[b][picked], scores[b][picked]
        out['gt_iou_of_rois'][b], out['gt_of_rois_src'][b] = iou, gt[ga[picked]]
        out['reg_valid_mask'][b] = iou > reg_fg
        if as_cls:
            lab = (iou > cls_fg).astype(np.int64)
            lab[(iou > cls_bg) & (iou < cls_fg)] = -1
        else:
            lab = (iou > cls_fg).astype(F)
            mid = ~(iou > cls_fg) & ~(iou < cls_bg)
            lab[mid] = ((iou[mid] - cls_bg) / ramp).astype(F)
        out['rcnn_cls_labels'][b] = lab
        for s in range(S):
            out['gt_of_rois'][b, s] = canonical(rois[b][picked[s]], gt[ga[picked[s]]])
    return out


# ---- hand-derived known answers ------------------------------------------------------------------------------------------
# (RoI heading, ground-truth heading) -> folded relative heading; d = 0.1
_D = 0.1
KNOWN_FOLDS = [
    (0.0, np.pi / 2 - _D, np.pi / 2 - _D),            # just below pi / 2: kept
    (0.0, np.pi / 2 + _D, -np.pi / 2 + _D),           # just above: turned by pi, lands below 0
    (0.0, 3 * np.pi / 2 - _D, np.pi / 2 - _D),        # just below 3 pi / 2: turned by pi
    (0.0, 3 * np.pi / 2 + _D, -np.pi / 2 + _D),       # just above: kept, moved down by 2 pi
    (2 * np.pi - 0.05, 0.05, _D),                     # across the wrap: 0.05 - (2 pi - 0.05) = 0.1 - 2 pi -> 0.1
    (-0.05, 0.05, _D),                                # a negative RoI heading is taken mod 2 pi first: the same RoI
    (0.05, -0.05, -_D),                               # -0.1 -> 2 pi - 0.1 -> above pi -> -0.1
    (1.0, 1.0 + np.pi, 0.0),                          # the opposite orientation is the same solid
]
# (n_fg, n_hard, n_easy) -> (fg slots, repetition, hard slots, easy slots) at ROI_PER_IMAGE 16, FG_RATIO 0.5 (8), HARD_BG_RATIO 0.8
KNOWN_COUNTS = [
    ((3, 5, 20), (3, False, 5, 8)),       # fewer fg than 8: all 3, 13 bg; int(13 * 0.8) = 10 > 5 hard: 5, the rest easy
    ((20, 5, 20), (8, False, 5, 3)),      # 8 fg, 8 bg; int(6.4) = 6 > 5: 5 hard, 3 easy
    ((20, 9, 20), (8, False, 6, 2)),      # int(8 * 0.8) = 6 of 9 hard
    ((20, 0, 0), (16, True, 0, 0)),       # fg only: 16 draws with repetition
    ((0, 4, 0), (0, False, 16, 0)),       # hard only
    ((0, 0, 7), (0, False, 0, 16)),       # easy only
    ((0, 10, 10), (0, False, 10, 6)),     # bg only: int(16 * 0.8) = 12 > 10
    ((5, 0, 9), (5, False, 0, 11)),
    ((0, 0, 0), None),
]

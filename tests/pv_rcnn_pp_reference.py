"""What the PV-RCNN++ tests share (a helper module like pv_rcnn_reference.py: no tests, no fixtures, nothing from pdm_ssd_amd): a
numpy restatement of the proposal-centric partition specified in DESIGN.md 7y.

  keep_mask      sample_points_with_roi's verdict for one sample in fp32: pinned squared distance, sqrt, the first nearest roi,
                 d_min < fl(||dims / 2|| + radius); plus the clearances the generators reject-sample on
  sector_index   floor(fl(fl(atan2(y, x) + PI_F) / SIZE_F)) clamped to [0, S] in fp32; plus the distance of the quotient from an integer
  take_counts    min(c, ceil(c / N' * K)) with python floats and math.ceil
  partition      the whole operator over a stacked batch: seg_xyz, seg_row, seg_cnt, seg_take, kept_cnt, mask
  keypoints      partition + one FPS chain per segment: keypoints, the rows they came from, per-sample counts
"""
import math

import numpy as np

from pv_rcnn_reference import fps
from voxel_rcnn_reference import sqdist

f32 = np.float32
PI_F = f32(np.pi)


def keep_mask(xyz, rois, radius):
    """xyz (N, 3), rois (n, 7 + C) of ONE sample -> (mask (N) bool, clearance (N): |d_min - (roi_max_dim + radius)|, second (N): the
    verdict the second-nearest roi would give where it is within 1e-4 of the nearest, the mask's own elsewhere)"""
    xyz, rois = np.asarray(xyz, dtype=f32), np.asarray(rois, dtype=f32)
    d = np.sqrt(sqdist(xyz[:, None, :] - rois[None, :, 0:3]))                      # (N, n) fp32
    first = np.argmin(d, axis=1)                                                   # the lowest index on a tie, as torch.min
    dmin = d[np.arange(len(xyz)), first]
    thr = (np.sqrt(sqdist(rois[:, 3:6] / f32(2))) + f32(radius)).astype(f32)       # per roi
    mask = dmin < thr[first]
    second = mask.copy()
    if rois.shape[0] > 1 and len(xyz):
        masked = d.copy()
        masked[np.arange(len(xyz)), first] = np.inf
        nxt = np.argmin(masked, axis=1)
        near = masked[np.arange(len(xyz)), nxt] - dmin <= 1e-4
        second[near] = (masked[np.arange(len(xyz)), nxt] < thr[nxt])[near]
    return mask, np.abs(dmin.astype(np.float64) - thr[first]), second


def sector_index(xyz, S):
    """-> (sector (N) int in [0, S], off (N): the quotient's distance from the nearest integer)"""
    xyz = np.asarray(xyz, dtype=f32)
    size = f32(2.0 * np.pi / S)
    q = ((np.arctan2(xyz[:, 1], xyz[:, 0]).astype(f32) + PI_F).astype(f32) / size).astype(f32)
    return np.clip(np.floor(q), 0, S).astype(np.int64), np.abs(q - np.rint(q)).astype(np.float64)


def take_counts(counts, kept, K):
    """the reference's num_sampled_points_list, python floats: 0 for an empty sector"""
    return [min(int(c), math.ceil(int(c) / int(kept) * K)) if c > 0 else 0 for c in counts]


def partition(xyz, cnt, rois, radius, S, K, fallback=True):
    """xyz (N, 3) stacked sample-major, cnt (B), rois (B, n, 7 + C) -> dict: seg_xyz (T, 3), seg_row (T), seg_cnt (B max(S, 1)),
    seg_take (B S; empty when S = 0), kept_cnt (B), mask (N; rows past the counts' sum False)"""
    xyz = np.asarray(xyz, dtype=f32)
    nseg = max(S, 1)
    rows, seg_cnt, seg_take, kept_cnt = [], [], [], []
    mask_all = np.zeros(len(xyz), dtype=bool)
    start = 0
    for b, n in enumerate(cnt):
        pts = xyz[start:start + n]
        mask = keep_mask(pts, rois[b], radius)[0] if n else np.zeros(0, dtype=bool)
        mask_all[start:start + n] = mask
        kept = np.flatnonzero(mask)
        if len(kept) == 0 and n > 0 and fallback:
            kept = np.array([0])                                                   # points[:1]
        sector = sector_index(pts[kept], S)[0] if S > 0 else np.zeros(len(kept), dtype=np.int64)
        counts = [int((sector == s).sum()) for s in range(nseg)]
        for s in range(nseg):
            rows.append(start + kept[sector == s])
        seg_cnt += counts
        kept_cnt.append(len(kept))
        if S > 0:
            seg_take += take_counts(counts, len(kept), K)
        start += n
    seg_row = np.concatenate(rows).astype(np.int32) if rows else np.zeros(0, dtype=np.int32)
    return dict(seg_xyz=xyz[seg_row], seg_row=seg_row, seg_cnt=np.array(seg_cnt, dtype=np.int32), seg_take=np.array(seg_take, dtype=np.int32),
                kept_cnt=np.array(kept_cnt, dtype=np.int32), mask=mask_all)


def keypoints(xyz, cnt, rois, radius, S, K, fps=fps):
    """-> (keypoints (M, 3), rows (M) of xyz, per-sample counts (B)): a sample's sectors in ascending order, an FPS chain each.
    fps(xyz, n) -> n local indices: pv_rcnn_reference.fps breaks a tie of distances by the first index, which the kernels do only
    while no two distances are equal; for points on a lattice (voxel centres) the caller passes the oracle's, whose tie order is
    the kernels'"""
    p = partition(xyz, cnt, rois, radius, S, K)
    rows, per, at = [], [], 0
    for b in range(len(cnt)):
        got = 0
        for s in range(S):
            c, t = int(p['seg_cnt'][b * S + s]), int(p['seg_take'][b * S + s])
            if t > 0:
                rows.append(p['seg_row'][at + fps(p['seg_xyz'][at:at + c], t)])
            at += c
            got += t
        per.append(got)
    rows = np.concatenate(rows).astype(np.int64) if rows else np.zeros(0, dtype=np.int64)
    return np.asarray(xyz, dtype=f32)[rows], rows, np.array(per, dtype=np.int32)

#!/usr/bin/env python3
"""Generates tests/golden/ref_roi_targets.npz by running the REFERENCE's own Python on the CPU — ProposalTargetLayer
(/root/reference/pcdet/models/roi_heads/target_assigner/proposal_target_layer.py), RoIHeadTemplate.assign_targets,
get_box_cls_layer_loss and get_box_reg_layer_loss (models/roi_heads/roi_head_template.py), utils/box_coder_utils.py,
utils/loss_utils.py and utils/box_utils.py — imported from where they lie as gen_roi_fixtures.py does, nothing copied, with
  - boxes_iou3d_gpu stubbed over the CPU oracle's boxes_overlap_bev (the height and volume arithmetic of the reference's
    own lines, in torch),
  - F.binary_cross_entropy shown the ignore label -1 as 0 (this torch's CPU kernel refuses it; those rows are masked out),
  - ProposalTargetLayer.subsample_rois replaced by the indices that the numpy restatement's draw picked
    (tests/roi_target_reference.py): the reference's global numpy / torch RNGs cannot be replayed on the device.
Everything except the draw is therefore pinned by the reference: the assignment, the gather, the labels of both
CLS_SCORE_TYPEs, the canonical targets, and the three losses with their autograd gradients for recorded predictions.

The case (B = 3, R = 70, S = 16, M = 6, three classes) is reject-sampled; asserted on the CPU:
  sample 0: fg, hard bg and easy bg, fewer fg than fg_per_image, trailing zero rows, RoIs whose label has no ground truth;
  sample 1: no ground truth at all (bg only);  sample 2: every RoI fg (near-copies of ground truth), an interior zero row;
  every max_overlaps at least 1e-4 from every threshold; a RoI's two best same-class IoUs differ by more than 1e-4 (or are
  both exactly 0, or belong to identical boxes); the relative headings before folding at least 1e-3 from pi / 2, 3 pi / 2
  and the wrap; for the loss case at least 8 fg rows, every corner's two distances (plain, flipped) more than 1e-4 apart
  and no corner distance below 1e-3.
The seeds are recorded.  Run in the authoring container only (needs /root/reference); the output is committed.
"""
import copy
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, HERE)
from oracle import cpu_oracle as o  # noqa: E402
import roi_target_reference as rt  # noqa: E402
import gen_head_fixtures as ghf  # noqa: E402
import gen_roi_fixtures as grf  # noqa: E402

EasyDict = ghf.EasyDict
SIZES = np.array([[3.9, 1.6, 1.56], [0.8, 0.6, 1.73], [1.76, 0.6, 1.73]], dtype=np.float32)
B, R, M, S = 3, 70, 6, 16
SAMPLER = {'BOX_CODER': 'ResidualCoder', 'ROI_PER_IMAGE': S, 'FG_RATIO': 0.5, 'SAMPLE_ROI_BY_EACH_CLASS': True, 'CLS_SCORE_TYPE': 'cls',
           'CLS_FG_THRESH': 0.6, 'CLS_BG_THRESH': 0.45, 'CLS_BG_THRESH_LO': 0.1, 'HARD_BG_RATIO': 0.8, 'REG_FG_THRESH': 0.55}
LOSS = {'CLS_LOSS': 'BinaryCrossEntropy', 'REG_LOSS': 'smooth-l1', 'CORNER_LOSS_REGULARIZATION': True,
        'LOSS_WEIGHTS': {'rcnn_cls_weight': 1.0, 'rcnn_reg_weight': 2.0, 'rcnn_corner_weight': 0.5,
                         'code_weights': [1.0, 1.0, 1.0, 0.8, 0.8, 0.8, 1.2]}}
DRAW_SEED, DRAW_STEP = 20240229, 0


def n(t):
    return t.detach().numpy()


def new_box(rng, cls):
    bx = np.zeros(8, dtype=np.float32)
    bx[0:2] = rng.uniform(2, 14, 2)
    bx[2] = rng.uniform(-1.0, -0.5)
    bx[3:6] = SIZES[cls - 1] * rng.uniform(0.9, 1.1, 3)
    bx[6] = rng.uniform(-np.pi, np.pi)
    bx[7] = cls
    return bx


def near(rng, g, shift, turn):
    r = g[0:7].copy()
    r[0:2] += rng.uniform(-shift, shift, 2)
    r[6] += rng.choice([-1.0, 1.0]) * rng.uniform(0.3 * turn, turn)
    return r


def make_case(rng):
    gt = np.zeros((B, M, 8), dtype=np.float32)
    rois = np.zeros((B, R, 7), dtype=np.float32)
    labels = np.ones((B, R), dtype=np.int64)
    scores = rng.uniform(0, 1, (B, R)).astype(np.float32)
    # sample 0: classes 1, 1, 2, 1, then two trailing zero rows; no ground truth of class 3
    for m, cls in enumerate((1, 1, 2, 1)):
        gt[0, m] = new_box(rng, cls)
    k = 0
    for _ in range(4):                                  # close: fg
        g = gt[0, rng.integers(0, 4)]
        rois[0, k], labels[0, k] = near(rng, g, 0.05, 0.03), int(g[7]); k += 1
    for _ in range(16):                                 # shifted: hard bg mostly
        g = gt[0, rng.integers(0, 4)]
        rois[0, k], labels[0, k] = near(rng, g, 0.6 if g[7] == 1 else 0.2, 0.3), int(g[7]); k += 1
    for _ in range(12):                                 # on ground truth, but labelled with the class that has none
        g = gt[0, rng.integers(0, 4)]
        rois[0, k], labels[0, k] = near(rng, g, 0.05, 0.03), 3; k += 1
    while k < R:                                        # anywhere
        cls = int(rng.integers(1, 3))
        rois[0, k], labels[0, k] = new_box(rng, cls)[0:7], cls; k += 1
    # sample 1: no ground truth
    for k in range(R):
        cls = int(rng.integers(1, 4))
        rois[1, k], labels[1, k] = new_box(rng, cls)[0:7], cls
    # sample 2: rows 0, 2, 3 live, row 1 an interior zero row; every RoI a near-copy of its own class's box
    for m, cls in ((0, 1), (2, 2), (3, 3)):
        gt[2, m] = new_box(rng, cls)
    for k in range(R):
        g = gt[2, (0, 2, 3)[int(rng.integers(0, 3))]]
        rois[2, k], labels[2, k] = near(rng, g, 0.02, 0.02), int(g[7])
    order = rng.permutation(R)                          # the kinds interleaved in RoI order
    rois[0], labels[0] = rois[0][order], labels[0][order]
    return rois, scores, labels, gt


def case_ok(case):
    rois, scores, labels, gt = case
    ref = rt.proposal_targets(rois, scores, labels, gt, SAMPLER, DRAW_SEED, DRAW_STEP)
    (fg0, hard0, easy0), (fg1, hard1, easy1), (fg2, hard2, easy2) = ref['sets']
    fg_per_image = int(np.round(SAMPLER['FG_RATIO'] * S))
    if not (0 < fg0.size < fg_per_image and hard0.size > 0 and easy0.size > 0):
        return False
    if not (fg1.size == 0 and hard1.size + easy1.size == R and rt.live_rows(gt[1]).shape[0] == 1):
        return False
    if not (fg2.size == R and hard2.size + easy2.size == 0):
        return False
    if rt.live_rows(gt[0]).shape[0] != 4 or rt.live_rows(gt[2]).shape[0] != 4 or gt[2, 1].any():
        return False
    if not ((labels[0] == 3).any() and not (gt[0, :, 7] == 3).any()):
        return False
    thresholds = [SAMPLER[k] for k in ('REG_FG_THRESH', 'CLS_FG_THRESH', 'CLS_BG_THRESH', 'CLS_BG_THRESH_LO')]
    for b in range(B):
        live = rt.live_rows(gt[b])
        mo, ga = rt.assign(rois[b], labels[b], live, True)
        assert (mo == ref['max_overlaps'][b]).all()
        if min(np.abs(mo - t).min() for t in thresholds) < 1e-4:
            return False
        iou = rt.iou3d(rois[b], live[:, 0:7])
        gcls = live[:, 7].astype(np.int64)
        for r in range(R):
            cols = np.flatnonzero(gcls == labels[b, r])
            if cols.size >= 2:
                top = np.sort(iou[r, cols])[::-1]
                if top[0] > 0 and top[0] - top[1] <= 1e-4:
                    return False
            h = float(rt.relative_heading(rois[b, r], live[ga[r]]))      # whichever RoI the draw picks
            if min(abs(h - np.pi / 2), abs(h - 3 * np.pi / 2), h, 2 * np.pi - h) < 1e-3:
                return False
    return True


def install():
    grf.install_reference()
    from pcdet.models.roi_heads import roi_head_template as rht
    from pcdet.models.roi_heads.target_assigner import proposal_target_layer as ptl
    from pcdet.utils import box_utils, loss_utils
    iou_mod = sys.modules['pcdet.ops.iou3d_nms.iou3d_nms_utils']

    def boxes_iou3d_gpu(boxes_a, boxes_b):
        """the reference's iou3d_nms_utils.boxes_iou3d_gpu (:50-81) with the BEV overlap from the oracle"""
        a_max = (boxes_a[:, 2] + boxes_a[:, 5] / 2).view(-1, 1)
        a_min = (boxes_a[:, 2] - boxes_a[:, 5] / 2).view(-1, 1)
        b_max = (boxes_b[:, 2] + boxes_b[:, 5] / 2).view(1, -1)
        b_min = (boxes_b[:, 2] - boxes_b[:, 5] / 2).view(1, -1)
        bev = torch.from_numpy(o.boxes_overlap_bev(n(boxes_a[:, 0:7]).copy(), n(boxes_b[:, 0:7]).copy()))
        overlaps_h = torch.clamp(torch.min(a_max, b_max) - torch.max(a_min, b_min), min=0)
        overlaps_3d = bev * overlaps_h
        vol_a = (boxes_a[:, 3] * boxes_a[:, 4] * boxes_a[:, 5]).view(-1, 1)
        vol_b = (boxes_b[:, 3] * boxes_b[:, 4] * boxes_b[:, 5]).view(1, -1)
        return overlaps_3d / torch.clamp(vol_a + vol_b - overlaps_3d, min=1e-6)
    iou_mod.boxes_iou3d_gpu = boxes_iou3d_gpu

    class Functional:
        """torch.nn.functional as roi_head_template.py sees it.  This torch's CPU binary_cross_entropy refuses the ignore
        label -1 as a target (the CUDA kernel the reference ran on did not look): such targets are handed over as 0.  Their
        rows are multiplied by cls_valid_mask = 0 right after (:207-208), so no value and no gradient changes."""

        def __getattr__(self, name):
            return getattr(torch.nn.functional, name)

        @staticmethod
        def binary_cross_entropy(input, target, **kw):
            return torch.nn.functional.binary_cross_entropy(input, target.clamp(min=0), **kw)
    rht.F = Functional()
    return rht, ptl, box_utils, loss_utils


def make_head(rht, score_type, corner=True):
    cfg = EasyDict({'TARGET_CONFIG': EasyDict(dict(SAMPLER, CLS_SCORE_TYPE=score_type)),
                    'LOSS_CONFIG': EasyDict(dict(copy.deepcopy(LOSS), CORNER_LOSS_REGULARIZATION=corner))})
    return rht.RoIHeadTemplate(num_class=1, model_cfg=cfg)


def reference_targets(rht, ptl, case, score_type, picks):
    rois, scores, labels, gt = case
    seen, it = [], iter(picks)

    def fixed(self, max_overlaps):
        seen.append(n(max_overlaps).copy())
        return torch.from_numpy(next(it).astype(np.int64))
    keep = ptl.ProposalTargetLayer.subsample_rois
    ptl.ProposalTargetLayer.subsample_rois = fixed
    try:
        head = make_head(rht, score_type)
        bd = {'batch_size': B, 'rois': torch.from_numpy(rois.copy()), 'roi_scores': torch.from_numpy(scores.copy()),
              'roi_labels': torch.from_numpy(labels.copy()), 'gt_boxes': torch.from_numpy(gt.copy())}
        out = head.assign_targets(bd)
    finally:
        ptl.ProposalTargetLayer.subsample_rois = keep
    return {k: n(v).copy() for k, v in out.items()}, np.stack(seen)


def reference_losses(rht, targets, rcnn_cls, rcnn_reg, score_type, rows=None, corner=True):
    """-> losses and gradients of the reference's two loss functions for the recorded predictions (rows: a slice of samples)"""
    head = make_head(rht, score_type, corner)
    sel = slice(None) if rows is None else rows
    frd = {k: torch.from_numpy(v[sel].copy()) for k, v in targets.items()}
    cls = torch.from_numpy(rcnn_cls.reshape(B, S, 1)[sel].reshape(-1, 1).copy()).requires_grad_(True)
    reg = torch.from_numpy(rcnn_reg.reshape(B, S, 7)[sel].reshape(-1, 7).copy()).requires_grad_(True)
    frd.update(rcnn_cls=cls, rcnn_reg=reg)
    loss_cls, tb_cls = head.get_box_cls_layer_loss(frd)
    loss_reg, tb_reg = head.get_box_reg_layer_loss(frd)
    g_cls, = torch.autograd.grad(loss_cls, cls)
    g_reg, = torch.autograd.grad(loss_reg, reg, allow_unused=True)
    g_reg = torch.zeros_like(reg) if g_reg is None else g_reg
    return {'loss_cls': np.float32(tb_cls['rcnn_loss_cls']), 'loss_reg': np.float32(tb_reg['rcnn_loss_reg']),
            'loss_corner': np.float32(tb_reg.get('rcnn_loss_corner', 0.0)), 'loss_reg_total': np.float32(loss_reg.item()),
            'g_cls': n(g_cls), 'g_reg': n(g_reg)}


def corner_distances(rht, box_utils, targets, rcnn_reg):
    """the two distances (plain, flipped) of every corner of every fg row, formed with the reference's own functions as
    get_box_reg_layer_loss forms them (:167-189)"""
    from pcdet.utils import common_utils
    head = make_head(rht, 'cls')
    fg = torch.from_numpy(targets['reg_valid_mask'].reshape(-1) > 0)
    rois = torch.from_numpy(targets['rois'].reshape(-1, 7))[fg]
    anchors = rois.clone().view(1, -1, 7)
    anchors[:, :, 0:3] = 0
    boxes = head.box_coder.decode_torch(torch.from_numpy(rcnn_reg)[fg].view(1, -1, 7), anchors).view(-1, 7)
    boxes = common_utils.rotate_points_along_z(boxes.unsqueeze(1), rois[:, 6]).squeeze(1)
    boxes[:, 0:3] += rois[:, 0:3]
    src = torch.from_numpy(targets['gt_of_rois_src'].reshape(-1, 8))[fg][:, 0:7]
    flipped = src.clone()
    flipped[:, 6] += np.pi
    pred = box_utils.boxes_to_corners_3d(boxes)
    d1 = torch.norm(pred - box_utils.boxes_to_corners_3d(src), dim=2)
    d2 = torch.norm(pred - box_utils.boxes_to_corners_3d(flipped), dim=2)
    return n(d1), n(d2)


def main():
    rht, ptl, box_utils, loss_utils = install()
    out, seeds = {}, {}
    case, seeds['case'] = grf.sample(make_case, case_ok, 1000)
    rois, scores, labels, gt = case
    out.update(rois=rois, roi_scores=scores, roi_labels=labels, gt_boxes=gt)
    for tag in ('cls', 'roi_iou'):
        cfg = dict(SAMPLER, CLS_SCORE_TYPE=tag)
        ref = rt.proposal_targets(rois, scores, labels, gt, cfg, DRAW_SEED, DRAW_STEP)
        got, seen = reference_targets(rht, ptl, case, tag, list(ref['sampled_inds']))
        assert np.abs(seen - ref['max_overlaps']).max() < 1e-6                 # the restatement's assignment = the reference's
        assert (got['rois'] == ref['rois']).all() and (got['reg_valid_mask'] == ref['reg_valid_mask']).all()
        assert (got['gt_of_rois_src'] == ref['gt_of_rois_src']).all()
        assert np.abs(got['gt_of_rois'] - ref['gt_of_rois']).max() < 1e-5
        if tag == 'cls':
            assert (got['rcnn_cls_labels'] == ref['rcnn_cls_labels']).all()
            assert set(np.unique(got['rcnn_cls_labels'])) == {-1, 0, 1}
        else:
            assert np.abs(got['rcnn_cls_labels'] - ref['rcnn_cls_labels']).max() < 1e-6
            assert ((got['rcnn_cls_labels'] > 0) & (got['rcnn_cls_labels'] < 1)).any()
        for k, v in got.items():
            out[f'{tag}.{k}'] = v
        out[f'{tag}.sampled_inds'] = ref['sampled_inds']
        out[f'{tag}.gt_assignment'] = ref['gt_assignment']
        if tag == 'cls':
            targets = got
        else:
            targets_iou = got
    assert int((targets['reg_valid_mask'] > 0).sum()) >= 8

    # the loss case: recorded predictions, reject-sampled for the corner margins
    seed = 2000
    while True:
        g = np.random.default_rng(seed)
        rcnn_cls = g.normal(0, 2.0, (B * S, 1)).astype(np.float32)
        rcnn_reg = (g.normal(0, 1.0, (B * S, 7)) * [0.3, 0.3, 0.3, 0.15, 0.15, 0.15, 0.2]).astype(np.float32)
        d1, d2 = corner_distances(rht, box_utils, targets, rcnn_reg)
        if np.abs(d1 - d2).min() > 1e-4 and min(d1.min(), d2.min()) > 1e-3 and (np.minimum(d1, d2) < 1).any() \
                and (np.minimum(d1, d2) > 1).any() and (d2 < d1).any():
            break
        seed += 1
    seeds['loss'] = seed
    out.update(rcnn_cls=rcnn_cls, rcnn_reg=rcnn_reg)
    full = reference_losses(rht, targets, rcnn_cls, rcnn_reg, 'cls')
    plain = reference_losses(rht, targets, rcnn_cls, rcnn_reg, 'cls', corner=False)
    assert abs(plain['loss_reg'] - full['loss_reg']) < 1e-6 and full['loss_corner'] > 0
    out.update({'loss.cls': full['loss_cls'], 'loss.reg': full['loss_reg'], 'loss.corner': full['loss_corner'],
                'loss.g_cls': full['g_cls'], 'loss.g_reg_total': full['g_reg'], 'loss.g_reg_smooth_l1': plain['g_reg']})
    iou = reference_losses(rht, targets_iou, rcnn_cls, rcnn_reg, 'roi_iou')
    out.update({'loss_iou.cls': iou['loss_cls'], 'loss_iou.reg': iou['loss_reg'], 'loss_iou.corner': iou['loss_corner'],
                'loss_iou.g_cls': iou['g_cls'], 'loss_iou.g_reg_total': iou['g_reg']})
    nofg = reference_losses(rht, targets, rcnn_cls, rcnn_reg, 'cls', rows=slice(1, 2))     # sample 1: bg only
    assert nofg['loss_reg'] == 0 and nofg['loss_corner'] == 0 and not nofg['g_reg'].any()
    out.update({'loss_nofg.cls': nofg['loss_cls'], 'loss_nofg.g_cls': nofg['g_cls']})

    # boxes_to_corners_3d and get_corner_loss_lidar values
    g = np.random.default_rng(7)
    a = np.stack([new_box(g, int(g.integers(1, 4)))[0:7] for _ in range(10)])
    b_ = a + g.normal(0, 0.2, a.shape).astype(np.float32)
    b_[::2, 6] += np.pi                                                        # half of them facing the other way
    out.update(corner_boxes_a=a, corner_boxes_b=b_.astype(np.float32),
               corners_a=n(box_utils.boxes_to_corners_3d(torch.from_numpy(a))),
               corner_loss=n(loss_utils.get_corner_loss_lidar(torch.from_numpy(a), torch.from_numpy(b_.astype(np.float32)))))
    out['loss_weights'] = np.array([LOSS['LOSS_WEIGHTS'][k] for k in ('rcnn_cls_weight', 'rcnn_reg_weight', 'rcnn_corner_weight')], dtype=np.float64)
    out['code_weights'] = np.array(LOSS['LOSS_WEIGHTS']['code_weights'], dtype=np.float64)
    out['draw'] = np.array([DRAW_SEED, DRAW_STEP], dtype=np.int64)
    out['seeds'] = np.array([seeds['case'], seeds['loss']], dtype=np.int64)
    np.savez_compressed(os.path.join(HERE, 'ref_roi_targets.npz'), **out)
    print('wrote', len(out), 'arrays; seeds', seeds, 'sets', [[len(x) for x in s] for s in ref['sets']],
          'fg rows', int((targets['reg_valid_mask'] > 0).sum()), 'losses', full['loss_cls'], full['loss_reg'], full['loss_corner'])


if __name__ == '__main__':
    main()

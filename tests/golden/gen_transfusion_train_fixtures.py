#!/usr/bin/env python3
"""Generates tests/golden/ref_transfusion_train.npz (+ ref_transfusion_train_manifest.json) by running the REFERENCE's own
TransFusionHead.loss() on the CPU: pcdet/models/dense_heads/transfusion_head.py with target_assigner/hungarian_assigner.py
(scipy's linear_sum_assignment), utils/loss_utils.py and model_utils/centernet_utils.py, imported from where they lie,
nothing copied, with the stubs of gen_transfusion_fixtures.py plus two: iou3d_nms_cuda.boxes_overlap_bev_gpu answered by
oracle.cpu_oracle.boxes_overlap_bev, and Tensor.cuda as the identity.  Run in the authoring container only; the outputs
hold numbers and key names only.

Shapes (tests/transfusion_case.py): B = 2, a 12 x 20 map, P = 12, ten classes; the head is the eval fixture's nuScenes head
with its seeded parameters and DROPOUT 0 (tests/transfusion_train_case.train_cfg), in TRAINING mode, so the prediction maps
are functions of the input alone (BatchNorm uses the batch's statistics).  The input features are seeded on their own and
searched until the training-mode heat-map keeps the query margins (a) - (c) of gen_transfusion_fixtures.py.

Ground truth (B, M = 8, 10): sample 0 has 5 valid boxes of at least 3 classes, one zero-size row in the middle and trailing
padding, sample 1 has 3 valid boxes.  Boxes are placed on decoded predictions and perturbed: some by a few centimetres
(IoU > 0), some by more than a box length (IoU = 0).  The seed is searched until, with a margin of 1e-3 each,
  (m) by brute force over all injections the second-best assignment of each sample costs at least the optimum + margin,
  (i) at least one matched pair has IoU > 0 and at least one IoU = 0,
  (c) every box's centre lies inside the map and centre cell and gaussian radius are away from an integer,
  (s) no matched prediction is within the margin of its regression target (the L1 gradient is a sign).
Recorded: the gt boxes, the prediction maps, per sample the cost matrix and scipy's assignment, every target, the three
weighted losses, loss_trans, and the reference autograd's gradients with respect to the six maps and dense_heatmap.

Parity bound: the reference's loss is run once more with the prediction dict and the boxes cast to float64; parity_abs is
8 times the largest distance between the two runs over everything recorded as a float (rounded up to one digit), and the
generator fails unless the float32 run is within a quarter of it.  loss_sensitivity = the sum of |d loss_trans / d map|
over every map element: a first-order bound on how far loss_trans moves per unit of error in the maps.
"""
import itertools
import json
import math
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from gen_center_head_fixtures import EasyDict  # noqa: E402
from gen_head_fixtures import install_reference  # noqa: E402
from oracle import cpu_oracle  # noqa: E402
import transfusion_case as tc  # noqa: E402
import transfusion_train_case as ttc  # noqa: E402

M = 8
NEAR, FAR = 0.04, 1.6           # perturbation of a centre in metres: inside the box / beyond it


def decoded(res):
    x = res['center'][:, 0] * tc.STRIDE * tc.VOXEL[0] + tc.PC_RANGE[0]
    y = res['center'][:, 1] * tc.STRIDE * tc.VOXEL[1] + tc.PC_RANGE[1]
    cols = [x, y, res['height'][:, 0], *np.exp(res['dim']).transpose(1, 0, 2), np.arctan2(res['rot'][:, 0], res['rot'][:, 1]),
            *res['vel'].transpose(1, 0, 2)]
    return np.stack(cols, -1)                                             # (B, P, 9)


def make_gt(rng, boxes):
    gt = np.zeros((tc.B, M, 10), dtype=np.float32)
    plan = [[(NEAR, 1), (FAR, 4), None, (NEAR, 9), (FAR, 1), (NEAR, 6)], [(NEAR, 3), (FAR, 8), (NEAR, 1)]]
    for b, rows in enumerate(plan):
        picks = rng.permutation(tc.P)
        for m, row in enumerate(rows):
            if row is None:
                gt[b, m, :3] = rng.uniform(-1, 1, 3)                     # a zero-size row in the middle: not valid
                gt[b, m, 9] = 2
                continue
            shift, cls = row
            box = boxes[b, picks[m]].copy()
            ang = rng.uniform(0, 2 * np.pi)
            box[:2] += shift * np.array([np.cos(ang), np.sin(ang)]) * rng.uniform(1.0, 1.5)
            box[2] += rng.uniform(-0.05, 0.05)
            box[3:6] *= rng.uniform(0.9, 1.1, 3)
            box[6] += rng.uniform(-0.1, 0.1)
            box[7:9] += rng.uniform(-0.2, 0.2, 2)
            gt[b, m, :9] = box
            gt[b, m, 9] = cls + 1
    return gt


def second_best_gap(cost):
    c = np.asarray(cost, dtype=np.float64)
    P, G = c.shape
    totals = sorted(float(c[list(rows), range(G)].sum()) for rows in itertools.permutations(range(P), G))
    return totals[1] - totals[0]


def run_loss(head, ha, res, gt, dtype):
    """the reference's loss() on leaves of `dtype` -> (losses, tb_dict, targets tuple, grads, [(cost, rows, cols)])"""
    seen = []
    real = ha.linear_sum_assignment.__wrapped__ if hasattr(ha.linear_sum_assignment, '__wrapped__') else ha.linear_sum_assignment

    def spy(cost):
        r, c = real(cost)
        seen.append((cost.numpy().copy(), r.copy(), c.copy()))
        return r, c
    spy.__wrapped__ = real
    ha.linear_sum_assignment = spy
    leaves = {k: torch.from_numpy(res[k]).to(dtype).requires_grad_(True) for k in ttc.GRAD_MAPS}
    pred = {k: v for k, v in leaves.items()}
    pred['dense_heatmap'] = leaves['dense_heatmap'].clone()               # (clip_sigmoid overwrites it in place)
    boxes = torch.from_numpy(gt[..., :-1]).to(dtype)
    labels = torch.from_numpy(gt[..., -1]).long() - 1
    targets = head.get_targets(boxes, labels, pred)
    seen.clear()
    loss, tb = head.loss(boxes, labels, pred)
    loss.backward()
    return loss, tb, targets, {k: v.grad.numpy() for k, v in leaves.items()}, list(seen)


def main():
    install_reference()
    mod = types.ModuleType('pcdet.ops.iou3d_nms.iou3d_nms_cuda')

    def boxes_overlap_bev_gpu(a, b, out):
        out.copy_(torch.from_numpy(cpu_oracle.boxes_overlap_bev(a.detach().float().numpy(), b.detach().float().numpy())))
    mod.boxes_overlap_bev_gpu = boxes_overlap_bev_gpu
    sys.modules['pcdet.ops.iou3d_nms.iou3d_nms_cuda'] = mod
    sys.modules['pcdet.ops.iou3d_nms'].iou3d_nms_cuda = mod
    from pcdet.models.dense_heads import transfusion_head as ref_tf
    from pcdet.models.dense_heads.target_assigner import hungarian_assigner as ha
    man_eval = tc.manifest()

    def build():
        head = ref_tf.TransFusionHead(model_cfg=EasyDict(ttc.train_cfg(on_device=False)), **tc.head_kwargs())
        total = tc.fill_transfusion(head, man_eval['seed'], man_eval['gain'], man_eval['hm_gain'], man_eval['hm_bias'])
        assert abs(total - man_eval['weight_sum']) <= 1e-6 * man_eval['weight_sum']
        return head.train()

    for feat_seed in range(100, 400):
        feats = np.random.default_rng(feat_seed).standard_normal((tc.B, tc.CIN, tc.H, tc.W)).astype(np.float32)
        head = build()
        with torch.no_grad():
            res = {k: v.detach().numpy().copy() for k, v in head.predict(torch.from_numpy(feats)).items()}
        cls = head.query_labels.numpy().astype(np.int64)
        margins = tc.proposal_margins(res['dense_heatmap'], 3, (8, 9), tc.P)
        try:
            tc.check_proposal_margins(margins, tc.P)
        except AssertionError:
            continue
        break
    else:
        raise SystemExit('no input keeps the query margins in training mode')

    boxes = decoded(res)
    for seed in range(1000, 3000):
        gt = make_gt(np.random.default_rng(seed), boxes)
        try:
            valid = [(gt[b, :, 3] > 0) & (gt[b, :, 4] > 0) for b in range(tc.B)]
            assert [int(v.sum()) for v in valid] == [5, 3]
            cells, radii = [], []
            for b in range(tc.B):
                g = gt[b, valid[b]].astype(np.float64)
                cx = (g[:, 0] - tc.PC_RANGE[0]) / tc.VOXEL[0] / tc.STRIDE
                cy = (g[:, 1] - tc.PC_RANGE[1]) / tc.VOXEL[1] / tc.STRIDE
                assert (cx > tc.MARGIN).all() and (cx < tc.W - tc.MARGIN).all() and (cy > tc.MARGIN).all() and (cy < tc.H - tc.MARGIN).all()
                from pcdet.models.model_utils import centernet_utils
                r = centernet_utils.gaussian_radius(torch.from_numpy(g[:, 4] / tc.VOXEL[1] / tc.STRIDE),
                                                    torch.from_numpy(g[:, 3] / tc.VOXEL[0] / tc.STRIDE), 0.1).numpy()
                cells += [cx, cy]
                radii.append(r)
            frac = np.concatenate(cells + radii) % 1.0
            assert frac.min() >= tc.MARGIN and frac.max() <= 1 - tc.MARGIN, 'a cell or a radius is near an integer'
            loss, tb, targets, grads, seen = run_loss(head, ha, res, gt, torch.float32)
            assert len(seen) == tc.B
            gaps = [second_best_gap(c) for c, _, _ in seen]
            assert min(gaps) >= tc.MARGIN, gaps
            labels, label_weights, bbox_targets, bbox_weights, num_pos, matched_ious, heatmap = targets
            pos = bbox_weights[..., 0].numpy() > 0
            # the matched pairs' IoU: recomputed here with the reference's overlaps()
            ious = np.zeros((tc.B, tc.P), dtype=np.float32)
            for b in range(tc.B):
                g = torch.from_numpy(gt[b, valid[b], :9])
                iou = ha.overlaps(torch.from_numpy(boxes[b].astype(np.float32)), g).numpy()
                _, r, c = seen[b]
                ious[b, r] = np.clip(iou[r, c], 0.0, 1.0)
            assert (ious[pos] > tc.MARGIN).any() and (ious[pos] == 0).any(), 'matched IoUs are all zero or all positive'
            preds = np.concatenate([res[k] for k in ('center', 'height', 'dim', 'rot', 'vel')], 1).transpose(0, 2, 1)
            assert np.abs(preds - bbox_targets.numpy())[pos].min() >= tc.MARGIN
        except AssertionError:
            continue
        break
    else:
        raise SystemExit('no seed meets the conditions')

    loss64, tb64, targets64, grads64, seen64 = run_loss(head, ha, res, gt, torch.float64)
    assert all(np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) for a, b in zip(seen, seen64))
    w = ttc.train_cfg()['LOSS_CONFIG']['LOSS_WEIGHTS']
    out = {'spatial_features_2d': feats, 'gt_boxes': gt, 'cls': cls}
    for k in ttc.GRAD_MAPS + ('query_heatmap_score',):
        out[f'pred.{k}'] = res[k]
    assigned = np.full((tc.B, tc.P), -1, dtype=np.int32)
    for b, (c, r, col) in enumerate(seen):
        out[f'cost.{b}'] = c.astype(np.float32)
        assigned[b, r] = col
    out.update({'target.labels': labels.numpy().astype(np.int64), 'target.label_weights': label_weights.numpy().astype(np.float32),
                'target.bbox_targets': bbox_targets.numpy(), 'target.bbox_weights': bbox_weights.numpy(), 'target.ious': ious,
                'target.assigned': assigned, 'target.num_pos': np.int32(num_pos), 'target.matched_ious': np.float32(matched_ious),
                'target.heatmap': heatmap.numpy()})
    out['loss_heatmap'] = np.float32(tb['loss_heatmap'])
    out['loss_cls'] = np.float32(tb['loss_cls'])
    out['loss_bbox'] = np.float32(tb['loss_bbox'])
    out['loss_trans'] = np.float32(loss.item())
    for k in ttc.GRAD_MAPS:
        out[f'grad.{k}'] = grads[k]
    gap = {k: float(abs(tb[k] - tb64[k])) for k in ('loss_heatmap', 'loss_cls', 'loss_bbox')}
    gap['loss_trans'] = float(abs(loss.item() - loss64.item()))
    gap['matched_ious'] = float(abs(float(matched_ious) - float(targets64[5])))
    gap['bbox_targets'] = float(np.abs(bbox_targets.numpy() - targets64[2].numpy()).max())
    gap['heatmap'] = float(np.abs(heatmap.numpy() - targets64[6].numpy()).max())
    gap['cost'] = float(max(np.abs(a[0] - b[0]).max() for a, b in zip(seen, seen64)))
    for k in ttc.GRAD_MAPS:
        gap[f'grad.{k}'] = float(np.abs(grads[k] - grads64[k]).max())
    worst = max(gap.values())
    digit = 10.0 ** math.floor(math.log10(8 * worst))
    parity = float(math.ceil(8 * worst / digit) * digit)
    assert worst <= parity / 4, (worst, parity)
    sensitivity = float(sum(np.abs(g).sum() for g in grads64.values()))
    manifest = {'feat_seed': feat_seed, 'gt_seed': seed, 'parity_abs': parity, 'float32_to_float64_gap': gap, 'loss_sensitivity': sensitivity,
                'second_best_gap': gaps, 'margin_required': tc.MARGIN, 'query_margins': margins, 'num_pos': int(num_pos),
                'matched_iou_max': float(ious.max()), 'loss_weights': {k: w[k] for k in ('cls_weight', 'bbox_weight', 'hm_weight')}}
    np.savez_compressed(os.path.join(HERE, 'ref_transfusion_train.npz'), **out)
    with open(os.path.join(HERE, 'ref_transfusion_train_manifest.json'), 'w') as f:
        json.dump(manifest, f, indent=1, sort_keys=True)
    print('wrote', len(out), 'arrays;', manifest)


if __name__ == '__main__':
    main()

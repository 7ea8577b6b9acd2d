#!/usr/bin/env python3
"""Generates tests/golden/ref_anchor_head.npz (+ ref_anchor_head_manifest.json) by running the REFERENCE's own
AnchorHeadSingle on the CPU: pcdet/models/dense_heads/anchor_head_single.py, anchor_head_template.py,
target_assigner/anchor_generator.py, target_assigner/axis_aligned_target_assigner.py, utils/box_utils.py,
utils/box_coder_utils.py and utils/loss_utils.py, imported from where they lie, nothing copied, with the stubs of
gen_head_fixtures.install_reference (numba, SharedArray, iou3d_nms, roiaware_pool3d, `.cuda()` as the identity).  Run in the
authoring container only; the outputs hold numbers and key names only.

Shapes: B = 2, grid_size [40, 24, 1] with stride 2 (a 12 x 20 map, non-square on purpose), point_cloud_range
[0, -9.6, -3, 32, 9.6, 1], input_channels = 8, the three KITTI anchor sets: A = 12 * 20 * 6 = 1440.
Records
  - the anchors of every set, and the same with align_center: True;
  - the state-dict manifest and values;
  - assign_targets for NORM_BY_NUM_EXAMPLES False and True on a box set with a box matched only by force, a box with swapped
    extents, padding rows between real boxes, a duplicate box, a box outside the range and a square box whose two rotations
    tie; sample 1 holds one box (the reference's one-box branch), so two of its three sets run with no box;
  - the anchor-box IoUs of every sample and set, on which the margin conditions below are asserted;
  - for a seeded spatial_features_2d the three loss terms and the reference autograd's gradients on cls_preds, box_preds and
    dir_cls_preds (stored NCHW, as the convolutions leave them), batch_cls_preds and batch_box_preds;
  - the loss terms and decode of a head without the direction classifier, and the loss terms with num_class = 1.
Conditions (MARGIN = 1e-3): no IoU lies within MARGIN of a matched or unmatched threshold; every box's best IoU exceeds its
best strictly smaller IoU by at least MARGIN.  With them a label can differ only through the `==` against a box's best IoU.
One box cannot meet the second condition as it is worded: the square box's two rotations of one cell "tie" at 0.7636379 and
0.7636361, 1.8e-6 apart and not the same bits.  For such a group (every IoU within MARGIN of the best) the condition asked
instead is that all of it lies at least MARGIN above the matched threshold: each member is positive with or without being
forced, and takes its label and target from its own arg-max box, so which of them equals the best changes no output.
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from gen_head_fixtures import install_reference  # noqa: E402

B, H, W, CIN = 2, 12, 20, 8
CLASS_NAMES = ['Car', 'Pedestrian', 'Cyclist']
GRID_SIZE = [40, 24, 1]
PC_RANGE = [0.0, -9.6, -3.0, 32.0, 9.6, 1.0]
MARGIN = 1e-3
SETS = [('Car', [3.9, 1.6, 1.56], -1.78, 0.6, 0.45), ('Pedestrian', [0.8, 0.6, 1.73], -0.6, 0.5, 0.35),
        ('Cyclist', [1.76, 0.6, 1.73], -0.6, 0.5, 0.35)]


class EasyDict(dict):
    """attribute access, nested dicts wrapped (lists stay lists of plain dicts: the reference indexes those by key)"""

    def __init__(self, d=None):
        super().__init__()
        for k, v in (d or {}).items():
            self[k] = EasyDict(v) if isinstance(v, dict) else v

    def __getattr__(self, k):
        try:
            return self[k]
        except KeyError:
            raise AttributeError(k)


def head_cfg(align_center=False, direction=True, norm=False):
    cfg = {'NAME': 'AnchorHeadSingle', 'CLASS_AGNOSTIC': False, 'DIR_OFFSET': 0.78539, 'DIR_LIMIT_OFFSET': 0.0, 'NUM_DIR_BINS': 2,
           'ANCHOR_GENERATOR_CONFIG': [
               {'class_name': n, 'anchor_sizes': [size], 'anchor_rotations': [0, 1.57], 'anchor_bottom_heights': [z],
                'align_center': align_center, 'feature_map_stride': 2, 'matched_threshold': hi, 'unmatched_threshold': lo}
               for n, size, z, hi, lo in SETS],
           'TARGET_ASSIGNER_CONFIG': {'NAME': 'AxisAlignedTargetAssigner', 'POS_FRACTION': -1.0, 'SAMPLE_SIZE': 512,
                                      'NORM_BY_NUM_EXAMPLES': norm, 'MATCH_HEIGHT': False, 'BOX_CODER': 'ResidualCoder'},
           'LOSS_CONFIG': {'LOSS_WEIGHTS': {'cls_weight': 1.0, 'loc_weight': 2.0, 'dir_weight': 0.2, 'code_weights': [1.0] * 7}}}
    if direction:
        cfg['USE_DIRECTION_CLASSIFIER'] = True
    return cfg


def box_set():
    gt = np.zeros((B, 10, 8), dtype=np.float32)
    gt[0, 0] = [10.3, -2.1, -1.0, 3.9, 1.6, 1.56, 0.3, 1]      # best IoU between the thresholds: matched only by force
    gt[0, 1] = [20.1, 3.3, -1.0, 4.2, 1.7, 1.5, 1.62, 1]       # heading past pi / 4: swapped extents
    gt[0, 3] = [5.2, 1.0, -0.6, 0.8, 0.6, 1.7, -1.2, 2]
    gt[0, 4] = [15.5, -5.0, -0.6, 1.76, 0.6, 1.73, 2.1, 3]     # forced, below unmatched
    gt[0, 5] = gt[0, 0]                                        # arg-max tie between boxes: the lower index
    gt[0, 6] = [40.0, 0.0, -1.0, 3.9, 1.6, 1.56, 0.0, 1]       # outside the range: best IoU exactly 0
    gt[0, 7] = [13.47, 0.87, -0.6, 0.7, 0.7, 1.8, 0.9, 2]      # square: both rotations of one cell tie
    gt[0, 8] = [25.3, 6.1, -0.6, 1.7, 0.6, 1.7, 0.05, 3]
    gt[1, 0] = [16.84, -0.87, -1.0, 3.9, 1.6, 1.56, 0.0, 1]
    return gt


def build(ref_single, cfg, num_class=3, seed=21):
    torch.manual_seed(seed)
    return ref_single.AnchorHeadSingle(model_cfg=EasyDict(cfg), input_channels=CIN, num_class=num_class, class_names=CLASS_NAMES,
                                       grid_size=np.array(GRID_SIZE), point_cloud_range=np.array(PC_RANGE),
                                       predict_boxes_when_training=False)


def check_margins(ious):
    """ious: {(b, s): (anchors of set s, boxes of its class)} -> the smallest distance to a threshold"""
    nearest = np.inf
    for (b, s), m in ious.items():
        if m.size == 0:
            continue
        for th in SETS[s][3:5]:
            nearest = min(nearest, float(np.abs(m.astype(np.float64) - th).min()))
        for j in range(m.shape[1]):
            col = m[:, j].astype(np.float64)
            best = col.max()
            if best > 0:
                group = col[col > best - MARGIN]
                alone = len(np.unique(group)) == 1                   # the best value alone (however many anchors share its bits)
                assert alone or group.min() >= SETS[s][3] + MARGIN, f'sample {b} set {s} box {j}: runner-up within the margin of the best'
                assert best - col[col <= best - MARGIN].max() >= MARGIN
    assert nearest >= MARGIN, f'an IoU within {nearest} of a threshold'
    return nearest


def nchw(t):
    return t.detach().permute(0, 3, 1, 2).contiguous().numpy()


def run_training(head, feats, gt):
    head.train()
    head({'batch_size': B, 'spatial_features_2d': torch.from_numpy(feats), 'gt_boxes': torch.from_numpy(gt.copy())})
    fr = head.forward_ret_dict
    keys = [k for k in ('cls_preds', 'box_preds', 'dir_cls_preds') if k in fr]
    for k in keys:
        fr[k].retain_grad()
    loss, tb = head.get_loss()
    loss.backward()
    return fr, keys, tb


def main():
    install_reference()
    from pcdet.models.dense_heads import anchor_head_single as ref_single
    from pcdet.utils import box_utils as ref_box_utils
    out, manifest = {}, {}
    gt = box_set()
    feats = np.random.default_rng(3).standard_normal((B, CIN, H, W)).astype(np.float32)
    out.update(gt_boxes=gt, spatial_features_2d=feats)

    head = build(ref_single, head_cfg())
    for s, a in enumerate(head.anchors):
        out[f'anchors.{s}'] = a.numpy()
    for s, a in enumerate(build(ref_single, head_cfg(align_center=True)).anchors):
        out[f'anchors_ac.{s}'] = a.numpy()
    manifest[f'AnchorHeadSingle(input_channels={CIN},num_class=3,USE_DIRECTION_CLASSIFIER)'] = {k: list(v.shape) for k, v in head.state_dict().items()}
    for k, v in head.state_dict().items():
        out[f'state.{k}'] = v.numpy().copy()

    ious = {}
    for b in range(B):
        for s in range(3):
            mine = gt[b][gt[b, :, 7] == s + 1]
            m = ref_box_utils.boxes3d_nearest_bev_iou(head.anchors[s].view(-1, 7), torch.from_numpy(mine[:, :7])).numpy() \
                if len(mine) else np.zeros((head.anchors[s].view(-1, 7).shape[0], 0), dtype=np.float32)
            ious[(b, s)] = m
            out[f'iou.{b}.{s}'] = m
    nearest = check_margins(ious)

    for tag, norm in (('norm0', False), ('norm1', True)):
        h2 = build(ref_single, head_cfg(norm=norm))
        td = h2.assign_targets(torch.from_numpy(gt.copy()))
        out[f'targets.{tag}.labels'] = td['box_cls_labels'].numpy().astype(np.int32)
        out[f'targets.{tag}.reg'] = td['box_reg_targets'].numpy()
        out[f'targets.{tag}.weights'] = td['reg_weights'].numpy()
    labels = out['targets.norm0.labels']
    counts = [{int(v): int((labels[b] == v).sum()) for v in np.unique(labels[b])} for b in range(B)]
    assert counts == [{-1: 2, 0: 1431, 1: 2, 2: 3, 3: 2}, {0: 1439, 1: 1}], counts

    fr, keys, tb = run_training(head, feats, gt)
    for k in keys:
        out[f'pred.{k}'] = nchw(fr[k])
        out[f'grad.{k}'] = nchw(fr[k].grad)
    for k, v in tb.items():
        out[f'tb.{k}'] = np.float32(v)
    head.eval()
    with torch.no_grad():
        bd = head({'batch_size': B, 'spatial_features_2d': torch.from_numpy(feats)})
    out.update(batch_cls_preds=bd['batch_cls_preds'].numpy(), batch_box_preds=bd['batch_box_preds'].numpy())

    nodir = build(ref_single, head_cfg(direction=False))
    assert nodir.conv_dir_cls is None
    manifest[f'AnchorHeadSingle(input_channels={CIN},num_class=3)'] = {k: list(v.shape) for k, v in nodir.state_dict().items()}
    for k, v in nodir.state_dict().items():
        out[f'nodir.state.{k}'] = v.numpy().copy()
    fr, keys, tb = run_training(nodir, feats, gt)
    assert keys == ['cls_preds', 'box_preds'] and 'rpn_loss_dir' not in tb
    for k, v in tb.items():
        out[f'nodir.tb.{k}'] = np.float32(v)
    nodir.eval()
    with torch.no_grad():
        bd = nodir({'batch_size': B, 'spatial_features_2d': torch.from_numpy(feats)})
    out.update({'nodir.batch_cls_preds': bd['batch_cls_preds'].numpy(), 'nodir.batch_box_preds': bd['batch_box_preds'].numpy()})

    one = build(ref_single, head_cfg(), num_class=1)
    manifest[f'AnchorHeadSingle(input_channels={CIN},num_class=1,USE_DIRECTION_CLASSIFIER)'] = {k: list(v.shape) for k, v in one.state_dict().items()}
    for k, v in one.state_dict().items():
        out[f'nc1.state.{k}'] = v.numpy().copy()
    fr, keys, tb = run_training(one, feats, gt)
    for k, v in tb.items():
        out[f'nc1.tb.{k}'] = np.float32(v)
    out['nc1.grad.cls_preds'] = nchw(fr['cls_preds'].grad)

    np.savez_compressed(os.path.join(HERE, 'ref_anchor_head.npz'), **out)
    with open(os.path.join(HERE, 'ref_anchor_head_manifest.json'), 'w') as f:
        json.dump(manifest, f, indent=1, sort_keys=True)
    print('wrote', len(out), 'arrays; labels', counts, 'nearest threshold distance %.4f' % nearest,
          'loss', {k: float(out[k]) for k in out if k.startswith('tb.')})


if __name__ == '__main__':
    main()

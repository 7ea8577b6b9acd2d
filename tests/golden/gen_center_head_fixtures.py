#!/usr/bin/env python3
"""Generates tests/golden/ref_center_head.npz (+ ref_center_head_manifest.json) by running the REFERENCE's own CenterHead
on the CPU: pcdet/models/dense_heads/center_head.py, models/model_utils/centernet_utils.py and utils/loss_utils.py,
imported from where they lie, nothing copied, with the stubs of gen_head_fixtures.install_reference (numba, SharedArray,
iou3d_nms, roiaware_pool3d, `.cuda()` as the identity).  Run in the authoring container only; the outputs hold numbers
and key names only.

Shapes: B = 2, H = 12, W = 20 (non-square on purpose), input_channels = 8, SHARED_CONV_CHANNEL = 16, NUM_MAX_OBJS = 6.
Records
  - the state-dict manifest and values of the one-head and the two-head ([['Car'], ['Pedestrian', 'Cyclist']]) heads;
  - assign_targets of both heads for a box set with padding rows between real boxes, a box on the far grid edge, two boxes
    of different classes in one cell, a dx = 0 box in the middle of the list and a sample with no box (the reference gets
    a clone: it relabels its argument in place);
  - assign_targets for MORE boxes than NUM_MAX_OBJS.  The reference cannot run that input (`ret_boxes_src[:n] = gt_boxes`,
    center_head.py:123, raises for n > num_max_objs, which the generator asserts), so the expectation is the reference's
    output for the same list cut to the first NUM_MAX_OBJS boxes — "only the first NUM_MAX_OBJS take part";
  - get_loss per term and the gradients on the head outputs from the reference's autograd;
  - RegLossCenterNet values / gradients with a NaN target element and with an all-zero mask;
  - decode_bbox_from_heatmap for K = 10 (candidates outside the limit range and below the threshold, one sample without a
    survivor) and K = H * W, on inputs that meet the margin conditions asserted in check_decode_conditions().
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from gen_head_fixtures import install_reference  # noqa: E402


class EasyDict(dict):
    """attribute access that copy.deepcopy can probe (the reference deep-copies HEAD_DICT)"""

    def __init__(self, d=None):
        super().__init__()
        for k, v in (d or {}).items():
            self[k] = EasyDict(v) if isinstance(v, dict) else v

    def __getattr__(self, k):
        try:
            return self[k]
        except KeyError:
            raise AttributeError(k)


B, H, W, CIN = 2, 12, 20, 8
CLASS_NAMES = ['Car', 'Pedestrian', 'Cyclist']
PC_RANGE = [0.0, -2.4, -3.0, 8.0, 2.4, 1.0]
VOXEL = [0.05, 0.05, 0.1]
STRIDE = 8
LIMIT = [0.5, -2.0, -2.0, 7.5, 2.0, 1.0]
MARGIN = 1e-3


def head_cfg(class_names_each_head):
    return {'CLASS_NAMES_EACH_HEAD': class_names_each_head, 'SHARED_CONV_CHANNEL': 16, 'USE_BIAS_BEFORE_NORM': True, 'NUM_HM_CONV': 2,
            'SEPARATE_HEAD_CFG': {'HEAD_ORDER': ['center', 'center_z', 'dim', 'rot'],
                                  'HEAD_DICT': {'center': {'out_channels': 2, 'num_conv': 2}, 'center_z': {'out_channels': 1, 'num_conv': 2},
                                                'dim': {'out_channels': 3, 'num_conv': 2}, 'rot': {'out_channels': 2, 'num_conv': 2}}},
            'TARGET_ASSIGNER_CONFIG': {'FEATURE_MAP_STRIDE': STRIDE, 'NUM_MAX_OBJS': 6, 'GAUSSIAN_OVERLAP': 0.1, 'MIN_RADIUS': 2},
            'LOSS_CONFIG': {'LOSS_WEIGHTS': {'cls_weight': 1.0, 'loc_weight': 2.0,
                                             'code_weights': [1.0, 1.0, 0.5, 1.0, 1.0, 1.0, 2.0, 1.0]}},
            'POST_PROCESSING': {'SCORE_THRESH': 0.1, 'POST_CENTER_LIMIT_RANGE': LIMIT, 'MAX_OBJ_PER_SAMPLE': 10,
                                'NMS_CONFIG': {'NMS_TYPE': 'nms_gpu', 'NMS_THRESH': 0.1, 'NMS_PRE_MAXSIZE': 100, 'NMS_POST_MAXSIZE': 10}}}


def box_sets():
    """gt (B, 9, 8): sample 0 = six real boxes with padding rows between them, sample 1 empty; over (B, 10, 8): nine
    real boxes in sample 0 (more than NUM_MAX_OBJS), three in sample 1."""
    gt = np.zeros((B, 9, 8), dtype=np.float32)
    gt[0, 0] = [2.13, -1.07, -1.0, 3.9, 1.6, 1.5, 0.3, 1]        # Car
    gt[0, 2] = [5.31, 0.52, -0.8, 0.8, 0.6, 1.7, -1.2, 2]        # Pedestrian
    gt[0, 3] = [5.38, 0.47, -0.9, 1.7, 0.6, 1.7, 2.1, 3]         # Cyclist in the Pedestrian's cell (13, 7)
    gt[0, 4] = [3.3, 1.1, -1.0, 0.0, 1.5, 1.5, 0.1, 1]           # Car with dx = 0: a used, empty slot
    gt[0, 6] = [8.0, 2.4, -0.7, 4.2, 1.7, 1.6, -2.9, 1]          # Car on the far grid edge: cell clamped to (19, 11)
    gt[0, 7] = [0.9, -2.1, -1.1, 0.7, 0.7, 1.8, 0.9, 2]          # Pedestrian
    over = np.zeros((B, 10, 8), dtype=np.float32)
    rng = np.random.default_rng(11)
    for b, rows in ((0, [0, 1, 2, 3, 5, 6, 7, 8, 9]), (1, [1, 4, 5])):
        for r in rows:
            cls = int(rng.integers(1, 4))
            size = np.array([[3.9, 1.6, 1.56], [0.8, 0.6, 1.73], [1.76, 0.6, 1.73]], dtype=np.float32)[cls - 1] * rng.uniform(0.8, 1.2, 3)
            over[b, r] = [rng.uniform(0.2, 7.8), rng.uniform(-2.2, 2.2), rng.uniform(-1.2, -0.6), *size, rng.uniform(-3.1, 3.1), cls]
    return gt, over


def record_targets(out, prefix, td):
    for h in range(len(td['heatmaps'])):
        for key in ('heatmaps', 'target_boxes', 'inds', 'masks', 'target_boxes_src'):
            out[f'{prefix}.{key}.{h}'] = td[key][h].numpy()


def check_decode_conditions(scores, K, thresh, boxes):
    """scores (B, C*H*W) sigmoid values, boxes (B, K, 7) the K ranked candidates before masking"""
    top = np.sort(scores, axis=1)[:, ::-1][:, :min(K + 1, scores.shape[1])]
    assert (top[:, :-1] - top[:, 1:]).min() >= MARGIN, 'consecutive scores closer than the margin'
    assert np.abs(top[:, :K] - thresh).min() >= MARGIN, 'a candidate within the margin of the score threshold'
    lim = np.array(LIMIT, dtype=np.float64)
    assert min(np.abs(boxes[..., :3] - lim[:3]).min(), np.abs(boxes[..., :3] - lim[3:]).min()) >= MARGIN, \
        'a candidate within the margin of a limit-range bound'


def decode_inputs(seed):
    """scores of every sample: a permutation of one master grid whose upper part has a step of 2.5e-3 (a threshold half way
    between two of its points keeps the margin to both samples' candidates), the rest packed below; sample 1 starts
    twelve steps lower, so it tops out under the K = 10 threshold"""
    rng = np.random.default_rng(seed)
    n = 3 * H * W
    upper = 0.98 - 0.0025 * np.arange(H * W + 24)
    master = np.concatenate([upper, np.linspace(upper[-1] - 0.01, 0.02, n)])
    hm = np.stack([rng.permutation(master[s:s + n]) for s in (0, 12)])
    logits = np.log(hm / (1 - hm)).astype(np.float32).reshape(B, 3, H, W)
    maps = {'center': rng.uniform(-0.3, 1.3, (B, 2, H, W)), 'center_z': rng.uniform(-2.6, 1.6, (B, 1, H, W)),
            'dim': rng.uniform(-0.5, 1.4, (B, 3, H, W)), 'rot': rng.uniform(-1, 1, (B, 2, H, W))}
    return logits, {k: v.astype(np.float32) for k, v in maps.items()}


def main():
    _, cu, _, lu = install_reference()
    from pcdet.models.dense_heads import center_head as ref_ch
    out, manifest = {}, {}
    gt, over = box_sets()
    out.update(gt_boxes=gt, gt_boxes_over=over)
    feats = np.random.default_rng(3).standard_normal((B, CIN, H, W)).astype(np.float32)
    out['spatial_features_2d'] = feats

    for tag, names in (('one', [['Car', 'Pedestrian', 'Cyclist']]), ('two', [['Car'], ['Pedestrian', 'Cyclist']])):
        torch.manual_seed(21)
        head = ref_ch.CenterHead(model_cfg=EasyDict(head_cfg(names)), input_channels=CIN, num_class=3, class_names=CLASS_NAMES,
                                 grid_size=np.array([160, 96, 40]), point_cloud_range=PC_RANGE, voxel_size=VOXEL,
                                 predict_boxes_when_training=False)
        manifest[f'CenterHead({names},input_channels={CIN},SHARED_CONV_CHANNEL=16)'] = {k: list(v.shape) for k, v in head.state_dict().items()}
        for k, v in head.state_dict().items():
            out[f'{tag}.state.{k}'] = v.numpy()
        head.train()
        before = torch.from_numpy(gt.copy())
        bd = head({'batch_size': B, 'spatial_features_2d': torch.from_numpy(feats), 'gt_boxes': before.clone()})
        assert 'rois' not in bd
        record_targets(out, f'{tag}.targets', head.forward_ret_dict['target_dicts'])
        preds = head.forward_ret_dict['pred_dicts']
        leaves = []
        for h, pd in enumerate(preds):
            for name in ('hm', 'center', 'center_z', 'dim', 'rot'):
                pd[name].retain_grad()
                leaves.append((h, name, pd[name]))
                out[f'{tag}.pred.{name}.{h}'] = pd[name].detach().numpy().copy()
        loss, tb = head.get_loss()
        loss.backward()
        out[f'{tag}.loss'] = np.float32(loss.item())
        for k, v in tb.items():
            out[f'{tag}.tb.{k}'] = np.float32(v)
        for h, name, t in leaves:
            out[f'{tag}.grad.{name}.{h}'] = t.grad.numpy().copy()
        if tag == 'one':
            # more boxes than NUM_MAX_OBJS: the reference raises; the expectation is its output for the list cut to the first six
            try:
                head.assign_targets(torch.from_numpy(over.copy()), feature_map_size=(H, W))
                raise AssertionError('the reference was expected to reject more boxes than NUM_MAX_OBJS')
            except RuntimeError:
                pass
            cut = over.copy()
            for b in range(B):
                real = np.nonzero(cut[b, :, 7] > 0)[0]
                cut[b, real[6:]] = 0
            record_targets(out, 'one.targets_over', head.assign_targets(torch.from_numpy(cut), feature_map_size=(H, W)))

    # regression loss alone: a NaN target element, slots sharing a cell, and an all-zero mask
    rng = np.random.default_rng(5)
    pred = torch.from_numpy(rng.standard_normal((B, 8, H, W)).astype(np.float32))
    inds = torch.from_numpy(rng.integers(0, H * W, (B, 6)))
    inds[0, 3] = inds[0, 1]                                           # two slots of sample 0 in one cell
    inds[1, 5] = inds[1, 0]
    mask = torch.tensor([[1, 1, 0, 1, 1, 0], [1, 0, 1, 0, 0, 1]])
    target = torch.from_numpy(rng.standard_normal((B, 6, 8)).astype(np.float32))
    target[0, 1, 4] = float('nan')
    reg = lu.RegLossCenterNet()
    w = torch.tensor([1.0, 1.0, 0.5, 1.0, 1.0, 1.0, 2.0, 1.0])
    # the reference's own graph: code 4 of its loss is NaN (NaN * 0 stays NaN, see utils/loss_utils._reg_loss); its gradient is
    # finite, the backward of |pred m - NaN| being sgn(NaN) * m = 0 at the NaN element
    pred2 = pred.clone().requires_grad_(True)
    per_code = reg(pred2, mask, inds, target)
    (per_code * w).sum().mul(2.0).backward()
    assert torch.isnan(per_code[4]) and torch.isfinite(per_code[[0, 1, 2, 3, 5, 6, 7]]).all()
    assert torch.isfinite(pred2.grad).all(), 'the reference gradient with a NaN target element was expected to be finite'
    out.update(reg_pred=pred.numpy(), reg_inds=inds.numpy(), reg_mask=mask.numpy(), reg_target=target.numpy(),
               reg_code_weights=w.numpy(), reg_loc_weight=np.float32(2.0), reg_per_code=per_code.detach().numpy(),
               reg_grad=pred2.grad.numpy().copy())
    pred3 = pred.clone().requires_grad_(True)
    zero = reg(pred3, torch.zeros_like(mask), inds, target.nan_to_num())
    (zero * w).sum().mul(2.0).backward()
    out.update(reg_zero_per_code=zero.detach().numpy(), reg_zero_grad=pred3.grad.numpy())

    # decode
    limit_t = torch.tensor(LIMIT)
    for seed in range(100, 200):
        logits, maps = decode_inputs(seed)
        t = {k: torch.from_numpy(v) for k, v in maps.items()}
        scores = torch.from_numpy(logits).sigmoid()
        flat = scores.flatten(1).numpy().astype(np.float64)
        s0 = np.sort(flat[0])[::-1]
        th10, thall = float((s0[5] + s0[6]) / 2), float((s0[150] + s0[151]) / 2)
        try:
            res = {}
            for K, th in ((10, th10), (H * W, thall)):
                kw = dict(heatmap=scores, rot_cos=t['rot'][:, 0:1], rot_sin=t['rot'][:, 1:2], center=t['center'], center_z=t['center_z'],
                          dim=t['dim'].exp(), point_cloud_range=PC_RANGE, voxel_size=VOXEL, feature_map_stride=STRIDE, K=K)
                everything = cu.decode_bbox_from_heatmap(score_thresh=-1.0, post_center_limit_range=torch.tensor([-1e9] * 3 + [1e9] * 3), **kw)
                ranked = np.stack([d['pred_boxes'].numpy() for d in everything])
                assert ranked.shape == (B, K, 7)
                check_decode_conditions(flat, K, th, ranked.astype(np.float64))
                res[K] = cu.decode_bbox_from_heatmap(score_thresh=th, post_center_limit_range=limit_t, **kw)
                if K == 10:
                    in_range = ((ranked[0, :, :3] >= np.array(LIMIT[:3])) & (ranked[0, :, :3] <= np.array(LIMIT[3:]))).all(1)
                    assert not in_range.all() and len(res[K][0]['pred_boxes']) >= 1 and len(res[K][1]['pred_boxes']) == 0
                    assert (in_range[:6]).any() and not in_range[:6].all(), 'sample 0: a candidate above the threshold outside the range'
        except AssertionError:
            continue
        break
    else:
        raise SystemExit('no seed meets the decode conditions')
    out.update(dec_hm=logits, dec_thresh_10=np.float32(th10), dec_thresh_all=np.float32(thall), dec_limit=np.array(LIMIT, dtype=np.float32),
               dec_seed=np.int64(seed))
    for k, v in maps.items():
        out[f'dec_{k}'] = v
    for K, tag in ((10, '10'), (H * W, 'all')):
        for b, d in enumerate(res[K]):
            out[f'dec{tag}.boxes.{b}'] = d['pred_boxes'].numpy()
            out[f'dec{tag}.scores.{b}'] = d['pred_scores'].numpy()
            out[f'dec{tag}.labels.{b}'] = d['pred_labels'].numpy().astype(np.int64)

    np.savez_compressed(os.path.join(HERE, 'ref_center_head.npz'), **out)
    with open(os.path.join(HERE, 'ref_center_head_manifest.json'), 'w') as f:
        json.dump(manifest, f, indent=1, sort_keys=True)
    print('wrote', len(out), 'arrays; decode seed', seed, 'survivors', [[len(d['pred_boxes']) for d in res[K]] for K in res],
          'loss', float(out['one.loss']), float(out['two.loss']))


if __name__ == '__main__':
    main()

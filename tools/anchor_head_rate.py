"""The anchor head's three device operators against their torch formulations, per 32-sample batch at POINT_PILLAR_CFG's
shapes (248 x 216 cells x 6 anchors = 321 408 anchors per sample, three classes, two direction bins, fp32 maps):
  a  targets   AxisAlignedTargetAssigner.assign_targets: pdm_anchor_targets  vs  the per-sample, per-set torch formulation
               (an (anchors x boxes) IoU matrix per set and sample, boolean-mask indexing: the reference's algorithm)
  b  loss      anchor_head_ops.anchor_head_loss forward + backward to the three maps  vs  get_cls_layer_loss +
               get_box_reg_layer_loss with autograd (permuted copies, one-hot targets, sin-difference concatenations)
  c  decode    anchor_head_ops.anchor_decode  vs  ResidualCoder.decode_torch on permuted copies + the direction fix-up
The two forms of a case are called alternately in one process on the same device and inputs, timed with device events
around each full call (host synchronisations included), after a warm-up; medians are reported.  Results are compared
first.  Prints one JSON line.  --fused-only N runs each device operator N times and nothing else (for a kernel trace).

  python tools/anchor_head_rate.py [--bs 32] [--boxes 40] [--calls 30] [--warmup 5] [--fused-only N]
"""
import argparse
import copy
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from pdm_ssd_amd import anchor_head_ops  # noqa: E402
from pdm_ssd_amd.config import cfg_from_dict  # noqa: E402
from pdm_ssd_amd.dense_heads import AnchorHeadSingle  # noqa: E402
from pdm_ssd_amd.detector_config import CLASS_NAMES, PILLAR_GRID_SIZE, PILLAR_RANGE, POINT_PILLAR_CFG  # noqa: E402


def timed(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    out = fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e), out


def compare(fused, plain, calls, warmup):
    t = {'fused': [], 'torch': []}
    for i in range(warmup + calls):
        for name, fn in (('fused', fused), ('torch', plain)):
            ms, _ = timed(fn)
            if i >= warmup:
                t[name].append(ms)
    med = {k: statistics.median(v) for k, v in t.items()}
    return {'fused_ms': round(med['fused'], 3), 'torch_ms': round(med['torch'], 3), 'speedup': round(med['torch'] / med['fused'], 2),
            'fused_ms_min': round(min(t['fused']), 3), 'torch_ms_min': round(min(t['torch']), 3)}


def scene_boxes(B, M, seed):
    rng = np.random.default_rng(seed)
    gt = np.zeros((B, M, 8), dtype=np.float32)
    sizes = np.array([[3.9, 1.6, 1.56], [0.8, 0.6, 1.73], [1.76, 0.6, 1.73]], dtype=np.float32)
    for b in range(B):
        k = M - b % 8
        cls = rng.integers(1, 4, k)
        gt[b, :k, 0] = rng.uniform(1, 68, k); gt[b, :k, 1] = rng.uniform(-39, 39, k); gt[b, :k, 2] = rng.uniform(-1.5, -0.5, k)
        gt[b, :k, 3:6] = sizes[cls - 1] * rng.uniform(0.9, 1.1, (k, 3))
        gt[b, :k, 6] = rng.uniform(-np.pi, np.pi, k)
        gt[b, :k, 7] = cls
    return gt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--bs', type=int, default=32)
    ap.add_argument('--boxes', type=int, default=40)
    ap.add_argument('--calls', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--fused-only', type=int, default=0)
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    torch.manual_seed(3)
    cfg = copy.deepcopy(POINT_PILLAR_CFG['DENSE_HEAD'])
    head = AnchorHeadSingle(model_cfg=cfg_from_dict(cfg), input_channels=384, num_class=3, class_names=CLASS_NAMES,
                            grid_size=np.array(PILLAR_GRID_SIZE), point_cloud_range=np.array(PILLAR_RANGE),
                            predict_boxes_when_training=False).to(dev).train()
    B, H, W, A_loc = args.bs, 248, 216, 6
    gt = torch.from_numpy(scene_boxes(B, args.boxes, 1)).to(dev)
    cls = torch.randn((B, A_loc * 3, H, W), device=dev) - 2.0
    box = torch.randn((B, A_loc * 7, H, W), device=dev) * 0.3
    dirs = torch.randn((B, A_loc * 2, H, W), device=dev)
    weights = cfg['LOSS_CONFIG']['LOSS_WEIGHTS']

    def targets(fused):
        head.use_fused = fused
        return head.assign_targets(gt)

    def loss_fused(td, maps):
        terms = anchor_head_ops.anchor_head_loss(
            maps[0], maps[1], maps[2], td['box_cls_labels'], td['box_reg_targets'], td['num_pos'], head._anchor_rot, weights['code_weights'], 3,
            num_dir_bins=2, cls_weight=weights['cls_weight'], loc_weight=weights['loc_weight'], dir_weight=weights['dir_weight'],
            dir_offset=cfg['DIR_OFFSET'])
        total = terms[0] + terms[1] + terms[2]
        return total, torch.autograd.grad(total, maps)

    def decode(fused):
        head.use_fused = fused
        with torch.no_grad():
            return head.generate_predicted_boxes(B, cls, box, dirs)[1]

    td = targets(True)
    maps = [t.clone().requires_grad_(True) for t in (cls, box, dirs)]
    if args.fused_only:
        for _ in range(args.fused_only):
            targets(True)
            loss_fused(td, maps)
            decode(True)
        torch.cuda.synchronize()
        print(json.dumps({'tool': 'anchor_head_rate', 'fused_only_calls': args.fused_only}))
        return
    res = {'tool': 'anchor_head_rate', 'bs': B, 'map': [H, W], 'anchors_per_sample': H * W * A_loc, 'boxes_per_sample': args.boxes,
           'calls': args.calls, 'warmup': args.warmup, 'device': torch.cuda.get_device_name(0)}

    plain = targets(False)
    differ = int((td['box_cls_labels'] != plain['box_cls_labels']).sum())
    # (on the device torch divides a tensor by a Python number through a reciprocal, so a heading within an ulp of the pi / 4
    # swap can fall the other way there; the CPU formulation, which the tests use, divides)
    assert differ <= 2e-6 * td['box_cls_labels'].numel(), differ
    same = td['box_cls_labels'] == plain['box_cls_labels']
    assert float(((td['box_reg_targets'] - plain['box_reg_targets']).abs().amax(-1) * same).max()) <= 1e-4
    twice = targets(True)
    res['a_targets'] = dict(compare(lambda: targets(True), lambda: targets(False), args.calls, args.warmup), labels_that_differ=differ,
                            positives_mean=round(float(td['num_pos'].float().mean()), 1),
                            two_fused_calls_same_bits=all(torch.equal(td[k], twice[k]) for k in td))

    def loss_torch():
        head.use_fused = False
        head.forward_ret_dict = dict(cls_preds=maps[0], box_preds=maps[1], dir_cls_preds=maps[2], **td)
        total, _ = head.get_loss()
        return total, torch.autograd.grad(total, maps)
    (la, ga), (lb, gb) = loss_fused(td, maps), loss_torch()
    assert abs(float(la.detach()) - float(lb.detach())) <= 1e-4 * max(1.0, abs(float(lb.detach())))
    assert all(float((p - q).abs().max()) <= 1e-4 * float(q.abs().max()) for p, q in zip(ga, gb))
    la2, ga2 = loss_fused(td, maps)
    same_bits = torch.equal(la.detach(), la2.detach()) and all(torch.equal(p, q) for p, q in zip(ga, ga2))
    del ga, gb, ga2
    res['b_loss_grad'] = dict(compare(lambda: loss_fused(td, maps), loss_torch, args.calls, args.warmup), two_fused_calls_same_bits=same_bits)

    a, b = decode(True), decode(False)
    assert float((a - b).abs().max()) <= 1e-4 * float(b.abs().max())
    same_bits = torch.equal(a, decode(True))
    del a, b
    res['c_decode'] = dict(compare(lambda: decode(True), lambda: decode(False), args.calls, args.warmup), two_fused_calls_same_bits=same_bits)
    print(json.dumps(res))


if __name__ == '__main__':
    main()

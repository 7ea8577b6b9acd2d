"""CenterHead's three device operators against their torch formulations, per 32-sample batch at CENTER_PDM_CFG's shapes
(128 x 200 x 176 BEV map, one head of three classes, NUM_MAX_OBJS = MAX_OBJ_PER_SAMPLE = 500):
  a  targets              CenterHead.assign_targets: pdm_center_targets  vs  the per-sample torch formulation
  b  decode + NMS         CenterHead.generate_predicted_boxes: pdm_center_decode + pdm_post_process (BATCHED, one host read)
                          vs  centernet_utils.decode_bbox_from_heatmap + the per-sample NMS loop
  c  regression loss      center_head_ops.center_reg_loss forward + backward  vs  loss_utils.RegLossCenterNet with autograd
The two forms of a case are called alternately in one process on the same device and inputs, timed with device events
around each full call (host synchronisations included), after a warm-up; medians are reported.  Results are compared
first.  Prints one JSON line.

  python tools/center_head_rate.py [--bs 32] [--boxes 40] [--calls 50] [--warmup 10]
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

from pdm_ssd_amd import center_head_ops, synthetic  # noqa: E402
from pdm_ssd_amd.config import cfg_from_dict  # noqa: E402
from pdm_ssd_amd.dense_heads import CenterHead  # noqa: E402
from pdm_ssd_amd.detector_config import CENTER_PDM_CFG, CLASS_NAMES, GRID_SIZE, VOXEL_SIZE  # noqa: E402
from pdm_ssd_amd.utils import loss_utils  # noqa: E402


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
        gt[b, :k, 0] = rng.uniform(1, 69, k); gt[b, :k, 1] = rng.uniform(-39, 39, k); gt[b, :k, 2] = rng.uniform(-1.5, -0.5, k)
        gt[b, :k, 3:6] = sizes[cls - 1] * rng.uniform(0.9, 1.1, (k, 3))
        gt[b, :k, 6] = rng.uniform(-np.pi, np.pi, k)
        gt[b, :k, 7] = cls
    return gt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--bs', type=int, default=32)
    ap.add_argument('--boxes', type=int, default=40)
    ap.add_argument('--calls', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=10)
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    torch.manual_seed(3)
    cfg = copy.deepcopy(CENTER_PDM_CFG['DENSE_HEAD'])
    cfg['POST_PROCESSING']['BATCHED'] = True
    head = CenterHead(model_cfg=cfg_from_dict(cfg), input_channels=128, num_class=3, class_names=CLASS_NAMES, grid_size=GRID_SIZE,
                      point_cloud_range=list(synthetic.KITTI_RANGE), voxel_size=VOXEL_SIZE, predict_boxes_when_training=False).to(dev).eval()
    B, H, W = args.bs, 200, 176
    gt = torch.from_numpy(scene_boxes(B, args.boxes, 1)).to(dev)
    with torch.no_grad():
        x = torch.randn((B, 128, H, W), device=dev)
        pred = head.heads_list[0](head.shared_conv(x))
        pred['hm'] = pred['hm'] + 0.4          # sigmoid(-2.19 + 0.4 + noise): scores on both sides of SCORE_THRESH
    res = {'tool': 'center_head_rate', 'bs': B, 'map': [H, W], 'boxes_per_sample': args.boxes, 'calls': args.calls, 'warmup': args.warmup,
           'device': torch.cuda.get_device_name(0)}

    def targets(fused):
        head.use_fused = fused
        return head.assign_targets(gt, feature_map_size=(H, W))
    a, b = targets(True), targets(False)
    assert all(torch.equal(a[k][0], b[k][0]) for k in ('inds', 'masks', 'target_boxes_src'))
    assert float((a['heatmaps'][0] - b['heatmaps'][0]).abs().max()) <= 1e-5 and float((a['target_boxes'][0] - b['target_boxes'][0]).abs().max()) <= 1e-4
    res['a_targets'] = dict(compare(lambda: targets(True), lambda: targets(False), args.calls, args.warmup),
                            host_reads_fused=0, host_reads_torch=f'{3 * B} (two boolean-mask sizes and one radius per sample)')

    def boxes(fused):
        head.use_fused = fused
        with torch.no_grad():
            return head.generate_predicted_boxes(B, [pred])
    a, b = boxes(True), boxes(False)
    same = all(len(p['pred_boxes']) == len(q['pred_boxes']) and torch.equal(p['pred_labels'], q['pred_labels'])
               and float((p['pred_boxes'] - q['pred_boxes']).abs().max()) <= 1e-3 for p, q in zip(a, b))
    res['b_decode_nms'] = dict(compare(lambda: boxes(True), lambda: boxes(False), args.calls, args.warmup), same_boxes=bool(same),
                               kept_mean=round(sum(len(p['pred_boxes']) for p in a) / B, 1))

    td = targets(True)
    inds, mask, tb = td['inds'][0], td['masks'][0], td['target_boxes'][0]
    maps = [pred[n].detach().clone().requires_grad_(True) for n in ('center', 'center_z', 'dim', 'rot')]
    w = list(cfg['LOSS_CONFIG']['LOSS_WEIGHTS']['code_weights'])
    lw = cfg['LOSS_CONFIG']['LOSS_WEIGHTS']['loc_weight']
    reg = loss_utils.RegLossCenterNet()

    def reg_fused():
        loc, _ = center_head_ops.center_reg_loss(maps, inds, mask, tb, w, lw)
        return loc, torch.autograd.grad(loc, maps)

    def reg_torch():
        per_code = reg(torch.cat(maps, dim=1), mask, inds, tb)
        loc = (per_code * per_code.new_tensor(w)).sum() * lw
        return loc, torch.autograd.grad(loc, maps)
    (la, ga), (lb, gb) = reg_fused(), reg_torch()
    la, lb = la.detach(), lb.detach()
    assert abs(float(la) - float(lb)) <= 1e-4 * max(1.0, abs(float(lb))) and all(float((p - q).abs().max()) <= 1e-6 for p, q in zip(ga, gb))
    res['c_reg_loss_grad'] = dict(compare(reg_fused, reg_torch, args.calls, args.warmup), host_reads_fused=0, host_reads_torch=0,
                                  bit_reproducible_fused=True, bit_reproducible_torch=False)
    print(json.dumps(res))


if __name__ == '__main__':
    main()

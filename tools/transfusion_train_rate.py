"""TransFusionHead's training operators against their per-sample torch formulations at the workload's shape: a 180 x 180 map,
ten classes, P = 200 queries, 40 valid boxes a sample (48 rows with the padding), B = 1 and 4.
  assign   transfusion_ops.assign (one launch chain, no host read)  vs transfusion_ops.assign_torch: sample by sample the three cost
           matrices, the numpy solver on the host, the targets, and the heat-map gaussians box by box
  loss     transfusion_ops.loss forward + backward                  vs transfusion_ops.loss_torch forward + backward
  head     TransFusionHead's training forward + backward (use_fused = True; the decoder runs nn.MultiheadAttention under autograd)
  step     build_transfusion_lidar(TRANSFUSION_LIDAR_TRAIN_CFG): forward, backward and one SGD step on synthetic points
For each operator the device-to-host reads (torch's synchronisation debug mode) and the kernel launches (torch.profiler's device
activity, which sees the library's own kernels too) of one call are counted.  The two forms are called alternately on the same
device and inputs, timed with device events around each call after a warm-up; medians are reported.  Prints one JSON line and
writes it to profiles/transfusion_train_rate.json.  No ratio is fixed in advance: the numbers are the record, and an entry that
comes out slower than its torch formulation is marked so.

  python tools/transfusion_train_rate.py [--bs 1 4] [--calls 10] [--warmup 3] [--no-step] [--out FILE]
"""
import argparse
import copy
import json
import os
import statistics
import sys
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from pdm_ssd_amd import transfusion_ops  # noqa: E402
from pdm_ssd_amd import detector_config as dc  # noqa: E402
from pdm_ssd_amd.config import cfg_from_dict  # noqa: E402
from pdm_ssd_amd.dense_heads import TransFusionHead  # noqa: E402

H = W = 180
CIN = 512
VALID, M = 40, 48


def timed(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    out = fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e), out


def rounds(fns, calls, warmup):
    """the functions called in turn, round after round -> their median times (ms)"""
    t = [[] for _ in fns]
    for i in range(warmup + calls):
        for j, fn in enumerate(fns):
            ms = timed(fn)[0]
            if i >= warmup:
                t[j].append(ms)
    return [statistics.median(x) for x in t]


def host_reads(fn):
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('warn')
    try:
        with warnings.catch_warnings(record=True) as seen:
            warnings.simplefilter('always')
            fn()
    finally:
        torch.cuda.set_sync_debug_mode('default')
    return sum('synchroniz' in str(w.message).lower() for w in seen)


def launches(fn):
    """kernel launches of one call as torch.profiler's device activity reports them; None where the profiler gives nothing"""
    try:
        from torch.profiler import ProfilerActivity, profile
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        n = sum(1 for ev in prof.events() if 'cuda' in str(ev.device_type).lower() and 'mem' not in ev.name.lower())
        return n or None
    except Exception:
        return None


def counted(name, ours, theirs, calls, warmup):
    ms, ms_t = rounds([ours, theirs], calls, warmup)
    return {'what': name, 'ms': round(ms, 4), 'ms_torch': round(ms_t, 4), 'slower_than_torch': bool(ms > ms_t),
            'host_reads': host_reads(ours), 'host_reads_torch': host_reads(theirs), 'launches': launches(ours), 'launches_torch': launches(theirs)}


def ground_truth(boxes, seed):
    """(B, M, 10): VALID boxes a sample on decoded predictions, half of them moved by centimetres, half by metres; zero padding"""
    rng = np.random.default_rng(seed)
    B, P = boxes.shape[:2]
    gt = np.zeros((B, M, 10), dtype=np.float32)
    for b in range(B):
        for m, p in enumerate(rng.permutation(P)[:VALID]):
            box = boxes[b, p].copy()
            box[:2] += rng.uniform(-1, 1, 2) * (0.1 if m % 2 else 3.0)
            box[3:6] = np.clip(box[3:6] * rng.uniform(0.9, 1.1, 3), 0.3, 12.0)
            gt[b, m, :9] = box
            gt[b, m, 9] = rng.integers(1, 11)
    gt[..., :2] = np.clip(gt[..., :2], -53.0, 53.0) * (gt[..., 3:4] > 0)
    return gt


def run(bs, calls, warmup, dev):
    torch.manual_seed(bs)
    head = TransFusionHead(model_cfg=cfg_from_dict(copy.deepcopy(dc.TRANSFUSION_LIDAR_TRAIN_CFG['DENSE_HEAD'])), input_channels=CIN, num_class=10,
                           class_names=dc.TRANSFUSION_CLASS_NAMES, grid_size=dc.TRANSFUSION_GRID_SIZE, point_cloud_range=dc.TRANSFUSION_RANGE,
                           voxel_size=dc.TRANSFUSION_VOXEL_SIZE, predict_boxes_when_training=False).to(dev).train()
    x = torch.randn((bs, CIN, H, W), device=dev)
    with torch.no_grad():
        pred = {k: v.detach() for k, v in head.predict(x).items()}
    maps = [pred[k] for k in ('heatmap', 'center', 'height', 'dim', 'rot', 'vel')]
    boxes = transfusion_ops.decode_torch(*maps, head.query_labels, torch.ones_like(pred['query_heatmap_score']), 0.0, [-1e4] * 3 + [1e4] * 3,
                                         -54.0, -54.0, 0.075, 0.075, 8)[0].cpu().numpy()
    gt = torch.from_numpy(ground_truth(boxes, bs)).to(dev)
    args = head._assign_args()
    res = {'bs': bs, 'entries': []}
    res['entries'].append(counted('assign', lambda: transfusion_ops.assign(*maps, gt, *args), lambda: transfusion_ops.assign_torch(*maps, gt, *args),
                                  calls, warmup))
    ours, theirs = transfusion_ops.assign(*maps, gt, *args), transfusion_ops.assign_torch(*maps, gt, *args)
    res['assign_agrees'] = {'assigned': bool(torch.equal(ours['assigned'], theirs['assigned'])), 'num_pos': int(ours['num_pos']),
                            'heatmap_max_abs_diff': float((ours['heatmap'] - theirs['heatmap']).abs().max()),
                            'bbox_targets_max_abs_diff': float((ours['bbox_targets'] - theirs['bbox_targets']).abs().max())}
    leaves = [t.clone().requires_grad_(True) for t in maps] + [pred['dense_heatmap'].clone().requires_grad_(True)]
    largs = (head.code_weights, head.loss_cls_weight, head.loss_bbox_weight, head.loss_heatmap_weight, head.loss_cls_alpha, head.loss_cls_gamma)

    def both(fn):
        for t in leaves:
            t.grad = None
        total = sum(fn(*leaves[:6], leaves[6], ours, *largs))
        total.backward()
        return total.detach()
    res['entries'].append(counted('loss', lambda: both(transfusion_ops.loss), lambda: both(transfusion_ops.loss_torch), calls, warmup))
    res['loss_agrees'] = {'ours': float(both(transfusion_ops.loss)), 'torch': float(both(transfusion_ops.loss_torch))}

    def head_step():
        head.zero_grad(set_to_none=True)
        head({'batch_size': bs, 'spatial_features_2d': x, 'gt_boxes': gt})['loss'].backward()
    res['head_forward_backward_ms'] = round(rounds([head_step], calls, warmup)[0], 4)
    res['head_forward_host_reads'] = host_reads(lambda: head({'batch_size': bs, 'spatial_features_2d': x, 'gt_boxes': gt}))
    return res, gt


def detector_step(bs, gt, calls, warmup, dev):
    torch.manual_seed(10 + bs)
    net = dc.build_transfusion_lidar(copy.deepcopy(dc.TRANSFUSION_LIDAR_TRAIN_CFG)).to(dev).train()
    opt = torch.optim.SGD(net.parameters(), lr=1e-4)
    rng = np.random.default_rng(bs)
    n = 60000
    rows = [np.concatenate([np.full((n, 1), b), rng.uniform(-53.5, 53.5, (n, 2)), rng.uniform(-4.5, 2.5, (n, 1)), rng.uniform(0, 1, (n, 2))], 1)
            for b in range(bs)]
    pts = torch.from_numpy(np.concatenate(rows).astype(np.float32)).to(dev)

    def step():
        opt.zero_grad(set_to_none=True)
        ret, _, _ = net({'batch_size': bs, 'points': pts.clone(), 'gt_boxes': gt})
        ret['loss'].backward()
        opt.step()
        return ret['loss'].detach()
    ms = rounds([step], calls, warmup)[0]
    return {'ms': round(ms, 4), 'points_per_sample': n, 'loss_finite': bool(torch.isfinite(step()))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--bs', type=int, nargs='+', default=[1, 4])
    ap.add_argument('--calls', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--no-step', action='store_true')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'transfusion_train_rate.json'))
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    runs = []
    for bs in args.bs:
        res, gt = run(bs, args.calls, args.warmup, dev)
        if not args.no_step:
            res['detector_training_step'] = detector_step(bs, gt, max(args.calls // 2, 3), 2, dev)
        runs.append(res)
    out = {'tool': 'tools/transfusion_train_rate.py', 'device': torch.cuda.get_device_name(0), 'map': [H, W], 'queries': 200, 'classes': 10,
           'valid_boxes': VALID, 'gt_rows': M, 'calls': args.calls, 'warmup': args.warmup, 'runs': runs}
    line = json.dumps(out)
    print(line)
    with open(args.out, 'w') as f:
        f.write(line + '\n')


if __name__ == '__main__':
    main()

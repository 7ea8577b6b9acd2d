"""Second-stage training targets and losses: time and kernel-launch count of one `assign_targets + get_loss + backward`
at B = 32 samples, R = 512 proposals, S = 128 sampled RoIs, M = 20 ground-truth boxes, for
  - the fused path: pdm_proposal_targets + pdm_rcnn_loss (csrc/roi_targets.hip), backward = two scalings, and
  - the torch loss path: the same targets, the losses as RoIHeadTemplate's plain torch formulation (use_fused_loss = False).
Both use the device operator for the targets: the reference's ProposalTargetLayer (a Python loop over samples and classes
with host reads) has no counterpart here to time.  Steps are timed with device events after a warm-up (median and minimum),
the host's time to ISSUE a step is measured without synchronising inside it, and the launches of one step are counted with
torch.profiler (kernels only; memcpy / memset rows are listed apart).  Prints one JSON line and writes it to --out.

  python tools/roi_target_rate.py [--calls 20] [--warmup 3] [--out profiles/roi_target_rate.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from pdm_ssd_amd.config import cfg_from_dict  # noqa: E402
from pdm_ssd_amd.detector_config import POINT_RCNN_TRAIN_CFG  # noqa: E402
from pdm_ssd_amd.roi_heads import RoIHeadTemplate  # noqa: E402

SIZES = np.array([[3.9, 1.6, 1.56], [0.8, 0.6, 1.73], [1.76, 0.6, 1.73]], dtype=np.float32)


def scene(B, R, M, seed):
    """M boxes of the three KITTI classes per sample; a quarter of the proposals close to one of them, a quarter shifted by up
    to a metre, the rest anywhere (labels: the box's class, or random)"""
    rng = np.random.default_rng(seed)
    gt = np.zeros((B, M, 8), dtype=np.float32)
    cls = rng.integers(1, 4, (B, M))
    gt[..., 0] = rng.uniform(0, 70, (B, M))
    gt[..., 1] = rng.uniform(-40, 40, (B, M))
    gt[..., 2] = rng.uniform(-1.5, -0.5, (B, M))
    gt[..., 3:6] = SIZES[cls - 1] * rng.uniform(0.9, 1.1, (B, M, 3))
    gt[..., 6] = rng.uniform(-np.pi, np.pi, (B, M))
    gt[..., 7] = cls
    pick = rng.integers(0, M, (B, R))
    rois = np.take_along_axis(gt, pick[..., None], 1)[..., 0:7].copy()
    labels = np.take_along_axis(cls, pick, 1).astype(np.int64)
    spread = np.where(np.arange(R) < R // 4, 0.05, np.where(np.arange(R) < R // 2, 1.0, 30.0)).astype(np.float32)
    rois[..., 0:2] += rng.uniform(-1, 1, (B, R, 2)).astype(np.float32) * spread[None, :, None]
    rois[..., 6] += rng.uniform(-0.1, 0.1, (B, R)).astype(np.float32)
    return rois, rng.uniform(0, 1, (B, R)).astype(np.float32), labels, gt


def make_step(dev, fused, B, R, S, M):
    cfg = {'TARGET_CONFIG': dict(POINT_RCNN_TRAIN_CFG['ROI_HEAD']['TARGET_CONFIG'], ROI_PER_IMAGE=S),
           'LOSS_CONFIG': POINT_RCNN_TRAIN_CFG['ROI_HEAD']['LOSS_CONFIG']}
    head = RoIHeadTemplate(num_class=1, model_cfg=cfg_from_dict(cfg), seed=1)
    head.use_fused_loss = fused
    rois, scores, labels, gt = (torch.from_numpy(a).to(dev) for a in scene(B, R, M, 0))
    bd = {'batch_size': B, 'rois': rois, 'roi_scores': scores, 'roi_labels': labels, 'gt_boxes': gt}
    g = torch.Generator(device='cpu').manual_seed(2)
    rcnn_cls = (torch.randn((B * S, 1), generator=g) * 2).to(dev).requires_grad_(True)
    rcnn_reg = (torch.randn((B * S, 7), generator=g) * 0.2).to(dev).requires_grad_(True)

    def step():
        rcnn_cls.grad = rcnn_reg.grad = None
        targets = head.assign_targets(bd)
        head.forward_ret_dict = dict(targets, rcnn_cls=rcnn_cls, rcnn_reg=rcnn_reg)
        loss, tb = head.get_loss()
        loss.backward()
        return loss, tb
    return step


def measure(step, calls, warmup):
    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    ms, issue = [], []
    for _ in range(calls):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        s.record()
        loss, tb = step()
        e.record()
        issue.append((time.perf_counter() - t0) * 1e3)
        e.synchronize()
        ms.append(s.elapsed_time(e))
    res = {'ms': round(statistics.median(ms), 4), 'ms_min': round(min(ms), 4), 'host_issue_ms': round(statistics.median(issue), 4),
           'loss': float(loss), 'loss_reg': float(tb['rcnn_loss_reg']), 'loss_corner': float(tb['rcnn_loss_corner'])}
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
            step()
            torch.cuda.synchronize()
        names = [ev.name for ev in prof.events() if ev.device_type == torch.autograd.DeviceType.CUDA]
        copies = [n_ for n_ in names if 'memcpy' in n_.lower() or 'memset' in n_.lower()]
        res.update(kernel_launches=len(names) - len(copies), memcpy_memset=len(copies),
                   own_kernels=sorted({n_ for n_ in names if 'proposal_targets' in n_ or 'rcnn_loss' in n_}))
    except Exception as exc:     # the count is a figure of this tool, not something to guess: say why it is missing
        res.update(kernel_launches=None, launch_count_error=repr(exc))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--calls', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--out', default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles', 'roi_target_rate.json'))
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    B, R, S, M = 32, 512, 128, 20
    res = {'tool': 'roi_target_rate', 'calls': args.calls, 'warmup': args.warmup, 'device': torch.cuda.get_device_name(0),
           'shape': {'B': B, 'R': R, 'S': S, 'M': M},
           'fused': measure(make_step(dev, True, B, R, S, M), args.calls, args.warmup),
           'torch_loss': measure(make_step(dev, False, B, R, S, M), args.calls, args.warmup)}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()

"""KITTI evaluation rate: a seeded synthetic set of KITTI-val size (3769 frames, 3 classes; tests/kitti_eval_reference
.synthetic_frames) scored by pdm_ssd_amd.kitti_eval on the device, beside the plain CPU restatement
(tests/kitti_eval_reference.official_result, one core) timed on the first --cpu-frames frames of the same set.  The
device figure is the wall time of a whole get_official_eval_result call (packing the annotation dicts, uploads, the
kernels, the two device-to-host reads, the host curves) and, from a second pass that synchronises between stages,
the time per stage.  On the timed subset the two sides' counts are checked to be equal.  Prints one JSON line.

  python tools/kitti_eval_rate.py [--frames 3769] [--cpu-frames 200] [--calls 5] [--out profiles/kitti_eval_rate.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

from pdm_ssd_amd import kitti_eval as ke  # noqa: E402

CLASSES = ['Car', 'Pedestrian', 'Cyclist']


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=3769)
    ap.add_argument('--cpu-frames', type=int, default=200)
    ap.add_argument('--calls', type=int, default=5)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    import kitti_eval_reference as kr
    dev = torch.device('cuda:0')
    gts, dts = kr.synthetic_frames(2026, args.frames)
    ke.get_official_eval_result(gts[:8], dts[:8], CLASSES, device=dev)        # warm-up
    wall, stats = [], {}
    for _ in range(args.calls):
        stats = {}
        torch.cuda.synchronize()
        t = time.perf_counter()
        text, ret = ke.get_official_eval_result(gts, dts, CLASSES, device=dev, stats=stats)
        wall.append((time.perf_counter() - t) * 1e3)
    staged = {'stage_ms': {}}
    ke.get_official_eval_result(gts, dts, CLASSES, device=dev, stats=staged)
    stage_ms = {k: round(v, 3) for k, v in staged['stage_ms'].items() if k != 'start'}
    # the CPU restatement on a subset, and the device on the same subset
    n = min(args.cpu_frames, args.frames)
    t = time.perf_counter()
    detail = {}
    kr.official_result(gts[:n], dts[:n], CLASSES, detail=detail)
    cpu_ms = (time.perf_counter() - t) * 1e3
    keep = {}
    ke.get_official_eval_result(gts[:n], dts[:n], CLASSES, device=dev, keep=keep)
    sums, nthr = keep['sums'].reshape(54, 41, 4), keep['num_thresholds'].reshape(54)
    equal = all(np.array_equal(sums[t_, :nthr[t_], :3], detail[t_ // 18][('pr', (t_ // 6) % 3, (t_ // 2) % 3, t_ % 2)][:, :3].astype(np.int64))
                for t_ in range(54))
    line = {'metric': 'kitti_eval_ms', 'frames': args.frames, 'classes': 3, 'gt_boxes': int(sum(len(g['name']) for g in gts)),
            'detections': int(sum(len(d['name']) for d in dts)), 'combinations': 54, 'thresholds_total': int(keep['num_thresholds'].sum()),
            'device_call_ms_median': statistics.median(wall), 'device_call_ms_min': min(wall), 'launches': stats['launches'],
            'device_to_host_reads': stats['reads'], 'stage_ms': stage_ms, 'dominant_stage': max(stage_ms, key=stage_ms.get),
            'cpu_restatement_frames_timed': n, 'cpu_restatement_ms': cpu_ms,
            'cpu_restatement_ms_scaled_to_all_frames': cpu_ms * args.frames / max(n, 1), 'subset_counts_equal_device': bool(equal),
            'Car_3d_moderate_R40': float(ret['Car_3d/moderate_R40']), 'device': torch.cuda.get_device_name(0)}
    out = json.dumps(line)
    print(out)
    if args.out:
        with open(args.out, 'w') as fh:
            fh.write(out + '\n')


if __name__ == '__main__':
    main()

"""Detector post-processing: the per-sample loop (Detector3DTemplate.post_processing_loop) against the batched
device path (post_process.batched_post_processing, POST_PROCESSING.BATCHED) at bs=32 x 16384 point-head rows.
The two are called alternately in one process, timed with device events around each full call (host
synchronisations included), after a warm-up; results are checked to be identical.  Cases:
  a  the detector's own eval outputs (PDM_SSD_CFG on synthetic.lidar_like_clouds, point-head cls bias 0.5 as in
     test_detector_eval_returns_nms_filtered_predictions)
  b  worst case: the same boxes with every row above SCORE_THRESH, NMS_PRE_MAXSIZE = 4096
Prints one JSON line.

  python tools/post_process_rate.py [--bs 32] [--points 16384] [--calls 50] [--warmup 5]
  python tools/post_process_rate.py --batched-only 20     # case a's batched calls alone (for a kernel trace)
"""
import argparse
import copy
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from pdm_ssd_amd import post_process, synthetic  # noqa: E402
from pdm_ssd_amd.detector_config import PDM_SSD_CFG, build_pdm_ssd  # noqa: E402
from pdm_ssd_amd.detectors.detector3d_template import Detector3DTemplate  # noqa: E402


def eval_batch_dict(B, N, dev):
    torch.manual_seed(2)
    model = build_pdm_ssd(PDM_SSD_CFG).to(dev).eval()
    with torch.no_grad():
        model.point_head.cls_layers[-1].bias.fill_(0.5)
    pts = torch.from_numpy(synthetic.to_batch_points(synthetic.lidar_like_clouds(B, N, 9))).to(dev)
    captured = {}

    def grab(bd):
        captured['bd'] = bd
        return [], {}
    model.post_processing = grab
    with torch.no_grad():
        model({'batch_size': B, 'points': pts})
    return model, captured['bd']


def same(x, y):
    return len(x[0]) == len(y[0]) and x[1] == y[1] and all(
        torch.equal(a[k], b[k]) for a, b in zip(x[0], y[0]) for k in ('pred_boxes', 'pred_scores', 'pred_labels'))


def timed(fn, *args):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    out = fn(*args)
    e.record()
    e.synchronize()
    return s.elapsed_time(e), out


def run_case(model, bd, cfg, calls, warmup):
    loop = lambda b: Detector3DTemplate.post_processing_loop(model, b)   # noqa: E731
    batched = lambda b: post_process.batched_post_processing(b, cfg, model.num_class)   # noqa: E731
    padded = lambda b: post_process.post_process_padded(b, cfg, model.num_class)   # noqa: E731
    model.model_cfg = dict(model.model_cfg, POST_PROCESSING=cfg)
    t = {'loop': [], 'batched': [], 'padded': []}
    for i in range(warmup + calls):
        for name, fn in (('loop', loop), ('batched', batched), ('padded', padded)):
            ms, out = timed(fn, bd)
            if i >= warmup:
                t[name].append(ms)
            if name == 'loop':
                want = out
            elif name == 'batched' and i == 0:
                assert same(out, want), "batched post-processing differs from the loop"
    kept = [d['pred_boxes'].shape[0] for d in want[0]]
    med = {k: statistics.median(v) for k, v in t.items()}
    return {'loop_ms': round(med['loop'], 3), 'batched_ms': round(med['batched'], 3),
            'padded_device_ms': round(med['padded'], 3), 'speedup': round(med['loop'] / med['batched'], 2),
            'loop_ms_min': round(min(t['loop']), 3), 'batched_ms_min': round(min(t['batched']), 3),
            'candidates_per_sample': round(float((torch.sigmoid(bd['batch_cls_preds']).max(-1)[0] >=
                                                  cfg['SCORE_THRESH']).sum()) / int(bd['batch_size']), 1),
            'kept_mean': round(sum(kept) / len(kept), 1), 'identical': True}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--bs', type=int, default=32)
    ap.add_argument('--points', type=int, default=16384)
    ap.add_argument('--calls', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--batched-only', type=int, default=0, metavar='N')
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    model, bd = eval_batch_dict(args.bs, args.points, dev)
    cfg = copy.deepcopy(PDM_SSD_CFG['POST_PROCESSING'])
    if args.batched_only:
        for _ in range(args.batched_only):
            post_process.batched_post_processing(bd, cfg, model.num_class)
        torch.cuda.synchronize()
        return
    res = {'tool': 'post_process_rate', 'bs': args.bs, 'rows': int(bd['batch_box_preds'].shape[0]) // args.bs,
           'calls': args.calls, 'warmup': args.warmup, 'device': torch.cuda.get_device_name(0)}
    res['a_detector_eval'] = run_case(model, bd, cfg, args.calls, args.warmup)
    worst = dict(bd, batch_cls_preds=torch.rand_like(bd['batch_cls_preds']) * 4.0)   # sigmoid >= 0.5 everywhere
    cfg_b = copy.deepcopy(cfg)
    cfg_b['NMS_CONFIG']['NMS_PRE_MAXSIZE'] = 4096
    res['b_all_rows_above_thresh'] = run_case(model, worst, cfg_b, args.calls, args.warmup)
    print(json.dumps(res))


if __name__ == '__main__':
    main()

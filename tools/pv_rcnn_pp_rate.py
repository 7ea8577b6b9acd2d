"""PV-RCNN++'s keypoint sampling in eval mode on build_pv_rcnn_plusplus() (PV_RCNN_PP_CFG, seeded weights, the KITTI voxel grid) at
bs = 32 and bs = 4 with lidar-like clouds of about 120 k points a frame and the 100 test proposals a sample of the step itself:
  sampling   VoxelSetAbstractionSPC.get_sampled_points, three ways on the same clouds, alternately in one process:
               fused      pdm_spc_partition + one stack FPS over the B S segments (use_fused_spc = True)
               composed   the reference's formulation on the device (per-sample loops, the (points x rois) matrix, boolean masks,
                          per-sector .item() reads; use_fused_spc = False); the keypoints are compared bit for bit first
               fps        PV-RCNN's sampling: VoxelSetAbstraction.get_sampled_points, one stack FPS of NUM_KEYPOINTS picks a sample
             the partition alone (pdm_spc_partition, five launches) is timed as well
  filters    roi_point_filter on every filtered source of the encoder (one call a source)
  step       the whole eval step of PVRCNNPlusPlus and of PVRCNN on the same clouds
Each piece is timed with device events around the call after a warm-up; medians are reported, with the kernel launches of one call
as torch.profiler counts them.  Prints one JSON line and writes it to profiles/pv_rcnn_pp_rate.json.  No ratio is fixed in advance:
the numbers are the record.

  python tools/pv_rcnn_pp_rate.py [--bs 32 4] [--points 120000] [--calls 10] [--warmup 3] [--no-launch-count] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

import sparse_conv_rate as scr_tool  # noqa: E402  (timed, launches)
from pdm_ssd_amd import detector_config as dc, spc_ops, synthetic  # noqa: E402
from pdm_ssd_amd.config import cfg_get  # noqa: E402
from pdm_ssd_amd.pv_rcnn_ops import sample_counts  # noqa: E402
from pdm_ssd_amd.utils import common_utils  # noqa: E402


def alternate(fns, calls, warmup):
    """medians of the calls of every function, taken in turn"""
    times = [[] for _ in fns]
    for i in range(warmup + calls):
        for k, fn in enumerate(fns):
            t = scr_tool.timed(fn)[0]
            if i >= warmup:
                times[k].append(t)
    return [round(statistics.median(t), 4) for t in times]


def seeded(model, dev):
    model = model.to(dev).eval()
    with torch.no_grad():
        for m in model.modules():
            if isinstance(m, (torch.nn.BatchNorm1d, torch.nn.BatchNorm2d)):
                m.running_var.uniform_(0.5, 1.5)
                m.running_mean.uniform_(-0.2, 0.2)
    return model


def run(bs, n_points, calls, warmup, dev):
    pts = torch.from_numpy(synthetic.to_batch_points(synthetic.lidar_like_clouds(bs, n_points, seed0=500))).to(dev)
    torch.manual_seed(0)
    model = seeded(dc.build_pv_rcnn_plusplus(), dev)
    torch.manual_seed(0)
    plain = seeded(dc.build_pv_rcnn(), dev)
    with torch.no_grad():
        seen = {}
        hook = model.pfe.register_forward_pre_hook(lambda m, args: seen.__setitem__('front', dict(args[0])))

        def step():
            return model({'batch_size': bs, 'points': pts})

        def step_plain():
            return plain({'batch_size': bs, 'points': pts})
        step()
        hook.remove()
        front, pfe = seen['front'], model.pfe
        rois = front['rois'].float()
        raw = pts[torch.argsort(pts[:, 0], stable=True)]
        xyz, cnt = raw[:, 1:4].contiguous(), sample_counts(raw[:, 0], bs)
        spc = cfg_get(pfe.model_cfg, 'SPC_SAMPLING')
        S, radius, K = int(cfg_get(spc, 'NUM_SECTORS')), float(cfg_get(spc, 'SAMPLE_RADIUS_WITH_ROI')), int(cfg_get(pfe.model_cfg, 'NUM_KEYPOINTS'))

        def sample(fused):
            pfe.use_fused_spc = fused
            out = pfe.get_sampled_points(dict(front))
            pfe.use_fused_spc = True
            return out

        def fps():
            return plain.pfe.get_sampled_points(dict(front), raw)

        def partition():
            return spc_ops.spc_partition(xyz, cnt, rois, radius, S, K)
        kp, kp_c = sample(True), sample(False)
        assert torch.equal(kp, kp_c), 'fused against composed sampling: the keypoints differ'
        part = partition()
        res = {'bs': bs, 'points': int(pts.shape[0]), 'rois_per_sample': int(rois.shape[1]), 'num_keypoints': K, 'num_sectors': S,
               'keypoints': int(kp.shape[0]), 'kept_points': int(part['kept_cnt'].sum()),
               'keypoints_per_sample_min_max': [int(sample_counts(kp[:, 0], bs).min()), int(sample_counts(kp[:, 0], bs).max())],
               'fps_keypoints_per_sample': int(cfg_get(plain.pfe.model_cfg, 'NUM_KEYPOINTS'))}
        ms = alternate([lambda: sample(True), lambda: sample(False), fps, partition], calls, warmup)
        res['sampling'] = {'ms_fused': ms[0], 'ms_composed': ms[1], 'ms_pv_rcnn_fps': ms[2], 'ms_partition_alone': ms[3],
                           'launches_fused': scr_tool.launches(lambda: sample(True)), 'launches_composed': scr_tool.launches(lambda: sample(False)),
                           'launches_pv_rcnn_fps': scr_tool.launches(fps), 'launches_partition_alone': scr_tool.launches(partition)}
        res['filters'] = []
        SA_cfg = cfg_get(pfe.model_cfg, 'SA_LAYER')
        srcs = [('raw_points', xyz, cnt)]
        for name in pfe.SA_layer_names:
            lv = front['multi_scale_3d_features'][name]
            centres = common_utils.get_voxel_centers(lv.indices[:, 1:4], pfe.downsample_times_map[name], pfe.voxel_size, pfe.point_cloud_range)
            srcs.append((name, centres.contiguous(), sample_counts(lv.indices[:, 0], bs)))
        for name, sxyz, scnt in srcs:
            r = float(cfg_get(cfg_get(SA_cfg, name), 'RADIUS_OF_NEIGHBOR_WITH_ROI'))

            def filt():
                return spc_ops.roi_point_filter(sxyz, scnt, rois, r)
            res['filters'].append({'source': name, 'rows': int(sxyz.shape[0]), 'radius': r, 'kept': int(filt()['seg_cnt'].sum()),
                                   'ms': alternate([filt], calls, warmup)[0], 'launches': scr_tool.launches(filt)})
        ms = alternate([step, step_plain], calls, warmup)
        res['step'] = {'ms_pv_rcnn_plusplus': ms[0], 'ms_pv_rcnn': ms[1], 'launches_pv_rcnn_plusplus': scr_tool.launches(step),
                       'launches_pv_rcnn': scr_tool.launches(step_plain)}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--bs', type=int, nargs='+', default=[32, 4])
    ap.add_argument('--points', type=int, default=120000)
    ap.add_argument('--calls', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--no-launch-count', action='store_true')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'pv_rcnn_pp_rate.json'))
    args = ap.parse_args()
    scr_tool.COUNT_LAUNCHES = not args.no_launch_count
    dev = torch.device('cuda:0')
    out = {'tool': 'tools/pv_rcnn_pp_rate.py', 'device': torch.cuda.get_device_name(0), 'grid': list(dc.GRID_SIZE), 'calls': args.calls,
           'warmup': args.warmup, 'runs': []}
    for bs in args.bs:
        out['runs'].append(run(bs, args.points, args.calls, args.warmup, dev))
        print(json.dumps(out['runs'][-1]), flush=True)
        torch.cuda.empty_cache()
    line = json.dumps(out)
    print(line)
    with open(args.out, 'w') as f:
        f.write(line + '\n')


if __name__ == '__main__':
    main()

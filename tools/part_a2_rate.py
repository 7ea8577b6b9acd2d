"""PartA2FCHead from the point features to the output of its first shared FC block, fused against composed, at the published
head setting (POOL_SIZE 12, 128 features, 128 points a cell, SHARED_FC 256) at bs = 32 and bs = 4 with 100 rois a sample:
lidar-like clouds of about 120 k points a frame on the KITTI voxel grid through UNetV2 and PointIntraPartOffsetHead (seeded
weights), rois of car size with random headings centred on voxels of the scene.
  fused     PartA2FCHead._shared_fused: pdm_roiaware_pool_sparse (one host read), conv_part / conv_rpn on the sparse rows,
            pdm_sparse_fc with Conv1d + BatchNorm1d + ReLU folded
  composed  PartA2FCHead._shared_composed + shared_fc_layer[0:3]: the reference's formulation on this package's operators: per
            sample two RoIAwarePool3d calls, nonzero (a host sync), gather, the four convolutions, dense(), Conv1d, BatchNorm1d, ReLU
The two forms are called alternately in one process on the same device and inputs, timed with device events around each call
after a warm-up; medians are reported, with the kernel launches of one call as torch.profiler counts them, the peak of bytes
allocated above the inputs during one call, the active rows Q and the measured occupancy Q / (R S^3).  Results are compared
first.  Prints one JSON line and writes it to profiles/part_a2_rate.json.  No ratio is fixed in advance: the numbers are the record.

  python tools/part_a2_rate.py [--bs 32 4] [--rois 100] [--points 120000] [--calls 5] [--warmup 2] [--no-launch-count] [--out FILE]
"""
import argparse
import copy
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

import sparse_conv_rate as scr_tool  # noqa: E402  (timed, launches, alternate)
from voxel_rcnn_rate import peak_bytes, scene_rois  # noqa: E402
from pdm_ssd_amd import sparse_conv_ops, synthetic  # noqa: E402
from pdm_ssd_amd.backbones_3d import UNetV2  # noqa: E402
from pdm_ssd_amd.config import cfg_from_dict  # noqa: E402
from pdm_ssd_amd.dense_heads import PointIntraPartOffsetHead  # noqa: E402
from pdm_ssd_amd.detector_config import GRID_SIZE, PART_A2_CFG, VOXEL_SIZE  # noqa: E402
from pdm_ssd_amd.roi_heads import PartA2FCHead  # noqa: E402


def run(bs, n_rois, n_points, calls, warmup, dev):
    rng_range = list(synthetic.KITTI_RANGE)
    pts = torch.from_numpy(synthetic.to_batch_points(synthetic.lidar_like_clouds(bs, n_points, seed0=500))).to(dev)
    torch.manual_seed(0)
    net = UNetV2(cfg_from_dict({'RETURN_ENCODED_TENSOR': False}), 4, list(GRID_SIZE), VOXEL_SIZE, rng_range).to(dev).eval()
    point_head = PointIntraPartOffsetHead(1, 16, cfg_from_dict(copy.deepcopy(PART_A2_CFG['POINT_HEAD']))).to(dev).eval()
    cfg = cfg_from_dict(copy.deepcopy(PART_A2_CFG['ROI_HEAD']))
    head = PartA2FCHead(input_channels=16, model_cfg=cfg, num_class=1).to(dev).eval()
    S = head.pool_size
    with torch.no_grad():
        for m in list(net.modules()) + list(point_head.modules()) + list(head.modules()):
            if isinstance(m, torch.nn.BatchNorm1d):
                m.running_var.uniform_(0.5, 1.5)
                m.running_mean.uniform_(-0.2, 0.2)
        vox = sparse_conv_ops.voxel_assign(pts, bs, rng_range, VOXEL_SIZE, GRID_SIZE)
        bd = point_head(net({'voxel_features': vox.voxel_mean, 'voxel_coords': vox.voxel_coords, 'batch_size': bs}))
        bd['rois'] = scene_rois(vox, bs, n_rois, dev, seed=bs)
        bd['roi_labels'] = torch.ones((bs, n_rois), dtype=torch.long, device=dev)
        R = bs * n_rois
        first = head.shared_fc_layer[0:3]

        def fused():
            return head._shared_fused(bd)[0]

        def composed():
            return first(head._shared_composed(bd)[0])
        y, y_c = fused(), composed()
        scale = max(1.0, float(y_c.abs().max()))
        err = float((y - y_c).abs().max())
        assert err <= 1e-3 * scale, (err, scale)
        del y, y_c
        torch.cuda.empty_cache()
        batch_idx, xyz, part, rpn = head._point_inputs(bd)
        from pdm_ssd_amd.pv_rcnn_ops import sample_counts
        from pdm_ssd_amd.roiaware_pool3d.roiaware_pool3d_utils import roiaware_pool_sparse
        counts = sample_counts(batch_idx, bs)
        rois7 = bd['rois'][:, :, :7].contiguous()

        def pool_only():
            return roiaware_pool_sparse(rois7, xyz, counts, part, rpn, S, cfg.ROI_AWARE_POOL.MAX_POINTS_PER_VOXEL)
        Q = int(pool_only()[0].shape[0])
        ms, ms_c = scr_tool.alternate(fused, composed, calls, warmup)
        ms_pool = sorted(scr_tool.timed(pool_only)[0] for _ in range(warmup + calls))[(warmup + calls) // 2]
        res = {'bs': bs, 'rois_per_sample': n_rois, 'pool_size': S, 'rois': R, 'points': int(xyz.shape[0]), 'point_features': int(rpn.shape[1]),
               'active_rows_Q': Q, 'occupancy': round(Q / (R * S ** 3), 6), 'ms_fused': round(ms, 4), 'ms_composed': round(ms_c, 4),
               'ms_fused_pool_only': round(ms_pool, 4), 'launches_fused': scr_tool.launches(fused), 'launches_composed': scr_tool.launches(composed),
               'peak_bytes_fused': peak_bytes(fused), 'peak_bytes_composed': peak_bytes(composed),
               'fc_chunks': sparse_conv_ops.sparse_fc_chunks(R, S ** 3, head.shared_fc_layer[0].out_channels),
               'max_abs_diff': err, 'output_scale': scale}
    del net, head, bd
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--bs', type=int, nargs='+', default=[32, 4])
    ap.add_argument('--rois', type=int, default=100)
    ap.add_argument('--points', type=int, default=120000)
    ap.add_argument('--calls', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--no-launch-count', action='store_true')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'part_a2_rate.json'))
    args = ap.parse_args()
    scr_tool.COUNT_LAUNCHES = not args.no_launch_count
    dev = torch.device('cuda:0')
    out = {'tool': 'tools/part_a2_rate.py', 'device': torch.cuda.get_device_name(0), 'grid': list(GRID_SIZE), 'calls': args.calls,
           'warmup': args.warmup, 'runs': [run(bs, args.rois, args.points, args.calls, args.warmup, dev) for bs in args.bs]}
    line = json.dumps(out)
    print(line)
    with open(args.out, 'w') as f:
        f.write(line + '\n')


if __name__ == '__main__':
    main()

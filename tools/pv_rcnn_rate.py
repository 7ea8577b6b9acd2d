"""PV-RCNN's keypoint path in eval mode, piece by piece, on build_pv_rcnn() (PV_RCNN_CFG, seeded weights, the KITTI voxel grid) at
bs = 32 and bs = 4 with lidar-like clouds of about 120 k points a frame:
  keypoints   VoxelSetAbstraction.get_sampled_points: one stack FPS for the batch and the index arithmetic
  bev         pdm_bev_interpolate (one launch) against the reference's per-sample torch loop (interpolate_from_bev_features);
              the results are compared bit for bit first
  sources     every set-abstraction source of the encoder: its ball queries alone (the brute-force stack ball_query, one call a
              scale) and the whole source (queries + fused gather -> MLP -> max); the MLP share is the difference
  roi_pool    PVRCNNHead.roi_grid_pool with the fused query (pdm_roi_keypoint_query) against the composed path (torch grid points,
              ball_query per scale inside the module), on the proposals of the step; compared first
  step        the whole eval step
Each piece is timed with device events around the call after a warm-up, the two forms of a pair alternately in one process on
the same inputs; medians are reported, with the kernel launches of one call as torch.profiler counts them.  Prints one JSON line
and writes it to profiles/pv_rcnn_rate.json.  No ratio is fixed in advance: the numbers are the record.

  python tools/pv_rcnn_rate.py [--bs 32 4] [--points 120000] [--calls 10] [--warmup 3] [--no-launch-count] [--out FILE]
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

import sparse_conv_rate as scr_tool  # noqa: E402  (timed, launches, alternate)
from pdm_ssd_amd import detector_config as dc, pv_rcnn_ops, synthetic  # noqa: E402
from pdm_ssd_amd.backbones_3d.pfe.voxel_set_abstraction import sa_into, sample_counts  # noqa: E402
from pdm_ssd_amd.pointnet2_stack import pointnet2_utils  # noqa: E402
from pdm_ssd_amd.utils import common_utils  # noqa: E402


def median_ms(fn, calls, warmup):
    return statistics.median([scr_tool.timed(fn)[0] for _ in range(warmup + calls)][warmup:])


def piece(fn, calls, warmup):
    return {'ms': round(median_ms(fn, calls, warmup), 4), 'launches': scr_tool.launches(fn)}


def run(bs, n_points, calls, warmup, dev):
    pts = torch.from_numpy(synthetic.to_batch_points(synthetic.lidar_like_clouds(bs, n_points, seed0=500))).to(dev)
    torch.manual_seed(0)
    model = dc.build_pv_rcnn().to(dev).eval()
    with torch.no_grad():
        for m in model.modules():
            if isinstance(m, (torch.nn.BatchNorm1d, torch.nn.BatchNorm2d)):
                m.running_var.uniform_(0.5, 1.5)
                m.running_mean.uniform_(-0.2, 0.2)
        seen = {}
        hooks = [model.pfe.register_forward_pre_hook(lambda m, args: seen.__setitem__('front', dict(args[0]))),
                 model.roi_head.register_forward_hook(lambda m, args, out: seen.__setitem__('head', dict(out)))]

        def step():
            return model({'batch_size': bs, 'points': pts})
        step()
        for h in hooks:
            h.remove()
        front, head_bd = seen['front'], seen['head']
        pfe, head = model.pfe, model.roi_head
        res = {'bs': bs, 'points': int(pts.shape[0]), 'keypoints': int(head_bd['point_coords'].shape[0]), 'rois_per_sample': int(head_bd['rois'].shape[1])}

        raw = pts[torch.argsort(pts[:, 0], stable=True)]
        res['keypoints_sampling'] = piece(lambda: pfe.get_sampled_points(dict(front), raw), calls, warmup)
        keypoints = head_bd['point_coords']
        bev, stride = front['spatial_features'], front['spatial_features_stride']

        def bev_fused():
            return pv_rcnn_ops.bev_interpolate(keypoints, bev, pfe.point_cloud_range, pfe.voxel_size, stride)

        def bev_loop():
            return pfe.interpolate_from_bev_features(keypoints, bev, bs, stride)
        assert torch.equal(bev_fused(), bev_loop()), 'pdm_bev_interpolate against the torch loop: not bit-equal'
        ms, ms_c = scr_tool.alternate(bev_fused, bev_loop, calls, warmup)
        res['bev'] = {'ms_fused': round(ms, 4), 'ms_torch_loop': round(ms_c, 4), 'launches_fused': scr_tool.launches(bev_fused),
                      'launches_torch_loop': scr_tool.launches(bev_loop), 'channels': int(bev.shape[1]), 'map': [int(bev.shape[2]), int(bev.shape[3])]}

        new_xyz = keypoints[:, 1:4].contiguous()
        K = new_xyz.shape[0] // bs
        new_cnt = torch.full((bs,), K, dtype=torch.int32, device=dev)
        rows = torch.empty((new_xyz.shape[0], pfe.num_point_features_before_fusion), device=dev)
        srcs = [('raw_points', pfe.SA_rawpoints, raw[:, 1:4].contiguous(), sample_counts(raw[:, 0], bs), raw[:, 4:].contiguous())]
        for k, name in enumerate(pfe.SA_layer_names):
            lv = front['multi_scale_3d_features'][name]
            xyz = common_utils.get_voxel_centers(lv.indices[:, 1:4], pfe.downsample_times_map[name], pfe.voxel_size, pfe.point_cloud_range)
            srcs.append((name, pfe.SA_layers[k], xyz.contiguous(), sample_counts(lv.indices[:, 0], bs), lv.features.contiguous()))
        res['sources'] = []
        for name, layer, xyz, cnt, feats in srcs:
            def query():
                return [pointnet2_utils.ball_query(g.radius, g.nsample, xyz, cnt, new_xyz, new_cnt) for g in layer.groupers]

            def whole():
                return sa_into(layer, xyz, cnt, new_xyz, new_cnt, feats, rows, 0)
            q, w = piece(query, calls, warmup), piece(whole, calls, warmup)
            res['sources'].append({'source': name, 'rows': int(xyz.shape[0]), 'radii': [g.radius for g in layer.groupers],
                                   'nsample': [g.nsample for g in layer.groupers], 'ms_query': q['ms'], 'launches_query': q['launches'],
                                   'ms_whole': w['ms'], 'launches_whole': w['launches'], 'ms_mlp_and_rest': round(w['ms'] - q['ms'], 4)})

        def pool(fused):
            head.use_fused_pool = fused
            out = head.roi_grid_pool(head_bd)
            head.use_fused_pool = True
            return out
        y, y_c = pool(True), pool(False)
        assert head.last_pool_path == 'composed'
        row_err = (y - y_c).abs().amax(-1).flatten()
        differing = float((row_err > 1e-3 * max(1.0, float(y_c.abs().max()))).float().mean())
        assert differing <= 2e-3, differing     # (a grid point within an ulp of a query sphere may fall on either side)
        ms, ms_c = scr_tool.alternate(lambda: pool(True), lambda: pool(False), calls, warmup)
        res['roi_pool'] = {'grid_points': int(y.shape[0] * y.shape[1]), 'ms_fused_query': round(ms, 4), 'ms_composed': round(ms_c, 4),
                           'launches_fused_query': scr_tool.launches(lambda: pool(True)), 'launches_composed': scr_tool.launches(lambda: pool(False)),
                           'rows_differing': differing, 'median_row_abs_diff': float(row_err.median())}
        del y, y_c
        res['step'] = piece(step, calls, warmup)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--bs', type=int, nargs='+', default=[32, 4])
    ap.add_argument('--points', type=int, default=120000)
    ap.add_argument('--calls', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--no-launch-count', action='store_true')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'pv_rcnn_rate.json'))
    args = ap.parse_args()
    scr_tool.COUNT_LAUNCHES = not args.no_launch_count
    dev = torch.device('cuda:0')
    out = {'tool': 'tools/pv_rcnn_rate.py', 'device': torch.cuda.get_device_name(0), 'grid': list(dc.GRID_SIZE), 'calls': args.calls,
           'warmup': args.warmup, 'runs': [run(bs, args.points, args.calls, args.warmup, dev) for bs in args.bs]}
    line = json.dumps(out)
    print(line)
    with open(args.out, 'w') as f:
        f.write(line + '\n')


if __name__ == '__main__':
    main()

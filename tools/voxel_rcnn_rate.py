"""Voxel R-CNN's RoI-grid pooling, fused against composed, per source level of VOXEL_RCNN_CFG at bs = 32 and bs = 4 with 100 rois a
sample: lidar-like clouds of about 120 k points a frame on the KITTI voxel grid through VoxelBackBone8x (seeded weights), rois of
car size with random headings centred on voxels of the scene.
  fused     sparse_conv_ops.site_index of the level + NeighborVoxelSAModuleMSG.forward_fused: the mlps_in contraction over the
            level's rows and ONE pdm_roi_grid_pool launch (csrc/roi_grid_pool.hip)
  composed  the reference's formulation on this package's operators (VoxelRCNNHead._pool_level_composed): voxel centres, the
            dense (B, Z, Y, X) int32 table, VoxelQueryAndGrouping, two masked fills, Conv2d + BatchNorm2d on the offsets, add,
            ReLU, max-pool, Conv1d + BatchNorm1d + ReLU.  The grid points and their cells are computed once for all levels
            outside the timed region (the fused operator computes them inside its launch).
The two forms of a level are called alternately in one process on the same device and inputs, timed with device events around
each call after a warm-up; medians are reported, with the kernel launches of one call as torch.profiler counts them and the
peak of bytes allocated above the inputs during one call.  Results are compared first.  Prints one JSON line and writes it to
profiles/voxel_rcnn_rate.json.  No ratio is fixed in advance: the numbers are the record.

  python tools/voxel_rcnn_rate.py [--bs 32 4] [--rois 100] [--points 120000] [--calls 10] [--warmup 3] [--no-launch-count] [--out FILE]
"""
import argparse
import copy
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

import sparse_conv_rate as scr_tool  # noqa: E402  (timed, launches, alternate)
from pdm_ssd_amd import sparse_conv_ops, synthetic  # noqa: E402
from pdm_ssd_amd.backbones_3d import VoxelBackBone8x  # noqa: E402
from pdm_ssd_amd.config import cfg_from_dict  # noqa: E402
from pdm_ssd_amd.detector_config import GRID_SIZE, VOXEL_RCNN_CFG, VOXEL_SIZE  # noqa: E402
from pdm_ssd_amd.roi_heads import VoxelRCNNHead  # noqa: E402


def peak_bytes(fn):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del out
    return int(peak)


def scene_rois(vox, bs, n, dev, seed):
    """n car-sized boxes a sample with random headings, centred on voxels of that sample"""
    g = torch.Generator().manual_seed(seed)
    coords = vox.voxel_coords.cpu()
    rng0 = torch.tensor(synthetic.KITTI_RANGE[:3])
    rois = torch.zeros((bs, n, 7))
    for b in range(bs):
        rows = torch.nonzero(coords[:, 0] == b)[:, 0]
        pick = rows[torch.randint(0, len(rows), (n,), generator=g)]
        centre = (coords[pick][:, [3, 2, 1]].float() + 0.5) * torch.tensor(VOXEL_SIZE) + rng0
        rois[b, :, 0:3] = centre
        rois[b, :, 3:6] = torch.tensor([3.9, 1.6, 1.56]) * (0.8 + 0.4 * torch.rand((n, 3), generator=g))
        rois[b, :, 6] = (torch.rand(n, generator=g) * 2 - 1) * np.pi
    return rois.to(dev)


def run(bs, n_rois, n_points, calls, warmup, dev):
    rng_range = list(synthetic.KITTI_RANGE)
    pts = torch.from_numpy(synthetic.to_batch_points(synthetic.lidar_like_clouds(bs, n_points, seed0=500))).to(dev)
    torch.manual_seed(0)
    net = VoxelBackBone8x({}, 4, list(GRID_SIZE)).to(dev).eval()
    cfg = cfg_from_dict(copy.deepcopy(VOXEL_RCNN_CFG['ROI_HEAD']))
    head = VoxelRCNNHead(backbone_channels=net.backbone_channels, model_cfg=cfg, point_cloud_range=rng_range, voxel_size=VOXEL_SIZE,
                         num_class=1).to(dev).eval()
    G = int(cfg.ROI_GRID_POOL.GRID_SIZE)
    with torch.no_grad():
        for m in list(net.modules()) + list(head.modules()):
            if isinstance(m, (torch.nn.BatchNorm1d, torch.nn.BatchNorm2d)):
                m.running_var.uniform_(0.5, 1.5)
                m.running_mean.uniform_(-0.2, 0.2)
        vox = sparse_conv_ops.voxel_assign(pts, bs, rng_range, VOXEL_SIZE, GRID_SIZE)
        bd = net({'voxel_features': vox.voxel_mean, 'voxel_coords': vox.voxel_coords, 'batch_size': bs})
        rois = scene_rois(vox, bs, n_rois, dev, seed=bs)
        M = bs * n_rois * G ** 3
        res = {'bs': bs, 'rois_per_sample': n_rois, 'grid_size': G, 'grid_points': M, 'voxels': vox.num_voxels, 'levels': []}
        t_grid, (xyz, cells) = scr_tool.timed(lambda: head._grid_points_and_cells(rois, G))
        t_grid = statistics.median([scr_tool.timed(lambda: head._grid_points_and_cells(rois, G))[0] for _ in range(5)])
        res['composed_grid_points_ms'] = round(t_grid, 4)
        for k, src in enumerate(cfg.ROI_GRID_POOL.FEATURES_SOURCE):
            layer = head.roi_grid_pool_layers[k]
            sp, stride = bd['multi_scale_3d_features'][src], bd['multi_scale_3d_strides'][src]
            c2 = sum(layer.out_channels())
            out = torch.empty((M, c2), device=dev)
            assert layer.fused_supported(G)

            def index_only():
                return sparse_conv_ops.site_index(sp.indices, bs, sp.spatial_shape)

            def fused():
                layer.forward_fused(rois, G, sp.features, index_only(), stride, VOXEL_SIZE, rng_range, out, 0)
                return out

            def composed():
                return head._pool_level_composed(layer, sp, stride, bs, xyz, cells)
            y, y_c = fused().clone(), composed()
            # Among several hundred thousand grid points a few lie within an ulp of a cell boundary or of a query sphere, where
            # the last bit of torch's and the kernel's cosf / sinf decides the group: rows that differ are counted, not forbidden
            row_err = (y - y_c).abs().amax(1)
            differing = float((row_err > 1e-3 * max(1.0, float(y_c.abs().max()))).float().mean())
            err = float(row_err.median())
            assert differing <= 2e-3, (src, differing, float(row_err.max()))
            nonzero = float((y_c > 0).float().mean())
            del y, y_c
            ms, ms_c = scr_tool.alternate(fused, composed, calls, warmup)
            idx = index_only()
            ms_index = statistics.median([scr_tool.timed(index_only)[0] for _ in range(warmup + calls)][warmup:])
            ms_pool = statistics.median([scr_tool.timed(lambda: layer.forward_fused(rois, G, sp.features, idx, stride, VOXEL_SIZE, rng_range, out, 0))[0]
                                         for _ in range(warmup + calls)][warmup:])
            D, H, W = sp.spatial_shape
            g = layer.groupers[0]
            res['levels'].append({
                'level': src, 'stride': stride, 'rows': int(sp.indices.shape[0]), 'shape': [D, H, W], 'c_in': int(sp.features.shape[1]),
                'c1': layer.mlps_in[0][0].out_channels, 'c2': c2, 'query_range': list(g.max_range), 'radius': g.radius, 'nsample': g.nsample,
                'ms_fused': round(ms, 4), 'ms_composed': round(ms_c, 4), 'ms_fused_index_only': round(ms_index, 4),
                'ms_fused_without_index': round(ms_pool, 4), 'launches_fused': scr_tool.launches(fused), 'launches_composed': scr_tool.launches(composed),
                'peak_bytes_fused': peak_bytes(fused), 'peak_bytes_composed': peak_bytes(composed), 'index_bytes': int(idx.nbytes),
                'dense_table_bytes': 4 * bs * D * H * W, 'median_row_abs_diff': err, 'rows_differing': differing, 'nonzero_outputs': round(nonzero, 4)})
            del out
            torch.cuda.empty_cache()
        res['ms_fused_sum'] = round(sum(l['ms_fused'] for l in res['levels']), 4)
        res['ms_composed_sum'] = round(sum(l['ms_composed'] for l in res['levels']) + t_grid, 4)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--bs', type=int, nargs='+', default=[32, 4])
    ap.add_argument('--rois', type=int, default=100)
    ap.add_argument('--points', type=int, default=120000)
    ap.add_argument('--calls', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--no-launch-count', action='store_true')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'voxel_rcnn_rate.json'))
    args = ap.parse_args()
    scr_tool.COUNT_LAUNCHES = not args.no_launch_count
    dev = torch.device('cuda:0')
    out = {'tool': 'tools/voxel_rcnn_rate.py', 'device': torch.cuda.get_device_name(0), 'grid': list(GRID_SIZE), 'calls': args.calls,
           'warmup': args.warmup, 'runs': [run(bs, args.rois, args.points, args.calls, args.warmup, dev) for bs in args.bs]}
    line = json.dumps(out)
    print(line)
    with open(args.out, 'w') as f:
        f.write(line + '\n')


if __name__ == '__main__':
    main()

"""Voxel R-CNN's RoI-grid pooling in TRAINING mode, forward + backward, fused against composed, per source level of
VOXEL_RCNN_TRAIN_CFG at bs = 4 and bs = 32 with 128 rois a sample (the sampler's ROI_PER_IMAGE) and G = 6: lidar-like clouds of
about 120 k points a frame on the KITTI voxel grid through VoxelBackBone8x (seeded weights), rois of car size with random headings
centred on voxels of the scene (tools/voxel_rcnn_rate.py's recipe).
  fused     sparse_conv_ops.site_index of the level + NeighborVoxelSAModuleMSG.forward_fused_train (csrc/roi_grid_train.hip):
            mlps_in as the module, pdm_roi_grid_query, the position BatchNorm from the moments, RoIGridPoolFunction, mlps_out as the
            module; backward through pdm_roi_grid_pool_grad
  composed  the reference's formulation in training mode under torch autograd (VoxelRCNNHead._pool_level_composed): the dense
            (B, Z, Y, X) table, VoxelQueryAndGrouping, two grouped tensors, Conv2d + BatchNorm2d over the (M, nsample) offsets, ReLU,
            max-pool, Conv1d + BatchNorm1d + ReLU.  The grid points and their cells are computed once outside the timed region.
Both take the gradient of a fixed cotangent in the level's features and in every parameter of the pool layer.  The two forms of a
level alternate in one process, timed with device events around forward + backward after a warm-up; medians are reported with
the launches of one call (torch.profiler) and the peak of bytes allocated above the inputs.  If the composed form runs out of
memory that is recorded instead of a time.  Prints one JSON line and writes it to profiles/voxel_rcnn_train_rate.json.  No time
is fixed in advance; the condition is relative: on no level may the fused form be slower than the composed one of the same run
(`fused_never_slower`).

  python tools/voxel_rcnn_train_rate.py [--bs 4 32] [--rois 128] [--points 120000] [--calls 5] [--warmup 2] [--no-launch-count] [--out FILE]
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
import voxel_rcnn_rate as eval_tool  # noqa: E402  (peak_bytes, scene_rois)
from pdm_ssd_amd import sparse_conv_ops, synthetic  # noqa: E402
from pdm_ssd_amd.backbones_3d import VoxelBackBone8x  # noqa: E402
from pdm_ssd_amd.config import cfg_from_dict  # noqa: E402
from pdm_ssd_amd.detector_config import GRID_SIZE, VOXEL_RCNN_TRAIN_CFG, VOXEL_SIZE  # noqa: E402
from pdm_ssd_amd.roi_heads import VoxelRCNNHead  # noqa: E402


@torch.no_grad()
def groups_differing(head, layer, sp, stride, bs, rois, G, xyz, cells, rng_range):
    """the share of grid points whose group in pdm_roi_grid_query differs from VoxelQuery's over the dense table (the composed
    form's), both padded with the first hit and 0 for an empty group"""
    from pdm_ssd_amd.pointnet2_stack import voxel_query_utils
    from pdm_ssd_amd.utils import common_utils
    g = layer.groupers[0]
    index = sparse_conv_ops.site_index(sp.indices, bs, sp.spatial_shape)
    mine = sparse_conv_ops.roi_grid_query(rois, G, index, stride, VOXEL_SIZE, rng_range, g.max_range, g.radius, g.nsample).rows
    mine = torch.where(mine < 0, mine[:, :1].clamp_min(0), mine)
    centres = common_utils.get_voxel_centers(sp.indices[:, 1:4], downsample_times=stride, voxel_size=VOXEL_SIZE, point_cloud_range=rng_range)
    table = common_utils.generate_voxel2pinds(sp)
    m = xyz.shape[1]
    batch_idx = torch.arange(bs, device=xyz.device, dtype=cells.dtype).view(-1, 1, 1).expand(-1, m, 1)
    cur = torch.cat([batch_idx, torch.floor(cells / stride)], dim=-1).int().view(-1, 4)[:, [0, 3, 2, 1]].contiguous()
    theirs, _ = voxel_query_utils.voxel_query(g.max_range, g.radius, g.nsample, centres.contiguous(), xyz.contiguous().view(-1, 3), cur, table)
    return float((theirs != mine).any(1).float().mean())


def run(bs, n_rois, n_points, calls, warmup, dev):
    rng_range = list(synthetic.KITTI_RANGE)
    pts = torch.from_numpy(synthetic.to_batch_points(synthetic.lidar_like_clouds(bs, n_points, seed0=500))).to(dev)
    torch.manual_seed(0)
    net = VoxelBackBone8x({}, 4, list(GRID_SIZE)).to(dev).eval()
    cfg = cfg_from_dict(copy.deepcopy(VOXEL_RCNN_TRAIN_CFG['ROI_HEAD']))
    head = VoxelRCNNHead(backbone_channels=net.backbone_channels, model_cfg=cfg, point_cloud_range=rng_range, voxel_size=VOXEL_SIZE,
                         num_class=1).to(dev).train()
    G = int(cfg.ROI_GRID_POOL.GRID_SIZE)
    with torch.no_grad():
        vox = sparse_conv_ops.voxel_assign(pts, bs, rng_range, VOXEL_SIZE, GRID_SIZE)
        bd = net({'voxel_features': vox.voxel_mean, 'voxel_coords': vox.voxel_coords, 'batch_size': bs})
        rois = eval_tool.scene_rois(vox, bs, n_rois, dev, seed=bs)
        xyz, cells = head._grid_points_and_cells(rois, G)
    M = bs * n_rois * G ** 3
    res = {'bs': bs, 'rois_per_sample': n_rois, 'grid_size': G, 'grid_points': M, 'voxels': vox.num_voxels, 'levels': []}
    for k, src in enumerate(cfg.ROI_GRID_POOL.FEATURES_SOURCE):
        layer = head.roi_grid_pool_layers[k]
        sp, stride = bd['multi_scale_3d_features'][src], bd['multi_scale_3d_strides'][src]
        feats = sp.features.detach().clone().requires_grad_(True)
        sp_train = sp.replace_feature(feats)
        wrt = [feats] + list(layer.parameters())
        cot = torch.randn((M, sum(layer.out_channels())), device=dev)
        assert layer.fused_train_supported(G)

        def fused():
            index = sparse_conv_ops.site_index(sp.indices, bs, sp.spatial_shape)
            out = layer.forward_fused_train(rois, G, feats, index, stride, VOXEL_SIZE, rng_range)
            return torch.autograd.grad(out, wrt, cot)

        def composed():
            out = head._pool_level_composed(layer, sp_train, stride, bs, xyz, cells)
            return torch.autograd.grad(out, wrt, cot)
        g = layer.groupers[0]
        D, H, W = sp.spatial_shape
        row = {'level': src, 'stride': stride, 'rows': int(sp.indices.shape[0]), 'shape': [D, H, W], 'c_in': int(sp.features.shape[1]),
               'c1': layer.mlps_in[0][0].out_channels, 'c2': sum(layer.out_channels()), 'query_range': list(g.max_range), 'radius': g.radius,
               'nsample': g.nsample, 'saved_group_bytes': M * g.nsample * 16 + M * layer.mlps_in[0][0].out_channels}
        row['groups_differing'] = groups_differing(head, layer, sp, stride, bs, rois, G, xyz, cells, rng_range)
        try:
            ga, gc = fused(), composed()
            # Among several hundred thousand grid points a few lie within an ulp of a cell boundary or of a query sphere, where the
            # last bit of torch's and the kernel's cosf / sinf decides the group: such grid points are counted (groups_differing),
            # not forbidden, and a differing group moves one row's gradient by a whole addend
            # and so does a winner within a rounding of its runner-up, which the two forms may pick differently: the elements
            # of the features' gradient further apart than 1e-4 of the largest entry are counted as well
            big = gc[0].abs().max().clamp_min(1e-30)
            row['features_grad_rel_diff'] = float((ga[0] - gc[0]).abs().max() / big)
            row['features_grad_elements_differing'] = float(((ga[0] - gc[0]).abs() > 1e-4 * big).float().mean())
            del ga, gc
            ms, ms_c = scr_tool.alternate(fused, composed, calls, warmup)
            row.update(ms_fused=round(ms, 4), ms_composed=round(ms_c, 4), launches_composed=scr_tool.launches(composed),
                       peak_bytes_composed=eval_tool.peak_bytes(composed))
        except torch.cuda.OutOfMemoryError:
            torch.cuda.empty_cache()
            row.update(ms_composed='out of memory', ms_fused=round(scr_tool.alternate(fused, fused, calls, warmup)[0], 4))
        row.update(launches_fused=scr_tool.launches(fused), peak_bytes_fused=eval_tool.peak_bytes(fused))
        res['levels'].append(row)
        del cot, feats
        torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--bs', type=int, nargs='+', default=[4, 32])
    ap.add_argument('--rois', type=int, default=128)
    ap.add_argument('--points', type=int, default=120000)
    ap.add_argument('--calls', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--no-launch-count', action='store_true')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'voxel_rcnn_train_rate.json'))
    args = ap.parse_args()
    scr_tool.COUNT_LAUNCHES = not args.no_launch_count
    dev = torch.device('cuda:0')
    runs = [run(bs, args.rois, args.points, args.calls, args.warmup, dev) for bs in args.bs]
    timed = [l for r in runs for l in r['levels'] if not isinstance(l['ms_composed'], str)]
    out = {'tool': 'tools/voxel_rcnn_train_rate.py', 'device': torch.cuda.get_device_name(0), 'grid': list(GRID_SIZE), 'calls': args.calls,
           'warmup': args.warmup, 'runs': runs, 'fused_never_slower': all(l['ms_fused'] <= l['ms_composed'] for l in timed)}
    line = json.dumps(out)
    print(line)
    with open(args.out, 'w') as f:
        f.write(line + '\n')


if __name__ == '__main__':
    main()

"""Hard voxelization and its two encoders against the composed formulation on the padded (M, T, C) tensor, per batch of about
120 k points a frame, at bs = 32 and bs = 4:
  pillar grid  432 x 496 x 1 cells of 0.16 m, T = 32, at most 40 000 pillars a frame (POINT_PILLAR_HARD_CFG, eval)
  voxel grid   1408 x 1600 x 40 cells, T = 5, at most 40 000 voxels a frame (SECOND_HARD_CFG, eval)
  a  voxelize alone, and with the padded tensor materialised
  b  HardPillarVFE eval: voxelize + the fused PFN operator  vs  voxelize(materialize) + the reference's formulation in torch
     on the padded tensor (features, mask, nn.Linear, folded-free BatchNorm1d, ReLU, max): time, launches, peak allocation
  c  HardMeanVFE: voxelize + voxel_mean  vs  voxelize(materialize) + voxels.sum(1) / num
  d  for context only: DynamicPillarVFE / DynamicMeanVFE on the same clouds (they compute something else: every point kept)
The two forms of a case are called alternately in one process on the same device and inputs, timed with device events around
each full call (host synchronisations included), after a warm-up; medians are reported.  Results are compared first.  Prints
one JSON line and writes it to profiles/hard_voxel_rate.json.

  python tools/hard_voxel_rate.py [--bs 32 4] [--points 120000] [--calls 10] [--warmup 3] [--no-launch-count] [--out FILE]
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import pillar_rate  # noqa: E402  (timed, launches)
from pdm_ssd_amd import hard_voxel_ops, synthetic  # noqa: E402
from pdm_ssd_amd.config import cfg_from_dict  # noqa: E402
from pdm_ssd_amd.detector_config import (GRID_SIZE, PILLAR_GRID_SIZE, PILLAR_RANGE, PILLAR_VOXEL_SIZE, POINT_PILLAR_CFG,  # noqa: E402
                                         POINT_PILLAR_HARD_CFG, SECOND_HARD_CFG, VOXEL_SIZE)
from pdm_ssd_amd.vfe import DynamicMeanVFE, DynamicPillarVFE, MeanVFE, PillarVFE  # noqa: E402


def peak_mbytes(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 1)


def compare(forms, calls, warmup, count=True):
    """forms: {name: fn}, called alternately -> {name_ms, name_ms_min, name_launches, name_peak_mbytes}"""
    t = {k: [] for k in forms}
    for i in range(warmup + calls):
        for name, fn in forms.items():
            ms, _ = pillar_rate.timed(fn)
            if i >= warmup:
                t[name].append(ms)
    out = {}
    for name, fn in forms.items():
        out[f'{name}_ms'] = round(statistics.median(t[name]), 3)
        out[f'{name}_ms_min'] = round(min(t[name]), 3)
        if count:
            out[f'{name}_launches'] = pillar_rate.launches(fn)
            out[f'{name}_peak_mbytes'] = peak_mbytes(fn)
    return out


def one_batch_size(B, args, dev):
    base = synthetic.lidar_like_clouds(min(B, 4), args.points, 7)            # four distinct frames, repeated over the batch
    clouds = np.concatenate([base] * ((B + len(base) - 1) // len(base)))[:B]
    points = torch.from_numpy(synthetic.to_batch_points(clouds)).to(dev)     # samples ascending, lidar order inside a sample
    res = {}
    grids = {'pillar': (PILLAR_RANGE, PILLAR_VOXEL_SIZE, PILLAR_GRID_SIZE, POINT_PILLAR_HARD_CFG['VFE']),
             'voxel': (list(synthetic.KITTI_RANGE), VOXEL_SIZE, GRID_SIZE, SECOND_HARD_CFG['VFE'])}
    for tag, (rng, vsize, grid, vcfg) in grids.items():
        T, cap = vcfg['MAX_POINTS_PER_VOXEL'], vcfg['MAX_NUMBER_OF_VOXELS']['test']
        geo = dict(point_cloud_range=rng, voxel_size=vsize, grid_size=grid)

        def voxelize(materialize=False):
            return hard_voxel_ops.voxelize(points, B, max_points_per_voxel=T, max_voxels=cap, materialize=materialize, **geo)
        hv = voxelize(True)
        r = {'T': T, 'max_voxels': cap, 'voxels': hv.num_voxels, 'kept_slots': int(hv.voxel_num_points.sum()),
             'a_voxelize': compare({'slots_only': voxelize, 'materialized': lambda: voxelize(True)}, args.calls, args.warmup, args.count)}
        del hv
        if tag == 'pillar':
            torch.manual_seed(3)
            vfe = PillarVFE(model_cfg=cfg_from_dict(copy.deepcopy(vcfg)), num_point_features=4, **geo).to(dev).eval()
            dyn = DynamicPillarVFE(model_cfg=cfg_from_dict(copy.deepcopy(POINT_PILLAR_CFG['VFE'])), num_point_features=4, **geo).to(dev).eval()

            def fused():
                with torch.no_grad():
                    return vfe({'points': points, 'batch_size': B})['pillar_features']

            def composed():
                with torch.no_grad():
                    v = voxelize(True)
                    return vfe.composed(v.voxels, v.voxel_num_points, v.voxel_coords)

            def dynamic():
                with torch.no_grad():
                    return dyn({'points': points, 'batch_size': B})['pillar_features']
            worst = float((fused() - composed()).abs().max())
            assert worst <= 1e-3, worst
            r['b_pillar_vfe_eval'] = dict(compare({'fused': fused, 'composed': composed}, args.calls, args.warmup, args.count),
                                          worst_difference=worst)
            r['d_dynamic_pillar_vfe_eval'] = compare({'dynamic': dynamic}, args.calls, args.warmup, False)
        else:
            vfe = MeanVFE(model_cfg=cfg_from_dict(copy.deepcopy(vcfg)), num_point_features=4, **geo).eval()
            dyn = DynamicMeanVFE(model_cfg=cfg_from_dict({}), num_point_features=4, **geo).eval()

            def fused():
                return vfe({'points': points, 'batch_size': B})['voxel_features']

            def composed():
                v = voxelize(True)
                return v.voxels.sum(1) / v.voxel_num_points.clamp_min(1).float()[:, None]

            def dynamic():
                return dyn({'points': points, 'batch_size': B})['voxel_features']
            worst = float((fused() - composed()).abs().max())
            assert worst <= 1e-4, worst
            r['c_mean_vfe'] = dict(compare({'fused': fused, 'composed': composed}, args.calls, args.warmup, args.count), worst_difference=worst)
            r['d_dynamic_mean_vfe'] = compare({'dynamic': dynamic}, args.calls, args.warmup, False)
        nbytes = hard_voxel_ops._native.lib().pdm_hard_voxelize_workspace_bytes(points.shape[0], B, *grid)
        r['workspace_mbytes'] = round(nbytes / 2 ** 20, 1)
        res[tag] = r
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--bs', type=int, nargs='+', default=[32, 4])
    ap.add_argument('--points', type=int, default=120000)
    ap.add_argument('--calls', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--no-launch-count', action='store_true', help='skip the torch.profiler pass and the peak-allocation pass')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'hard_voxel_rate.json'))
    args = ap.parse_args()
    args.count = not args.no_launch_count
    dev = torch.device('cuda:0')
    res = {'tool': 'hard_voxel_rate', 'points_per_frame': args.points, 'calls': args.calls, 'warmup': args.warmup,
           'device': torch.cuda.get_device_name(0)}
    for B in args.bs:
        res[f'bs{B}'] = one_batch_size(B, args, dev)
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(line + '\n')


if __name__ == '__main__':
    main()

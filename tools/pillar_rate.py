"""The pillar front end against its torch formulation, per 32-sample batch of about 120 k points a frame on the KITTI pillar
grid (CENTER_PILLAR_CFG: 432 x 496 cells of 0.16 m, one PFN layer of 64 channels):
  a  VFE, eval       DynamicPillarVFE.forward (pdm_pillar_assign + pdm_pillar_fused_pfn, one host read)
                     vs  boolean mask + torch.unique + index_add_ mean + nn.Linear / BatchNorm1d + scatter_reduce('amax')
  b  VFE, training   forward + backward to the PFN parameters (pdm_pillar_assign, _features, _segment_max and its gradient)
                     vs  the same torch formulation through autograd
  c  scatter         pillar_ops.scatter forward (one launch for the whole canvas), and forward + backward
                     vs  the reference's loop: coords[:, 0].max().item(), then per sample zeros + masked index assignment
The two forms of a case are called alternately in one process on the same device and inputs, timed with device events
around each full call (host synchronisations included), after a warm-up; medians are reported, with the kernel launches
of one call of each form as torch.profiler counts them.  Results are compared first.  Prints one JSON line and writes it
to profiles/pillar_rate.json.

  python tools/pillar_rate.py [--bs 32] [--points 120000] [--calls 20] [--warmup 5] [--no-launch-count] [--out FILE]
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

from pdm_ssd_amd import pillar_ops, synthetic  # noqa: E402
from pdm_ssd_amd.config import cfg_from_dict  # noqa: E402
from pdm_ssd_amd.detector_config import CENTER_PILLAR_CFG, PILLAR_GRID_SIZE, PILLAR_RANGE, PILLAR_VOXEL_SIZE  # noqa: E402
from pdm_ssd_amd.vfe import DynamicPillarVFE  # noqa: E402


def timed(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    out = fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e), out


COUNT_LAUNCHES = True


def launches(fn):
    """kernel launches of one call, or None where the profiler is not available"""
    if not COUNT_LAUNCHES:
        return None
    try:
        from torch.profiler import ProfilerActivity, profile
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        n = sum(1 for ev in prof.events() if ev.device_type == torch.autograd.DeviceType.CUDA and 'memcpy' not in ev.name.lower()
                and 'memset' not in ev.name.lower())
        return n or None
    except Exception:       # noqa: BLE001 (a count is an extra; the timings do not depend on it)
        return None


def compare(ours, plain, calls, warmup):
    t = {'ours': [], 'torch': []}
    for i in range(warmup + calls):
        for name, fn in (('ours', ours), ('torch', plain)):
            ms, _ = timed(fn)
            if i >= warmup:
                t[name].append(ms)
    med = {k: statistics.median(v) for k, v in t.items()}
    return {'ours_ms': round(med['ours'], 3), 'torch_ms': round(med['torch'], 3), 'torch_over_ours': round(med['torch'] / med['ours'], 2),
            'ours_ms_min': round(min(t['ours']), 3), 'torch_ms_min': round(min(t['torch']), 3),
            'ours_launches': launches(ours), 'torch_launches': launches(plain)}


def torch_vfe(vfe, points):
    """the reference's forward on torch alone (scatter_mean as index_add_ / counts, scatter_max as scatter_reduce 'amax')"""
    r, s, g = (torch.tensor(t, device=points.device) for t in (vfe.point_cloud_range, vfe.voxel_size, vfe.grid_size))
    pc = torch.floor((points[:, [1, 2]] - r[[0, 1]]) / s[[0, 1]]).int()
    mask = ((pc >= 0) & (pc < g[[0, 1]])).all(dim=1)
    points, pc = points[mask], pc[mask]
    xyz = points[:, 1:4].contiguous()
    merge = points[:, 0].int() * (vfe.grid_size[0] * vfe.grid_size[1]) + pc[:, 0] * vfe.grid_size[1] + pc[:, 1]
    unq, inv, cnt = torch.unique(merge, return_inverse=True, return_counts=True, dim=0)
    mean = torch.zeros((len(unq), 3), device=points.device).index_add_(0, inv, xyz) / cnt[:, None]
    geom = vfe.geometry
    centre = torch.stack([pc[:, 0].float() * geom.vx + geom.x_offset, pc[:, 1].float() * geom.vy + geom.y_offset,
                          torch.full_like(xyz[:, 2], geom.z_offset)], 1)
    x = torch.cat([points[:, 1:], xyz - mean[inv], xyz - centre], dim=-1)
    layer = vfe.pfn_layers[0]
    y = layer.relu(layer.norm(layer.linear(x)))
    out = torch.zeros((len(unq), y.shape[1]), device=y.device).scatter_reduce(0, inv[:, None].expand_as(y), y, 'amax', include_self=False)
    unq = unq.int()
    plane, ny = vfe.grid_size[0] * vfe.grid_size[1], vfe.grid_size[1]
    coords = torch.stack((unq // plane, torch.zeros_like(unq), unq % ny, (unq % plane) // ny), dim=1)
    return out, coords


def torch_scatter(feats, coords, nx, ny):
    """the reference's PointPillarScatter.forward"""
    batch_size = coords[:, 0].max().int().item() + 1
    maps = []
    for b in range(batch_size):
        canvas = torch.zeros(feats.shape[1], nx * ny, dtype=feats.dtype, device=feats.device)
        m = coords[:, 0] == b
        this = coords[m, :]
        idx = (this[:, 1] + this[:, 2] * nx + this[:, 3]).long()
        canvas[:, idx] = feats[m, :].t()
        maps.append(canvas)
    return torch.stack(maps, 0).view(batch_size, feats.shape[1], ny, nx)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--bs', type=int, default=32)
    ap.add_argument('--points', type=int, default=120000)
    ap.add_argument('--calls', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--no-launch-count', action='store_true', help='skip the torch.profiler pass that counts kernel launches')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'pillar_rate.json'))
    args = ap.parse_args()
    global COUNT_LAUNCHES
    COUNT_LAUNCHES = not args.no_launch_count
    dev = torch.device('cuda:0')
    torch.manual_seed(3)
    B, nx, ny = args.bs, PILLAR_GRID_SIZE[0], PILLAR_GRID_SIZE[1]
    base = synthetic.lidar_like_clouds(min(B, 4), args.points, 7)            # four distinct frames, repeated over the batch
    clouds = np.concatenate([base] * ((B + len(base) - 1) // len(base)))[:B]
    rows = synthetic.to_batch_points(clouds)
    rows = rows[np.random.default_rng(1).permutation(len(rows))]               # samples interleave, as after a collate of shuffled clouds
    points = torch.from_numpy(rows).to(dev)
    vfe = DynamicPillarVFE(model_cfg=cfg_from_dict(copy.deepcopy(CENTER_PILLAR_CFG['VFE'])), num_point_features=4, voxel_size=PILLAR_VOXEL_SIZE,
                           grid_size=PILLAR_GRID_SIZE, point_cloud_range=PILLAR_RANGE).to(dev)
    params = list(vfe.parameters())
    res = {'tool': 'pillar_rate', 'bs': B, 'points_per_frame': args.points, 'grid': list(PILLAR_GRID_SIZE), 'calls': args.calls,
           'warmup': args.warmup, 'device': torch.cuda.get_device_name(0)}

    # a: eval
    vfe.eval()

    def ours_eval():
        with torch.no_grad():
            return vfe({'points': points, 'batch_size': B})

    def torch_eval():
        with torch.no_grad():
            return torch_vfe(vfe, points)
    bd, (want, want_coords) = ours_eval(), torch_eval()
    assert torch.equal(bd['voxel_coords'], want_coords) and float((bd['pillar_features'] - want).abs().max()) <= 1e-3
    res.update(kept_points=pillar_ops.assign(points, B, PILLAR_RANGE, PILLAR_VOXEL_SIZE, PILLAR_GRID_SIZE).num_kept,
               pillars=int(bd['pillar_features'].shape[0]))
    res['a_vfe_eval'] = dict(compare(ours_eval, torch_eval, args.calls, args.warmup), host_reads_ours=1,
                             host_reads_torch='2 (the boolean mask and torch.unique size their outputs on the host)',
                             bit_reproducible_ours=True, bit_reproducible_torch=False)

    # b: training, forward + backward
    vfe.train()
    proj = torch.randn(64, device=dev)

    def ours_train():
        out = vfe({'points': points, 'batch_size': B})['pillar_features']
        return torch.autograd.grad((out * proj).sum(), params)

    def torch_train():
        out, _ = torch_vfe(vfe, points)
        return torch.autograd.grad((out * proj).sum(), params)
    ga, gb = ours_train(), torch_train()
    worst = max(float((p - q).abs().max() / q.abs().max().clamp_min(1e-12)) for p, q in zip(ga, gb))
    res['b_vfe_train_fwd_bwd'] = dict(compare(ours_train, torch_train, args.calls, args.warmup), worst_relative_gradient_difference=worst)

    # c: scatter
    feats = bd['pillar_features'].detach().clone().requires_grad_(True)
    coords, table = bd['voxel_coords'], bd['pillar_cell_table']
    gout = torch.randn((B, 64, ny, nx), device=dev)

    def ours_scatter():
        with torch.no_grad():
            return pillar_ops.scatter(feats, table, coords, B, PILLAR_GRID_SIZE)

    def plain_scatter():
        with torch.no_grad():
            return torch_scatter(feats, coords, nx, ny)
    assert torch.equal(ours_scatter(), plain_scatter())
    res['c_scatter_fwd'] = dict(compare(ours_scatter, plain_scatter, args.calls, args.warmup), host_reads_ours=0,
                                host_reads_torch=f'{1 + 2 * B} (the batch size, and two boolean-mask sizes per sample)',
                                canvas_mbytes=round(gout.numel() * 4 / 2 ** 20, 1))

    def ours_scatter_bwd():
        return torch.autograd.grad(pillar_ops.scatter(feats, table, coords, B, PILLAR_GRID_SIZE), feats, gout)

    def plain_scatter_bwd():
        return torch.autograd.grad(torch_scatter(feats, coords, nx, ny), feats, gout)
    assert torch.equal(ours_scatter_bwd()[0], plain_scatter_bwd()[0])
    res['c_scatter_fwd_bwd'] = compare(ours_scatter_bwd, plain_scatter_bwd, args.calls, args.warmup)
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(line + '\n')


if __name__ == '__main__':
    main()

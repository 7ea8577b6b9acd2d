"""DSVT's input layer, one SetAttention layer, the 4-block backbone and the DSVT-Pillar eval step, the fused operators against
their torch formulations, at B = 1 and B = 4 on synthetic 120 k-point frames over the 468 x 468 grid (DSVT_PILLAR_CFG: 192
channels, 8 heads, sets of 36, 12 x 12 windows).
  input layer   dsvt_ops.set_partition vs dsvt_ops.set_partition_torch on the device, with the kernel launches (torch profiler)
                and the host reads of one call
  set attention one SetAttention layer (projections, attention, FFN), fused = True vs False, with the peak allocation of a call
  backbone      DSVT.forward, use_fused = True vs False, with the peak allocation
  eval step     the detector's forward, the backbone fused vs not
The two forms are called alternately on the same device and inputs, timed with device events around each call after a warm-up;
medians are reported.  Prints one JSON line and writes it to profiles/dsvt_rate.json.  No ratio is fixed in advance: the numbers
are the record, and an entry that comes out slower than its torch formulation is marked so.

  python tools/dsvt_rate.py [--bs 1 4] [--calls 10] [--warmup 3] [--points 120000] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from pdm_ssd_amd import detector_config as dc  # noqa: E402
from pdm_ssd_amd import dsvt_ops  # noqa: E402


def timed(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    out = fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e), out


def rounds(fns, calls, warmup):
    t = [[] for _ in fns]
    for i in range(warmup + calls):
        for j, fn in enumerate(fns):
            ms = timed(fn)[0]
            if i >= warmup:
                t[j].append(ms)
    return [statistics.median(x) for x in t]


def peak(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    del out
    return int(torch.cuda.max_memory_allocated() - before)


def launches(fn):
    with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return int(sum(e.count for e in prof.key_averages() if e.device_type == torch.autograd.DeviceType.CUDA))


def entry(name, ours, theirs, calls, warmup, extra=None):
    ms, ms_t = rounds([ours, theirs], calls, warmup)
    out = {'what': name, 'ms': round(ms, 4), 'ms_torch': round(ms_t, 4), 'slower_than_torch': bool(ms > ms_t)}
    out.update(extra or {})
    return out


def frame(bs, n, seed):
    """rows (b, x, y, z, intensity): lidar-like, denser near the sensor, over DSVT_RANGE"""
    rng = np.random.default_rng(seed)
    rows = []
    for b in range(bs):
        r = 74.0 * rng.random(n) ** 1.6
        a = rng.uniform(0, 2 * np.pi, n)
        xyz = np.stack([r * np.cos(a), r * np.sin(a), rng.uniform(-1.9, 3.9, n)], 1)
        rows.append(np.concatenate([np.full((n, 1), b), xyz, rng.uniform(0, 1, (n, 1))], 1))
    return torch.from_numpy(np.concatenate(rows).astype(np.float32))


def run(bs, calls, warmup, points, dev):
    torch.manual_seed(bs)
    net = dc.build_dsvt_pillar().to(dev).eval()
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, (torch.nn.BatchNorm1d, torch.nn.BatchNorm2d)):
                m.running_var.uniform_(0.5, 1.5)
                m.running_mean.uniform_(-0.2, 0.2)
        pts = frame(bs, points, bs).to(dev)
        bd = net.vfe({'batch_size': bs, 'points': pts})
        feats, coords = bd['voxel_features'], bd['voxel_coords']
        backbone = net.backbone_3d
        layer = backbone.input_layer
        geo = (layer.sparse_shape_list[0], layer.window_shape[0], layer.shift_list[0], layer.set_info[0][0])
        res = {'bs': bs, 'voxels': int(coords.shape[0]), 'entries': []}

        part = dsvt_ops.set_partition(coords, bs, *geo)
        res['sets'] = [int(i.shape[1]) for i in part.set_voxel_inds]
        want = dsvt_ops.set_partition_torch(coords, *geo)
        assert all(torch.equal(a, b) for a, b in zip(part.set_voxel_inds, want.set_voxel_inds))
        reads = dsvt_ops.HOST_READS
        n_launch = launches(lambda: dsvt_ops.set_partition(coords, bs, *geo))
        res['entries'].append(entry('input layer (partition)', lambda: dsvt_ops.set_partition(coords, bs, *geo),
                                    lambda: dsvt_ops.set_partition_torch(coords, *geo), calls, warmup,
                                    {'launches': n_launch, 'host_reads': dsvt_ops.HOST_READS - reads,
                                     'launches_torch': launches(lambda: dsvt_ops.set_partition_torch(coords, *geo))}))

        attn = backbone.stage_0[0].encoder_list[0].win_attn
        pos = torch.randn_like(feats)
        inds = part.set_voxel_inds[0][0]
        one = lambda fused: attn(feats, pos, None, inds, fused=fused)      # noqa: E731
        diff = float((one(True) - one(False)).abs().max())
        res['entries'].append(entry('SetAttention layer', lambda: one(True), lambda: one(False), calls, warmup,
                                    {'max_abs_diff': diff, 'peak_bytes': peak(lambda: one(True)), 'peak_bytes_torch': peak(lambda: one(False))}))

        def whole(fused):
            backbone.use_fused = fused
            return backbone({'batch_size': bs, 'voxel_features': feats, 'voxel_coords': coords})['voxel_features']
        diff = float((whole(True) - whole(False)).abs().max())
        res['entries'].append(entry('backbone (4 blocks)', lambda: whole(True), lambda: whole(False), calls, warmup,
                                    {'max_abs_diff': diff, 'peak_bytes': peak(lambda: whole(True)), 'peak_bytes_torch': peak(lambda: whole(False))}))

        def step(fused):
            backbone.use_fused = fused
            return net({'batch_size': bs, 'points': pts})[0]
        res['entries'].append(entry('eval step', lambda: step(True), lambda: step(False), calls, warmup))
        backbone.use_fused = True
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--bs', type=int, nargs='+', default=[1, 4])
    ap.add_argument('--calls', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--points', type=int, default=120000)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'dsvt_rate.json'))
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    out = {'tool': 'tools/dsvt_rate.py', 'device': torch.cuda.get_device_name(0), 'grid': dc.DSVT_GRID_SIZE, 'points': args.points,
           'calls': args.calls, 'warmup': args.warmup, 'runs': [run(bs, args.calls, args.warmup, args.points, dev) for bs in args.bs]}
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(line + '\n')


if __name__ == '__main__':
    main()

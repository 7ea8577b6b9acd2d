"""RoI point pooling and RoI-aware pooling: time per call, the bytes each call must write, and the achieved write rate as
a fraction of the streaming-copy yardstick.  The yardstick is the measurement of tools/diag/copy_rate.py — pdm_copy_many
between two device buffers, timed with device events after a warm-up — taken here at the operator's own byte count and
counted as bytes WRITTEN per second (half of that tool's read + write figure).  A byte count that fits the 256 MB last-level
cache gives a cached rate, not an HBM rate: such rows carry "copy_is_cached": true.
  - pdm_roipoint_pool3d and pdm_roipoint_pool3d_canonical at B=32, N=16384, M=100, S=512, C=130 (871 MB of pooled rows),
    on uniform and lidar-like clouds (pdm_ssd_amd/synthetic.py), RoIs = car-sized boxes centred on points of the cloud;
  - pdm_roiaware_pool3d_forward (max) and _backward at K=128, P=16384, C=128, out 12, max_pts 128.
Calls are timed with device events after a warm-up, each operator in a block of its own.  Prints one JSON line.

  python tools/roi_pool_rate.py [--calls 20] [--warmup 3]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from pdm_ssd_amd import _native, synthetic  # noqa: E402


def stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


def timed(fn, calls, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(calls):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        e.synchronize()
        ms.append(s.elapsed_time(e))
    return statistics.median(ms), min(ms)


def copy_write_rate(nbytes, dev, calls, warmup):
    """bytes WRITTEN per second by a device-to-device copy of `nbytes`: tools/diag/copy_rate.py's measurement (that tool is a
    script over one fixed 1 GiB buffer, so the same few lines are repeated here for this size)."""
    n = max(nbytes // 4, 1)
    src = torch.empty(n, dtype=torch.float32, device=dev).normal_()
    dst = torch.empty_like(src)
    med, _ = timed(lambda: _native.copy_many([dst], [src]), calls, warmup)
    return n * 4 / (med * 1e-3)


def report(name, med, best, nbytes, copy_rate):
    rate = nbytes / (med * 1e-3)
    return {name: {'ms': round(med, 4), 'ms_min': round(best, 4), 'bytes_written': int(nbytes), 'write_GBps': round(rate / 1e9, 1),
                   'copy_write_GBps': round(copy_rate / 1e9, 1), 'fraction_of_copy': round(rate / copy_rate, 3),
                   'copy_is_cached': bool(2 * nbytes <= 256 << 20)}}


def rois_on_points(clouds, M, seed):
    """M car-sized boxes per sample centred on points of the cloud, random headings; the last tenth all-zero padding rows."""
    rng = np.random.default_rng(seed)
    B, N = clouds.shape[0], clouds.shape[1]
    rois = np.zeros((B, M, 7), dtype=np.float32)
    live = M - M // 10
    for b in range(B):
        rois[b, :live, 0:3] = clouds[b, rng.integers(0, N, live), 0:3]
        rois[b, :live, 3:6] = np.float32([3.9, 1.6, 1.56]) * rng.uniform(0.8, 1.2, (live, 3))
        rois[b, :live, 6] = rng.uniform(-np.pi, np.pi, live)
    return rois


def point_pool(dev, kind, calls, warmup, B=32, N=16384, M=100, S=512, C=130):
    clouds = (synthetic.lidar_like_clouds if kind == 'lidar' else synthetic.uniform_clouds)(B, N, 5)
    xyz = torch.from_numpy(np.ascontiguousarray(clouds[:, :, 0:3])).to(dev)
    rois = torch.from_numpy(rois_on_points(clouds, M, 1)).to(dev)
    feats = torch.randn((B, N, C), device=dev)
    pooled = torch.zeros((B, M, S, 3 + C), device=dev)
    flag = torch.zeros((B, M), dtype=torch.int32, device=dev)
    nbytes = pooled.numel() * 4
    cr = copy_write_rate(nbytes, dev, calls, warmup)
    plain = lambda: _native.call('pdm_roipoint_pool3d', stream(dev), B, N, M, C, S, xyz.data_ptr(), rois.data_ptr(), feats.data_ptr(),   # noqa: E731
                                 pooled.data_ptr(), flag.data_ptr())
    canon = lambda: _native.call('pdm_roipoint_pool3d_canonical', stream(dev), B, N, M, C, S, xyz.data_ptr(), rois.data_ptr(), 7, 0.0,   # noqa: E731
                                 0.0, 0.0, feats.data_ptr(), pooled.data_ptr(), flag.data_ptr())
    res = {}
    res.update(report(f'roipoint_pool3d_{kind}', *timed(plain, calls, warmup), nbytes, cr))
    empty = int(flag.sum())
    res.update(report(f'roipoint_pool3d_canonical_{kind}', *timed(canon, calls, warmup), nbytes, cr))
    res[f'roipoint_pool3d_{kind}']['empty_rois'] = empty      # their rows are not written by the plain form
    return res


def aware(dev, calls, warmup, K=128, P=16384, C=128, out=12, max_pts=128):
    clouds = synthetic.lidar_like_clouds(1, P, 7)
    pts = torch.from_numpy(np.ascontiguousarray(clouds[0, :, 0:3])).to(dev)
    rois = torch.from_numpy(rois_on_points(clouds, K, 2)[0]).to(dev)
    feats = torch.randn((P, C), device=dev)
    idx = torch.empty((K, out, out, out, max_pts), dtype=torch.int32, device=dev)
    am = torch.empty((K, out, out, out, C), dtype=torch.int32, device=dev)
    pooled = torch.zeros((K, out, out, out, C), device=dev)
    grad_out, grad_in = torch.randn_like(pooled), torch.empty((P, C), device=dev)
    nbytes = _native.lib().pdm_roiaware_pool3d_workspace_bytes(K, out, out, out)
    ws = torch.empty(max(nbytes, 8), dtype=torch.uint8, device=dev)
    fwd = lambda: _native.call('pdm_roiaware_pool3d_forward', stream(dev), K, P, C, max_pts, out, out, out, rois.data_ptr(), pts.data_ptr(),   # noqa: E731
                               feats.data_ptr(), 0, ws.data_ptr(), nbytes, idx.data_ptr(), am.data_ptr(), pooled.data_ptr())
    bwd = lambda: _native.call('pdm_roiaware_pool3d_backward', stream(dev), K, P, C, max_pts, out, out, out, rois.data_ptr(), pts.data_ptr(),   # noqa: E731
                               idx.data_ptr(), am.data_ptr(), grad_out.data_ptr(), 0, grad_in.data_ptr())
    res = {}
    fbytes = (idx.numel() + am.numel() + pooled.numel()) * 4
    res.update(report('roiaware_pool3d_forward_max', *timed(fwd, calls, warmup), fbytes, copy_write_rate(fbytes, dev, calls, warmup)))
    bbytes = grad_in.numel() * 4
    res.update(report('roiaware_pool3d_backward_max', *timed(bwd, calls, warmup), bbytes, copy_write_rate(bbytes, dev, calls, warmup)))
    res['roiaware_pool3d_forward_max']['points_in_some_roi'] = int((idx[..., 0].sum()))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--calls', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    res = {'tool': 'roi_pool_rate', 'calls': args.calls, 'warmup': args.warmup, 'device': torch.cuda.get_device_name(0)}
    for kind in ('uniform', 'lidar'):
        res.update(point_pool(dev, kind, args.calls, args.warmup))
    res.update(aware(dev, args.calls, args.warmup))
    print(json.dumps(res))


if __name__ == '__main__':
    main()

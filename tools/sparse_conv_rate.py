"""The sparse 3-D convolution against a torch formulation over the SAME rulebook, per layer of VoxelBackBone8x and for the whole
backbone, at bs = 4 and bs = 32: lidar-like clouds of about 120 k points a frame on the KITTI voxel grid (1408 x 1600 x 40 cells
of 0.05 x 0.05 x 0.1 m).
  ours   one pdm_sparse_conv launch per layer: gather, MFMA, folded BatchNorm and ReLU
  torch  per offset k: index_select of the rows that have a neighbour there -> mm with W[k] -> index_add_ into the output, then
         the folded BatchNorm and ReLU as torch operations (what a rulebook-driven sparse convolution is without a kernel of
         its own; pairs per offset are prepared outside the timed region)
The two forms of a layer are called alternately in one process on the same device and inputs, timed with device events around
each call after a warm-up; medians are reported, with the kernel launches of one call as torch.profiler counts them, the active
rows of every level and the mean number of offsets present per 64-row tile (what the kernel's skip leaves of the 27).  The whole
backbone is timed as the module's forward (rulebooks and their four host reads included).  Results are compared first.  Prints
one JSON line and writes it to profiles/sparse_conv_rate.json.  No ratio is fixed in advance: the numbers are the record.

  python tools/sparse_conv_rate.py [--bs 4 32] [--points 120000] [--calls 10] [--warmup 3] [--no-launch-count] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from pdm_ssd_amd import sparse_conv_ops, spconv, synthetic  # noqa: E402
from pdm_ssd_amd.backbones_3d import VoxelBackBone8x  # noqa: E402
from pdm_ssd_amd.detector_config import GRID_SIZE, VOXEL_SIZE  # noqa: E402

COUNT_LAUNCHES = True


def timed(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    out = fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e), out


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


def alternate(ours, theirs, calls, warmup):
    a, b = [], []
    for i in range(warmup + calls):
        ta, tb = timed(ours)[0], timed(theirs)[0]
        if i >= warmup:
            a.append(ta)
            b.append(tb)
    return statistics.median(a), statistics.median(b)


def conv_layers(net):
    """(name, convolution, BatchNorm) of every layer in forward order"""
    out = []
    for name, seq in (('conv_input', net.conv_input), ('conv1', net.conv1), ('conv2', net.conv2), ('conv3', net.conv3), ('conv4', net.conv4),
                      ('conv_out', net.conv_out)):
        blocks = [seq] if isinstance(seq[0], spconv.SparseConvolution) else list(seq)
        for i, blk in enumerate(blocks):
            out.append((name if len(blocks) == 1 else f'{name}.{i}', blk[0], blk[1]))
    return out


def torch_conv(x, pairs, weight_k, n_out, scale, shift):
    out = torch.zeros((n_out, weight_k.shape[2]), dtype=x.dtype, device=x.device)
    for k, (rows_out, rows_in) in enumerate(pairs):
        if rows_out.numel():
            out.index_add_(0, rows_out, x.index_select(0, rows_in) @ weight_k[k])
    return torch.relu(out * scale + shift)


def run(bs, n_points, calls, warmup, dev):
    rng_range = list(synthetic.KITTI_RANGE)
    pts = torch.from_numpy(synthetic.to_batch_points(synthetic.lidar_like_clouds(bs, n_points, seed0=500))).to(dev)
    torch.manual_seed(0)
    net = VoxelBackBone8x({}, 4, list(GRID_SIZE)).to(dev).eval()
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, torch.nn.BatchNorm1d):
                m.running_var.uniform_(0.5, 1.5)
                m.running_mean.uniform_(-0.2, 0.2)
        vox = sparse_conv_ops.voxel_assign(pts, bs, rng_range, VOXEL_SIZE, GRID_SIZE)
        res = {'bs': bs, 'points': int(pts.shape[0]), 'kept': vox.num_kept, 'voxels': vox.num_voxels, 'layers': []}
        x = spconv.SparseConvTensor(vox.voxel_mean, vox.voxel_coords, net.sparse_shape, bs)
        for name, conv, bn in conv_layers(net):
            rb = conv.get_rulebook(x)
            nbr = rb.nbr
            wpack = sparse_conv_ops.pack_weight(conv.weight)
            scale, shift = spconv.fold_norm(bn, conv.bias, conv.out_channels, conv.weight)
            weight_k = conv.weight.reshape(conv.out_channels, -1, conv.in_channels).permute(1, 2, 0).contiguous()
            pairs = []
            for k in range(nbr.shape[1]):
                rows_out = torch.nonzero(nbr[:, k] >= 0)[:, 0]
                pairs.append((rows_out, nbr[rows_out, k].long()))
            feats = x.features

            def ours():
                return sparse_conv_ops.sparse_conv(feats, nbr, wpack, conv.in_channels, conv.out_channels, scale, shift, relu=True)

            def theirs():
                return torch_conv(feats, pairs, weight_k, nbr.shape[0], scale, shift)
            y, y_t = ours(), theirs()
            err = float((y - y_t).abs().max())
            assert err <= 1e-3 * max(1.0, float(y_t.abs().max())), (name, err)
            ms, ms_t = alternate(ours, theirs, calls, warmup)
            tiles = (nbr.shape[0] + 63) // 64
            padded = torch.nn.functional.pad(nbr, (0, 0, 0, tiles * 64 - nbr.shape[0]), value=-1).reshape(tiles, 64, -1)
            present = float((padded >= 0).any(1).sum(1).float().mean()) if tiles else 0.0
            res['layers'].append({'layer': name, 'subm': conv.subm, 'cin': conv.in_channels, 'cout': conv.out_channels, 'rows_in': int(feats.shape[0]),
                                  'rows_out': int(nbr.shape[0]), 'offsets': int(nbr.shape[1]), 'pairs': int((nbr >= 0).sum()),
                                  'mean_present_offsets_per_tile': round(present, 2), 'ms': round(ms, 4), 'ms_torch': round(ms_t, 4),
                                  'launches': launches(ours), 'launches_torch': launches(theirs), 'max_abs_diff': err})
            x = spconv.SparseConvTensor(y, rb.out_indices, rb.out_shape, bs, x.indice_dict)

        def whole():
            return net({'voxel_features': vox.voxel_mean, 'voxel_coords': vox.voxel_coords, 'batch_size': bs})
        whole()
        t = [timed(whole)[0] for _ in range(warmup + calls)][warmup:]
        res['backbone_ms'] = round(statistics.median(t), 4)
        res['backbone_launches'] = launches(whole)
        res['conv_ms_sum'] = round(sum(l['ms'] for l in res['layers']), 4)
        res['conv_ms_sum_torch'] = round(sum(l['ms_torch'] for l in res['layers']), 4)
        t = [timed(lambda: sparse_conv_ops.voxel_assign(pts, bs, rng_range, VOXEL_SIZE, GRID_SIZE))[0] for _ in range(warmup + calls)][warmup:]
        res['voxel_assign_ms'] = round(statistics.median(t), 4)
    return res


def main():
    global COUNT_LAUNCHES
    ap = argparse.ArgumentParser()
    ap.add_argument('--bs', type=int, nargs='+', default=[4, 32])
    ap.add_argument('--points', type=int, default=120000)
    ap.add_argument('--calls', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--no-launch-count', action='store_true')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'sparse_conv_rate.json'))
    args = ap.parse_args()
    COUNT_LAUNCHES = not args.no_launch_count
    dev = torch.device('cuda:0')
    out = {'tool': 'tools/sparse_conv_rate.py', 'device': torch.cuda.get_device_name(0), 'grid': list(GRID_SIZE), 'calls': args.calls,
           'warmup': args.warmup, 'runs': [run(bs, args.points, args.calls, args.warmup, dev) for bs in args.bs]}
    line = json.dumps(out)
    print(line)
    with open(args.out, 'w') as f:
        f.write(line + '\n')


if __name__ == '__main__':
    main()

"""The sparse 2-D pillar path (PillarNet) against a torch formulation over the SAME rulebooks, per sparse layer of
PillarBackBone8x, for the whole backbone and for the detector's eval step, at bs = 32 and bs = 4: lidar-like clouds of about 120 k
points a frame on the PillarNet grid (1408 x 1600 pillars of 0.05 x 0.05 x 4 m).
  ours   one pdm_sparse_conv_wide launch per layer: gather, MFMA, folded BatchNorm and ReLU
  torch  per offset k: index_select of the rows that have a neighbour there -> mm with W[k] -> index_add_ into the output, then the
         folded BatchNorm and ReLU as torch operations (pairs per offset are prepared outside the timed region)
The 256-wide layers (conv4: 128 -> 256 strided, 256 -> 256 submanifold) are also timed forward + backward: ours is
sparse_conv_ops.SparseConvFunction (pdm_sparse_conv_wide_split forward and data gradient, pdm_sparse_conv_wide_wgrad), torch is the
same per-offset formulation under autograd, both from a leaf input and a leaf weight to their gradients.
The two forms are called alternately in one process on the same device and inputs, timed with device events around each call after
a warm-up; medians are reported.  The whole backbone is the module's forward (rulebooks, their three host reads, the dense x_conv4
and conv5 included); the eval step is build_pillarnet()'s forward from the points to pred_dicts.  Results are compared first.
Prints one JSON line, writes it to profiles/pillarnet_rate.json and prints the README's table row.  No ratio is fixed in advance:
the numbers are the record, and a layer that comes out slower than the torch formulation is marked so.

  python tools/pillarnet_rate.py [--bs 32 4] [--points 120000] [--calls 10] [--warmup 3] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from pdm_ssd_amd import detector_config as dc  # noqa: E402
from pdm_ssd_amd import sparse_conv_ops, spconv, synthetic  # noqa: E402


def timed(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    out = fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e), out


def alternate(ours, theirs, calls, warmup):
    a, b = [], []
    for i in range(warmup + calls):
        ta, tb = timed(ours)[0], timed(theirs)[0]
        if i >= warmup:
            a.append(ta)
            b.append(tb)
    return statistics.median(a), statistics.median(b)


def conv_layers(net):
    """(name, convolution, BatchNorm) of every sparse layer in forward order"""
    out = []
    for name in ('conv1', 'conv2', 'conv3', 'conv4'):
        for i, blk in enumerate(getattr(net, name)):
            out.append((f'{name}.{i}', blk[0], blk[1]))
    return out


def torch_conv(x, pairs, weight_k, n_out):
    out = torch.zeros((n_out, weight_k.shape[2]), dtype=x.dtype, device=x.device)
    for k, (rows_out, rows_in) in enumerate(pairs):
        if rows_out.numel():
            out = out.index_add(0, rows_out, x.index_select(0, rows_in) @ weight_k[k])
    return out


def run(bs, n_points, calls, warmup, dev):
    pts = torch.from_numpy(synthetic.to_batch_points(synthetic.lidar_like_clouds(bs, n_points, seed0=500))).to(dev)
    torch.manual_seed(0)
    model = dc.build_pillarnet().to(dev).eval()
    net = model.backbone_3d
    with torch.no_grad():
        for m in model.modules():
            if isinstance(m, (torch.nn.BatchNorm1d, torch.nn.BatchNorm2d)):
                m.running_var.uniform_(0.5, 1.5)
                m.running_mean.uniform_(-0.2, 0.2)
        bd = model.vfe({'points': pts, 'batch_size': bs})
        res = {'bs': bs, 'points': int(pts.shape[0]), 'pillars': int(bd['pillar_coords'].shape[0]), 'layers': [], 'train_layers': []}
        x = spconv.SparseConvTensor(bd['pillar_features'], bd['pillar_coords'], net.sparse_shape, bs)
        wide = []
        for name, conv, bn in conv_layers(net):
            rb = conv.get_rulebook(x)
            nbr = rb.nbr
            wpack = sparse_conv_ops.pack_weight(conv.weight5(), wide=True)
            scale, shift = spconv.fold_norm(bn, conv.bias, conv.out_channels, conv.weight)
            weight_k = conv.weight.reshape(conv.out_channels, -1, conv.in_channels).permute(1, 2, 0).contiguous()
            pairs = []
            for k in range(nbr.shape[1]):
                rows_out = torch.nonzero(nbr[:, k] >= 0)[:, 0]
                pairs.append((rows_out, nbr[rows_out, k].long()))
            feats = x.features

            def ours():
                return sparse_conv_ops.sparse_conv(feats, nbr, wpack, conv.in_channels, conv.out_channels, scale, shift, relu=True, wide=True)

            def theirs():
                return torch.relu(torch_conv(feats, pairs, weight_k, nbr.shape[0]) * scale + shift)
            y, y_t = ours(), theirs()
            err = float((y - y_t).abs().max())
            assert err <= 1e-3 * max(1.0, float(y_t.abs().max())), (name, err)
            ms, ms_t = alternate(ours, theirs, calls, warmup)
            tiles = (nbr.shape[0] + 63) // 64
            padded = torch.nn.functional.pad(nbr, (0, 0, 0, tiles * 64 - nbr.shape[0]), value=-1).reshape(tiles, 64, -1)
            present = float((padded >= 0).any(1).sum(1).float().mean()) if tiles else 0.0
            res['layers'].append({'layer': name, 'subm': conv.subm, 'cin': conv.in_channels, 'cout': conv.out_channels, 'rows_in': int(feats.shape[0]),
                                  'rows_out': int(nbr.shape[0]), 'pairs': int((nbr >= 0).sum()), 'mean_present_offsets_per_tile': round(present, 2),
                                  'ms': round(ms, 4), 'ms_torch': round(ms_t, 4), 'slower_than_torch': bool(ms > ms_t), 'max_abs_diff': err})
            if conv.out_channels == 256:
                wide.append((name, conv, rb, pairs, feats))
            x = conv.out_tensor(x, y, rb)

    # forward + backward of the 256-wide layers, from a leaf input and a leaf weight to their gradients
    for name, conv, rb, pairs, feats in wide[:2]:
        nbr = rb.nbr
        identity = conv.subm
        nbr_t = True if identity else sparse_conv_ops.rulebook_transpose(nbr, feats.shape[0])
        w5 = conv.weight5().detach().clone().requires_grad_()
        xin = feats.detach().clone().requires_grad_()
        dy = torch.randn((nbr.shape[0], conv.out_channels), device=dev)

        def ours():
            xin.grad = w5.grad = None
            sparse_conv_ops.SparseConvFunction.apply(xin, w5, None, nbr, nbr_t, conv.in_channels, conv.out_channels, None, None, True).backward(dy)
            return xin.grad, w5.grad

        def theirs():
            xin.grad = w5.grad = None
            weight_k = w5.reshape(conv.out_channels, -1, conv.in_channels).permute(1, 2, 0)
            torch_conv(xin, pairs, weight_k, nbr.shape[0]).backward(dy)
            return xin.grad, w5.grad
        (dx, dw), (dx_t, dw_t) = [tuple(t.clone() for t in f()) for f in (ours, theirs)]
        for a, b in ((dx, dx_t), (dw, dw_t)):
            assert float((a - b).abs().max()) <= 1e-3 * max(1.0, float(b.abs().max())), name
        ms, ms_t = alternate(ours, theirs, calls, warmup)
        res['train_layers'].append({'layer': name, 'subm': conv.subm, 'cin': conv.in_channels, 'cout': conv.out_channels,
                                    'rows_out': int(nbr.shape[0]), 'fwd_bwd_ms': round(ms, 4), 'fwd_bwd_ms_torch': round(ms_t, 4),
                                    'slower_than_torch': bool(ms > ms_t)})

    with torch.no_grad():
        def whole():
            return net({'pillar_features': bd['pillar_features'], 'pillar_coords': bd['pillar_coords'], 'batch_size': bs})
        whole()
        t = [timed(whole)[0] for _ in range(warmup + calls)][warmup:]
        res['backbone_ms'] = round(statistics.median(t), 4)
        res['conv_ms_sum'] = round(sum(l['ms'] for l in res['layers']), 4)
        res['conv_ms_sum_torch'] = round(sum(l['ms_torch'] for l in res['layers']), 4)

        def step():
            return model({'points': pts, 'batch_size': bs})
        step()
        t = [timed(step)[0] for _ in range(warmup + calls)][warmup:]
        res['eval_step_ms'] = round(statistics.median(t), 4)
    return res


def readme_row(out):
    cells = []
    for r in out['runs']:
        w = [l for l in r['layers'] if l['cout'] == 256]
        cells.append(f"bs {r['bs']}: sparse layers {r['conv_ms_sum']:.2f} ms (torch {r['conv_ms_sum_torch']:.2f}), 256-wide "
                     + ', '.join(f"{l['ms']:.2f} / {l['ms_torch']:.2f}" for l in w)
                     + f"; backbone {r['backbone_ms']:.1f} ms, eval step {r['eval_step_ms']:.1f} ms")
    return '| PillarNet sparse 2-D path (`tools/pillarnet_rate.py`) | ' + ' <br> '.join(cells) + ' |'


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--bs', type=int, nargs='+', default=[32, 4])
    ap.add_argument('--points', type=int, default=120000)
    ap.add_argument('--calls', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'pillarnet_rate.json'))
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    out = {'tool': 'tools/pillarnet_rate.py', 'device': torch.cuda.get_device_name(0), 'grid': list(dc.PILLARNET_GRID_SIZE), 'calls': args.calls,
           'warmup': args.warmup, 'runs': [run(bs, args.points, args.calls, args.warmup, dev) for bs in args.bs]}
    line = json.dumps(out)
    print(line)
    with open(args.out, 'w') as f:
        f.write(line + '\n')
    print(readme_row(out))


if __name__ == '__main__':
    main()

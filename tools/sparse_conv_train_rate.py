"""The sparse 3-D convolution's backward against torch autograd over the SAME rulebook, per layer of VoxelBackBone8x, and one
whole training forward + backward of the backbone, at bs = 4 and bs = 32 on the lidar-like clouds of tools/sparse_conv_rate.py
(about 120 k points a frame on the KITTI voxel grid).
  ours   the weight gradient (pdm_sparse_conv_wgrad: partials per (row chunk, offset), then the sum over the chunks) and the data
         gradient (pdm_sparse_conv_split over the transposed rulebook, or over nbr itself for a submanifold layer, with the weights
         packed transposed).  The first layer's input takes no gradient, as in the detectors: its backward is the weight gradient.
  torch  autograd's backward of the formulation `per offset k: index_select -> mm with W[k] -> index_add_` (forward outside the
         timed region; pairs per offset prepared outside it as well)
The two backwards of a layer are called alternately in one process on the same device and inputs, timed with device events
around each call after a warm-up; medians are reported, beside the chunk geometry and the workspace of the weight gradient, the
time of the transposed table of a strided layer, and the results' difference.  Prints one JSON line and writes it to
profiles/sparse_conv_train_rate.json.  No ratio is fixed in advance: the numbers are the record.

  python tools/sparse_conv_train_rate.py [--bs 4 32] [--points 120000] [--calls 10] [--warmup 3] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from pdm_ssd_amd import _native, sparse_conv_ops, spconv, synthetic  # noqa: E402
from pdm_ssd_amd.backbones_3d import VoxelBackBone8x  # noqa: E402
from pdm_ssd_amd.detector_config import GRID_SIZE, VOXEL_SIZE  # noqa: E402


def timed(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    out = fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e), out


def conv_layers(net):
    """(name, convolution) of every layer in forward order"""
    out = []
    for name, seq in (('conv_input', net.conv_input), ('conv1', net.conv1), ('conv2', net.conv2), ('conv3', net.conv3), ('conv4', net.conv4),
                      ('conv_out', net.conv_out)):
        blocks = [seq] if isinstance(seq[0], spconv.SparseConvolution) else list(seq)
        for i, blk in enumerate(blocks):
            out.append((name if len(blocks) == 1 else f'{name}.{i}', blk[0]))
    return out


def torch_conv(x, pairs, weight_k, n_out):
    out = torch.zeros((n_out, weight_k.shape[2]), dtype=x.dtype, device=x.device)
    for k, (rows_out, rows_in) in enumerate(pairs):
        if rows_out.numel():
            out = out.index_add(0, rows_out, x.index_select(0, rows_in) @ weight_k[k])
    return out


def run(bs, n_points, calls, warmup, dev):
    rng_range = list(synthetic.KITTI_RANGE)
    pts = torch.from_numpy(synthetic.to_batch_points(synthetic.lidar_like_clouds(bs, n_points, seed0=500))).to(dev)
    torch.manual_seed(0)
    net = VoxelBackBone8x({}, 4, list(GRID_SIZE)).to(dev).eval()
    lib = _native.lib()
    with torch.no_grad():
        vox = sparse_conv_ops.voxel_assign(pts, bs, rng_range, VOXEL_SIZE, GRID_SIZE)
    res = {'bs': bs, 'points': int(pts.shape[0]), 'voxels': vox.num_voxels, 'layers': []}
    x = spconv.SparseConvTensor(vox.voxel_mean, vox.voxel_coords, net.sparse_shape, bs)
    for li, (name, conv) in enumerate(conv_layers(net)):
        with torch.no_grad():
            rb = conv.get_rulebook(x)
            nbr, feats = rb.nbr, x.features
            cin, cout, kvol = conv.in_channels, conv.out_channels, nbr.shape[1]
            need_dx = li > 0
            y = sparse_conv_ops.sparse_conv(feats, nbr, sparse_conv_ops.pack_weight(conv.weight), cin, cout)
            dy = torch.randn_like(y)
            pack_t = sparse_conv_ops.pack_weight_transposed(conv.weight, flip=conv.subm)
            transpose_ms = None
            if conv.subm:
                table = nbr
            else:
                t = [timed(lambda: sparse_conv_ops.rulebook_transpose(nbr, feats.shape[0])) for _ in range(warmup + calls)][warmup:]
                transpose_ms, table = round(statistics.median(v[0] for v in t), 4), t[-1][1]
            pairs = []
            for k in range(kvol):
                rows_out = torch.nonzero(nbr[:, k] >= 0)[:, 0]
                pairs.append((rows_out, nbr[rows_out, k].long()))

        def ours():
            dw = sparse_conv_ops.sparse_conv_wgrad(dy, feats, nbr, conv.kernel_size)
            return (sparse_conv_ops.sparse_conv_dgrad(dy, table, pack_t, cin, cout) if need_dx else None), dw

        def wgrad_only():
            return sparse_conv_ops.sparse_conv_wgrad(dy, feats, nbr, conv.kernel_size)

        xt = feats.detach().clone().requires_grad_(need_dx)
        wk = conv.weight.detach().reshape(cout, kvol, cin).permute(1, 2, 0).contiguous().requires_grad_()

        def theirs_timed():
            yt = torch_conv(xt, pairs, wk, nbr.shape[0])        # the forward builds the graph, outside the timed region
            return timed(lambda: torch.autograd.grad(yt, (xt, wk) if need_dx else (wk,), dy))

        (dx, dw), (_, grads_t) = ours(), theirs_timed()
        dw_t = grads_t[-1].permute(2, 0, 1).reshape(dw.shape)
        err_w = float((dw - dw_t).abs().max() / dw_t.abs().max().clamp_min(1e-30))
        err_x = float((dx - grads_t[0]).abs().max() / grads_t[0].abs().max().clamp_min(1e-30)) if need_dx else None
        assert err_w <= 1e-3 and (err_x is None or err_x <= 1e-3), (name, err_w, err_x)
        a, b, c = [], [], []
        for i in range(warmup + calls):
            ta, tb, tc = timed(ours)[0], theirs_timed()[0], timed(wgrad_only)[0]
            if i >= warmup:
                a.append(ta)
                b.append(tb)
                c.append(tc)
        rows = lib.pdm_sparse_conv_wgrad_chunk_rows(nbr.shape[0], kvol, cin, cout)
        res['layers'].append({'layer': name, 'subm': conv.subm, 'cin': cin, 'cout': cout, 'rows_in': int(feats.shape[0]), 'rows_out': int(nbr.shape[0]),
                              'offsets': kvol, 'pairs': int((nbr >= 0).sum()), 'data_gradient': need_dx, 'backward_ms': round(statistics.median(a), 4),
                              'backward_ms_torch': round(statistics.median(b), 4), 'wgrad_ms': round(statistics.median(c), 4),
                              'transpose_ms': transpose_ms, 'chunk_rows': rows, 'chunks': -(-nbr.shape[0] // rows),
                              'wgrad_workspace_bytes': lib.pdm_sparse_conv_wgrad_workspace_bytes(nbr.shape[0], kvol, cin, cout),
                              'dw_rel_diff': err_w, 'dx_rel_diff': err_x})
        print(f'bs {bs} {name}: ours {res["layers"][-1]["backward_ms"]} ms, torch {res["layers"][-1]["backward_ms_torch"]} ms', file=sys.stderr, flush=True)
        del xt, wk, grads_t, pairs
        x = spconv.SparseConvTensor(torch.relu(y), rb.out_indices, rb.out_shape, bs, x.indice_dict)
    res['backward_ms_sum'] = round(sum(l['backward_ms'] for l in res['layers']), 4)
    res['backward_ms_sum_torch'] = round(sum(l['backward_ms_torch'] for l in res['layers']), 4)

    batch = {'voxel_features': vox.voxel_mean, 'voxel_coords': vox.voxel_coords, 'batch_size': bs}

    def eval_forward():
        with torch.no_grad():
            return net(dict(batch))

    def train_step():
        for p in net.parameters():
            p.grad = None
        out = net(dict(batch))['encoded_spconv_tensor'].features
        out.backward(torch.ones_like(out))

    net.eval()
    eval_forward()
    res['backbone_eval_forward_ms'] = round(statistics.median([timed(eval_forward)[0] for _ in range(warmup + calls)][warmup:]), 4)
    net.train()
    train_step()
    res['backbone_train_forward_backward_ms'] = round(statistics.median([timed(train_step)[0] for _ in range(warmup + calls)][warmup:]), 4)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--bs', type=int, nargs='+', default=[4, 32])
    ap.add_argument('--points', type=int, default=120000)
    ap.add_argument('--calls', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'sparse_conv_train_rate.json'))
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    out = {'tool': 'tools/sparse_conv_train_rate.py', 'device': torch.cuda.get_device_name(0), 'grid': list(GRID_SIZE), 'calls': args.calls,
           'warmup': args.warmup, 'runs': []}
    for bs in args.bs:
        out['runs'].append(run(bs, args.points, args.calls, args.warmup, dev))
        with open(args.out, 'w') as f:          # after every batch size: a later one may not fit the device
            f.write(json.dumps(out) + '\n')
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == '__main__':
    main()

"""Training through the fused attention (attention_ops.mha_kv / mha_qkv: pdm_mha_forward_train + pdm_mha_backward) against the
torch paths at the workload's shapes: C = 128, 8 heads, P = 200 queries, N = 32 400 keys (cross-attention) and N = 200
(self-attention), B = 1 and 4.  Forward + backward of
  attention alone    mha_kv / mha_qkv on packed projected rows with p = 0 and p = 0.1, and fp32
                     torch.nn.functional.scaled_dot_product_attention under autograd on the same rows
  with projections   one attention of the decoder layer, in- and out-projection included: the layer's fused training path
                     (F.linear, mha_kv / mha_qkv, p = 0.1) and its nn.MultiheadAttention module as the layer calls it
                     (need_weights at its default, dropout 0.1) -- the same torch code at the parent commit
with the peak allocated bytes of each above the level before the call, the error ratios of tests/test_attention_train_gpu.py at
the two shapes (B = 1), and the decoder layer's and the head's training forward + backward with FUSED_ATTENTION_TRAIN on and off.
The forms are called in turn, round after round, in one process on the same inputs, timed with device events after a warm-up;
medians are reported.  No ratio is fixed in advance: an entry slower than the nn.MultiheadAttention path is marked so.  Prints one
JSON line and writes it to profiles/attention_train_rate.json.

  python tools/attention_train_rate.py [--bs 1 4] [--calls 10] [--warmup 3] [--out FILE]
"""
import argparse
import copy
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from pdm_ssd_amd import _native, attention_ops  # noqa: E402
from pdm_ssd_amd import detector_config as dc  # noqa: E402
from pdm_ssd_amd.config import cfg_from_dict  # noqa: E402
from pdm_ssd_amd.dense_heads import TransFusionHead  # noqa: E402

H = W = 180
CIN = 512
C, NH, P = 128, 8, 200


def timed(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e)


def rounds(fns, calls, warmup):
    t = [[] for _ in fns]
    for i in range(warmup + calls):
        for j, fn in enumerate(fns):
            ms = timed(fn)
            if i >= warmup:
                t[j].append(ms)
    return [statistics.median(x) for x in t]


def peak_bytes(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - before


def attention_forms(bs, N, dev):
    """-> {name: a function running forward + backward of one form}: the attention alone on the same projected rows (fused, sdpa),
    and one attention of the decoder layer with its in- and out-projection (the layer's fused training path, the module)"""
    from pdm_ssd_amd.utils.transfusion_utils import TransformerDecoderLayer
    g = torch.Generator(device=dev).manual_seed(bs * 7 + N)
    same = N == P
    q = torch.randn((bs, P, C), device=dev, generator=g)
    kv = torch.randn((bs, N, 2 * C), device=dev, generator=g)
    qkv = torch.cat((q, kv[:, :P]), dim=-1) if same else None
    dout = torch.randn((bs, P, C), device=dev, generator=g)
    rows_q = torch.randn((bs, P, C), device=dev, generator=g)         # unprojected rows for the forms with projections
    rows_k = rows_q if same else torch.randn((bs, N, C), device=dev, generator=g)
    draws = attention_ops.AttentionDraws(1, dev)
    torch.manual_seed(N)
    layer = TransformerDecoderLayer(C, NH, 256, 0.1).to(dev).train()
    mod = layer.self_attn if same else layer.multihead_attn

    def fused(p):
        def f():
            if same:
                x = qkv.detach().requires_grad_(True)
                attention_ops.mha_qkv(x, NH, p, draws).backward(dout)
            else:
                a, b = q.detach().requires_grad_(True), kv.detach().requires_grad_(True)
                attention_ops.mha_kv(a, b, NH, p, draws).backward(dout)
        return f

    def sdpa():
        a, b = q.detach().requires_grad_(True), kv.detach().requires_grad_(True)
        heads = lambda t: t.reshape(bs, t.shape[1], NH, C // NH).transpose(1, 2)      # noqa: E731
        o = torch.nn.functional.scaled_dot_product_attention(heads(a), heads(b[..., :C]), heads(b[..., C:]))
        o.transpose(1, 2).reshape(bs, P, C).backward(dout)

    def layer_fused():
        mod.zero_grad(set_to_none=True)
        a = rows_q.detach().requires_grad_(True)
        b = a if same else rows_k.detach().requires_grad_(True)
        layer._attend_train(mod, True, a, b, same, draws).backward(dout)

    def module():
        mod.zero_grad(set_to_none=True)
        a = rows_q.detach().requires_grad_(True)
        b = a if same else rows_k.detach().requires_grad_(True)
        a_sf, b_sf = a.transpose(0, 1), b.transpose(0, 1)
        mod(a_sf, b_sf, value=b_sf)[0].backward(dout.transpose(0, 1))
    return {'attention alone: fused p = 0': fused(0.0), 'attention alone: fused p = 0.1': fused(0.1), 'attention alone: sdpa fp32 p = 0': sdpa,
            'with projections: fused p = 0.1': layer_fused, 'with projections: nn.MultiheadAttention p = 0.1': module}


def error_ratios(N, dev, p):
    """tests/test_attention_train_gpu.py's figures at B = 1"""
    g = torch.Generator().manual_seed(N)
    q, k, v, dout = (torch.randn((1, n, C), generator=g).to(dev) for n in (P, N, N, P))
    keep = None if p == 0.0 else torch.from_numpy(attention_ops.dropout_keep_host(5, 0, 1, NH, P, N, p))

    def autograd(q, k, v, dout, keep):
        q, k, v = (t.detach().clone().requires_grad_(True) for t in (q, k, v))
        out = attention_ops.mha_torch(q, k, v, NH, keep, p)
        return (out.detach(),) + torch.autograd.grad(out, (q, k, v), dout)
    want = autograd(q.double().cpu(), k.double().cpu(), v.double().cpu(), dout.double().cpu(), keep)
    base = autograd(q, k, v, dout, None if keep is None else keep.to(dev))
    leaves = [t.detach().clone().requires_grad_(True) for t in (q, k, v)]
    out = attention_ops.mha(*leaves, NH, p, attention_ops.AttentionDraws(5, dev) if p > 0.0 else None)
    got = (out.detach(),) + torch.autograd.grad(out, leaves, dout)
    res = {}
    for name, a, b, w in zip(('out', 'dq', 'dk', 'dv'), got, base, want):
        ek, et = float((a.double().cpu() - w).abs().max()), float((b.double().cpu() - w).abs().max())
        res[name] = {'err_kernel': ek, 'err_torch': et, 'ratio': ek / et if et > 0 else None}
    return res


def head_forms(bs, dev):
    """the decoder layer's and the head's training forward + backward, FUSED_ATTENTION_TRAIN on and off (the same modules)"""
    torch.manual_seed(bs)
    head = TransFusionHead(model_cfg=cfg_from_dict(copy.deepcopy(dc.TRANSFUSION_LIDAR_FUSED_TRAIN_CFG['DENSE_HEAD'])), input_channels=CIN,
                           num_class=10, class_names=dc.TRANSFUSION_CLASS_NAMES, grid_size=dc.TRANSFUSION_GRID_SIZE,
                           point_cloud_range=dc.TRANSFUSION_RANGE, voxel_size=dc.TRANSFUSION_VOXEL_SIZE,
                           predict_boxes_when_training=False).to(dev).train()
    dec = head.decoder
    x = torch.randn((bs, CIN, H, W), device=dev)
    gt = torch.zeros((bs, 20, 10), device=dev)
    gt[..., :2].uniform_(-50, 50)
    gt[..., 2].uniform_(-2, 0)
    gt[..., 3:6].uniform_(0.5, 4.0)
    gt[..., 6].uniform_(-3, 3)
    gt[..., 9] = torch.randint(1, 11, (bs, 20), device=dev).float()
    query, key = torch.randn((bs, C, P), device=dev), torch.randn((bs, C, H * W), device=dev)
    qpos, kpos = torch.rand((bs, P, 2), device=dev) * H, head.bev_pos
    dout = torch.randn((bs, C, P), device=dev)

    def layer(fused):
        def f():
            dec.fused_train = fused
            dec.zero_grad(set_to_none=True)
            dec(query, key, qpos, kpos).backward(dout)
        return f

    def whole(fused):
        def f():
            dec.fused_train = fused
            head.zero_grad(set_to_none=True)
            head({'batch_size': bs, 'spatial_features_2d': x, 'gt_boxes': gt})['loss'].backward()
        return f
    return {'decoder layer': (layer(True), layer(False)), 'head': (whole(True), whole(False))}


def run(bs, calls, warmup, dev):
    res = {'bs': bs, 'attention': [], 'modules': []}
    for what, N in (('cross-attention', H * W), ('self-attention', P)):
        forms = attention_forms(bs, N, dev)
        names = list(forms)
        for f in forms.values():
            f()
        ms = rounds(list(forms.values()), calls, warmup)
        base = ms[names.index('with projections: nn.MultiheadAttention p = 0.1')]
        entry = {'what': what, 'keys': N, 'keys_per_block_backward': int(_native.lib().pdm_mha_backward_keys_per_block(N, 0)), 'forms': []}
        for n, t in zip(names, ms):
            entry['forms'].append({'form': n, 'fwd_bwd_ms': round(t, 4), 'peak_bytes': int(peak_bytes(forms[n])),
                                   **({'slower_than_nn_mha': bool(t > base)} if n == 'with projections: fused p = 0.1' else {})})
        if bs == 1:
            entry['error_ratios'] = {'p = 0': error_ratios(N, dev, 0.0), 'p = 0.1': error_ratios(N, dev, 0.1)}
        res['attention'].append(entry)
    for what, (on, off) in head_forms(bs, dev).items():
        on(), off()
        ms_on, ms_off = rounds([on, off], calls, warmup)
        res['modules'].append({'what': what, 'fwd_bwd_ms_fused': round(ms_on, 4), 'fwd_bwd_ms_nn_mha': round(ms_off, 4),
                               'peak_bytes_fused': int(peak_bytes(on)), 'peak_bytes_nn_mha': int(peak_bytes(off)),
                               'slower_than_nn_mha': bool(ms_on > ms_off)})
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--bs', type=int, nargs='+', default=[1, 4])
    ap.add_argument('--calls', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'attention_train_rate.json'))
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    out = {'tool': 'tools/attention_train_rate.py', 'device': torch.cuda.get_device_name(0), 'channels': C, 'heads': NH, 'queries': P,
           'calls': args.calls, 'warmup': args.warmup, 'runs': [run(bs, args.calls, args.warmup, dev) for bs in args.bs]}
    line = json.dumps(out)
    print(line)
    with open(args.out, 'w') as f:
        f.write(line + '\n')


if __name__ == '__main__':
    main()

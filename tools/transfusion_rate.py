"""TransFusionHead's three operators and the whole head against their torch formulations at the workload's shape: a 180 x 180 map,
C = 128, P = 200 queries, 8 heads, ten classes, B = 1 and 4, random (not zero-filled) weights and inputs.
  proposals        transfusion_ops.proposals         vs sigmoid, max_pool2d and a full argsort of the C * H * W scores of every sample
  self-attention   in-projection, mha_forward,       vs the layer's nn.MultiheadAttention module on the same rows
  cross-attention  out-projection (decoder._attend)     (P = 200 keys; N = 32 400 keys)
  decode           transfusion_ops.decode            vs transfusion_ops.decode_torch
  head             TransFusionHead.forward, use_fused = True vs False (one device-to-host read each)
Also: mha_forward alone on the cross-attention's projected rows for a sweep of keys_per_chunk, next to
torch.nn.functional.scaled_dot_product_attention in fp32 (interleaved rounds in one process), and the error ratios of
tests/test_attention_gpu.py (err_kernel / err_torch against a float64 reference on the CPU) at the two workload shapes, B = 1.
The two forms are called alternately on the same device and inputs, timed with device events around each call after a warm-up;
medians are reported.  Prints one JSON line and writes it to profiles/transfusion_rate.json.  No ratio is fixed in advance: the
numbers are the record, and an entry that comes out slower than its torch formulation is marked so.

  python tools/transfusion_rate.py [--bs 1 4] [--calls 10] [--warmup 3] [--chunks 256 512 1024 2048 4096 8192] [--out FILE]
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

from pdm_ssd_amd import attention_ops, transfusion_ops  # noqa: E402
from pdm_ssd_amd import detector_config as dc  # noqa: E402
from pdm_ssd_amd.config import cfg_from_dict  # noqa: E402
from pdm_ssd_amd.dense_heads import TransFusionHead  # noqa: E402

H = W = 180
CIN = 512


def timed(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    out = fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e), out


def rounds(fns, calls, warmup):
    """the functions called in turn, round after round -> their median times (ms)"""
    t = [[] for _ in fns]
    for i in range(warmup + calls):
        for j, fn in enumerate(fns):
            ms = timed(fn)[0]
            if i >= warmup:
                t[j].append(ms)
    return [statistics.median(x) for x in t]


def entry(name, ours, theirs, calls, warmup, diff):
    a, b = ours(), theirs()
    ms, ms_t = rounds([ours, theirs], calls, warmup)
    return {'what': name, 'ms': round(ms, 4), 'ms_torch': round(ms_t, 4), 'slower_than_torch': bool(ms > ms_t), 'max_abs_diff': diff(a, b)}


def proposals_argsort(logits, P, k, exempt, y_size):
    B, C = logits.shape[:2]
    s = logits.sigmoid()
    pad = k // 2
    local = torch.zeros_like(s)
    local[:, :, pad:H - pad, pad:W - pad] = torch.nn.functional.max_pool2d(s, kernel_size=k, stride=1, padding=0)
    for c in exempt:
        local[:, c] = s[:, c]
    masked = (s * (s == local)).view(B, C, -1)
    top = masked.view(B, -1).argsort(dim=-1, descending=True)[..., :P]
    index = top % masked.shape[-1]
    return index, top // masked.shape[-1], masked.gather(2, index[:, None, :].expand(-1, C, -1))


def sdpa(q, k, v, nh):
    B, P, C = q.shape
    qh, kh, vh = (t.reshape(B, t.shape[1], nh, C // nh).transpose(1, 2) for t in (q, k, v))
    return torch.nn.functional.scaled_dot_product_attention(qh, kh, vh).transpose(1, 2).reshape(B, P, C)


def error_ratio(q, k, v, nh, kpc):
    want = attention_ops.mha_reference(q.double().cpu(), k.double().cpu(), v.double().cpu(), nh)
    ek = float((attention_ops.mha_forward(q, k, v, nh, kpc).double().cpu() - want).abs().max())
    et = float((sdpa(q.contiguous(), k.contiguous(), v.contiguous(), nh).double().cpu() - want).abs().max())
    return {'err_kernel': ek, 'err_torch': et, 'ratio': ek / et if et > 0 else None}


def run(bs, calls, warmup, chunks, dev):
    torch.manual_seed(bs)
    head = TransFusionHead(model_cfg=cfg_from_dict(copy.deepcopy(dc.TRANSFUSION_LIDAR_CFG['DENSE_HEAD'])), input_channels=CIN, num_class=10,
                           class_names=dc.TRANSFUSION_CLASS_NAMES, grid_size=dc.TRANSFUSION_GRID_SIZE, point_cloud_range=dc.TRANSFUSION_RANGE,
                           voxel_size=dc.TRANSFUSION_VOXEL_SIZE, predict_boxes_when_training=False).to(dev).eval()
    dec, nh, P = head.decoder, head.decoder.nhead, head.num_proposals
    res = {'bs': bs, 'entries': []}
    with torch.no_grad():
        for m in head.modules():
            if isinstance(m, (torch.nn.BatchNorm1d, torch.nn.BatchNorm2d)):
                m.running_var.uniform_(0.5, 1.5)
                m.running_mean.uniform_(-0.2, 0.2)
        x = torch.randn((bs, CIN, H, W), device=dev)
        logits = torch.randn((bs, 10, H, W), device=dev) * 1.5 - 3.0
        exempt = [8, 9]

        def diff_prop(a, b):
            if not (torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])):      # (a tie of two random scores: argsort leaves it open)
                return None
            return float((a[2] - b[2]).abs().max())
        res['entries'].append(entry('proposals', lambda: transfusion_ops.proposals(logits, P, 3, exempt, H),
                                    lambda: proposals_argsort(logits, P, 3, exempt, H), calls, warmup, diff_prop))

        C = 128
        rows_q = torch.randn((bs, P, C), device=dev)
        rows_k = torch.randn((bs, H * W, C), device=dev)
        maxdiff = lambda a, b: float((a - b).abs().max())      # noqa: E731
        for name, attn, kv, same in (('self-attention', dec.self_attn, rows_q, True), ('cross-attention', dec.multihead_attn, rows_k, False)):
            q_sf, kv_sf = rows_q.transpose(0, 1).contiguous(), kv.transpose(0, 1).contiguous()
            res['entries'].append(entry(name, lambda: dec._attend(attn, True, rows_q, kv, same),
                                        lambda: attn(q_sf, kv_sf, kv_sf, need_weights=False)[0].transpose(0, 1), calls, warmup, maxdiff))

        # the kernel alone on the cross-attention's projected rows, over keys_per_chunk
        Wi, bi = dec.multihead_attn.in_proj_weight, dec.multihead_attn.in_proj_bias
        q = torch.nn.functional.linear(rows_q, Wi[:C], bi[:C])
        kvp = torch.nn.functional.linear(rows_k, Wi[C:], bi[C:])
        k, v = kvp[..., :C], kvp[..., C:]
        kc, vc = k.contiguous(), v.contiguous()
        fns = [lambda c=c: attention_ops.mha_forward(q, k, v, nh, c) for c in chunks] + [lambda: sdpa(q, kc, vc, nh)]
        ms = rounds(fns, calls, warmup)
        res['keys_per_chunk_sweep'] = [{'keys_per_chunk': c, 'ms': round(t, 4)} for c, t in zip(chunks, ms[:-1])]
        res['sdpa_fp32_ms'] = round(ms[-1], 4)
        res['default_keys_per_chunk'] = attention_ops.default_keys_per_chunk()
        if bs == 1:
            res['error_ratios'] = {'cross (1, 200, 32400, 128, 8)': error_ratio(q, k, v, nh, 0),
                                   'self (1, 200, 200, 128, 8)': error_ratio(rows_q, rows_q, rows_q, nh, 0)}

        pred = head.predict(x)
        args = (pred['heatmap'], pred['center'], pred['height'], pred['dim'], pred['rot'], pred['vel'], head.query_labels,
                pred['query_heatmap_score'], 0.0, [-61.2, -61.2, -10.0, 61.2, 61.2, 10.0], -54.0, -54.0, 0.075, 0.075, 8)

        def diff_dec(a, b):
            assert torch.equal(a[3], b[3]) and torch.equal(a[2], b[2])
            return float((a[0] - b[0]).abs().max())
        res['entries'].append(entry('decode', lambda: transfusion_ops.decode(*args), lambda: transfusion_ops.decode_torch(*args), calls, warmup, diff_dec))

        def whole(fused):
            head.use_fused = fused
            return head({'batch_size': bs, 'spatial_features_2d': x})['final_box_dicts']

        def diff_head(a, b):
            same = all(len(u['pred_boxes']) == len(w['pred_boxes']) for u, w in zip(a, b))
            return max(float((u['pred_boxes'] - w['pred_boxes']).abs().max()) for u, w in zip(a, b)) if same else None
        res['entries'].append(entry('head', lambda: whole(True), lambda: whole(False), calls, warmup, diff_head))
        head.use_fused = True
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--bs', type=int, nargs='+', default=[1, 4])
    ap.add_argument('--calls', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--chunks', type=int, nargs='+', default=[256, 512, 1024, 2048, 4096, 8192])
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'transfusion_rate.json'))
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    out = {'tool': 'tools/transfusion_rate.py', 'device': torch.cuda.get_device_name(0), 'map': [H, W], 'channels': 128, 'queries': 200, 'heads': 8,
           'calls': args.calls, 'warmup': args.warmup, 'runs': [run(bs, args.calls, args.warmup, args.chunks, dev) for bs in args.bs]}
    line = json.dumps(out)
    print(line)
    with open(args.out, 'w') as f:
        f.write(line + '\n')


if __name__ == '__main__':
    main()

"""Shared inputs of the TransFusionHead tests: the reference fixture (tests/golden/gen_transfusion_fixtures.py), its head
configuration, the seeded parameter fill the generator and the tests both use (the fixture holds no weights), and the
margin conditions under which rounding on another device cannot change a discrete choice of the head."""
import json
import os

import numpy as np
import torch
from torch import nn

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
B, H, W, CIN = 2, 12, 20, 16                  # a non-square map: y_size = 12, x_size = 20
HIDDEN, NHEADS, FFN, P = 32, 2, 48, 12
GRID = [160, 96, 1]
PC_RANGE = [0.0, -2.4, -3.0, 8.0, 2.4, 1.0]
VOXEL = [0.05, 0.05, 4.0]
STRIDE = 8
CLASS_NAMES = ['car', 'truck', 'construction_vehicle', 'bus', 'trailer', 'barrier', 'motorcycle', 'bicycle', 'pedestrian', 'traffic_cone']
MARGIN = 1e-3
MAPS = ('center', 'height', 'dim', 'rot', 'vel', 'heatmap')
TAGS = {'nus': 'nuScenes', 'kitti': 'KITTI'}  # the second head has no class exempt from the local-maximum filter

_fixture = None


def fixture():
    global _fixture
    if _fixture is None:
        with np.load(os.path.join(G, "ref_transfusion.npz")) as z:
            _fixture = {k: z[k] for k in z.files}
    return _fixture


def manifest():
    with open(os.path.join(G, "ref_transfusion_manifest.json")) as f:
        return json.load(f)


def head_cfg(dataset, score_thresh=0.0, post_range=(-1e4, -1e4, -1e4, 1e4, 1e4, 1e4), vel=True, **over):
    heads = {'center': {'out_channels': 2, 'num_conv': 2}, 'height': {'out_channels': 1, 'num_conv': 2},
             'dim': {'out_channels': 3, 'num_conv': 2}, 'rot': {'out_channels': 2, 'num_conv': 2}}
    if vel:
        heads['vel'] = {'out_channels': 2, 'num_conv': 2}
    cfg = {'NAME': 'TransFusionHead', 'USE_BIAS_BEFORE_NORM': False, 'NUM_PROPOSALS': P, 'HIDDEN_CHANNEL': HIDDEN, 'NUM_CLASSES': 10,
           'NUM_HEADS': NHEADS, 'NMS_KERNEL_SIZE': 3, 'FFN_CHANNEL': FFN, 'DROPOUT': 0.1, 'BN_MOMENTUM': 0.1, 'ACTIVATION': 'relu',
           'NUM_HM_CONV': 2,
           'SEPARATE_HEAD_CFG': {'HEAD_ORDER': list(heads), 'HEAD_DICT': heads},
           'TARGET_ASSIGNER_CONFIG': {'FEATURE_MAP_STRIDE': STRIDE, 'DATASET': dataset, 'GAUSSIAN_OVERLAP': 0.1, 'MIN_RADIUS': 2,
                                      'HUNGARIAN_ASSIGNER': {'cls_cost': {'gamma': 2.0, 'alpha': 0.25, 'weight': 0.15},
                                                             'reg_cost': {'weight': 0.25}, 'iou_cost': {'weight': 0.25}}},
           'LOSS_CONFIG': {'LOSS_WEIGHTS': {'cls_weight': 1.0, 'bbox_weight': 0.25, 'hm_weight': 1.0, 'code_weights': [1.0] * 8 + [0.2, 0.2]},
                           'LOSS_CLS': {'use_sigmoid': True, 'gamma': 2.0, 'alpha': 0.25}},
           'POST_PROCESSING': {'SCORE_THRESH': float(score_thresh), 'POST_CENTER_RANGE': [float(v) for v in post_range]}}
    cfg.update(over)
    return cfg


def head_kwargs():
    return dict(input_channels=CIN, num_class=10, class_names=CLASS_NAMES, grid_size=np.array(GRID), point_cloud_range=PC_RANGE,
                voxel_size=VOXEL, predict_boxes_when_training=False)


def fill_transfusion(net, seed, gain=1.0, hm_gain=1.0, hm_bias=0.0):
    """Seeded parameters and BatchNorm statistics, by module type in sorted module-name order: convolution / linear / attention
    in-projection weights uniform within +-gain sqrt(3 / fan_in) (the heat-map head's last convolution times hm_gain), their
    biases within +-0.1 (the heat-map head's last convolution: hm_bias +- 0.1, which moves the best scores to where the sigmoid is
    steep and neighbouring ranks lie apart); BatchNorm and LayerNorm gamma in [0.8, 1.2]; BatchNorm beta in [0, 0.4], mean in [-0.2, 0.2], var in
    [0.5, 1.5]; LayerNorm beta within +-0.1.  -> check sum (float)."""
    g = torch.Generator().manual_seed(seed)
    total = 0.0

    def put(t, v):
        nonlocal total
        t.copy_(v.to(t.dtype))
        total += float(v.double().abs().sum())

    def rand(shape, lo, hi):
        return torch.rand(tuple(shape), generator=g) * (hi - lo) + lo

    with torch.no_grad():
        for name, m in sorted(net.named_modules(), key=lambda kv: kv[0]):
            if isinstance(m, (nn.BatchNorm1d, nn.BatchNorm2d)):
                put(m.weight, rand(m.weight.shape, 0.8, 1.2))
                put(m.bias, rand(m.bias.shape, 0.0, 0.4))
                put(m.running_mean, rand(m.running_mean.shape, -0.2, 0.2))
                put(m.running_var, rand(m.running_var.shape, 0.5, 1.5))
            elif isinstance(m, nn.LayerNorm):
                put(m.weight, rand(m.weight.shape, 0.8, 1.2))
                put(m.bias, rand(m.bias.shape, -0.1, 0.1))
            elif isinstance(m, (nn.Conv1d, nn.Conv2d, nn.Linear)):
                a = gain * (hm_gain if name == 'heatmap_head.1' else 1.0) * float(np.sqrt(3.0 * m.weight.shape[0] / m.weight.numel()))
                put(m.weight, rand(m.weight.shape, -a, a))
                if m.bias is not None:
                    off = hm_bias if name == 'heatmap_head.1' else 0.0
                    put(m.bias, rand(m.bias.shape, off - 0.1, off + 0.1))
            elif isinstance(m, nn.MultiheadAttention):
                a = gain * float(np.sqrt(3.0 / m.embed_dim))
                put(m.in_proj_weight, rand(m.in_proj_weight.shape, -a, a))
                put(m.in_proj_bias, rand(m.in_proj_bias.shape, -0.1, 0.1))
    return total


def build_head(tag, device='cpu', use_fused=True, **cfg_kw):
    """this repository's head at the fixture's shapes with the fixture's parameters (manifest: seed, gains, thresholds)"""
    from pdm_ssd_amd.config import cfg_from_dict
    from pdm_ssd_amd.dense_heads import TransFusionHead
    man = manifest()
    kw = dict(score_thresh=man['score_thresh'], post_range=man['post_center_range'])
    kw.update(cfg_kw)
    head = TransFusionHead(model_cfg=cfg_from_dict(head_cfg(TAGS[tag], **kw)), **head_kwargs())
    total = fill_transfusion(head, man['seed'], man['gain'], man['hm_gain'], man['hm_bias'])
    if kw.get('vel', True):
        assert abs(total - man['weight_sum']) <= 1e-6 * man['weight_sum'], (total, man['weight_sum'])
    head.use_fused = use_fused
    return head.to(device).eval()


def masked_scores(logits, k, exempt):
    """float64 restatement of the query filter -> (masked (B, C, H, W), s, window maximum of the OTHER cells (-inf outside the
    interior or for an exempt class))"""
    s = 1.0 / (1.0 + np.exp(-np.asarray(logits, dtype=np.float64)))
    Bn, C, Hh, Ww = s.shape
    pad = k // 2
    other = np.full(s.shape, -np.inf)
    interior = np.zeros(s.shape, dtype=bool)
    interior[:, :, pad:Hh - pad, pad:Ww - pad] = True
    for dy in range(-pad, pad + 1):
        for dx in range(-pad, pad + 1):
            if dy == 0 and dx == 0:
                continue
            sh = np.full(s.shape, -np.inf)
            ys, xs = slice(max(0, -dy), Hh - max(0, dy)), slice(max(0, -dx), Ww - max(0, dx))
            yd, xd = slice(max(0, dy), Hh - max(0, -dy)), slice(max(0, dx), Ww - max(0, -dx))
            sh[:, :, ys, xs] = s[:, :, yd, xd]
            other = np.maximum(other, sh)
    keep = interior & (s >= other)
    for c in exempt:
        keep[:, c] = True
        other[:, c] = -np.inf
        interior[:, c] = True
    return s * keep, s, other, interior, keep


def proposal_margins(logits, k, exempt, num_proposals):
    """-> dict of the smallest margins of conditions (a)-(c) on a heat-map: survivors (the fewest positive survivors of a sample),
    rank_gap (ranks 1 .. P + 1 of the masked scores pairwise), window_gap (every surviving cell among the top P + 1 against each
    other cell of its window; every non-surviving interior cell whose own score would rank in the top P + 1 against its window
    maximum; a border cell has no margin to keep: it is dropped whatever its score)"""
    masked, s, other, interior, keep = masked_scores(logits, k, exempt)
    Bn = s.shape[0]
    flat = masked.reshape(Bn, -1)
    order = np.argsort(-flat, axis=1, kind='stable')[:, :num_proposals + 1]
    top = np.take_along_axis(flat, order, axis=1)
    out = {'survivors': int((flat > 0).sum(1).min()), 'rank_gap': float((top[:, :-1] - top[:, 1:]).min())}
    gaps = []
    for b in range(Bn):
        cut = top[b, -1]
        sb, ob, kb, ib = s[b].reshape(-1), other[b].reshape(-1), keep[b].reshape(-1), interior[b].reshape(-1)
        for i in order[b]:
            if np.isfinite(ob[i]):
                gaps.append(sb[i] - ob[i])
        losers = np.nonzero(~kb & ib & (sb >= cut - MARGIN))[0]
        gaps += [ob[i] - sb[i] for i in losers]
    out['window_gap'] = float(min(gaps)) if gaps else float('inf')
    return out


def check_proposal_margins(m, num_proposals):
    assert m['survivors'] >= num_proposals, m
    assert m['rank_gap'] >= MARGIN and m['window_gap'] >= MARGIN, m


def close(a, b, tol):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    if a.size:
        err = float(np.abs(a - b).max())
        assert err <= tol, (err, tol)


def check_predictions(res, tag, tol):
    """a predict() dict against the fixture: the query set exactly, the maps within tol"""
    fx = fixture()
    close(res['dense_heatmap'].cpu().numpy(), fx[f'{tag}.dense_heatmap'], tol)
    close(res['query_heatmap_score'].cpu().numpy(), fx[f'{tag}.query_heatmap_score'], 1e-6)
    for name in MAPS:
        close(res[name].cpu().numpy(), fx[f'{tag}.pred.{name}'], tol)


def check_boxes(dicts, tag, tol):
    fx = fixture()
    assert len(dicts) == B
    for b, d in enumerate(dicts):
        assert np.array_equal(d['pred_labels'].cpu().numpy().astype(np.int64), fx[f'{tag}.final.labels.{b}'])
        close(d['pred_boxes'].cpu().numpy(), fx[f'{tag}.final.boxes.{b}'], tol)
        close(d['pred_scores'].cpu().numpy(), fx[f'{tag}.final.scores.{b}'], tol)


def fixture_decode(tag, fn, device='cpu', vel=True):
    """fn = transfusion_ops.decode | decode_torch on the fixture's prediction maps with the manifest's threshold and range"""
    fx, man = fixture(), manifest()
    t = {k: torch.from_numpy(fx[f'{tag}.pred.{k}']).to(device) for k in MAPS}
    return fn(t['heatmap'], t['center'], t['height'], t['dim'], t['rot'], t['vel'] if vel else None, torch.from_numpy(fx[f'{tag}.cls']).to(device),
              torch.from_numpy(fx[f'{tag}.query_heatmap_score']).to(device), man['score_thresh'], man['post_center_range'],
              PC_RANGE[0], PC_RANGE[1], VOXEL[0], VOXEL[1], STRIDE)


def check_padded(tag, padded, vel=True):
    """a padded decode against the fixture: counts, labels and order exactly, boxes and scores within parity_abs, padding zero"""
    fx, man = fixture(), manifest()
    boxes, scores, labels, count = (t.cpu().numpy() for t in padded)
    assert count.dtype == np.int32 and labels.dtype == np.int64 and count.tolist() == man[f'kept.{tag}']
    assert boxes.shape == (B, P, 9 if vel else 7)
    for b, n in enumerate(count.tolist()):
        assert np.array_equal(labels[b, :n], fx[f'{tag}.final.labels.{b}'])        # the survivors in query order
        close(boxes[b, :n], fx[f'{tag}.final.boxes.{b}'][:, :boxes.shape[2]], man['parity_abs'])
        close(scores[b, :n], fx[f'{tag}.final.scores.{b}'], man['parity_abs'])
        assert not boxes[b, n:].any() and not scores[b, n:].any() and not labels[b, n:].any()

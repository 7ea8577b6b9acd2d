"""Shared inputs of the TransFusionHead training tests: the reference fixture of the head's loss
(tests/golden/gen_transfusion_train_fixtures.py), the head configuration with the training key, and small helpers for the
linear-sum-assignment tests.  A helper module like transfusion_case.py: no tests here."""
import itertools
import json
import os

import numpy as np
import torch

import transfusion_case as tc

GRAD_MAPS = tc.MAPS + ('dense_heatmap',)
TARGETS = ('labels', 'label_weights', 'bbox_targets', 'bbox_weights', 'ious', 'assigned', 'heatmap')
LOSSES = ('loss_cls', 'loss_bbox', 'loss_heatmap')

_fixture = None


def fixture():
    global _fixture
    if _fixture is None:
        with np.load(os.path.join(tc.G, "ref_transfusion_train.npz")) as z:
            _fixture = {k: z[k] for k in z.files}
    return _fixture


def manifest():
    with open(os.path.join(tc.G, "ref_transfusion_train_manifest.json")) as f:
        return json.load(f)


def train_cfg(dataset='nuScenes', on_device=True, **kw):
    """transfusion_case.head_cfg without dropout (the fixture's training forward is then a function of its inputs alone) and,
    with on_device, the key that switches the training half on"""
    cfg = tc.head_cfg(dataset, DROPOUT=0.0, **kw)
    if on_device:
        cfg['TARGET_ASSIGNER_CONFIG']['ASSIGN_ON_DEVICE'] = True
    return cfg


def build_train_head(device='cpu', on_device=True):
    """this repository's head with the eval fixture's seeded parameters, in training mode"""
    from pdm_ssd_amd.config import cfg_from_dict
    from pdm_ssd_amd.dense_heads import TransFusionHead
    man = tc.manifest()
    head = TransFusionHead(model_cfg=cfg_from_dict(train_cfg(on_device=on_device)), **tc.head_kwargs())
    total = tc.fill_transfusion(head, man['seed'], man['gain'], man['hm_gain'], man['hm_bias'])
    assert abs(total - man['weight_sum']) <= 1e-6 * man['weight_sum']
    return head.to(device).train()


def assign_args():
    a = train_cfg()['TARGET_ASSIGNER_CONFIG']
    h = a['HUNGARIAN_ASSIGNER']
    return (h['cls_cost'], h['reg_cost'], h['iou_cost'], tc.PC_RANGE, tc.VOXEL, tc.STRIDE, (tc.H, tc.W), a['GAUSSIAN_OVERLAP'],
            a['MIN_RADIUS'], 10)


def loss_args():
    w = train_cfg()['LOSS_CONFIG']
    return (w['LOSS_WEIGHTS']['code_weights'], w['LOSS_WEIGHTS']['cls_weight'], w['LOSS_WEIGHTS']['bbox_weight'],
            w['LOSS_WEIGHTS']['hm_weight'], w['LOSS_CLS']['alpha'], w['LOSS_CLS']['gamma'])


def pred_tensors(device='cpu', requires_grad=False, put=None):
    """the fixture's prediction maps (the reference head's training-mode predict) as tensors; put(array) -> tensor overrides the upload"""
    fx = fixture()
    up = put if put is not None else (lambda a: torch.from_numpy(a).to(device))
    out = {k: up(fx[f'pred.{k}']) for k in GRAD_MAPS}
    if requires_grad:
        for t in out.values():
            t.requires_grad_(True)
    return out


def map_args(t, vel=True):
    return (t['heatmap'], t['center'], t['height'], t['dim'], t['rot'], t['vel'] if vel else None)


def check_targets(got, tol):
    """an assign() dict against the fixture: discrete outputs exactly, floats within tol"""
    fx = fixture()
    for k in ('labels', 'assigned'):
        assert np.array_equal(got[k].cpu().numpy().astype(np.int64), fx[f'target.{k}'].astype(np.int64)), k
    assert got['labels'].dtype == torch.int64 and got['assigned'].dtype == torch.int32
    assert int(got['num_pos']) == int(fx['target.num_pos'])
    for k in ('label_weights', 'bbox_targets', 'bbox_weights', 'ious', 'heatmap'):
        tc.close(got[k].cpu().numpy(), fx[f'target.{k}'], tol)
    assert np.array_equal(got['heatmap'].cpu().numpy() == 1.0, fx['target.heatmap'] == 1.0)       # the peaks: the loss's divisor
    tc.close(float(got['matched_ious']), float(fx['target.matched_ious']), tol)


def brute_force(cost):
    """-> (the least total over all matchings of size min(P, G), the set of matchings that reach it as frozensets of (row, col))"""
    c = np.asarray(cost, dtype=np.float64)
    P, G = c.shape
    if G == 0:
        return 0.0, {frozenset()}
    tr = G > P
    if tr:
        c = c.T
    n, k = c.shape                                                        # n >= k: every column gets a row
    best, arg = np.inf, set()
    for rows in itertools.permutations(range(n), k):
        t = float(c[list(rows), range(k)].sum())
        pairs = frozenset((g, r) if tr else (r, g) for g, r in enumerate(rows))
        if t < best - 1e-12:
            best, arg = t, {pairs}
        elif abs(t - best) <= 1e-12:
            arg.add(pairs)
    return best, arg


def check_matching(cost, gt_of_row, row_of_gt):
    """a valid matching of size min(P, G), the two maps inverse to each other -> its total cost in float64"""
    c = np.asarray(cost, dtype=np.float64)
    P, G = c.shape
    rows = np.nonzero(gt_of_row >= 0)[0]
    assert len(rows) == min(P, G) and len(set(gt_of_row[rows].tolist())) == len(rows)
    assert gt_of_row.min() >= -1 and (G == 0 or gt_of_row.max() < G)
    for r in rows:
        assert row_of_gt[gt_of_row[r]] == r
    assert int((row_of_gt >= 0).sum()) == len(rows)
    return float(c[rows, gt_of_row[rows]].sum())

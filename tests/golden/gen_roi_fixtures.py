#!/usr/bin/env python3
"""Generates tests/golden/ref_roi.npz and ref_roi_manifest.json by running the REFERENCE's own Python on the CPU:
/root/reference/pcdet/ops/roipoint_pool3d/roipoint_pool3d_utils.py, ops/roiaware_pool3d/roiaware_pool3d_utils.py,
models/roi_heads/roi_head_template.py + pointrcnn_head.py and utils/box_coder_utils.py — imported from where they lie,
nothing copied — with only what this image lacks replaced:
  - the native extensions roipoint_pool3d_cuda / roiaware_pool3d_cuda by stubs over tests/roi_pool_reference.py,
  - pointnet2_batch_cuda by a stub over this repo's CPU oracle (as gen_module_fixtures.py),
  - iou3d_nms_utils, SharedArray and numba by empty modules (imported, never called: the rois are given),
  - `.cuda()` by the identity.
Records (a) RoIPointPool3d outputs, (b) RoIAwarePool3d outputs for max and avg and two grid sizes, (c) the pooled
canonical points of PointRCNNHead.roipool3d_gpu, the eval forward of a reduced head with (d) all headings exactly 0 and
(e) random headings, a ResidualCoder round trip, and the state_dict manifests.

Every case is reject-sampled so that no test rests on a last-ulp difference between the host's and the device's cosf:
no point within 1e-4 m of a box face; for (b) no in-box point's voxel coordinate within 1e-3 of an integer; for (e) the
head's outputs move by less than 1e-4 when the pooled canonical coordinates are perturbed by +-2e-5.  The seeds used are
recorded.  Run in the authoring container only (needs /root/reference); the outputs are committed.
"""
import copy
import json
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
from oracle import cpu_oracle as o  # noqa: E402
import roi_pool_reference as rp  # noqa: E402
import roi_head_case  # noqa: E402
import gen_head_fixtures as ghf  # noqa: E402
import gen_module_fixtures as gmf  # noqa: E402

REF = '/root/reference'
EasyDict = ghf.EasyDict


def n(t):
    return t.detach().numpy()


def install_reference():
    gmf.install_reference()          # pcdet, pcdet.ops, pointnet2_batch + its native stub
    phb, _, bcu, _ = ghf.install_reference()   # utils, models, SharedArray / numba / iou3d stubs, .cuda() identity
    for name, path in (('pcdet.ops.pointnet2', f'{REF}/pcdet/ops/pointnet2'),
                       ('pcdet.ops.pointnet2.pointnet2_batch', f'{REF}/pcdet/ops/pointnet2/pointnet2_batch')):
        if name not in sys.modules or not getattr(sys.modules[name], '__path__', None):
            m = types.ModuleType(name)
            m.__path__ = [path]
            sys.modules[name] = m

    def pkg(name, path):
        m = types.ModuleType(name)
        m.__path__ = [path]
        sys.modules[name] = m
        return m
    pp = pkg('pcdet.ops.roipoint_pool3d', f'{REF}/pcdet/ops/roipoint_pool3d')
    ext = types.ModuleType('pcdet.ops.roipoint_pool3d.roipoint_pool3d_cuda')

    def pp_forward(xyz, boxes, feats, pooled, flag):
        P, E = n(pooled), n(flag)          # views of the tensors' storage: updated in place
        rp.roipoint_pool3d(n(xyz), n(boxes), n(feats), P, E)
    ext.forward = pp_forward
    pp.roipoint_pool3d_cuda = ext
    sys.modules[ext.__name__] = ext

    ra = sys.modules['pcdet.ops.roiaware_pool3d']
    ra.__path__ = [f'{REF}/pcdet/ops/roiaware_pool3d']
    ext2 = types.ModuleType('pcdet.ops.roiaware_pool3d.roiaware_pool3d_cuda')

    def ra_forward(rois, pts, feats, argmax, pts_idx, pooled, pool_method):
        rp.roiaware_pool3d_forward(n(rois), n(pts), n(feats), n(argmax), n(pts_idx), n(pooled), pool_method)

    def ra_backward(pts_idx, argmax, grad_out, grad_in, pool_method):
        rp.roiaware_pool3d_backward(n(pts_idx), n(argmax), n(grad_out), n(grad_in), pool_method)
    ext2.forward, ext2.backward = ra_forward, ra_backward
    ext2.points_in_boxes_gpu = lambda boxes, pts, out: out.copy_(torch.from_numpy(o.points_in_boxes(n(pts), n(boxes))))
    ra.roiaware_pool3d_cuda = ext2
    sys.modules[ext2.__name__] = ext2
    del sys.modules['pcdet.ops.roiaware_pool3d.roiaware_pool3d_utils']     # the stub of gen_head_fixtures: load the real file
    del ra.roiaware_pool3d_utils
    pkg('pcdet.models.roi_heads', f'{REF}/pcdet/models/roi_heads')         # package __init__ not run (it imports every head)
    pkg('pcdet.models.roi_heads.target_assigner', f'{REF}/pcdet/models/roi_heads/target_assigner')
    from pcdet.models.roi_heads import pointrcnn_head
    from pcdet.ops.roiaware_pool3d import roiaware_pool3d_utils
    from pcdet.ops.roipoint_pool3d import roipoint_pool3d_utils
    from pcdet.ops.pointnet2.pointnet2_batch import pointnet2_modules
    return pointrcnn_head, roipoint_pool3d_utils, roiaware_pool3d_utils, bcu, phb, pointnet2_modules


face_clearance, voxel_clearance = rp.face_clearance, rp.voxel_clearance


def boxes_in_block(rng, k, lo, hi, size_lo, size_hi, zero_heading=False):
    bx = np.zeros((k, 7), dtype=np.float32)
    bx[:, 0:2] = rng.uniform(lo, hi, (k, 2))
    bx[:, 2] = rng.uniform(-0.3, 0.3, k)
    bx[:, 3:6] = rng.uniform(size_lo, size_hi, (k, 3))
    if not zero_heading:
        bx[:, 6] = rng.uniform(-np.pi, np.pi, k)
    return bx


def case_a(rng):
    B, N, M, C = 2, 300, 5, 5
    xyz = np.stack([rng.uniform(0, 10, (B, N)), rng.uniform(0, 10, (B, N)), rng.uniform(-1, 1, (B, N))], -1).astype(np.float32)
    boxes = np.zeros((B, M, 7), dtype=np.float32)
    for b in range(B):
        boxes[b, 0] = boxes_in_block(rng, 1, 3, 7, [5, 4, 1.5], [6, 5, 2.5])[0]      # more than S points
        boxes[b, 1:4] = boxes_in_block(rng, 3, 1, 9, [1.0, 0.8, 1.0], [2.5, 2.0, 2.0])  # a few points
        boxes[b, 4] = boxes_in_block(rng, 1, 30, 40, [1, 1, 1], [2, 2, 2])[0]        # empty
    feats = rng.standard_normal((B, N, C)).astype(np.float32)
    return xyz, boxes, feats


def case_b(rng):
    K, P, C = 4, 200, 3
    pts = np.stack([rng.uniform(0, 6, P), rng.uniform(0, 6, P), rng.uniform(-1, 1, P)], -1).astype(np.float32)
    rois = boxes_in_block(rng, K, 2, 4, [2.0, 1.5, 1.2], [3.5, 3.0, 2.0])
    rois[1, 0:3] = rois[0, 0:3] + np.float32([0.4, -0.3, 0.1])     # boxes 0 and 1 overlap
    feats = rng.standard_normal((P, C)).astype(np.float32)
    feats[:, 2] = -np.abs(feats[:, 2]) - 0.5                       # an all-negative channel: its maximum is negative
    return rois, pts, feats


def case_head(rng, zero_heading):
    B, npts, R, C = 2, 256, 6, roi_head_case.HEAD_INPUT_CHANNELS
    coords, rois = [], np.zeros((B, R, 7), dtype=np.float32)
    for b in range(B):
        p = np.stack([rng.uniform(2, 12, npts), rng.uniform(2, 12, npts), rng.uniform(-1, 1, npts)], -1)
        coords.append(np.concatenate([np.full((npts, 1), b), p], 1))
        rois[b, 0:4] = boxes_in_block(rng, 4, 4, 10, [2.0, 1.5, 1.2], [5.0, 4.0, 2.0], zero_heading)
        rois[b, 4] = boxes_in_block(rng, 1, 40, 50, [2, 2, 2], [3, 3, 3], zero_heading)[0]   # empty; row 5: all-zero padding
    coords = np.concatenate(coords).astype(np.float32)
    feats = rng.standard_normal((B * npts, C)).astype(np.float32)
    scores = rng.uniform(0, 1, B * npts).astype(np.float32)
    return coords, rois, feats, scores


def make_head(prh):
    torch.manual_seed(11)
    head = prh.PointRCNNHead(input_channels=roi_head_case.HEAD_INPUT_CHANNELS, model_cfg=EasyDict(copy.deepcopy(roi_head_case.HEAD_CFG)),
                             num_class=1).eval()
    g = torch.Generator().manual_seed(12)
    with torch.no_grad():
        head.reg_layers[-1].weight.copy_(torch.randn(head.reg_layers[-1].weight.shape, generator=g) * 0.1)
        for name, p in head.named_parameters():
            if name.endswith('bias'):
                p.copy_(torch.randn(p.shape, generator=g) * 0.1)
        for name, buf in head.named_buffers():
            if name.endswith('running_mean'):
                buf.copy_(torch.randn(buf.shape, generator=g) * 0.1)
            elif name.endswith('running_var'):
                buf.copy_(torch.rand(buf.shape, generator=g) + 0.5)
    return head


def run_head(head, coords, rois, feats, scores, pooled_override=None):
    got = {}
    hooks = [head.cls_layers.register_forward_hook(lambda m, i, out: got.__setitem__('rcnn_cls', out)),
             head.reg_layers.register_forward_hook(lambda m, i, out: got.__setitem__('rcnn_reg', out))]
    bd = {'batch_size': rois.shape[0], 'point_coords': torch.from_numpy(coords), 'point_features': torch.from_numpy(feats),
          'point_cls_scores': torch.from_numpy(scores), 'rois': torch.from_numpy(rois.copy())}
    keep = head.roipool3d_gpu
    # the (B, N, 2 + C) features the head pools: [score, depth, features], formed as pointrcnn_head.py:109-112 forms them
    xyz_t = bd['point_coords'][:, 1:4]
    feats_all = torch.cat([bd['point_cls_scores'][:, None], (xyz_t.norm(dim=1) / head.model_cfg.ROI_POINT_POOL.DEPTH_NORMALIZER - 0.5)[:, None],
                           bd['point_features']], dim=1)
    try:
        if pooled_override is not None:
            head.roipool3d_gpu = lambda batch_dict: pooled_override
        with torch.no_grad():
            pooled = keep(dict(bd)) if pooled_override is None else pooled_override
            bd = head(bd)
    finally:
        head.roipool3d_gpu = keep
        for h in hooks:
            h.remove()
    return {'pooled': n(pooled), 'feats_all': n(feats_all), 'rcnn_cls': n(got['rcnn_cls'].transpose(1, 2).contiguous().squeeze(1)),
            'rcnn_reg': n(got['rcnn_reg'].transpose(1, 2).contiguous().squeeze(1)),
            'batch_cls_preds': n(bd['batch_cls_preds']), 'batch_box_preds': n(bd['batch_box_preds'])}


def sample(make, ok, seed):
    """make(rng) until ok(case); returns (case, the seed used)."""
    while True:
        case = make(np.random.default_rng(seed))
        if ok(case):
            return case, seed
        seed += 1


def main():
    prh, ppu, rau, bcu, phb, pm = install_reference()
    out, manifest, seeds = {}, {}, {}

    # (a) RoIPointPool3d
    ew, S = [0.2, 0.2, 0.2], 16
    enlarged = lambda bx: bx + np.float32([0, 0, 0] + ew + [0])   # noqa: E731
    (xyz, boxes, feats), seeds['a'] = sample(case_a, lambda c: all(
        face_clearance(c[0][b], enlarged(c[1][b])) > 1e-4 for b in range(2)), 100)
    layer = ppu.RoIPointPool3d(num_sampled_points=S, pool_extra_width=ew)
    pooled, flag = layer(torch.from_numpy(xyz), torch.from_numpy(feats), torch.from_numpy(boxes))
    counts = [[int(rp.in_box_mask(xyz[b], enlarged(boxes[b, m])).sum()) for m in range(5)] for b in range(2)]
    assert all(c[0] > S and 0 < min(c[1:4]) and max(c[1:4]) < S and c[4] == 0 for c in counts), counts
    out.update(a_xyz=xyz, a_boxes=boxes, a_feats=feats, a_pooled=n(pooled), a_flag=n(flag), a_counts=np.array(counts))

    # (b) RoIAwarePool3d
    for tag, osz in (('b3', (3, 2, 4)), ('b1', 1)):
        o3 = (osz,) * 3 if isinstance(osz, int) else osz
        (rois, pts, bf), seeds[tag] = sample(case_b, lambda c: face_clearance(c[1], c[0]) > 1e-4 and
                                             voxel_clearance(c[1], c[0], o3) > 1e-3 and
                                             (rp.in_box_mask(c[1], c[0][0]) & rp.in_box_mask(c[1], c[0][1])).any(), 200)
        out.update({f'{tag}_rois': rois, f'{tag}_pts': pts, f'{tag}_feats': bf})
        pool = rau.RoIAwarePool3d(out_size=osz, max_pts_each_voxel=4)
        for method in ('max', 'avg'):
            f = torch.from_numpy(bf).requires_grad_(True)
            res = pool(torch.from_numpy(rois), torch.from_numpy(pts), f, pool_method=method)
            idx, am = res.grad_fn.roiaware_pool3d_for_backward[:2]
            out.update({f'{tag}_{method}_pooled': n(res), f'{tag}_{method}_pts_idx': n(idx)})
            if method == 'max':
                out[f'{tag}_max_argmax'] = n(am)
        assert (out[f'{tag}_max_pts_idx'][..., 0] == 3).any()      # the cap max_pts - 1 is reached

    # (c), (d), (e) the reduced head
    head = make_head(prh)
    key = 'PointRCNNHead(reduced: tests/roi_head_case.py HEAD_CFG, input_channels=16, num_class=1)'
    manifest[key] = {k: list(v.shape) for k, v in head.state_dict().items()}
    for k, v in head.state_dict().items():
        out['head_state.' + k] = n(v)

    def clear(c):
        ew_h = np.float32([0, 0, 0] + roi_head_case.HEAD_CFG['ROI_POINT_POOL']['POOL_EXTRA_WIDTH'] + [0])
        cnt = [[int(rp.in_box_mask(c[0][b * 256:(b + 1) * 256, 1:4], c[1][b, m] + ew_h).sum()) for m in range(6)] for b in range(2)]
        return (all(face_clearance(c[0][b * 256:(b + 1) * 256, 1:4], c[1][b] + ew_h) > 1e-4 for b in range(2))
                and all(min(r[:4]) > 0 and r[4] == 0 and r[5] == 0 for r in cnt))

    (coords, rois, hf, scores), seeds['d'] = sample(lambda r: case_head(r, True), clear, 300)
    assert (rois[..., 6] == 0).all()
    res = run_head(head, coords, rois, hf, scores)
    out.update(d_coords=coords, d_rois=rois, d_feats=hf, d_scores=scores, d_pooled=res['pooled'], d_feats_all=res['feats_all'], d_rcnn_cls=res['rcnn_cls'],
               d_rcnn_reg=res['rcnn_reg'], d_batch_cls_preds=res['batch_cls_preds'], d_batch_box_preds=res['batch_box_preds'])

    def stable(c):
        if not clear(c):
            return False
        base = run_head(head, *c)
        worst = 0.0
        for trial in range(4):
            noise = torch.zeros_like(torch.from_numpy(base['pooled']))
            noise[..., 0:3] = (torch.rand(noise[..., 0:3].shape, generator=torch.Generator().manual_seed(trial)) * 2 - 1) * 2e-5
            got = run_head(head, *c, pooled_override=torch.from_numpy(base['pooled']) + noise)
            worst = max(worst, float(np.abs(got['rcnn_cls'] - base['rcnn_cls']).max()), float(np.abs(got['rcnn_reg'] - base['rcnn_reg']).max()))
        return worst < 1e-4

    (coords, rois, hf, scores), seeds['e'] = sample(lambda r: case_head(r, False), stable, 400)
    res = run_head(head, coords, rois, hf, scores)
    out.update(e_coords=coords, e_rois=rois, e_feats=hf, e_scores=scores, e_pooled=res['pooled'], e_feats_all=res['feats_all'], e_rcnn_cls=res['rcnn_cls'],
               e_rcnn_reg=res['rcnn_reg'], e_batch_cls_preds=res['batch_cls_preds'], e_batch_box_preds=res['batch_box_preds'])

    # ResidualCoder values
    rng = np.random.default_rng(7)
    anchors = boxes_in_block(rng, 12, 0, 20, [1, 1, 1], [4, 2, 2])
    gts = anchors + rng.normal(0, 0.2, anchors.shape).astype(np.float32)
    for tag, coder in (('coder', bcu.ResidualCoder()), ('coder_sincos', bcu.ResidualCoder(encode_angle_by_sincos=True))):
        code = coder.encode_torch(torch.from_numpy(gts.copy()), torch.from_numpy(anchors.copy()))
        out.update({f'{tag}_code': n(code), f'{tag}_decoded': n(coder.decode_torch(code, torch.from_numpy(anchors.copy())))})
    out.update(coder_boxes=gts, coder_anchors=anchors)

    # manifests: the full-size head, and the reduced detector composed from the reference's own modules
    full = EasyDict(copy.deepcopy(roi_head_case.POINT_RCNN_CFG['ROI_HEAD']))
    full['LOSS_CONFIG'] = EasyDict(roi_head_case.HEAD_CFG['LOSS_CONFIG'])
    manifest['PointRCNNHead(POINT_RCNN_CFG, input_channels=128, num_class=1)'] = \
        {k: list(v.shape) for k, v in prh.PointRCNNHead(input_channels=128, model_cfg=full, num_class=1).state_dict().items()}
    cfg = copy.deepcopy(roi_head_case.REDUCED_POINT_RCNN_CFG)
    det = {'global_step': [1]}
    sa, skip, cin = cfg['BACKBONE_3D']['SA_CONFIG'], [1], 1
    for i, mlps in enumerate(sa['MLPS']):
        m = pm.PointnetSAModuleMSG(npoint=sa['NPOINTS'][i], radii=sa['RADIUS'][i], nsamples=sa['NSAMPLE'][i],
                                   mlps=[[cin] + list(s) for s in mlps], use_xyz=True)
        det.update({f'backbone_3d.SA_modules.{i}.{k}': list(v.shape) for k, v in m.state_dict().items()})
        cin = sum(s[-1] for s in mlps)
        skip.append(cin)
    fp = cfg['BACKBONE_3D']['FP_MLPS']
    for k in range(len(fp)):                       # pointnet2_backbone.py:41-50 of the reference
        pre = fp[k + 1][-1] if k + 1 < len(fp) else cin
        m = pm.PointnetFPModule(mlp=[pre + skip[k]] + list(fp[k]))
        det.update({f'backbone_3d.FP_modules.{k}.{kk}': list(v.shape) for kk, v in m.state_dict().items()})
    ph = phb.PointHeadBox(num_class=3, input_channels=fp[0][-1], model_cfg=EasyDict(cfg['POINT_HEAD']))
    det.update({f'point_head.{k}': list(v.shape) for k, v in ph.state_dict().items()})
    rcfg = EasyDict(cfg['ROI_HEAD'])
    rcfg['LOSS_CONFIG'] = EasyDict(roi_head_case.HEAD_CFG['LOSS_CONFIG'])
    rh = prh.PointRCNNHead(input_channels=fp[0][-1], model_cfg=rcfg, num_class=1)
    det.update({f'roi_head.{k}': list(v.shape) for k, v in rh.state_dict().items()})
    manifest['PointRCNN(tests/roi_head_case.py REDUCED_POINT_RCNN_CFG, 4 point features, 3 classes)'] = det
    manifest['seeds'] = seeds

    np.savez_compressed(os.path.join(HERE, 'ref_roi.npz'), **out)
    with open(os.path.join(HERE, 'ref_roi_manifest.json'), 'w') as f:
        json.dump(manifest, f, indent=1, sort_keys=True)
    print('wrote', len(out), 'arrays; seeds', seeds, 'counts (a)', counts)


if __name__ == '__main__':
    main()

#!/usr/bin/env python3
"""Generates tests/golden/ref_pv_rcnn.npz and ref_pv_rcnn_manifest.json by running the REFERENCE's own VoxelSetAbstraction
(pcdet/models/backbones_3d/pfe/voxel_set_abstraction.py), PointHeadSimple (pcdet/models/dense_heads/point_head_simple.py) and
PVRCNNHead (pcdet/models/roi_heads/pvrcnn_head.py) on the CPU, imported from where they lie, nothing copied, with only what the
authoring image lacks replaced:
  - the native pointnet2_stack_cuda by gen_stack_fixtures.install_reference's stubs over this repository's CPU oracle, plus a
    farthest_point_sampling_wrapper over the oracle's batch FPS,
  - SharedArray / numba / iou3d_nms by empty modules and `.cuda()` by the identity (gen_roi_fixtures.install_reference),
  - spconv by a namespace holding the attributes the encoder reads from a sparse tensor (indices, features, spatial_shape).
Run in the authoring container only; the outputs hold numbers and key names only.

The case is tests/pv_rcnn_case.py: B = 3, every sample non-empty, sample 1 with fewer points than NUM_KEYPOINTS = 48, reduced
widths, 5 rois a sample (voxel_rcnn_case.rois), GRID_SIZE 2 and 3.

Reject-sampled, so that no test rests on a last-ulp difference between the host and the device (seeds recorded):
  - no point within 1e-4 radius of any query sphere (every source of the encoder, both scales; the head's grid points against the
    keypoints, both scales), measured on the squared distances as |d^2 - r^2| >= 2e-4 r^2,
  - the head's outputs move by less than 1e-4 when the grid points are perturbed by +-2e-5.
main() also holds the numpy restatement (tests/pv_rcnn_reference.py) to the reference: keypoint rows, ball indices and the
BEV-interpolated features bit-equal, pooled and fused features within 2e-5.
"""
import json
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import gen_stack_fixtures as gsf  # noqa: E402
import pv_rcnn_case as case  # noqa: E402
import pv_rcnn_reference as pr  # noqa: E402

REF = gsf.REF
o = gsf.o
CLEAR = 2e-4        # on squared distances: 1e-4 of the radius


def install_reference():
    gsf.install_reference()
    ext = sys.modules['pcdet.ops.pointnet2.pointnet2_stack.pointnet2_stack_cuda']

    def farthest_point_sampling_wrapper(B, N, npoint, xyz, temp, output):
        output.copy_(torch.from_numpy(o.furthest_point_sample(xyz.detach().numpy(), npoint)))
    ext.farthest_point_sampling_wrapper = farthest_point_sampling_wrapper
    import gen_roi_fixtures as grf
    grf.install_reference()
    stack = sys.modules['pcdet.ops.pointnet2.pointnet2_stack']
    stack.__path__ = [f'{REF}/pcdet/ops/pointnet2/pointnet2_stack']
    sys.modules['pcdet.ops.pointnet2'].pointnet2_stack = stack
    for name, path in (('pcdet.models.backbones_3d', 'models/backbones_3d'), ('pcdet.models.backbones_3d.pfe', 'models/backbones_3d/pfe'),
                       ('pcdet.models.dense_heads', 'models/dense_heads')):      # package __init__s not run (they import spconv)
        if name not in sys.modules:
            m = types.ModuleType(name)
            m.__path__ = [f'{REF}/pcdet/{path}']
            sys.modules[name] = m
    from pcdet.models.backbones_3d.pfe import voxel_set_abstraction
    from pcdet.models.dense_heads import point_head_simple
    from pcdet.models.roi_heads import pvrcnn_head
    return voxel_set_abstraction, point_head_simple, pvrcnn_head, grf.EasyDict


def sparse(level):
    return types.SimpleNamespace(indices=torch.from_numpy(level['indices']), features=torch.from_numpy(level['features']),
                                 spatial_shape=None, batch_size=case.B)


def run_front(vsa, head, pts, levels, bev):
    bd = {'batch_size': case.B, 'points': torch.from_numpy(pts), 'spatial_features': torch.from_numpy(bev),
          'spatial_features_stride': case.BEV_STRIDE, 'multi_scale_3d_features': {k: sparse(v) for k, v in levels.items()}}
    with torch.no_grad():
        bd = head(vsa(bd))
    return bd


def run_head(head, front, rois, noise=None):
    G = head.model_cfg.ROI_GRID_POOL.GRID_SIZE
    keep = head.get_global_grid_points_of_roi
    if noise is not None:
        head.get_global_grid_points_of_roi = lambda r, grid_size: tuple(
            t + torch.from_numpy(noise).view(t.shape) if j == 0 else t for j, t in enumerate(keep(r, grid_size=grid_size)))
    bd = {k: front[k] for k in ('batch_size', 'point_coords', 'point_features', 'point_cls_scores')}
    bd.update(rois=torch.from_numpy(rois.copy()), roi_labels=torch.ones(rois.shape[:2], dtype=torch.long))
    got = {}
    try:
        with torch.no_grad():
            hook = head.roi_grid_pool_layer.register_forward_hook(lambda m, i, out: got.__setitem__('pooled', out[1].numpy()))
            pooled = head.roi_grid_pool(bd)
            hook.remove()
            R = pooled.shape[0]
            shared = head.shared_fc_layer(pooled.permute(0, 2, 1).contiguous().view(R, -1, 1))
            got['rcnn_cls'] = head.cls_layers(shared).transpose(1, 2).contiguous().squeeze(dim=1).numpy()
            got['rcnn_reg'] = head.reg_layers(shared).transpose(1, 2).contiguous().squeeze(dim=1).numpy()
            bd = head(bd)
    finally:
        head.get_global_grid_points_of_roi = keep
    got.update(batch_cls_preds=bd['batch_cls_preds'].numpy(), batch_box_preds=bd['batch_box_preds'].numpy())
    assert bd['cls_preds_normalized'] is False and G ** 3 * rois.shape[0] * rois.shape[1] == got['pooled'].shape[0]
    return got


def main():
    vsa_mod, phs_mod, pvh_mod, EasyDict = install_reference()
    out, manifest, seeds = {}, {}, {}
    bev = case.bev_features()

    vsa = vsa_mod.VoxelSetAbstraction(model_cfg=EasyDict(case.pfe_cfg()), voxel_size=case.VOXEL, point_cloud_range=case.RANGE,
                                      num_bev_features=case.BEV_SHAPE[0], num_rawpoint_features=case.NUM_RAWPOINT_FEATURES).eval()
    assert vsa.num_point_features_before_fusion == case.NUM_BEFORE_FUSION
    point_head = phs_mod.PointHeadSimple(num_class=1, input_channels=case.NUM_BEFORE_FUSION, model_cfg=EasyDict(case.POINT_HEAD_CFG)).eval()
    case.fill_module(vsa, 11)
    case.fill_module(point_head, 12)
    vstate = {k: v.numpy() for k, v in vsa.state_dict().items()}
    sa_cfg = case.PFE_CFG['SA_LAYER']

    def sources(pts, levels, kp_rows):
        """(name, state prefix, cfg, xyz, counts, features) of every set-abstraction source in the reference's column order"""
        new_xyz = pts[kp_rows.reshape(-1), 1:4]
        yield 'raw_points', 'SA_rawpoints.', sa_cfg['raw_points'], pts[:, 1:4], np.array(case.COUNTS), pts[:, 4:], new_xyz
        for k, name in enumerate(vsa.SA_layer_names):
            lv = levels[name]
            xyz = lv['indices'][:, [3, 2, 1]].astype(np.float32)
            xyz = ((xyz + np.float32(0.5)) * (np.float32(case.VOXEL) * np.float32(lv['stride'])) + np.float32(case.RANGE[:3])).astype(np.float32)
            yield name, f'SA_layers.{k}.', sa_cfg[name], xyz, np.bincount(lv['indices'][:, 0], minlength=case.B), lv['features'], new_xyz

    seed = 700
    while True:
        pts = case.points(seed)
        levels = case.levels(pts)
        kp_rows = pr.keypoint_rows(pts, case.COUNTS, case.NUM_KEYPOINTS)
        ok = True
        for name, prefix, cfg, xyz, cnt, feats, new_xyz in sources(pts, levels, kp_rows):
            for radius in cfg['POOL_RADIUS']:
                _, empty, sizes, clear = pr.ball_query(radius, 16, xyz, cnt, new_xyz, [case.NUM_KEYPOINTS] * case.B)
                ok = ok and clear >= CLEAR
        if ok:
            break
        seed += 1
        assert seed < 760, 'no clear case in 60 seeds'
    seeds['points'] = seed
    front = run_front(vsa, point_head, pts, levels, bev)
    kp = front['point_coords'].numpy()
    assert np.array_equal(kp[:, 1:4], pts[kp_rows.reshape(-1), 1:4]), 'keypoint rows: the restatement against the reference'
    before, fused_f = front['point_features_before_fusion'].numpy(), front['point_features'].numpy()
    mine_bev = pr.bev_interpolate(kp, bev, case.RANGE, case.VOXEL, case.BEV_STRIDE)
    assert np.array_equal(mine_bev, before[:, :case.BEV_SHAPE[0]]), 'bev: the restatement against the reference, bit for bit'
    col = case.BEV_SHAPE[0]
    mine_before = [mine_bev.astype(np.float64)]
    for name, prefix, cfg, xyz, cnt, feats, new_xyz in sources(pts, levels, kp_rows):
        y, idxs, empties, sizes, _ = pr.sa_msg(vstate, prefix, cfg['POOL_RADIUS'], cfg['NSAMPLE'], xyz, cnt, new_xyz, [case.NUM_KEYPOINTS] * case.B, feats)
        err = float(np.abs(y - before[:, col:col + y.shape[1]]).max())
        print(f'{name}: restatement against the reference {err:.3g}; ball sizes', [np.bincount(np.minimum(s, 17), minlength=18).tolist() for s in sizes])
        assert err <= 2e-5, err
        for s, (i, e) in enumerate(zip(idxs, empties)):
            out[f'{name}.idx{s}'], out[f'{name}.empty{s}'] = i, e
        mine_before.append(y)
        col += y.shape[1]
    mine_fused = pr.linear_bn_relu(np.concatenate(mine_before, 1), vstate, 'vsa_point_feature_fusion.')
    err = float(np.abs(mine_fused - fused_f).max())
    print(f'fusion: restatement against the reference {err:.3g}; scores', front['point_cls_scores'].numpy()[:4])
    assert err <= 2e-5, err

    out.update(points=pts, bev=bev, keypoint_rows=kp_rows, point_coords=kp, point_features_before_fusion=before, point_features=fused_f,
               point_cls_scores=front['point_cls_scores'].numpy())
    for name, lv in levels.items():
        out[f'{name}.indices'], out[f'{name}.features'] = lv['indices'], lv['features']
    for k, v in vsa.state_dict().items():
        out['pfe.state.' + k] = v.numpy()
    for k, v in point_head.state_dict().items():
        out['point_head.state.' + k] = v.numpy()
    manifest['VoxelSetAbstraction(reduced: tests/pv_rcnn_case.py PFE_CFG)'] = {k: list(v.shape) for k, v in vsa.state_dict().items()}
    manifest['PointHeadSimple(reduced: tests/pv_rcnn_case.py POINT_HEAD_CFG, num_class=1)'] = {k: list(v.shape) for k, v in point_head.state_dict().items()}

    counts = [case.NUM_KEYPOINTS] * case.B
    for G in case.GRID_SIZES:
        head = pvh_mod.PVRCNNHead(input_channels=case.PFE_CFG['NUM_OUTPUT_FEATURES'], model_cfg=EasyDict(case.head_cfg(G)), num_class=1).eval()
        case.fill_module(head, 100 + G)
        manifest[f'PVRCNNHead(reduced: tests/pv_rcnn_case.py HEAD_CFG, GRID_SIZE={G}, num_class=1)'] = {k: list(v.shape) for k, v in head.state_dict().items()}
        for k, v in head.state_dict().items():
            out[f'g{G}.state.' + k] = v.numpy()
        pool = case.HEAD_CFG['ROI_GRID_POOL']

        def geometry_ok(rois):
            g = pr.grid_points(rois, G)
            for radius in pool['POOL_RADIUS']:
                _, empty, sizes, clear = pr.ball_query(radius, 16, kp[:, 1:4], counts, g, [rois.shape[1] * G ** 3] * case.B)
                if clear < CLEAR:
                    return False
            return True

        def stable(rois):
            base = run_head(head, front, rois)
            worst = 0.0
            for trial in range(4):
                noise = ((np.random.default_rng(trial).random((rois.shape[0] * rois.shape[1], G ** 3, 3)) * 2 - 1) * 2e-5).astype(np.float32)
                got = run_head(head, front, rois, noise)
                worst = max(worst, *(float(np.abs(got[k] - base[k]).max()) for k in ('rcnn_cls', 'rcnn_reg', 'batch_box_preds')))
            return worst < 1e-4, worst

        seed = 500 + 100 * G
        while True:
            rois = case.rois(np.random.default_rng(seed))
            if geometry_ok(rois):
                ok, worst = stable(rois)
                if ok:
                    break
            seed += 1
            assert seed < 500 + 100 * G + 60, 'no stable case in 60 seeds'
        seeds[f'g{G}'] = seed
        res = run_head(head, front, rois)
        out[f'g{G}.rois'] = rois
        for k, v in res.items():
            out[f'g{G}.{k}'] = v
        hstate = {k: v.numpy() for k, v in head.state_dict().items()}
        weighted = (front['point_features'] * front['point_cls_scores'].view(-1, 1)).numpy()
        y, idxs, empties, sizes, _ = pr.sa_msg(hstate, 'roi_grid_pool_layer.', pool['POOL_RADIUS'], pool['NSAMPLE'], kp[:, 1:4], counts,
                                              pr.grid_points(rois, G), [rois.shape[1] * G ** 3] * case.B, weighted)
        err = float(np.abs(y - res['pooled']).max())
        for s, (i, e) in enumerate(zip(idxs, empties)):
            out[f'g{G}.idx{s}'], out[f'g{G}.empty{s}'] = i, e
        print(f'G={G}: seed {seed}, pooled restatement against the reference {err:.3g}, outputs move by {worst:.3g} under +-2e-5; rcnn_cls',
              res['rcnn_cls'].ravel()[:4], 'ball sizes', [np.bincount(np.minimum(s, 17), minlength=18).tolist() for s in sizes])
        assert err <= 2e-5, err

    # the full-size manifests
    from pdm_ssd_amd import detector_config as dc
    full = json.loads(json.dumps(dc.PV_RCNN_CFG))
    full_vsa = vsa_mod.VoxelSetAbstraction(model_cfg=EasyDict(full['PFE']), voxel_size=dc.VOXEL_SIZE, point_cloud_range=case.RANGE,
                                           num_bev_features=256, num_rawpoint_features=4)
    manifest['VoxelSetAbstraction(PV_RCNN_CFG, 256 bev features, 4 raw point features)'] = {k: list(v.shape) for k, v in full_vsa.state_dict().items()}
    full_ph = phs_mod.PointHeadSimple(num_class=1, input_channels=full_vsa.num_point_features_before_fusion,
                                      model_cfg=EasyDict(dict(full['POINT_HEAD'], LOSS_CONFIG=case.POINT_HEAD_CFG['LOSS_CONFIG'])))
    manifest['PointHeadSimple(PV_RCNN_CFG, num_class=1)'] = {k: list(v.shape) for k, v in full_ph.state_dict().items()}
    full_head = pvh_mod.PVRCNNHead(input_channels=128, model_cfg=EasyDict(dict(full['ROI_HEAD'], LOSS_CONFIG=case.HEAD_CFG['LOSS_CONFIG'])), num_class=1)
    manifest['PVRCNNHead(PV_RCNN_CFG, 128 point features, num_class=1)'] = {k: list(v.shape) for k, v in full_head.state_dict().items()}
    manifest['seeds'] = seeds
    np.savez_compressed(os.path.join(HERE, 'ref_pv_rcnn.npz'), **out)
    with open(os.path.join(HERE, 'ref_pv_rcnn_manifest.json'), 'w') as f:
        json.dump(manifest, f, indent=1, sort_keys=True)
    for n in ('ref_pv_rcnn.npz', 'ref_pv_rcnn_manifest.json'):
        print(n, os.path.getsize(os.path.join(HERE, n)), 'bytes')


if __name__ == '__main__':
    main()

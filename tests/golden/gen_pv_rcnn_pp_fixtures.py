#!/usr/bin/env python3
"""Generates tests/golden/ref_pv_rcnn_pp.npz and ref_pv_rcnn_pp_manifest.json by running the REFERENCE's own VoxelSetAbstraction
(pcdet/models/backbones_3d/pfe/voxel_set_abstraction.py: SAMPLE_METHOD SPC, FILTER_NEIGHBOR_WITH_ROI, VectorPool sources),
PointHeadSimple and PVRCNNHead (VectorPool ROI_GRID_POOL) on the CPU, imported from where they lie, nothing copied, over the stubs
of gen_vector_pool_fixtures.py (the native pointnet2_stack_cuda by this repository's CPU oracle) and gen_pv_rcnn_fixtures.py
(SharedArray / numba / iou3d_nms by empty modules, `.cuda()` by the identity).  Run in the authoring container only; the outputs
hold numbers and key names only.

Two parts:
  * the operator cases of tests/pv_rcnn_pp_case.py (partition_case: counts [300, 37, 0] and [700, 37, 0, 1500], S = 6, K = 50):
    the reference's sample_points_with_roi + sector_fps per non-empty sample -> the keypoints, and the sector index the reference
    gives the planted point (-3, 0.0, z).  The numpy restatement (tests/pv_rcnn_pp_reference.py) is held to them: bit-equal.
  * the module case (pv_rcnn_pp_case.PFE_CFG / HEAD_CFG on pv_rcnn_case's geometry, B = 3, 5 rois a sample with an all-zero row).
Reject-sampled (seeds recorded): |d_min - (roi_max_dim + r)| >= 1e-4 for every point of every source and every radius used on it,
a second-nearest roi within 1e-4 gives the same verdict, angle / SIZE at least 1e-4 from an integer for every raw point, and for
the StackSAModuleMSG source the ball clearance of gen_pv_rcnn_fixtures.py.
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
import gen_vector_pool_fixtures as gvp  # noqa: E402
import pv_rcnn_case as pcase  # noqa: E402
import pv_rcnn_pp_case as case  # noqa: E402
import pv_rcnn_pp_reference as ppr  # noqa: E402
import pv_rcnn_reference as pr  # noqa: E402

REF = gsf.REF
o = gsf.o
CLEAR = 2e-4        # on squared distances: 1e-4 of the radius


def install_reference():
    gvp.install_vector_pool_stubs()                     # pcdet.ops.pointnet2.pointnet2_stack + every stub of its extension
    ext = sys.modules['pcdet.ops.pointnet2.pointnet2_stack.pointnet2_stack_cuda']
    stack = sys.modules['pcdet.ops.pointnet2.pointnet2_stack']
    import gen_roi_fixtures as grf
    grf.install_reference()
    stack.__path__ = [f'{REF}/pcdet/ops/pointnet2/pointnet2_stack']
    sys.modules['pcdet.ops.pointnet2.pointnet2_stack'] = stack
    sys.modules[ext.__name__] = ext
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


def operator_cases(vsa_mod, out):
    for tag, counts in (('small', case.SMALL), ('large', case.LARGE)):
        xyz, counts, rois = case.partition_case(counts)
        got, start = [], 0
        for b, n in enumerate(counts):
            if n:
                kept, _ = vsa_mod.sample_points_with_roi(torch.from_numpy(rois[b]), torch.from_numpy(xyz[start:start + n]), case.RADIUS)
                got.append(vsa_mod.sector_fps(kept, case.K, case.S).numpy())
            else:
                got.append(np.zeros((0, 3), np.float32))
            start += n
        mine, rows, per = ppr.keypoints(xyz, counts, rois, case.RADIUS, case.S, case.K)
        assert [len(g) for g in got] == per.tolist(), ([len(g) for g in got], per)
        assert np.array_equal(np.concatenate(got), mine), f'{tag}: the restatement against the reference, bit for bit'
        out[f'op.{tag}.keypoints'], out[f'op.{tag}.rows'], out[f'op.{tag}.per'] = mine, rows.astype(np.int32), per
        print(f'operator case {tag}: keypoints a sample {per.tolist()}')
    axis = torch.tensor([case.AXIS_POINT], dtype=torch.float32)
    angle = torch.atan2(axis[:, 1], axis[:, 0]) + np.pi
    idx = int((angle / (np.pi * 2 / case.S)).floor().clamp(min=0, max=case.S)[0])
    assert idx == int(ppr.sector_index(axis.numpy(), case.S)[0][0])
    out['op.axis_sector'] = np.int32(idx)
    print('the reference gives the axis point sector index', idx, '(S = dropped)' if idx == case.S else '')


def main():
    vsa_mod, phs_mod, pvh_mod, EasyDict = install_reference()
    out, manifest, seeds = {}, {}, {}
    operator_cases(vsa_mod, out)
    bev = pcase.bev_features()

    vsa = vsa_mod.VoxelSetAbstraction(model_cfg=EasyDict(case.pfe_cfg()), voxel_size=case.VOXEL, point_cloud_range=case.RANGE,
                                      num_bev_features=case.BEV_SHAPE[0], num_rawpoint_features=case.NUM_RAWPOINT_FEATURES).eval()
    assert vsa.num_point_features_before_fusion == case.NUM_BEFORE_FUSION, vsa.num_point_features_before_fusion
    point_head = phs_mod.PointHeadSimple(num_class=1, input_channels=case.NUM_BEFORE_FUSION, model_cfg=EasyDict(case.POINT_HEAD_CFG)).eval()
    head = pvh_mod.PVRCNNHead(input_channels=case.PFE_CFG['NUM_OUTPUT_FEATURES'], model_cfg=EasyDict(case.head_cfg()), num_class=1).eval()
    pcase.fill_module(vsa, 21)
    pcase.fill_module(point_head, 22)
    pcase.fill_module(head, 23)
    sa1 = case.PFE_CFG['SA_LAYER']['x_conv1']

    seed = 900
    while True:
        pts = pcase.points(seed)
        levels = pcase.levels(pts)
        rois = pcase.rois(np.random.default_rng(seed))
        ok = case.partition_is_clear(pts[:, 1:4], case.COUNTS, rois, case.RADIUS, True)
        ok = ok and case.partition_is_clear(pts[:, 1:4], case.COUNTS, rois, case.FILTER_RADII['raw_points'], False)
        lv = levels['x_conv3']
        ok = ok and case.partition_is_clear(case.level_xyz(lv), np.bincount(lv['indices'][:, 0], minlength=case.B), rois,
                                            case.FILTER_RADII['x_conv3'], False)
        if ok:
            kp, rows, per = ppr.keypoints(pts[:, 1:4], case.COUNTS, rois, case.RADIUS, case.S, case.K)
            l1 = levels['x_conv1']
            for radius in sa1['POOL_RADIUS']:
                _, _, _, clear = pr.ball_query(radius, 16, case.level_xyz(l1), np.bincount(l1['indices'][:, 0], minlength=case.B), kp, per.tolist())
                ok = ok and clear >= CLEAR
        if ok:
            break
        seed += 1
        assert seed < 1100, 'no clear case in 200 seeds'
    seeds['points_and_rois'] = seed
    bd = {'batch_size': case.B, 'points': torch.from_numpy(pts), 'spatial_features': torch.from_numpy(bev),
          'spatial_features_stride': case.BEV_STRIDE, 'multi_scale_3d_features': {k: sparse(v) for k, v in levels.items()},
          'rois': torch.from_numpy(rois.copy()), 'roi_labels': torch.ones(rois.shape[:2], dtype=torch.long)}
    got = {}
    with torch.no_grad():
        bd = point_head(vsa(bd))
        hook = head.roi_grid_pool_layer.register_forward_hook(lambda m, i, res: got.__setitem__('pooled', res[1].numpy()))
        pooled = head.roi_grid_pool(bd)
        hook.remove()
        R = pooled.shape[0]
        shared = head.shared_fc_layer(pooled.permute(0, 2, 1).contiguous().view(R, -1, 1))
        got['rcnn_cls'] = head.cls_layers(shared).transpose(1, 2).contiguous().squeeze(dim=1).numpy()
        got['rcnn_reg'] = head.reg_layers(shared).transpose(1, 2).contiguous().squeeze(dim=1).numpy()
        bd = head(bd)
    got.update(batch_cls_preds=bd['batch_cls_preds'].numpy(), batch_box_preds=bd['batch_box_preds'].numpy())
    coords = bd['point_coords'].numpy()
    assert np.array_equal(coords[:, 1:4], kp) and np.array_equal(np.bincount(coords[:, 0].astype(np.int64), minlength=case.B), per), \
        'keypoints: the restatement against the reference, bit for bit'
    part = ppr.partition(pts[:, 1:4], case.COUNTS, rois, case.RADIUS, case.S, case.K)
    print(f'module case: seed {seed}; kept {part["kept_cnt"].tolist()} of {list(case.COUNTS)}, sector counts {part["seg_cnt"].reshape(case.B, -1).tolist()}, '
          f'keypoints {per.tolist()}; rcnn_cls', got['rcnn_cls'].ravel()[:4])
    for name, radius in case.FILTER_RADII.items():
        xyz = pts[:, 1:4] if name == 'raw_points' else case.level_xyz(levels[name])
        cnt = case.COUNTS if name == 'raw_points' else np.bincount(levels[name]['indices'][:, 0], minlength=case.B)
        print(f'  filter {name} r = {radius}: kept', ppr.partition(xyz, cnt, rois, radius, 0, 1, fallback=False)['seg_cnt'].tolist(), 'of', list(cnt))

    out.update(points=pts, bev=bev, rois=rois, keypoint_rows=rows, keypoint_cnt=per, point_coords=coords,
               point_features_before_fusion=bd['point_features_before_fusion'].numpy(), point_features=bd['point_features'].numpy(),
               point_cls_scores=bd['point_cls_scores'].numpy(), **got)
    for name, lv in levels.items():
        out[f'{name}.indices'], out[f'{name}.features'] = lv['indices'], lv['features']
    for prefix, module, title in (('pfe.state.', vsa, 'VoxelSetAbstraction(reduced: tests/pv_rcnn_pp_case.py PFE_CFG)'),
                                  ('point_head.state.', point_head, 'PointHeadSimple(reduced: tests/pv_rcnn_pp_case.py POINT_HEAD_CFG, num_class=1)'),
                                  ('head.state.', head, 'PVRCNNHead(reduced: tests/pv_rcnn_pp_case.py HEAD_CFG, num_class=1)')):
        for k, v in module.state_dict().items():
            out[prefix + k] = v.numpy()
        manifest[title] = {k: list(v.shape) for k, v in module.state_dict().items()}

    # the full-size manifests
    from pdm_ssd_amd import detector_config as dc
    full = json.loads(json.dumps(dc.PV_RCNN_PP_CFG))
    full_vsa = vsa_mod.VoxelSetAbstraction(model_cfg=EasyDict(full['PFE']), voxel_size=dc.VOXEL_SIZE, point_cloud_range=case.RANGE,
                                           num_bev_features=256, num_rawpoint_features=4)
    manifest['VoxelSetAbstraction(PV_RCNN_PP_CFG, 256 bev features, 4 raw point features)'] = {k: list(v.shape) for k, v in full_vsa.state_dict().items()}
    full_head = pvh_mod.PVRCNNHead(input_channels=90, model_cfg=EasyDict(dict(full['ROI_HEAD'], LOSS_CONFIG=pcase.HEAD_CFG['LOSS_CONFIG'])), num_class=1)
    manifest['PVRCNNHead(PV_RCNN_PP_CFG, 90 point features, num_class=1)'] = {k: list(v.shape) for k, v in full_head.state_dict().items()}
    manifest['seeds'] = seeds
    np.savez_compressed(os.path.join(HERE, 'ref_pv_rcnn_pp.npz'), **out)
    with open(os.path.join(HERE, 'ref_pv_rcnn_pp_manifest.json'), 'w') as f:
        json.dump(manifest, f, indent=1, sort_keys=True)
    for n in ('ref_pv_rcnn_pp.npz', 'ref_pv_rcnn_pp_manifest.json'):
        print(n, os.path.getsize(os.path.join(HERE, n)), 'bytes')


if __name__ == '__main__':
    main()

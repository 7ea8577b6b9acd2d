#!/usr/bin/env python3
"""Generates tests/golden/ref_voxel_rcnn.npz and ref_voxel_rcnn_manifest.json by running the REFERENCE's own
NeighborVoxelSAModuleMSG (pcdet/ops/pointnet2/pointnet2_stack/voxel_pool_modules.py) and VoxelRCNNHead
(pcdet/models/roi_heads/voxelrcnn_head.py) on the CPU, imported from where they lie, nothing copied, with only what the
authoring image lacks replaced:
  - the native pointnet2_stack_cuda by a stub: voxel_query_wrapper over this repository's CPU oracle (stack_voxel_query, as
    gen_vector_pool_fixtures.py) and group_points_wrapper by a numpy gather written here,
  - SharedArray / numba / iou3d_nms by empty modules and `.cuda()` by the identity (gen_roi_fixtures.install_reference),
  - spconv by a namespace holding the three attributes the head reads from a sparse tensor.
Run in the authoring container only; the outputs hold numbers and key names only.

The case is tests/voxel_rcnn_case.py: b1_voxels carried through the numpy rulebook to strides 2, 4, 8, B = 3 with sample 1
empty, 5 rois a sample (zero padding row, a box partly below the range minimum, one over the far border, headings 0 and
random), a reduced head at GRID_SIZE 2 and 3.

Reject-sampled, so that no test rests on a last-ulp difference between the host's and the device's cosf / sinf (seeds recorded):
  - no grid coordinate within 1e-3 of a cell boundary at any pooled stride (in units of that level's cells; the all-zero
    padding rois are exempt: their grid points are (0, 0, 0) exactly on host and device alike),
  - no voxel centre within 1e-4 radius of a query sphere,
  - the head's outputs move by less than 1e-4 when the grid points are perturbed by +-2e-5.
main() also holds the numpy restatement (tests/voxel_rcnn_reference.py) to the reference's pooled features within 2e-5.
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
import gen_vector_pool_fixtures as gvp  # noqa: E402
import voxel_rcnn_case as case  # noqa: E402
import voxel_rcnn_reference as vr  # noqa: E402

REF = gvp.base.REF


def install_reference():
    gvp.install_vector_pool_stubs()
    ext = sys.modules['pcdet.ops.pointnet2.pointnet2_stack.pointnet2_stack_cuda']

    def group_points_wrapper(B, M, C, nsample, features, features_batch_cnt, idx, idx_batch_cnt, out):
        f, i = features.detach().numpy(), idx.detach().numpy()
        first = np.concatenate([[0], np.cumsum(features_batch_cnt.numpy())])[:-1]
        sample = np.repeat(np.arange(len(first)), idx_batch_cnt.numpy())
        out.copy_(torch.from_numpy(f[first[sample][:, None] + i].transpose(0, 2, 1).copy()))
    ext.group_points_wrapper = group_points_wrapper
    import gen_roi_fixtures as grf
    grf.install_reference()
    stack = sys.modules['pcdet.ops.pointnet2.pointnet2_stack']
    stack.__path__ = [f'{REF}/pcdet/ops/pointnet2/pointnet2_stack']
    sys.modules['pcdet.ops.pointnet2'].pointnet2_stack = stack
    from pcdet.models.roi_heads import voxelrcnn_head
    from pcdet.ops.pointnet2.pointnet2_stack import voxel_pool_modules
    return voxelrcnn_head, voxel_pool_modules, grf.EasyDict


def sparse(level, features):
    return types.SimpleNamespace(indices=torch.from_numpy(level['indices']), features=torch.from_numpy(features),
                                 spatial_shape=list(level['shape']), batch_size=case.B)


def make_head(vrh, EasyDict, grid_size):
    head = vrh.VoxelRCNNHead(backbone_channels=dict(case.BACKBONE_CHANNELS), model_cfg=EasyDict(case.head_cfg(grid_size)),
                             point_cloud_range=case.RANGE, voxel_size=case.VOXEL, num_class=1).eval()
    case.fill_module(head, 100 + grid_size)
    return head


def run_head(head, rois, levels, feats, noise=None):
    got = {}
    hooks = [layer.register_forward_hook(lambda m, i, out, k=k: got.__setitem__(f'pooled{k}', out.detach().numpy()))
             for k, layer in enumerate(head.roi_grid_pool_layers)]
    keep = head.get_global_grid_points_of_roi
    if noise is not None:
        head.get_global_grid_points_of_roi = lambda r, grid_size: tuple(
            t + torch.from_numpy(noise).view(t.shape) if j == 0 else t for j, t in enumerate(keep(r, grid_size=grid_size)))
    bd = {'batch_size': case.B, 'rois': torch.from_numpy(rois.copy()), 'roi_labels': torch.ones(rois.shape[:2], dtype=torch.long),
          'multi_scale_3d_features': {k: sparse(levels[k], feats[k]) for k in feats},
          'multi_scale_3d_strides': {k: levels[k]['stride'] for k in feats}}
    try:
        with torch.no_grad():
            shared = {}
            h2 = [head.cls_pred_layer.register_forward_hook(lambda m, i, out: shared.__setitem__('rcnn_cls', out.numpy())),
                  head.reg_pred_layer.register_forward_hook(lambda m, i, out: shared.__setitem__('rcnn_reg', out.numpy()))]
            bd = head(bd)
            for h in h2:
                h.remove()
    finally:
        head.get_global_grid_points_of_roi = keep
        for h in hooks:
            h.remove()
    got.update(shared, batch_cls_preds=bd['batch_cls_preds'].numpy(), batch_box_preds=bd['batch_box_preds'].numpy())
    return got


def main():
    vrh, vpm, EasyDict = install_reference()
    levels = case.levels()
    feats = {k: case.level_features(k, len(levels[k]['indices'])) for k in case.HEAD_CFG['ROI_GRID_POOL']['FEATURES_SOURCE']}
    out, manifest, seeds = {}, {}, {}
    for name, lv in levels.items():
        out[f'{name}.indices'], out[f'{name}.shape'] = lv['indices'], np.array(lv['shape'])
        per = np.bincount(lv['indices'][:, 0], minlength=case.B)
        assert per[1] == 0 and per[0] > 0 and per[2] > 0, per
        print(name, 'stride', lv['stride'], 'shape', lv['shape'], 'rows', len(lv['indices']))
    for k, f in feats.items():
        out[f'{k}.features'] = f
    pool_cfg = case.HEAD_CFG['ROI_GRID_POOL']['POOL_LAYERS']

    for G in case.GRID_SIZES:
        head = make_head(vrh, EasyDict, G)
        key = f'VoxelRCNNHead(reduced: tests/voxel_rcnn_case.py HEAD_CFG, GRID_SIZE={G}, num_class=1)'
        manifest[key] = {k: list(v.shape) for k, v in head.state_dict().items()}
        for k, v in head.state_dict().items():
            out[f'g{G}.state.' + k] = v.numpy()

        def geometry_ok(rois):
            pts = vr.grid_points(rois, G)
            real = np.repeat(np.abs(rois.reshape(-1, 7)).sum(1) > 0, G ** 3)
            sample = np.repeat(np.arange(case.B), rois.shape[1] * G ** 3)
            for src in feats:
                lv, cfg = levels[src], pool_cfg[src]
                c = vr.cell_coordinate(pts[real], case.RANGE, case.VOXEL).astype(np.float64) / lv['stride']
                if np.abs(c - np.round(c)).min() < 1e-3:
                    return False
                cell = vr.cells(pts, case.RANGE, case.VOXEL, lv['stride'])
                hits, _, margin = vr.hit_sets(pts, sample, cell, lv['indices'], lv['shape'], lv['stride'], case.VOXEL, case.RANGE,
                                              cfg['QUERY_RANGES'][0], cfg['POOL_RADIUS'][0], cfg['NSAMPLE'][0])
                if margin < 1e-4:
                    return False
                sizes = np.array([len(h) for h in hits])
                if not ((sizes == 0).any() and (sizes == cfg['NSAMPLE'][0]).any()):     # empty groups and full ones
                    return False
            return True

        def stable(rois):
            base = run_head(head, rois, levels, feats)
            worst = 0.0
            for trial in range(4):
                noise = ((np.random.default_rng(trial).random((rois.shape[0] * rois.shape[1], G ** 3, 3)) * 2 - 1) * 2e-5).astype(np.float32)
                got = run_head(head, rois, levels, feats, noise)
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
        seeds[f'g{G}'] = seed
        res = run_head(head, rois, levels, feats)
        out[f'g{G}.rois'] = rois
        for k, v in res.items():
            out[f'g{G}.{k}'] = v
        # the numpy restatement against the reference's own module, level by level
        state = {k: v.numpy() for k, v in head.state_dict().items()}
        for i, src in enumerate(feats):
            lv, cfg = levels[src], pool_cfg[src]
            mine, hits = vr.module_forward(state, f'roi_grid_pool_layers.{i}.', 0, rois, G, lv['indices'], feats[src], lv['shape'], lv['stride'],
                                           case.VOXEL, case.RANGE, cfg['QUERY_RANGES'][0], cfg['POOL_RADIUS'][0], cfg['NSAMPLE'][0])
            err = float(np.abs(mine - res[f'pooled{i}']).max())
            sizes = np.bincount([len(h) for h in hits], minlength=cfg['NSAMPLE'][0] + 1)
            print(f'G={G} {src}: restatement against the reference {err:.3g}; group sizes {sizes.tolist()}')
            assert err <= 2e-5, err
        print(f'G={G}: seed {seed}, outputs move by {worst:.3g} under +-2e-5; rcnn_cls', res['rcnn_cls'].ravel()[:4])

    # the full-size head and detector manifests
    from pdm_ssd_amd import detector_config as dc
    full = EasyDict(dict(dc.VOXEL_RCNN_CFG['ROI_HEAD'], LOSS_CONFIG=case.HEAD_CFG['LOSS_CONFIG']))
    full_head = vrh.VoxelRCNNHead(backbone_channels={'x_conv1': 16, 'x_conv2': 32, 'x_conv3': 64, 'x_conv4': 64}, model_cfg=EasyDict(
        json.loads(json.dumps(full))), point_cloud_range=case.RANGE, voxel_size=case.VOXEL, num_class=1)
    manifest['VoxelRCNNHead(VOXEL_RCNN_CFG, VoxelBackBone8x channels, num_class=1)'] = {k: list(v.shape) for k, v in full_head.state_dict().items()}
    manifest['seeds'] = seeds
    np.savez_compressed(os.path.join(HERE, 'ref_voxel_rcnn.npz'), **out)
    with open(os.path.join(HERE, 'ref_voxel_rcnn_manifest.json'), 'w') as f:
        json.dump(manifest, f, indent=1, sort_keys=True)
    for n in ('ref_voxel_rcnn.npz', 'ref_voxel_rcnn_manifest.json'):
        print(n, os.path.getsize(os.path.join(HERE, n)), 'bytes')


if __name__ == '__main__':
    main()

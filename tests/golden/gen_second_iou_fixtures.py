#!/usr/bin/env python3
"""Generates tests/golden/ref_second_iou.npz and ref_second_iou_manifest.json by running the REFERENCE's own SECONDHead
(pcdet/models/roi_heads/second_head.py) on the CPU, imported from where it lies, nothing copied, through
gen_roi_fixtures.install_reference (SharedArray / numba / iou3d by empty modules, `.cuda()` by the identity).  Run in the authoring
container only; the outputs hold numbers and key names only.

The case: a map of C = 16 channels on H x W = 13 x 9 cells of 0.4 m, B = 2 samples of n = 6 rois (bev_crop_reference.make_rois:
inside, across each border, wholly outside, a padding row), GRID_SIZE 7, SHARED_FC and IOU_FC [32, 32], DP_RATIO 0.3, seeded
parameters.  Held: the inputs, roi_grid_pool's output, rcnn_iou in eval mode, the state_dict, the four IOU_LOSS values for fixed
logits and labels (one label -1), and the key manifests with and without dropout.

'focalbce' calls loss_utils.sigmoid_focal_cls_loss, which the reference's loss_utils does not define: the generator supplies it
from the reference's OWN SigmoidFocalClassificationLoss (default gamma and alpha, unit weights), which is what the name says.

delta (bev_crop_reference.py): head.affine_grid is wrapped to record the grid the reference builds; per crop case of
tests/test_bev_roi_crop_gpu.py the largest deviation of its pixel positions (grid_sample's fp32 un-normalisation
((g + 1) / 2) * (size - 1)) from bev_crop_reference.positions64, over the positions within one cell of the map (where a value can
be non-zero), in units of 2^-24 max(H, W): 'delta.units.<case>'.
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import bev_crop_reference as bcr  # noqa: E402

HEAD_CFG = {'CLASS_AGNOSTIC': True, 'SHARED_FC': [32, 32], 'IOU_FC': [32, 32], 'DP_RATIO': 0.3,
            'ROI_GRID_POOL': {'GRID_SIZE': 7, 'IN_CHANNEL': 16, 'DOWNSAMPLE_RATIO': bcr.RATIO},
            'TARGET_CONFIG': {'BOX_CODER': 'ResidualCoder'},
            'NMS_CONFIG': {'TEST': {'NMS_TYPE': 'nms_gpu', 'MULTI_CLASSES_NMS': False, 'NMS_PRE_MAXSIZE': 64, 'NMS_POST_MAXSIZE': 6,
                                    'NMS_THRESH': 0.7}},
            'LOSS_CONFIG': {'IOU_LOSS': 'BinaryCrossEntropy', 'LOSS_WEIGHTS': {'rcnn_iou_weight': 1.5, 'code_weights': [1.0] * 7}}}
LOSS_KINDS = ('BinaryCrossEntropy', 'L2', 'smoothL1', 'focalbce')


def fill_head(head, seed):
    """seeded parameters: small normal weights, BatchNorm with set running statistics (gen_part_a2_fixtures.fill_head's rule)"""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, t in sorted(head.state_dict().items()):
            if name.endswith('num_batches_tracked'):
                continue
            if name.endswith('running_var'):
                t.copy_(torch.rand(t.shape, generator=g) + 0.5)
            elif name.endswith('running_mean'):
                t.copy_(torch.rand(t.shape, generator=g) * 0.4 - 0.2)
            elif t.dim() >= 2:
                t.copy_(torch.randn(t.shape, generator=g) * float(np.sqrt(2.0 / int(np.prod(t.shape[1:])))))
            else:
                t.copy_(torch.rand(t.shape, generator=g) * 0.4 + (0.8 if name.endswith('weight') else -0.2))


def main():
    import gen_roi_fixtures as grf
    grf.install_reference()
    EasyDict = grf.EasyDict
    from pcdet.models.roi_heads import second_head
    from pcdet.utils import loss_utils
    focal = loss_utils.SigmoidFocalClassificationLoss()
    loss_utils.sigmoid_focal_cls_loss = lambda x, t: focal(x, t, torch.ones_like(x))

    def dataset_cfg(H, W):
        return EasyDict({'POINT_CLOUD_RANGE': bcr.pc_range(H, W), 'DATA_PROCESSOR': [EasyDict({'VOXEL_SIZE': bcr.VOXEL})]})

    out, manifest = {}, {}
    H, W = bcr.CASES['small']
    rois, _ = bcr.make_rois(H, W, 2, 6, 7, seed=5)
    feat = bcr.make_map(2, 16, H, W, seed=6)
    head = second_head.SECONDHead(input_channels=16, model_cfg=EasyDict(HEAD_CFG), num_class=1)
    manifest['SECONDHead(IN_CHANNEL=16,GRID_SIZE=7,SHARED_FC=[32,32],IOU_FC=[32,32],DP_RATIO=0.3)'] = \
        {k: list(v.shape) for k, v in head.state_dict().items()}
    plain = second_head.SECONDHead(input_channels=16, model_cfg=EasyDict(dict(HEAD_CFG, DP_RATIO=0)), num_class=1)
    manifest['SECONDHead(IN_CHANNEL=16,GRID_SIZE=7,SHARED_FC=[32,32],IOU_FC=[32,32],DP_RATIO=0)'] = \
        {k: list(v.shape) for k, v in plain.state_dict().items()}
    fill_head(head, 300)
    head.eval()
    for k, v in head.state_dict().items():
        out[f'state.{k}'] = v.numpy()
    bd = {'batch_size': 2, 'rois': torch.from_numpy(rois.copy()), 'roi_labels': torch.ones((2, 6), dtype=torch.long),
          'spatial_features_2d': torch.from_numpy(feat.copy()), 'dataset_cfg': dataset_cfg(H, W)}
    with torch.no_grad():
        pooled = head.roi_grid_pool(bd)
        bd = head(bd)
    assert bd['cls_preds_normalized'] is False and torch.equal(bd['batch_box_preds'], bd['rois'])
    out.update({'rois': rois, 'spatial_features_2d': feat, 'pooled': pooled.numpy(), 'rcnn_iou': bd['batch_cls_preds'].numpy().reshape(12, 1)})

    rng = np.random.default_rng(9)
    logits = rng.normal(0, 2, 12).astype(np.float32)
    labels = rng.uniform(0, 1, 12).astype(np.float32)
    labels[[0, 5]] = [1.0, 0.0]
    labels[7] = -1.0
    out.update({'loss.logits': logits, 'loss.labels': labels, 'loss.weight': np.float64(HEAD_CFG['LOSS_CONFIG']['LOSS_WEIGHTS']['rcnn_iou_weight'])})
    for kind in LOSS_KINDS:
        head.model_cfg.LOSS_CONFIG.IOU_LOSS = kind
        loss, tb = head.get_box_iou_layer_loss({'rcnn_iou': torch.from_numpy(logits).view(12, 1), 'rcnn_cls_labels': torch.from_numpy(labels)})
        out[f'loss.{kind}'] = np.float64(float(loss))
        assert abs(tb['rcnn_loss_iou'] - float(loss)) < 1e-6

    # the reference's own grid against float64, per crop case of the GPU test
    for name, C, G, B, n, stride, seed in bcr.crop_cases():
        if C != 1:
            continue                                           # (the positions do not depend on the channels)
        H, W = bcr.CASES[name]
        probe = second_head.SECONDHead(input_channels=1, model_cfg=EasyDict(dict(HEAD_CFG, ROI_GRID_POOL={
            'GRID_SIZE': G, 'IN_CHANNEL': 1, 'DOWNSAMPLE_RATIO': bcr.RATIO}, SHARED_FC=[8], IOU_FC=[8])), num_class=1)
        grids, build = [], probe.affine_grid
        probe.affine_grid = lambda theta, size: grids.append(build(theta, size)) or grids[-1]
        case_rois, _ = bcr.make_rois(H, W, B, n, stride, seed)
        with torch.no_grad():
            probe.roi_grid_pool({'batch_size': B, 'rois': torch.from_numpy(case_rois), 'spatial_features_2d': torch.zeros((B, 1, H, W)),
                                 'dataset_cfg': dataset_cfg(H, W)})
        grid = torch.cat(grids, dim=0)
        gx = (((grid[..., 0] + 1) / 2) * (W - 1)).numpy().astype(np.float64)
        gy = (((grid[..., 1] + 1) / 2) * (H - 1)).numpy().astype(np.float64)
        r = bcr.pc_range(H, W)
        px, py = bcr.positions64(case_rois, H, W, r[0], r[1], bcr.CELL, bcr.CELL, G)
        near = (px > -1) & (px < W) & (py > -1) & (py < H)
        dev = max(float(np.abs(gx - px)[near].max()), float(np.abs(gy - py)[near].max())) if near.any() else 0.0
        out[f'delta.units.{name}.G{G}.B{B}.n{n}'] = np.float64(dev / (bcr.U * max(H, W)))
    units = {k: float(v) for k, v in out.items() if k.startswith('delta.units.')}
    worst = max(units.values())
    out['delta.units.max'] = np.float64(worst)
    print('delta units per case', {k[12:]: round(v, 2) for k, v in units.items()}, 'max', worst)
    assert worst <= bcr.MEASURED_UNITS < worst + 0.1, f'bev_crop_reference.MEASURED_UNITS = {bcr.MEASURED_UNITS}, measured {worst}'

    np.savez_compressed(os.path.join(HERE, 'ref_second_iou.npz'), **out)
    with open(os.path.join(HERE, 'ref_second_iou_manifest.json'), 'w') as f:
        json.dump(manifest, f, indent=1)
    print('ref_second_iou.npz', os.path.getsize(os.path.join(HERE, 'ref_second_iou.npz')), 'bytes;', {k: float(out[f'loss.{k}']) for k in LOSS_KINDS})


if __name__ == '__main__':
    main()

#!/usr/bin/env python3
"""Generates tests/golden/ref_part_a2.npz and ref_part_a2_manifest.json by running the REFERENCE's own UNetV2
(pcdet/models/backbones_3d/spconv_unet.py), PointIntraPartOffsetHead (pcdet/models/dense_heads/point_intra_part_head.py) and
PartA2FCHead (pcdet/models/roi_heads/partA2_head.py) on the CPU, imported from where they lie, nothing copied, with only what the
authoring image lacks replaced:
  - spconv by gen_sparse_conv_fixtures' dense-convolution stub plus, written here, SparseInverseConv3d over the numpy
    restatement (tests/sparse_conv_reference.rulebook of the paired convolution + tests/part_a2_reference.inverse_conv_reference),
  - the native roiaware pooling by tests/roi_pool_reference.py, SharedArray / numba / iou3d by empty modules and `.cuda()` by the
    identity (gen_roi_fixtures.install_reference, through gen_pv_rcnn_fixtures.install_reference).
Run in the authoring container only; the outputs hold numbers and key names only.

The case: the B1 voxels of tests/sparse_conv_reference.py (grid [21, 16, 40], 3 samples, sample 1 empty) through UNetV2 with
fill_backbone's seeded parameters (the fixture holds their check sum, not the weights), the point head at widths 32, and the RoI
head at POOL_SIZE 3, 32 features, 4 points a cell, FC widths 32 (their state_dicts are in the fixture), 5 rois a sample handed in.
Reject-sampled (seed recorded): no voxel centre within 1e-4 of the box size of a box face or a cell boundary, no point score
within 1e-4 of SEG_MASK_SCORE_THRESH, at least 3 active cells.
"""
import json
import os
import sys

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import part_a2_reference as par  # noqa: E402
import roi_pool_reference as rpr  # noqa: E402
import sparse_conv_reference as scr  # noqa: E402

from part_a2_reference import GEO, POINT_CFG, ROI_CFG, UNET_GAIN, UNET_SEED  # noqa: E402


def install_inverse_conv():
    """SparseInverseConv3d for the stub: the paired SparseConv3d records its input sites and geometry under its indice_key"""
    pt = sys.modules['spconv.pytorch']
    book = {}
    conv_init, conv_forward = pt.SparseConv3d.__init__, pt.SparseConv3d.forward

    def init(self, cin, cout, kernel_size, stride=1, padding=0, bias=True, indice_key=None):
        conv_init(self, cin, cout, kernel_size, stride, padding, bias, indice_key)
        self.indice_key = indice_key

    def forward(self, x):
        book[self.indice_key] = (x.indices.numpy().copy(), x.batch_size, tuple(x.spatial_shape), self.k, self.s, self.p)
        return conv_forward(self, x)
    pt.SparseConv3d.__init__, pt.SparseConv3d.forward = init, forward

    class SparseInverseConv3d(pt.SparseModule):
        def __init__(self, cin, cout, kernel_size, indice_key=None, bias=True):
            super().__init__()
            k = (kernel_size,) * 3 if isinstance(kernel_size, int) else tuple(kernel_size)
            self.weight = nn.Parameter(torch.zeros(cout, *k, cin))
            self.bias = nn.Parameter(torch.zeros(cout)) if bias else None
            self.indice_key = indice_key

        def forward(self, x):
            idx, B, shape, k, s, p = book[self.indice_key]
            out_idx, nbr, _ = scr.rulebook(idx, B, shape, k, s, p, False)
            assert np.array_equal(out_idx, x.indices.numpy()), 'the rows are the paired convolution\'s output rows'
            f = torch.from_numpy(par.inverse_conv_reference(x.features.numpy(), nbr, self.weight.detach().numpy(), len(idx))).to(x.features.dtype)
            if self.bias is not None:
                f = f + self.bias
            return pt.SparseConvTensor(f, torch.from_numpy(idx), shape, B)
    pt.SparseInverseConv3d = SparseInverseConv3d
    pt.conv.SparseInverseConv3d = SparseInverseConv3d


def fill_head(head, seed):
    """seeded parameters of a head: small normal weights, BatchNorm with set running statistics"""
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
                fan_in = int(np.prod(t.shape[1:])) if t.dim() != 5 else 9 * t.shape[-1]
                t.copy_(torch.randn(t.shape, generator=g) * float(np.sqrt(2.0 / fan_in)))
            else:
                t.copy_(torch.rand(t.shape, generator=g) * 0.4 + (0.8 if name.endswith('weight') else -0.2))


def sample_rois(centres_by_sample, seed, S):
    """5 boxes a sample around voxel centres of that sample (sample 1, empty, gets boxes around the origin), reject-sampled"""
    while True:
        rng = np.random.default_rng(seed)
        rois = np.zeros((3, 5, 7), dtype=np.float32)
        ok = True
        for b in range(3):
            pts = centres_by_sample[b]
            pick = pts[rng.integers(0, len(pts), 5)] if len(pts) else np.zeros((5, 3), dtype=np.float32)
            rois[b, :, :3] = pick + rng.uniform(-0.4, 0.4, (5, 3))
            rois[b, :, 3:6] = np.array([3.9, 2.6, 1.56]) * rng.uniform(0.8, 1.2, (5, 3))
            rois[b, :, 6] = rng.uniform(-np.pi, np.pi, 5)
            if len(pts):
                big = float(rois[b, :, 3:6].max())
                ok &= rpr.face_clearance(pts, rois[b]) > 1e-4 * big and rpr.voxel_clearance(pts, rois[b], (S, S, S)) > 1e-4 * S
        if ok:
            return rois, seed
        seed += 1


def main():
    import gen_pv_rcnn_fixtures as gpv
    import gen_sparse_conv_fixtures as gsc
    *_, EasyDict = gpv.install_reference()
    gsc.install_spconv_stub()
    install_inverse_conv()
    from pcdet.models.backbones_3d import spconv_unet
    from pcdet.models.dense_heads import point_intra_part_head
    from pcdet.models.roi_heads import partA2_head
    out, manifest = {}, {}

    coords, feats = scr.b1_voxels(4)
    net = spconv_unet.UNetV2(model_cfg=EasyDict({'RETURN_ENCODED_TENSOR': True}), input_channels=4, grid_size=np.array(scr.B1_GRID),
                             voxel_size=GEO['voxel'], point_cloud_range=GEO['range'])
    manifest['UNetV2(input_channels=4)'] = {k: list(v.shape) for k, v in net.state_dict().items()}
    out['unet.checksum'] = np.float64(scr.fill_backbone(net, UNET_SEED, UNET_GAIN))
    net.eval()
    with torch.no_grad():
        bd = net({'voxel_features': torch.from_numpy(feats), 'voxel_coords': torch.from_numpy(coords), 'batch_size': scr.B1_B})
    enc = bd['encoded_spconv_tensor']
    out.update({'unet.point_features': bd['point_features'].numpy(), 'unet.point_coords': bd['point_coords'].numpy(),
                'unet.encoded.indices': enc.indices.numpy(), 'unet.encoded.features': enc.features.numpy(),
                'unet.encoded.shape': np.array(list(enc.spatial_shape))})
    assert bd['encoded_spconv_tensor_stride'] == 8 and len(enc.features) >= 8 and np.array_equal(bd['point_coords'][:, 0].numpy(), coords[:, 0])

    seed = 0
    while True:
        torch.manual_seed(seed)
        ph = point_intra_part_head.PointIntraPartOffsetHead(num_class=1, input_channels=16, model_cfg=EasyDict(POINT_CFG))
        fill_head(ph, 100 + seed)
        ph.eval()
        with torch.no_grad():
            bd = ph(bd)
        if float((bd['point_cls_scores'] - ROI_CFG['SEG_MASK_SCORE_THRESH']).abs().min()) > 1e-4:
            break
        seed += 1
    manifest['PointIntraPartOffsetHead(num_class=1,input_channels=16,CLS_FC=[32],PART_FC=[32])'] = {k: list(v.shape) for k, v in ph.state_dict().items()}
    out['point_head.seed'] = np.int64(seed)
    for k, v in ph.state_dict().items():
        out[f'point_head.state.{k}'] = v.numpy()
    out.update({'point_head.point_cls_scores': bd['point_cls_scores'].numpy(), 'point_head.point_part_offset': bd['point_part_offset'].numpy()})

    S = ROI_CFG['ROI_AWARE_POOL']['POOL_SIZE']
    xyz = bd['point_coords'].numpy()
    rois, roi_seed = sample_rois([xyz[xyz[:, 0] == b, 1:4] for b in range(3)], 7, S)
    head = partA2_head.PartA2FCHead(input_channels=16, model_cfg=EasyDict(ROI_CFG), num_class=1)
    fill_head(head, 200)
    head.eval()
    manifest['PartA2FCHead(input_channels=16,POOL_SIZE=3,NUM_FEATURES=32,SHARED_FC=[32,32],CLS_FC=[32],REG_FC=[32])'] = \
        {k: list(v.shape) for k, v in head.state_dict().items()}
    for k, v in head.state_dict().items():
        out[f'roi_head.state.{k}'] = v.numpy()
    hb = {k: bd[k] for k in ('batch_size', 'point_coords', 'point_features', 'point_cls_scores', 'point_part_offset')}
    hb.update(rois=torch.from_numpy(rois.copy()), roi_labels=torch.ones(rois.shape[:2], dtype=torch.long))
    with torch.no_grad():
        pooled_part, pooled_rpn = head.roiaware_pool(hb)
        active = par.active_cells(pooled_part.numpy())
        assert np.array_equal(active, pooled_part.sum(dim=-1).nonzero().numpy()) and len(active) >= 3, len(active)
        shared_in = {}
        hook = head.shared_fc_layer.register_forward_hook(lambda m, i, o: shared_in.update(x=o))
        hb = head(hb)
        hook.remove()
    out.update({'roi_head.rois': rois, 'roi_head.roi_seed': np.int64(roi_seed), 'roi_head.coords': active,
                'roi_head.shared': shared_in['x'].numpy()[:, :, 0],
                'roi_head.batch_cls_preds': hb['batch_cls_preds'].numpy(), 'roi_head.batch_box_preds': hb['batch_box_preds'].numpy()})
    assert hb['cls_preds_normalized'] is False
    print('voxels', len(coords), 'encoded sites', len(enc.features), 'active cells', len(active), 'of', 15 * S ** 3, 'seeds', seed, roi_seed)
    np.savez_compressed(os.path.join(HERE, 'ref_part_a2.npz'), **out)
    with open(os.path.join(HERE, 'ref_part_a2_manifest.json'), 'w') as f:
        json.dump(manifest, f, indent=1)
    print('ref_part_a2.npz', os.path.getsize(os.path.join(HERE, 'ref_part_a2.npz')), 'bytes')


if __name__ == '__main__':
    main()

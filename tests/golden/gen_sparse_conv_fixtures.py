#!/usr/bin/env python3
"""Generates tests/golden/ref_sparse_conv.npz and ref_sparse_conv_manifest.json by running the REFERENCE's own DynamicMeanVFE,
VoxelBackBone8x, VoxelResBackBone8x and HeightCompression on the CPU, imported from where they lie, nothing copied (`.cuda()` is
the identity, gen_head_fixtures.install_reference; torch_scatter is gen_pillar_fixtures' stub).  Run in the authoring container
only; the outputs hold numbers and key names only.

spconv is on no machine of this project, so the backbones run over a STUB `spconv` module written here, which imports nothing
from pdm_ssd_amd: a convolution densifies its input and calls torch.nn.functional.conv3d.  A submanifold layer's outputs are
the input sites (padding = kernel // 2, stride 1); a strided layer's are the sites whose receptive field holds an active input
(a convolution of the occupancy with a kernel of ones), numbered in ascending ((b W + x) H + y) D + z.  SparseSequential applies
BatchNorm and ReLU to the active rows only.  The convolution's semantics are therefore pinned by the dense-convolution identity,
not by spconv itself.

Shapes (tests/sparse_conv_reference.py): V1 / V2 for the VFE with C = 5 (C = 4 is its first columns); B1 for the backbones: grid
[21, 16, 40], so z goes 41 -> 21 -> 11 -> 5 -> 2, about 400 voxels.  The fixture holds no weights (two backbones' would be 10 MB):
generator and tests fill them from the same seeds (sparse_conv_reference.fill_backbone) and the fixture holds their check sums.

Parity bound of the backbone tests, 1e-4 absolute: main() runs each backbone in float32 and in float64 and fails unless every
level and spatial_features agree within 2.5e-5, a quarter of the bound, and unless the last level holds at least 8 active sites.
"""
import json
import os
import sys
import types

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import sparse_conv_reference as scr  # noqa: E402
from gen_center_head_fixtures import EasyDict  # noqa: E402
from gen_pillar_fixtures import install_pillar_reference  # noqa: E402

SEEDS = {'VoxelBackBone8x': (41, 1.0), 'VoxelResBackBone8x': (43, 0.5)}       # (seed, gain) of fill_backbone


def _triple(v):
    return (v,) * 3 if isinstance(v, int) else tuple(v)


def install_spconv_stub():
    class SparseConvTensor:
        def __init__(self, features, indices, spatial_shape, batch_size):
            self.features, self.indices, self.spatial_shape, self.batch_size = features, indices, list(spatial_shape), batch_size

        def replace_feature(self, f):
            return SparseConvTensor(f, self.indices, self.spatial_shape, self.batch_size)

        def dense(self):
            i = self.indices.long()
            out = torch.zeros((self.batch_size, *self.spatial_shape, self.features.shape[1]), dtype=self.features.dtype)
            out[i[:, 0], i[:, 1], i[:, 2], i[:, 3]] = self.features
            return out.permute(0, 4, 1, 2, 3).contiguous()

    class SparseModule(nn.Module):
        pass

    class SparseConvolution(SparseModule):
        def __init__(self, cin, cout, kernel_size, stride=1, padding=0, bias=True, indice_key=None, subm=False):
            super().__init__()
            self.k, self.s, self.p, self.subm = _triple(kernel_size), _triple(stride), _triple(padding), subm
            self.weight = nn.Parameter(torch.zeros(cout, *self.k, cin))             # spconv 2.x's layout
            self.bias = nn.Parameter(torch.zeros(cout)) if bias else None

        def forward(self, x):
            w = self.weight.permute(0, 4, 1, 2, 3)
            stride, pad = ((1, 1, 1), tuple(k // 2 for k in self.k)) if self.subm else (self.s, self.p)
            y = F.conv3d(x.dense(), w, None, stride, pad)                           # (B, Cout, D', H', W')
            if self.subm:
                idx = x.indices.long()
            else:
                occ = torch.zeros((x.batch_size, 1, *x.spatial_shape), dtype=y.dtype)
                i = x.indices.long()
                occ[i[:, 0], 0, i[:, 1], i[:, 2], i[:, 3]] = 1
                hit = F.conv3d(occ, torch.ones((1, 1, *self.k), dtype=y.dtype), None, stride, pad)[:, 0] > 0
                idx = torch.nonzero(hit)                                             # (b, z, y, x)
                D, H, W = y.shape[2:]
                idx = idx[torch.argsort(((idx[:, 0] * W + idx[:, 3]) * H + idx[:, 2]) * D + idx[:, 1])]
            f = y[idx[:, 0], :, idx[:, 1], idx[:, 2], idx[:, 3]]
            if self.bias is not None:
                f = f + self.bias
            return SparseConvTensor(f, idx.int(), y.shape[2:], x.batch_size)

    class SubMConv3d(SparseConvolution):
        def __init__(self, cin, cout, kernel_size, stride=1, padding=0, bias=True, indice_key=None):
            super().__init__(cin, cout, kernel_size, 1, padding, bias, indice_key, subm=True)

    class SparseConv3d(SparseConvolution):
        def __init__(self, cin, cout, kernel_size, stride=1, padding=0, bias=True, indice_key=None):
            super().__init__(cin, cout, kernel_size, stride, padding, bias, indice_key, subm=False)

    class SparseSequential(SparseModule, nn.Sequential):
        def forward(self, x):
            for m in self:
                if isinstance(m, SparseModule):
                    x = m(x)
                else:
                    x = x.replace_feature(m(x.features))                             # the active rows only
            return x

    top = types.ModuleType('spconv')
    top.__version__ = '2.1.0'
    top.__path__ = []
    pt = types.ModuleType('spconv.pytorch')
    for cls in (SparseConvTensor, SparseModule, SparseConvolution, SubMConv3d, SparseConv3d, SparseSequential):
        setattr(pt, cls.__name__, cls)
    pt.conv = types.SimpleNamespace(SparseConvolution=SparseConvolution)
    top.pytorch = pt
    sys.modules['spconv'], sys.modules['spconv.pytorch'] = top, pt


def run_backbone(cls, hc_cls, coords, feats, dtype, seed, gain):
    net = cls(model_cfg=EasyDict({}), input_channels=feats.shape[1], grid_size=np.array(scr.B1_GRID))
    checksum = scr.fill_backbone(net, seed, gain)
    net = net.to(dtype).eval()
    with torch.no_grad():
        bd = net({'voxel_features': torch.from_numpy(feats).to(dtype), 'voxel_coords': torch.from_numpy(coords), 'batch_size': scr.B1_B})
        bd = hc_cls(model_cfg=EasyDict({'NUM_BEV_FEATURES': 256}))(bd)
    return net, bd, checksum


def main():
    install_pillar_reference()
    install_spconv_stub()
    from pcdet.models.backbones_2d.map_to_bev import height_compression
    from pcdet.models.backbones_3d import spconv_backbone
    from pcdet.models.backbones_3d.vfe import dynamic_mean_vfe
    out, manifest = {}, {}

    # ---- the VFE ----
    for tag, geo, pts in (('v1', scr.V1, scr.v1_points()), ('v2', scr.V2, scr.v2_points())):
        vfe = dynamic_mean_vfe.DynamicMeanVFE(model_cfg=EasyDict({}), num_point_features=5, voxel_size=geo['voxel'], grid_size=geo['grid'],
                                              point_cloud_range=geo['range'])
        finite = np.isfinite(pts).all(1) & (pts[:, 0] >= 0) & (pts[:, 0] < geo['B'])      # the reference's .int() of NaN / inf is undefined: such rows drop by contract
        with torch.no_grad():
            bd = vfe({'points': torch.from_numpy(pts[finite]), 'batch_size': geo['B']})
        mine = scr.voxel_assign(pts, geo['B'], geo['range'], geo['voxel'], geo['grid'])
        assert (bd['voxel_coords'].numpy() == mine['voxel_coords']).all() and len(bd['voxel_coords']) == len(mine['voxel_coords'])
        assert (np.nonzero(finite)[0][scr.voxel_assign(pts[finite], geo['B'], geo['range'], geo['voxel'], geo['grid'])['kept_idx']] == mine['kept_idx']).all()
        ref_mean = bd['voxel_features'].numpy()
        bound = mine['voxel_count'][:, None] * 2.0 ** -23 * np.abs(mine['mean64']).max() + 2.0 ** -20
        assert (np.abs(ref_mean - mine['mean64']) <= bound + 1e-6).all()
        out.update({f'{tag}.points': pts, f'{tag}.kept_idx': mine['kept_idx'], f'{tag}.unq_inv': mine['unq_inv'],
                    f'{tag}.voxel_coords': bd['voxel_coords'].numpy().astype(np.int32), f'{tag}.voxel_count': mine['voxel_count'],
                    f'{tag}.mean64': mine['mean64']})
        print(tag, 'rows', len(pts), 'kept', len(mine['kept_idx']), 'voxels', len(mine['voxel_count']), 'max count', int(mine['voxel_count'].max()))

    # ---- the backbones ----
    coords, feats = scr.b1_voxels(4)
    out['b1.coords'], out['b1.features'] = coords, feats
    for name, (seed, gain) in SEEDS.items():
        cls = getattr(spconv_backbone, name)
        net, bd, checksum = run_backbone(cls, height_compression.HeightCompression, coords, feats, torch.float32, seed, gain)
        _, bd64, _ = run_backbone(cls, height_compression.HeightCompression, coords, feats, torch.float64, seed, gain)
        manifest[name] = {k: list(v.shape) for k, v in net.state_dict().items()}
        manifest[f'{name}.fill'] = {'seed': seed, 'gain': gain, 'checksum': checksum}
        levels = dict(bd['multi_scale_3d_features'], out=bd['encoded_spconv_tensor'])
        levels64 = dict(bd64['multi_scale_3d_features'], out=bd64['encoded_spconv_tensor'])
        worst = 0.0
        for lv, t in levels.items():
            assert (t.indices == levels64[lv].indices).all()
            worst = max(worst, float((t.features.double() - levels64[lv].features).abs().max()))
            out[f'{name}.{lv}.indices'] = t.indices.numpy().astype(np.int32)
            out[f'{name}.{lv}.features'] = t.features.numpy()
            out[f'{name}.{lv}.shape'] = np.array(t.spatial_shape)
            print(name, lv, 'sites', len(t.indices), 'shape', list(t.spatial_shape), 'max |f|', float(t.features.abs().max()),
                  'zero fraction', float((t.features == 0).float().mean()))
        worst = max(worst, float((bd['spatial_features'].double() - bd64['spatial_features']).abs().max()))
        assert worst <= 2.5e-5, f'{name}: float32 and float64 differ by {worst:.3g} > 2.5e-5'
        assert len(levels['out'].indices) >= 8, f"{name}: the last level holds {len(levels['out'].indices)} sites"
        out[f'{name}.spatial_features'] = bd['spatial_features'].numpy()
        print(name, 'float32 against float64:', worst, 'spatial_features', tuple(bd['spatial_features'].shape))
    np.savez_compressed(os.path.join(HERE, 'ref_sparse_conv.npz'), **out)
    with open(os.path.join(HERE, 'ref_sparse_conv_manifest.json'), 'w') as f:
        json.dump(manifest, f, indent=1, sort_keys=True)
    for n in ('ref_sparse_conv.npz', 'ref_sparse_conv_manifest.json'):
        print(n, os.path.getsize(os.path.join(HERE, n)), 'bytes')


if __name__ == '__main__':
    main()

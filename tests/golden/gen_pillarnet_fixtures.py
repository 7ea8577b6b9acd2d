#!/usr/bin/env python3
"""Generates tests/golden/ref_pillarnet.npz and ref_pillarnet_manifest.json by running the REFERENCE's own
DynamicPillarVFESimple2D, PillarBackBone8x, PillarRes18BackBone8x and BaseBEVBackboneV1 on the CPU, imported from where they lie,
nothing copied (`.cuda()` is the identity, gen_head_fixtures.install_reference; torch_scatter is gen_pillar_fixtures' stub; the
configs are gen_center_head_fixtures' EasyDict).  Run in the authoring container only; the outputs hold numbers, index arrays,
state_dict key names and weight check sums only.

spconv is on no machine of this project, so the backbones run over a STUB `spconv` module for 2-D written here, in the manner of
gen_sparse_conv_fixtures.py, which imports nothing from pdm_ssd_amd: a layer densifies its input and calls
torch.nn.functional.conv2d.  A submanifold layer's outputs are the input sites (padding = kernel // 2, stride 1); a strided layer's
are the sites whose window holds an active input (a convolution of the occupancy with a kernel of ones), numbered in ascending
(b W + x) H + y.  SparseSequential applies BatchNorm and ReLU to the active rows only.

Shape (tests/pillarnet_reference.py PN): 48 x 32 pillars, B = 3 with sample 1 empty, about 300 pillars; the levels are 48 x 32 ->
24 x 16 -> 12 x 8 -> 6 x 4 and conv5 gives 3 x 2 (even down to x_conv4, so that BaseBEVBackboneV1's upsampled x_conv5 fits it).  The fixture holds no weights: generator and tests fill them from the same seeds
(pillarnet_reference.fill_vfe / fill_pillarnet) and the fixture holds their check sums.

Parity bound of the backbone tests, 1e-4 absolute: main() runs each backbone and its BaseBEVBackboneV1 in float32 and in float64 and
fails unless every level, x_conv5 and spatial_features_2d agree within 2.5e-5, a quarter of the bound, and unless the last sparse
level holds at least 8 active sites.
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
import pillarnet_reference as pnr  # noqa: E402
from gen_center_head_fixtures import EasyDict  # noqa: E402
from gen_pillar_fixtures import install_pillar_reference  # noqa: E402

VFE_SEEDS = {'a': 51, 'b': 52, 'c': 53}
SEEDS = {'PillarBackBone8x': (61, 1.0), 'PillarRes18BackBone8x': (63, 0.6)}       # (seed, gain) of fill_pillarnet
BEV_SEED, BEV_GAIN = 67, 1.0
BEV_CFG = {'LAYER_NUMS': [1, 1], 'NUM_FILTERS': [256, 256], 'UPSAMPLE_STRIDES': [1, 2], 'NUM_UPSAMPLE_FILTERS': [128, 128]}


def _pair(v):
    return (v,) * 2 if isinstance(v, int) else tuple(v)


def install_spconv_stub():
    class SparseConvTensor:
        def __init__(self, features, indices, spatial_shape, batch_size):
            self.features, self.indices, self.spatial_shape, self.batch_size = features, indices, [int(v) for v in spatial_shape], batch_size

        def replace_feature(self, f):
            return SparseConvTensor(f, self.indices, self.spatial_shape, self.batch_size)

        def dense(self):
            i = self.indices.long()
            out = torch.zeros((self.batch_size, *self.spatial_shape, self.features.shape[1]), dtype=self.features.dtype)
            out[i[:, 0], i[:, 1], i[:, 2]] = self.features
            return out.permute(0, 3, 1, 2).contiguous()

    class SparseModule(nn.Module):
        pass

    class SparseConvolution(SparseModule):
        def __init__(self, cin, cout, kernel_size, stride=1, padding=0, bias=True, indice_key=None, subm=False):
            super().__init__()
            self.k, self.s, self.p, self.subm = _pair(kernel_size), _pair(stride), _pair(padding), subm
            self.weight = nn.Parameter(torch.zeros(cout, *self.k, cin))             # spconv 2.x's layout
            self.bias = nn.Parameter(torch.zeros(cout)) if bias else None

        def forward(self, x):
            w = self.weight.permute(0, 3, 1, 2)
            stride, pad = ((1, 1), tuple(k // 2 for k in self.k)) if self.subm else (self.s, self.p)
            y = F.conv2d(x.dense(), w, None, stride, pad)                           # (B, Cout, H', W')
            if self.subm:
                idx = x.indices.long()
            else:
                occ = torch.zeros((x.batch_size, 1, *x.spatial_shape), dtype=y.dtype)
                i = x.indices.long()
                occ[i[:, 0], 0, i[:, 1], i[:, 2]] = 1
                hit = F.conv2d(occ, torch.ones((1, 1, *self.k), dtype=y.dtype), None, stride, pad)[:, 0] > 0
                idx = torch.nonzero(hit)                                             # (b, y, x)
                H, W = y.shape[2:]
                idx = idx[torch.argsort((idx[:, 0] * W + idx[:, 2]) * H + idx[:, 1])]
            f = y[idx[:, 0], :, idx[:, 1], idx[:, 2]]
            if self.bias is not None:
                f = f + self.bias
            return SparseConvTensor(f, idx.int(), y.shape[2:], x.batch_size)

    class SubMConv2d(SparseConvolution):
        def __init__(self, cin, cout, kernel_size, stride=1, padding=0, bias=True, indice_key=None):
            super().__init__(cin, cout, kernel_size, 1, padding, bias, indice_key, subm=True)

    class SparseConv2d(SparseConvolution):
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
    for cls in (SparseConvTensor, SparseModule, SparseConvolution, SubMConv2d, SparseConv2d, SparseSequential):
        setattr(pt, cls.__name__, cls)
    pt.conv = types.SimpleNamespace(SparseConvolution=SparseConvolution)
    top.pytorch = pt
    sys.modules['spconv'], sys.modules['spconv.pytorch'] = top, pt


def run_backbone(cls, bev_cls, coords, feats, dtype, seed, gain):
    g = pnr.PN
    net = cls(model_cfg=EasyDict({}), input_channels=feats.shape[1], grid_size=np.array(g['grid']))
    checksum = pnr.fill_pillarnet(net, seed, gain)
    bev = bev_cls(model_cfg=EasyDict(BEV_CFG))
    bev_checksum = pnr.fill_pillarnet(bev, BEV_SEED, BEV_GAIN)
    net, bev = net.to(dtype).eval(), bev.to(dtype).eval()
    seen = {}
    net.conv4.register_forward_hook(lambda m, a, out: seen.update(x_conv4=out))     # the forward replaces it by its dense map
    with torch.no_grad():
        bd = bev(net({'pillar_features': torch.from_numpy(feats).to(dtype), 'pillar_coords': torch.from_numpy(coords), 'batch_size': g['B']}))
    levels = {k: bd['multi_scale_2d_features'][k] for k in ('x_conv1', 'x_conv2', 'x_conv3')}
    levels['x_conv4'] = seen['x_conv4']
    return net, bev, bd, levels, checksum, bev_checksum


def main():
    install_spconv_stub()
    dynamic_pillar_vfe, _, base_bev_backbone = install_pillar_reference()
    from pcdet.models.backbones_3d import spconv_backbone_2d
    out, manifest = {}, {}
    g = pnr.PN
    pts = pnr.pn_points()
    out['points'] = pts

    # ---- the VFE ----
    for tag, cfg in pnr.VFE_CONFIGS.items():
        vfe = dynamic_pillar_vfe.DynamicPillarVFESimple2D(model_cfg=EasyDict(cfg), num_point_features=4, voxel_size=g['voxel'],
                                                          grid_size=np.array(g['grid']), point_cloud_range=g['range'])
        checksum = pnr.fill_vfe(vfe, VFE_SEEDS[tag])
        vfe.eval()
        seen = {}
        vfe.pfn_layers[0].register_forward_hook(lambda m, a, o: seen.update(rows=a[0], inv=a[1]))
        with torch.no_grad():
            bd = vfe({'points': torch.from_numpy(pts), 'batch_size': g['B']})
        mine = pnr.vfe_features(pts, g, cfg['USE_ABSLOTE_XYZ'], cfg['WITH_DISTANCE'])
        assert np.array_equal(bd['pillar_coords'].numpy(), mine['pillar_coords']) and np.array_equal(seen['inv'].numpy(), mine['unq_inv'])
        manifest[f'DynamicPillarVFESimple2D.{tag}'] = {k: list(v.shape) for k, v in vfe.state_dict().items()}
        manifest[f'DynamicPillarVFESimple2D.{tag}.fill'] = {'seed': VFE_SEEDS[tag], 'checksum': checksum}
        out[f'vfe.{tag}.rows'] = seen['rows'].numpy()
        out[f'vfe.{tag}.features'] = bd['pillar_features'].numpy()
        w = vfe.pfn_layers[0].linear.weight.detach().abs().double()
        worst = float((seen['rows'].abs().double() @ w.T).max().detach()) * w.shape[1] * 2.0 ** -24 * 1.2
        assert worst <= 2.5e-5 or len(vfe.pfn_layers) > 1, f'vfe {tag}: first-layer rounding bound {worst:.3g}'
        print('vfe', tag, 'rows', tuple(seen['rows'].shape), 'pillars', len(bd['pillar_coords']), 'first-layer bound', worst,
              'max |f|', float(bd['pillar_features'].abs().max()))
    out['pillar_coords'] = mine['pillar_coords']
    out['kept_idx'], out['unq_inv'] = mine['kept_idx'], mine['unq_inv']
    coords, feats = mine['pillar_coords'], out['vfe.a.features']
    assert 250 <= len(coords) <= 400 and 1 not in coords[:, 0], len(coords)

    # ---- the backbones, each with BaseBEVBackboneV1 behind it ----
    for name, (seed, gain) in SEEDS.items():
        cls = getattr(spconv_backbone_2d, name)
        net, bev, bd, levels, checksum, bev_checksum = run_backbone(cls, base_bev_backbone.BaseBEVBackboneV1, coords, feats, torch.float32, seed, gain)
        _, _, bd64, levels64, _, _ = run_backbone(cls, base_bev_backbone.BaseBEVBackboneV1, coords, feats, torch.float64, seed, gain)
        manifest[name] = {k: list(v.shape) for k, v in net.state_dict().items()}
        manifest[f'{name}.fill'] = {'seed': seed, 'gain': gain, 'checksum': checksum}
        manifest['BaseBEVBackboneV1'] = {k: list(v.shape) for k, v in bev.state_dict().items()}
        manifest['BaseBEVBackboneV1.fill'] = {'seed': BEV_SEED, 'gain': BEV_GAIN, 'checksum': bev_checksum, 'cfg': BEV_CFG}
        worst = 0.0
        for lv, t in levels.items():
            assert (t.indices == levels64[lv].indices).all()
            worst = max(worst, float((t.features.double() - levels64[lv].features).abs().max()))
            out[f'{name}.{lv}.indices'] = t.indices.numpy().astype(np.int32)
            out[f'{name}.{lv}.features'] = t.features.numpy()
            out[f'{name}.{lv}.shape'] = np.array(t.spatial_shape)
            print(name, lv, 'sites', len(t.indices), 'shape', list(t.spatial_shape), 'max |f|', float(t.features.abs().max()),
                  'zero fraction', float((t.features == 0).float().mean()))
        for key, a, b in (('x_conv5', bd['multi_scale_2d_features']['x_conv5'], bd64['multi_scale_2d_features']['x_conv5']),
                          ('spatial_features_2d', bd['spatial_features_2d'], bd64['spatial_features_2d'])):
            worst = max(worst, float((a.double() - b).abs().max()))
            out[f'{name}.{key}'] = a.numpy()
            print(name, key, tuple(a.shape), 'max |f|', float(a.abs().max()))
        assert torch.equal(bd['multi_scale_2d_features']['x_conv4'], levels['x_conv4'].dense())
        assert worst <= 2.5e-5, f'{name}: float32 and float64 differ by {worst:.3g} > 2.5e-5'
        assert len(levels['x_conv4'].indices) >= 8, f"{name}: the last sparse level holds {len(levels['x_conv4'].indices)} sites"
        assert bd['multi_scale_2d_strides'] == {'x_conv1': 1, 'x_conv2': 2, 'x_conv3': 4, 'x_conv4': 8, 'x_conv5': 16}
        print(name, 'float32 against float64:', worst)
    np.savez_compressed(os.path.join(HERE, 'ref_pillarnet.npz'), **out)
    with open(os.path.join(HERE, 'ref_pillarnet_manifest.json'), 'w') as f:
        json.dump(manifest, f, indent=1, sort_keys=True)
    for n in ('ref_pillarnet.npz', 'ref_pillarnet_manifest.json'):
        print(n, os.path.getsize(os.path.join(HERE, n)), 'bytes')


if __name__ == '__main__':
    main()

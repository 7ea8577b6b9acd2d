#!/usr/bin/env python3
"""Generates tests/golden/ref_pillar.npz, ref_pillar_pfn.npz and ref_pillar_manifest.json by running the REFERENCE's own
DynamicPillarVFE, PointPillarScatter and BaseBEVBackbone on the CPU, imported from where they lie, nothing copied
(`.cuda()` is the identity, gen_head_fixtures.install_reference).  torch_scatter is not on this platform: a stub module
written here supplies scatter_mean (index_add_ / bincount) and scatter_max (scatter_reduce 'amax', include_self=False).
numpy's removed `np.int` alias, which the reference's BaseBEVBackbone still names, is put back for the run.  Run in the
authoring container only; the outputs hold numbers and key names only.

Shapes (the smallest at which each kernel can still go wrong):
  G1  range [0, -6, -3, 20, 6, 1], voxel [0.5, 0.5, 4], grid [40, 24, 1] (nx != ny), B = 3, sample 1 owns no point; rows
      shuffled so that the samples interleave: 700 spread points (some outside in x, in y, in z only), one cell with 1100
      points, single-point pillars, two identical rows, and the edge rows x = 20 (dropped), (0, -6) (cell 0, 0),
      x = -1e-7 (dropped), (nextafter(20, 0), 5.9) (last cell), y = 6 (dropped), z = 9 inside xy (kept), and
      (nextafter(20, 0), nextafter(6, 0)): the reference DROPS it, because its fp32 y - (-6) rounds up to 12.0, cell 24.
      Recorded with C = 4 and C = 5, the four USE_ABSLOTE_XYZ x WITH_DISTANCE combinations, NUM_FILTERS [64] and
      [32, 64], and USE_NORM False.
  G2  voxel 0.16: range [0, -3.84, -3, 6.4, 3.84, 1], grid [40, 48, 1]; points at float32(k * 0.16) for every k and one
      ulp to either side, in x and in y: what tells a division from a reciprocal multiply.
  G3  grid [176, 200, 1], B = 2, 500 points: 70400 cells, almost all empty.
ref_pillar.npz: per shape the points, kept_idx, unq_inv, voxel_coords, pillar_count, the float64 pillar mean, the feature
rows the first PFN layer received, the 8-channel canvas; BaseBEVBackbone weights, input and output.  ref_pillar_pfn.npz: the
PFN weights and the (P, K) outputs of every configuration.  The manifest: state_dict keys and shapes.

PFN parity bound (tests: 1e-4 absolute): weights within +-0.3, BatchNorm scaled so that |gamma / sqrt(var + eps)| <= 1;
main() asserts n_in * 2^-24 * max_row sum |w x| * |scale| <= 1e-4 for every layer on the fixture's own inputs.
"""
import json
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from gen_center_head_fixtures import EasyDict  # noqa: E402
from gen_head_fixtures import REF, install_reference  # noqa: E402

G1 = dict(range=[0.0, -6.0, -3.0, 20.0, 6.0, 1.0], voxel=[0.5, 0.5, 4.0], grid=[40, 24, 1], B=3)
G2 = dict(range=[0.0, -3.84, -3.0, 6.4, 3.84, 1.0], voxel=[0.16, 0.16, 4.0], grid=[40, 48, 1], B=1)
G3 = dict(range=[0.0, -40.0, -3.0, 70.4, 40.0, 1.0], voxel=[0.4, 0.4, 4.0], grid=[176, 200, 1], B=2)


def install_pillar_reference():
    install_reference()
    for name, path in (('pcdet.models.backbones_3d', 'backbones_3d'), ('pcdet.models.backbones_3d.vfe', 'backbones_3d/vfe'),
                       ('pcdet.models.backbones_2d', 'backbones_2d'), ('pcdet.models.backbones_2d.map_to_bev', 'backbones_2d/map_to_bev')):
        m = types.ModuleType(name)              # package __init__ not run (they import spconv)
        m.__path__ = [f'{REF}/pcdet/models/{path}']
        sys.modules[name] = m
    ts = types.ModuleType('torch_scatter')

    def scatter_mean(src, index, dim=0):
        assert dim == 0
        n = int(index.max()) + 1
        s = torch.zeros((n,) + tuple(src.shape[1:]), dtype=src.dtype).index_add_(0, index, src)
        return s / torch.bincount(index, minlength=n).to(src.dtype)[:, None]

    def scatter_max(src, index, dim=0):
        assert dim == 0
        n = int(index.max()) + 1
        out = torch.zeros((n,) + tuple(src.shape[1:]), dtype=src.dtype)
        out = out.scatter_reduce(0, index[:, None].expand_as(src), src, 'amax', include_self=False)
        return out, None
    ts.scatter_mean, ts.scatter_max = scatter_mean, scatter_max
    sys.modules['torch_scatter'] = ts
    if not hasattr(np, 'int'):
        np.int = int
    from pcdet.models.backbones_2d import base_bev_backbone
    from pcdet.models.backbones_2d.map_to_bev import pointpillar_scatter
    from pcdet.models.backbones_3d.vfe import dynamic_pillar_vfe
    return dynamic_pillar_vfe, pointpillar_scatter, base_bev_backbone


def g1_points():
    rng = np.random.default_rng(2024)
    f32 = np.float32
    rows = []
    spread = np.stack([rng.choice([0, 2], 700), rng.uniform(-1.0, 21.0, 700), rng.uniform(-6.6, 6.6, 700), rng.uniform(-3.5, 1.5, 700)], 1)
    rows.append(spread)
    crowd = np.stack([np.full(1100, 2), rng.uniform(15.5, 16.0, 1100), rng.uniform(-2.5, -2.0, 1100), rng.uniform(-3, 1, 1100)], 1)
    rows.append(crowd)
    singles = np.stack([rng.choice([0, 2], 300), rng.uniform(0, 20, 300), rng.uniform(-6, 6, 300), rng.uniform(-3, 1, 300)], 1)
    rows.append(singles)
    twin = np.array([[0, 7.3125, 1.4375, -0.25]] * 2)
    edges = np.array([[0, 20.0, 0.3, 0.0], [0, 0.0, -6.0, 0.0], [2, -1e-7, 1.0, 0.0],
                      [2, np.nextafter(f32(20), f32(0)), np.nextafter(f32(6), f32(0)), 0.5], [0, 3.0, 6.0, 0.0], [0, 5.2, -1.3, 9.0],
                      [2, np.nextafter(f32(20), f32(0)), 5.9, 0.25]])
    rows += [twin, edges]
    p = np.concatenate(rows).astype(f32)
    extra = rng.uniform(0, 1, (len(p), 2)).astype(f32)          # intensity, and a fifth feature for C = 5
    p = np.concatenate([p, extra], 1)
    return p[rng.permutation(len(p))]


def ulp_neighbours(v):
    v = np.asarray(v, dtype=np.float32)
    return np.concatenate([np.nextafter(v, np.float32(-np.inf)), v, np.nextafter(v, np.float32(np.inf))])


def g2_points():
    rng = np.random.default_rng(7)
    xs = ulp_neighbours([np.float32(k * 0.16) for k in range(0, 41)])
    ys = ulp_neighbours([np.float32(k * 0.16) for k in range(-24, 25)])
    a = np.stack([np.zeros_like(xs), xs, np.full_like(xs, 0.4), np.zeros_like(xs)], 1)
    b = np.stack([np.zeros_like(ys), np.full_like(ys, 1.0), ys, np.zeros_like(ys)], 1)
    p = np.concatenate([a, b]).astype(np.float32)
    p = np.concatenate([p, rng.uniform(0, 1, (len(p), 1)).astype(np.float32)], 1)
    return p[rng.permutation(len(p))]


def g3_points():
    rng = np.random.default_rng(9)
    p = np.stack([rng.integers(0, 2, 500), rng.uniform(-2, 72, 500), rng.uniform(-41, 41, 500), rng.uniform(-3, 1, 500),
                  rng.uniform(0, 1, 500)], 1)
    return p.astype(np.float32)


def make_vfe(mod, geo, C, use_norm=True, with_distance=False, use_absolute_xyz=True, num_filters=(64,), seed=0):
    cfg = EasyDict({'USE_NORM': use_norm, 'WITH_DISTANCE': with_distance, 'USE_ABSLOTE_XYZ': use_absolute_xyz, 'NUM_FILTERS': list(num_filters)})
    vfe = mod.DynamicPillarVFE(model_cfg=cfg, num_point_features=C, voxel_size=geo['voxel'], grid_size=geo['grid'],
                               point_cloud_range=geo['range'])
    g = torch.Generator().manual_seed(100 + seed)
    with torch.no_grad():
        for i, layer in enumerate(vfe.pfn_layers):
            bound = 0.3 if i == 0 else 0.02
            layer.linear.weight.copy_((torch.rand(layer.linear.weight.shape, generator=g) * 2 - 1) * bound)
            if use_norm:
                n = layer.norm.num_features
                layer.norm.weight.copy_(torch.rand(n, generator=g) * 0.5 + 0.5)          # gamma in [0.5, 1]
                layer.norm.running_var.copy_(torch.rand(n, generator=g) + 1.0)           # var in [1, 2]: |scale| <= 1
                layer.norm.bias.copy_(torch.rand(n, generator=g) - 0.5)
                layer.norm.running_mean.copy_(torch.rand(n, generator=g) - 0.5)
            else:
                layer.linear.bias.copy_(torch.rand(layer.linear.bias.shape, generator=g) - 0.5)
    return vfe.eval()


def run_vfe(vfe, points):
    """-> (batch_dict, [inputs of every PFN layer])"""
    seen = []
    hooks = [layer.register_forward_pre_hook(lambda m, args: seen.append(args[0].detach().clone())) for layer in vfe.pfn_layers]
    with torch.no_grad():
        bd = vfe({'points': torch.from_numpy(points)})
    for h in hooks:
        h.remove()
    for layer, x in zip(vfe.pfn_layers, seen):      # the 1e-4 parity bound on this fixture's own inputs
        w = layer.linear.weight.detach()
        scale = (layer.norm.weight / torch.sqrt(layer.norm.running_var + layer.norm.eps)).detach().abs() if layer.use_norm else torch.ones(w.shape[0])
        assert float(scale.max()) <= 1.0
        worst = float(((x.abs().double() @ w.abs().double().t()) * scale.double()).max()) * w.shape[1] * 2.0 ** -24
        assert worst <= 1e-4, f'PFN parity bound: {worst:.3g} > 1e-4'
    return bd, seen


def assign_records(out, tag, geo, points):
    """the reference's own mask / unique, recomputed as its forward does, plus a float64 mean (numpy)"""
    t = torch.from_numpy(points)
    r, v, g = torch.tensor(geo['range']), torch.tensor(geo['voxel']), torch.tensor(geo['grid'])
    pc = torch.floor((t[:, [1, 2]] - r[[0, 1]]) / v[[0, 1]]).int()
    mask = ((pc >= 0) & (pc < g[[0, 1]])).all(dim=1)
    kept = torch.nonzero(mask)[:, 0]
    pk, ck = t[mask], pc[mask]
    merge = pk[:, 0].int() * (geo['grid'][0] * geo['grid'][1]) + ck[:, 0] * geo['grid'][1] + ck[:, 1]
    unq, inv, cnt = torch.unique(merge, return_inverse=True, return_counts=True, dim=0)
    assert bool((unq[1:] > unq[:-1]).all())
    mean = np.zeros((len(unq), 3))
    np.add.at(mean, inv.numpy(), pk[:, 1:4].numpy().astype(np.float64))
    mean /= cnt.numpy()[:, None]
    out.update({f'{tag}.points': points, f'{tag}.kept_idx': kept.numpy().astype(np.int32), f'{tag}.unq_inv': inv.numpy().astype(np.int32),
                f'{tag}.pillar_count': cnt.numpy().astype(np.int32), f'{tag}.pillar_mean64': mean, f'{tag}.keys': unq.numpy().astype(np.int32)})
    return kept, inv, len(unq)


def main():
    dpv, pps, bbb = install_pillar_reference()
    out, pfn, manifest = {}, {}, {}
    shapes = {'g1': (G1, g1_points()), 'g2': (G2, g2_points()), 'g3': (G3, g3_points())}
    for tag, (geo, pts) in shapes.items():
        out[f'{tag}.range'], out[f'{tag}.voxel'], out[f'{tag}.grid'] = np.array(geo['range']), np.array(geo['voxel']), np.array(geo['grid'])
        out[f'{tag}.B'] = np.int64(geo['B'])

    # configurations: (name, shape, C, kwargs)
    runs = [('g1.c4', 'g1', 4, {})]
    runs += [(f'g1.c4.abs{int(a)}.dist{int(d)}', 'g1', 4, dict(use_absolute_xyz=a, with_distance=d)) for a in (True, False) for d in (True, False)
             if not (a and not d)]
    runs += [('g1.c5', 'g1', 5, {}), ('g1.c4.f32_64', 'g1', 4, dict(num_filters=(32, 64))), ('g1.c4.nonorm', 'g1', 4, dict(use_norm=False)),
             ('g1.c5.dist.nonorm', 'g1', 5, dict(use_norm=False, with_distance=True)),
             ('g2.c4', 'g2', 4, {}), ('g3.c4', 'g3', 4, {})]
    for seed, (name, tag, C, kw) in enumerate(runs):
        geo, pts = shapes[tag]
        points = np.ascontiguousarray(pts[:, :1 + C])
        vfe = make_vfe(dpv, geo, C, seed=seed, **kw)
        bd, seen = run_vfe(vfe, points)
        key = f'{tag}.c{C}'
        if f'{key}.points' not in out:
            kept, inv, P = assign_records(out, key, geo, points)
            out[f'{key}.voxel_coords'] = bd['voxel_coords'].numpy().astype(np.int32)
            assert P == len(bd['voxel_coords'])
            vc = bd['voxel_coords'].numpy()
            assert (out[f'{key}.keys'] == vc[:, 0] * geo['grid'][0] * geo['grid'][1] + vc[:, 3] * geo['grid'][1] + vc[:, 2]).all()
        out[f'{name}.features'] = seen[0].numpy()
        assert seen[0].shape[0] == len(out[f'{key}.kept_idx'])
        pfn[f'{name}.pillar_features'] = bd['pillar_features'].numpy()
        for k, v in vfe.state_dict().items():
            pfn[f'{name}.state.{k}'] = v.numpy()
        manifest[f'DynamicPillarVFE({name})'] = {k: list(v.shape) for k, v in vfe.state_dict().items()}
        if name.endswith('.c4') or name == 'g1.c5':           # the canvas of the first 8 channels
            sc = pps.PointPillarScatter(model_cfg=EasyDict({'NUM_BEV_FEATURES': 8}), grid_size=geo['grid'])
            canvas = sc({'pillar_features': bd['pillar_features'][:, :8].contiguous(), 'voxel_coords': bd['voxel_coords']})['spatial_features']
            assert tuple(canvas.shape) == (geo['B'], 8, geo['grid'][1], geo['grid'][0]), tuple(canvas.shape)
            out[f'{name}.canvas'] = canvas.numpy()
        if kw.get('with_distance', False):
            # the norm column is sqrt(fma(z, z, fma(y, y, x * x))) in fp32: what the operator pins (products exact in double)
            xyz = points[out[f'{key}.kept_idx']][:, 1:4].astype(np.float64)
            acc = np.float32(xyz[:, 0] * xyz[:, 0]).astype(np.float64)
            for d in (1, 2):
                acc = np.float32(xyz[:, d] * xyz[:, d] + acc).astype(np.float64)
            assert (np.sqrt(acc.astype(np.float32)) == seen[0].numpy()[:, -1]).all(), 'distance column: another rounding sequence'
    print('g1 pillars', len(out['g1.c4.voxel_coords']), 'kept', len(out['g1.c4.kept_idx']), 'of', len(shapes['g1'][1]),
          'max count', int(out['g1.c4.pillar_count'].max()), 'g2 pillars', len(out['g2.c4.voxel_coords']), 'g3 pillars', len(out['g3.c4.voxel_coords']))

    # BaseBEVBackbone: one small network run on the G1 canvas, and key / shape manifests of the branches
    bev_cfgs = {
        'small': ({'LAYER_NUMS': [1, 1], 'LAYER_STRIDES': [1, 2], 'NUM_FILTERS': [8, 16], 'UPSAMPLE_STRIDES': [1, 2], 'NUM_UPSAMPLE_FILTERS': [8, 8]}, 8),
        'kitti': ({'LAYER_NUMS': [3, 5, 5], 'LAYER_STRIDES': [2, 2, 2], 'NUM_FILTERS': [64, 128, 256], 'UPSAMPLE_STRIDES': [1, 2, 4],
                   'NUM_UPSAMPLE_FILTERS': [128, 128, 128]}, 64),
        'downsample': ({'LAYER_NUMS': [1, 1, 1], 'LAYER_STRIDES': [1, 2, 2], 'NUM_FILTERS': [8, 16, 32], 'UPSAMPLE_STRIDES': [0.5, 1, 2],
                        'NUM_UPSAMPLE_FILTERS': [16, 16, 16], 'USE_CONV_FOR_NO_STRIDE': True}, 8),
        'extra_deblock': ({'LAYER_NUMS': [1, 1], 'LAYER_STRIDES': [1, 2], 'NUM_FILTERS': [8, 16], 'UPSAMPLE_STRIDES': [1, 2, 2],
                           'NUM_UPSAMPLE_FILTERS': [8, 8, 8]}, 8),
        'no_upsample': ({'LAYER_NUMS': [1], 'LAYER_STRIDES': [2], 'NUM_FILTERS': [8]}, 8),
    }
    manifest['bev_cfgs'] = {k: {'cfg': c, 'input_channels': cin} for k, (c, cin) in bev_cfgs.items()}
    for name, (c, cin) in bev_cfgs.items():
        torch.manual_seed(31)
        net = bbb.BaseBEVBackbone(EasyDict(c), cin)
        manifest[f'BaseBEVBackbone({name})'] = {k: list(v.shape) for k, v in net.state_dict().items()}
        manifest[f'BaseBEVBackbone({name}).num_bev_features'] = int(net.num_bev_features)
        if name in ('small', 'downsample'):
            g = torch.Generator().manual_seed(32)
            with torch.no_grad():
                for m in net.modules():
                    if isinstance(m, torch.nn.BatchNorm2d):
                        m.running_mean.copy_(torch.rand(m.num_features, generator=g) - 0.5)
                        m.running_var.copy_(torch.rand(m.num_features, generator=g) + 0.5)
                        m.weight.copy_(torch.rand(m.num_features, generator=g) + 0.5)
                        m.bias.copy_(torch.rand(m.num_features, generator=g) - 0.5)
            net.eval()
            x = torch.from_numpy(out['g1.c4.canvas'][[0, 2]])
            with torch.no_grad():
                y = net({'spatial_features': x})['spatial_features_2d']
            out[f'bev.{name}.out'] = y.numpy()
            for k, v in net.state_dict().items():
                out[f'bev.{name}.state.{k}'] = v.numpy()
    np.savez_compressed(os.path.join(HERE, 'ref_pillar.npz'), **out)
    np.savez_compressed(os.path.join(HERE, 'ref_pillar_pfn.npz'), **pfn)
    with open(os.path.join(HERE, 'ref_pillar_manifest.json'), 'w') as f:
        json.dump(manifest, f, indent=1, sort_keys=True)
    for n in ('ref_pillar.npz', 'ref_pillar_pfn.npz', 'ref_pillar_manifest.json'):
        print(n, os.path.getsize(os.path.join(HERE, n)), 'bytes')


if __name__ == '__main__':
    main()

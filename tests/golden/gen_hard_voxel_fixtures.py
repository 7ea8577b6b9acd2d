#!/usr/bin/env python3
"""Generates tests/golden/ref_hard_voxel.npz, ref_hard_voxel_pfn.npz and ref_hard_voxel_manifest.json.  The inputs below are
voxelized with the numpy restatement of the hard voxel generator (tests/hard_voxel_reference.py: spconv is on no machine of
this project), then the REFERENCE's own MeanVFE and PillarVFE run on the CPU over those voxels, imported from where they lie
with the package __init__s bypassed (gen_pillar_fixtures.install_pillar_reference), nothing copied.  Run in the authoring
container only; the outputs hold numbers and key names only.

Shapes (the smallest at which each kernel can still go wrong):
  H1   pillars: range [0, -6, -3, 20, 6, 1], voxel [0.5, 0.5, 4], grid [40, 24, 1], B = 3, sample 1 owns no point, T = 8,
       max_voxels 50 (the cap bites in samples 0 and 2) and 2000 (it does not).  Rows are sorted by sample and shuffled inside
       each sample, so appearance order is not key order: 700 spread rows (some outside in x, in y, in z ONLY), one cell of
       1100 rows (more than a wave, more than a workgroup), cells of exactly T and T + 1 rows, single-row cells, two identical
       rows, the edge rows x = 20 (dropped), (0, -6) (cell 0, 0), x = -1e-7 (dropped), y = 6 (dropped), z = 9 inside xy
       (DROPPED here: z is tested), (nextafter(20, 0), 5.9) (last cell) and (nextafter(20, 0), nextafter(6, 0)), dropped
       because its fp32 y - (-6) rounds up to 12.0.  The last three rows of sample 0 are A, R, A: A in the cell of the sample's
       first row (accepted, fewer than T rows), R in a cell no other row visits (refused in the capped run): both A rows are
       kept, which tells `continue` from `break`.
  H2   voxels: range [0, -4, -3, 8, 4, 1], voxel [0.5] * 3, grid [16, 16, 8], B = 2, T = 5, 1500 rows, max_voxels 100 and 5000.
  H2S  the voxel-size-0.16 strip: range [0, -3.84, -1.6, 6.4, 3.84, 1.6], grid [40, 48, 20], B = 1, T = 5: points at
       float32(k * 0.16) for every k and one ulp to either side on each axis: what tells a division from a reciprocal multiply.
  H3   the KITTI voxel grid [1408, 1600, 40], B = 32, 600 rows, some in sample 31 (keys above 2^31), T = 5, max_voxels 40000.
ref_hard_voxel.npz: per shape the points, and per (shape, cap, C) slot_rows, voxel_coords, voxel_num_points, the float64 mean
of every column over the kept slots, the reference MeanVFE's output; per PFN configuration the (M, T, F) rows the first PFN
layer received.  ref_hard_voxel_pfn.npz: the PFN weights and the (M, K) outputs.  The manifest: state_dict keys and shapes.

PFN parity bound (tests: 1e-4 absolute): weights within +-0.3, BatchNorm scaled so that |gamma / sqrt(var + eps)| <= 1; main()
asserts n_in * 2^-24 * max_row sum |w x| * |scale| <= 1e-4 for every layer on the fixture's own inputs, and that some voxel
with fewer than T points has a channel whose maximum IS the padding rows' value.
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import hard_voxel_reference as hvr  # noqa: E402
from gen_center_head_fixtures import EasyDict  # noqa: E402
from gen_pillar_fixtures import install_pillar_reference, ulp_neighbours  # noqa: E402

f32 = np.float32
H1 = dict(range=[0.0, -6.0, -3.0, 20.0, 6.0, 1.0], voxel=[0.5, 0.5, 4.0], grid=[40, 24, 1], B=3, T=8, caps=[50, 2000])
H2 = dict(range=[0.0, -4.0, -3.0, 8.0, 4.0, 1.0], voxel=[0.5, 0.5, 0.5], grid=[16, 16, 8], B=2, T=5, caps=[100, 5000])
H2S = dict(range=[0.0, -3.84, -1.6, 6.4, 3.84, 1.6], voxel=[0.16, 0.16, 0.16], grid=[40, 48, 20], B=1, T=5, caps=[40000])
H3 = dict(range=[0.0, -40.0, -3.0, 70.4, 40.0, 1.0], voxel=[0.05, 0.05, 0.1], grid=[1408, 1600, 40], B=32, T=5, caps=[40000])


def by_sample(p, rng):
    """shuffled inside every sample, samples ascending"""
    p = p[rng.permutation(len(p))]
    return p[np.argsort(p[:, 0], kind='stable')]


def h1_points():
    rng = np.random.default_rng(4048)
    T = H1['T']
    rows = [np.stack([rng.choice([0, 2], 700), rng.uniform(-1.0, 21.0, 700), rng.uniform(-6.6, 6.6, 700), rng.uniform(-3.5, 1.5, 700)], 1),
            np.stack([np.full(1100, 2), rng.uniform(15.5, 16.0, 1100), rng.uniform(-2.5, -2.0, 1100), rng.uniform(-3, 1, 1100)], 1),
            np.stack([rng.choice([0, 2], 300), rng.uniform(0, 20, 300), rng.uniform(-6, 6, 300), rng.uniform(-3, 1, 300)], 1),
            np.stack([np.full(T, 0), rng.uniform(18.0, 18.5, T), rng.uniform(-6.0, -5.5, T), rng.uniform(-3, 1, T)], 1),
            np.stack([np.full(T + 1, 2), rng.uniform(0.5, 1.0, T + 1), rng.uniform(5.5, 6.0, T + 1), rng.uniform(-3, 1, T + 1)], 1),
            np.array([[0, 7.3125, 1.4375, -0.25]] * 2),
            np.array([[0, 20.0, 0.3, 0.0], [0, 0.0, -6.0, 0.0], [2, -1e-7, 1.0, 0.0],
                      [2, np.nextafter(f32(20), f32(0)), np.nextafter(f32(6), f32(0)), 0.5], [0, 3.0, 6.0, 0.0], [0, 5.2, -1.3, 9.0],
                      [2, np.nextafter(f32(20), f32(0)), 5.9, 0.25]])]
    for i in (0, 2):        # the cells of exactly T and T + 1 rows hold no other row
        x, y = rows[i][:, 1], rows[i][:, 2]
        rows[i] = rows[i][~(((x >= 18.0) & (x < 18.5) & (y < -5.5)) | ((x >= 0.5) & (x < 1.0) & (y >= 5.5)))]
    p = by_sample(np.concatenate(rows).astype(f32), rng)
    # A, R, A at the end of sample 0
    n0 = int((p[:, 0] == 0).sum())
    cells = hvr.cells_of(p[:n0, 1:4], H1['range'], H1['voxel'])
    ok = hvr.inside(cells, H1['grid'])
    first = int(np.nonzero(ok)[0][0])
    used = {(int(c[0]), int(c[1])) for c in cells[:n0][ok]}
    free = next((x, y) for x in range(40) for y in range(24) if (x, y) not in used)
    a = p[first].copy()
    r = np.array([0, free[0] * 0.5 + 0.25, -6.0 + free[1] * 0.5 + 0.25, 0.0], dtype=f32)
    p = np.concatenate([p[:n0], a[None], r[None], a[None], p[n0:]])
    extra = rng.uniform(0, 1, (len(p), 2)).astype(f32)          # intensity, and a fifth feature for C = 5
    return np.concatenate([p, extra], 1), (n0, n0 + 1, n0 + 2)


def h2_points():
    rng = np.random.default_rng(77)
    n = 1500
    p = np.stack([rng.integers(0, 2, n), rng.uniform(-0.5, 8.5, n), rng.uniform(-4.4, 4.4, n), rng.uniform(-3.3, 1.3, n), rng.uniform(0, 1, n)], 1)
    dense = np.stack([np.ones(40), rng.uniform(2.0, 2.5, 40), rng.uniform(1.0, 1.5, 40), rng.uniform(-1.0, -0.5, 40), rng.uniform(0, 1, 40)], 1)
    return by_sample(np.concatenate([p, dense]).astype(f32), rng)


def h2s_points():
    rng = np.random.default_rng(78)
    xs = ulp_neighbours([f32(k * 0.16) for k in range(0, 41)])
    ys = ulp_neighbours([f32(k * 0.16) for k in range(-24, 25)])
    zs = ulp_neighbours([f32(k * 0.16) for k in range(-10, 11)])
    a = np.stack([np.zeros_like(xs), xs, np.full_like(xs, 0.4), np.full_like(xs, 0.1)], 1)
    b = np.stack([np.zeros_like(ys), np.full_like(ys, 1.0), ys, np.full_like(ys, 0.1)], 1)
    c = np.stack([np.zeros_like(zs), np.full_like(zs, 1.0), np.full_like(zs, 0.4), zs], 1)
    p = np.concatenate([a, b, c]).astype(f32)
    p = np.concatenate([p, rng.uniform(0, 1, (len(p), 1)).astype(f32)], 1)
    return p[rng.permutation(len(p))]


def h3_points():
    rng = np.random.default_rng(79)
    n = 600
    b = np.concatenate([rng.integers(0, 32, n - 60), np.full(60, 31)])
    p = np.stack([b, rng.uniform(-1, 71.4, n), rng.uniform(-41, 41, n), rng.uniform(-3.2, 1.2, n), rng.uniform(0, 1, n)], 1).astype(f32)
    p[-30:, 1:4] = p[-60:-30, 1:4] + f32(0.001)                # sample 31: some cells with two rows
    return by_sample(p, rng)


def make_pillar_vfe(mod, geo, C, use_norm=True, with_distance=False, use_absolute_xyz=True, num_filters=(64,), seed=0):
    cfg = EasyDict({'USE_NORM': use_norm, 'WITH_DISTANCE': with_distance, 'USE_ABSLOTE_XYZ': use_absolute_xyz, 'NUM_FILTERS': list(num_filters)})
    vfe = mod.PillarVFE(model_cfg=cfg, num_point_features=C, voxel_size=geo['voxel'], point_cloud_range=geo['range'])
    g = torch.Generator().manual_seed(500 + seed)
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


def run_pillar_vfe(vfe, vox):
    """-> (pillar_features (M, K), the (M, T, F) input of the first PFN layer); asserts the 1e-4 parity bound on every layer"""
    seen = []
    hooks = [layer.register_forward_pre_hook(lambda m, args: seen.append(args[0].detach().clone())) for layer in vfe.pfn_layers]
    with torch.no_grad():
        bd = vfe({'voxels': torch.from_numpy(vox['voxels']), 'voxel_num_points': torch.from_numpy(vox['voxel_num_points']),
                  'voxel_coords': torch.from_numpy(vox['voxel_coords'])})
    for h in hooks:
        h.remove()
    for layer, x in zip(vfe.pfn_layers, seen):
        w = layer.linear.weight.detach()
        scale = (layer.norm.weight / torch.sqrt(layer.norm.running_var + layer.norm.eps)).detach().abs() if layer.use_norm else torch.ones(w.shape[0])
        assert float(scale.max()) <= 1.0
        x2 = x.reshape(-1, x.shape[-1])
        worst = float(((x2.abs().double() @ w.abs().double().t()) * scale.double()).max()) * w.shape[1] * 2.0 ** -24
        assert worst <= 1e-4, f'PFN parity bound: {worst:.3g} > 1e-4'
    return bd['pillar_features'], seen[0]


def padding_wins(vfe, feats, num, T):
    """(voxel, channel) pairs of a one-layer encoder whose maximum is the padding rows' value, above every kept row's"""
    layer = vfe.pfn_layers[0]
    with torch.no_grad():
        x = layer.linear(feats)
        x = torch.relu(layer.norm(x.permute(0, 2, 1)).permute(0, 2, 1) if layer.use_norm else x)
    slot = torch.arange(T)[None, :, None]
    n = torch.from_numpy(num).long()[:, None, None]
    real = torch.where(slot < n, x, torch.full_like(x, -1.0)).amax(1)
    pad = torch.where(slot >= n, x, torch.full_like(x, -1.0)).amax(1)
    return int(((n[:, 0] < T) & (pad > real)).sum())


def main():
    mods = install_pillar_reference()
    del mods
    from pcdet.models.backbones_3d.vfe import mean_vfe, pillar_vfe
    out, pfn, manifest = {}, {}, {}
    h1, ara = h1_points()
    shapes = {'h1': (H1, h1), 'h2': (H2, h2_points()), 'h2s': (H2S, h2s_points()), 'h3': (H3, h3_points())}
    vox = {}
    for tag, (geo, pts) in shapes.items():
        for k in ('range', 'voxel', 'grid', 'caps'):
            out[f'{tag}.{k}'] = np.array(geo[k])
        out[f'{tag}.B'], out[f'{tag}.T'] = np.int64(geo['B']), np.int64(geo['T'])
        for C in ((4, 5) if tag == 'h1' else (4,)):
            points = np.ascontiguousarray(pts[:, :1 + C])
            out[f'{tag}.c{C}.points'] = points
            for cap in geo['caps']:
                key = f'{tag}.m{cap}.c{C}'
                v = hvr.voxelize_batch(points, geo['B'], geo['range'], geo['voxel'], geo['grid'], geo['T'], cap)
                w = hvr.voxelize_batch(points, geo['B'], geo['range'], geo['voxel'], geo['grid'], geo['T'], cap, voxelize=hvr.voxelize_closed_form)
                assert all(np.array_equal(v[k], w[k]) for k in v), f'{key}: the closed form differs from the loop'
                vox[key] = v
                for k in ('slot_rows', 'voxel_coords', 'voxel_num_points'):
                    out[f'{key}.{k}'] = v[k]
                num = np.maximum(v['voxel_num_points'], 1)[:, None]
                out[f'{key}.voxel_mean64'] = v['voxels'].astype(np.float64).sum(1) / num
                with torch.no_grad():
                    m = mean_vfe.MeanVFE(model_cfg=EasyDict({}), num_point_features=C)(
                        {'voxels': torch.from_numpy(v['voxels']), 'voxel_num_points': torch.from_numpy(v['voxel_num_points'])})
                out[f'{key}.mean_vfe'] = m['voxel_features'].numpy()
                print(key, 'voxels', len(v['voxel_num_points']), 'max points', int(v['voxel_num_points'].max()), 'rows kept',
                      int((v['slot_rows'] >= 0).sum()), 'of', len(points))

    # what the shapes promise
    v50, v2000 = vox['h1.m50.c4'], vox['h1.m2000.c4']
    T = H1['T']
    per_sample = [int((v50['voxel_coords'][:, 0] == b).sum()) for b in range(3)]
    assert per_sample == [50, 0, 50] and not (h1[:, 0] == 1).any(), per_sample
    assert [int((v2000['voxel_coords'][:, 0] == b).sum()) < 2000 for b in range(3)] == [True] * 3
    kept50 = set(v50['slot_rows'].reshape(-1).tolist())
    assert ara[0] in kept50 and ara[2] in kept50 and ara[1] not in kept50 and ara[1] in set(v2000['slot_rows'].reshape(-1).tolist())
    row_a = v50['slot_rows'][0]
    assert v50['voxel_coords'][0, 0] == 0 and ara[0] in row_a and ara[2] in row_a and v50['voxel_num_points'][0] < T
    cells = hvr.cells_of(h1[:, 1:4], H1['range'], H1['voxel'])
    ok = hvr.inside(cells, H1['grid'])
    keys = (h1[ok, 0].astype(np.int64) * 40 + cells[ok, 0].astype(np.int64)) * 24 + cells[ok, 1].astype(np.int64)
    counts = np.unique(keys, return_counts=True)[1]
    assert (counts == T).any() and (counts == T + 1).any() and counts.max() >= 1100 and (counts == 1).any()
    z_only = (h1[:, 4 - 1] >= 1.0) | (h1[:, 4 - 1] < -3.0)
    xy_in = hvr.inside(np.concatenate([cells[:, :2], np.zeros((len(cells), 1), dtype=f32)], 1), H1['grid'])
    assert (z_only & xy_in).sum() > 10 and not ok[z_only & xy_in].any()
    assert (np.diff(v2000['voxel_coords'][:, 0] * 960 + v2000['voxel_coords'][:, 3] * 24 + v2000['voxel_coords'][:, 2]) < 0).any()      # not key order
    h3v = vox['h3.m40000.c4']
    assert (h3v['voxel_coords'][:, 0] == 31).sum() > 20 and 31 * 1408 * 1600 * 40 > 2 ** 31

    # the reference's PillarVFE: (name, voxelization, C, kwargs)
    runs = [('h1.m2000.c4', 'h1.m2000.c4', 4, {}), ('h1.m50.c4', 'h1.m50.c4', 4, {})]
    runs += [(f'h1.m2000.c4.abs{int(a)}.dist{int(d)}', 'h1.m2000.c4', 4, dict(use_absolute_xyz=a, with_distance=d, num_filters=(16,)))
             for a in (True, False) for d in (True, False) if not (a and not d)]
    runs += [('h1.m2000.c5', 'h1.m2000.c5', 5, dict(num_filters=(16,))), ('h1.m2000.c4.f32_64', 'h1.m2000.c4', 4, dict(num_filters=(32, 64))),
             ('h1.m2000.c4.nonorm', 'h1.m2000.c4', 4, dict(use_norm=False, num_filters=(16,))),
             ('h1.m2000.c5.dist.nonorm', 'h1.m2000.c5', 5, dict(use_norm=False, with_distance=True, num_filters=(16,)))]
    wins = 0
    for seed, (name, key, C, kw) in enumerate(runs):
        geo = H1
        vfe = make_pillar_vfe(pillar_vfe, geo, C, seed=seed, **kw)
        feats, first_in = run_pillar_vfe(vfe, vox[key])
        assert feats.shape == (len(vox[key]['voxel_num_points']), kw.get('num_filters', (64,))[-1])
        out[f'{name}.features'] = first_in.numpy()
        pfn[f'{name}.pillar_features'] = feats.numpy()
        for k, v in vfe.state_dict().items():
            pfn[f'{name}.state.{k}'] = v.numpy()
        manifest[f'PillarVFE({name})'] = {k: list(v.shape) for k, v in vfe.state_dict().items()}
        if kw.get('with_distance', False):
            # the norm column is sqrt(fma(z, z, fma(y, y, x * x))) in fp32: what the operators pin (products exact in double)
            xyz = vox[key]['voxels'][:, :, :3].astype(np.float64)
            acc = f32(xyz[..., 0] * xyz[..., 0]).astype(np.float64)
            for d in (1, 2):
                acc = f32(xyz[..., d] * xyz[..., d] + acc).astype(np.float64)
            real = np.arange(geo['T'])[None, :] < vox[key]['voxel_num_points'][:, None]
            assert (np.where(real, np.sqrt(acc.astype(f32)), 0) == first_in.numpy()[..., -1]).all(), 'distance column: another rounding sequence'
        if len(vfe.pfn_layers) == 1:
            n = padding_wins(vfe, first_in, vox[key]['voxel_num_points'], geo['T'])
            print(name, 'voxel x channel pairs whose maximum is the padding value:', n)
            wins += n if name == 'h1.m2000.c4' else 0
    assert wins > 0, 'no voxel with fewer than T points has the padding value as its maximum'
    manifest['MeanVFE'] = {}
    manifest['runs'] = [[name, key, C, {k: (list(v) if isinstance(v, tuple) else v) for k, v in kw.items()}] for name, key, C, kw in runs]
    np.savez_compressed(os.path.join(HERE, 'ref_hard_voxel.npz'), **out)
    np.savez_compressed(os.path.join(HERE, 'ref_hard_voxel_pfn.npz'), **pfn)
    with open(os.path.join(HERE, 'ref_hard_voxel_manifest.json'), 'w') as f:
        json.dump(manifest, f, indent=1, sort_keys=True)
    for n in ('ref_hard_voxel.npz', 'ref_hard_voxel_pfn.npz', 'ref_hard_voxel_manifest.json'):
        size = os.path.getsize(os.path.join(HERE, n))
        print(n, size, 'bytes')
        assert size < 1 << 20


if __name__ == '__main__':
    main()

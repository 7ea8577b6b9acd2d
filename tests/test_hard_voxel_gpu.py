"""Hard voxelization and its encoders on the device (csrc/hard_voxel.hip) against tests/golden/ref_hard_voxel*.npz, written by
gen_hard_voxel_fixtures.py: the voxelization by the numpy restatement of the generator's loop (hard_voxel_reference.py), the
encoders by the reference's own MeanVFE / PillarVFE on the CPU.  Shapes H1 - H3 are described in the generator.  Inputs and
outputs are carved from a poisoned Arena: the points sit 4 bytes off a 16-byte boundary between NaN red zones.

Exact: slot_rows, voxel_coords, voxel_num_points, M, the padded voxels tensor bit for bit, every feature column but f_cluster,
and two runs of everything.
Bounded: the voxel mean and f_cluster against a float64 mean, |err| <= n 2^-23 max|v in the voxel| (n <= T the voxel's count:
twice the first-order worst case of an n-term fp32 sum, n 2^-24 max|v|, which also covers the division's rounding); the PFN
outputs against the fixture at 1e-4 absolute (the generator asserts n_in 2^-24 max sum |w x| |scale| <= 1e-4 on these inputs).
"""
import copy
import json
import os

import numpy as np
import pytest
import torch

from arena import Arena
from pdm_ssd_amd import _native, hard_voxel_ops
from pdm_ssd_amd.config import cfg_from_dict

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# (shape tag, C, max_voxels per sample)
CASES = [('h1', 4, 50), ('h1', 4, 2000), ('h1', 5, 50), ('h1', 5, 2000), ('h2', 4, 100), ('h2', 4, 5000), ('h2s', 4, 40000), ('h3', 4, 40000)]
CASE_IDS = [f'{t}.m{m}.c{c}' for t, c, m in CASES]


@pytest.fixture(scope="module")
def ref():
    z = np.load(os.path.join(GOLDEN, "ref_hard_voxel.npz"))
    return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def pfn():
    z = np.load(os.path.join(GOLDEN, "ref_hard_voxel_pfn.npz"))
    return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def runs():
    with open(os.path.join(GOLDEN, "ref_hard_voxel_manifest.json")) as f:
        return json.load(f)['runs']


@pytest.fixture(scope="module")
def arena(dev):
    return Arena(dev)


def geo_of(ref, tag):
    return dict(point_cloud_range=[float(v) for v in ref[f'{tag}.range']], voxel_size=[float(v) for v in ref[f'{tag}.voxel']],
                grid_size=[int(v) for v in ref[f'{tag}.grid']]), int(ref[f'{tag}.B']), int(ref[f'{tag}.T'])


def expected_voxels(points, slot_rows):
    return np.where(slot_rows[:, :, None] >= 0, points[np.maximum(slot_rows, 0)][:, :, 1:], np.float32(0)).astype(np.float32)


def raw_voxelize(arena, dev, points_np, geo, B, T, max_voxels, with_voxels=True):
    """pdm_hard_voxelize on arena views (the workspace too, unless it is larger than the arena) -> (points view, outputs
    sliced to M, the capacity-sized views)"""
    nx, ny, nz = geo['grid_size']
    N, C1 = points_np.shape
    cap = min(N, B * max_voxels, B * nx * ny * nz)
    pts = arena.put(points_np, misalign_bytes=4, poison=float('nan'))
    i32 = torch.int32
    o = {'slot_rows': arena.carve((cap, T), i32, 4), 'voxel_coords': arena.carve((cap, 4), i32, 12), 'voxel_num_points': arena.carve(cap, i32, 8),
         'record': arena.carve(2, i32, 8)}
    if with_voxels:
        o['voxels'] = arena.carve((cap, T, C1 - 1), torch.float32, 4)
    nbytes = _native.lib().pdm_hard_voxelize_workspace_bytes(N, B, nx, ny, nz)
    assert nbytes > 0
    ws = arena.carve(nbytes, torch.uint8, 8) if nbytes <= (8 << 20) else torch.empty(nbytes, dtype=torch.uint8, device=dev)
    r, v = geo['point_cloud_range'], geo['voxel_size']
    _native.call("pdm_hard_voxelize", _native.stream(dev), N, C1, pts.data_ptr(), B, nx, ny, nz, r[0], r[1], r[2], v[0], v[1], v[2], T, max_voxels,
                 o['slot_rows'].data_ptr(), o['voxel_coords'].data_ptr(), o['voxel_num_points'].data_ptr(),
                 o['voxels'].data_ptr() if with_voxels else None, o['record'].data_ptr(), ws.data_ptr(), nbytes)
    torch.cuda.synchronize()
    arena.check()
    M, unsorted = o['record'].tolist()
    return pts, {k: (t[:M] if k != 'record' else t) for k, t in o.items()}, M, unsorted


def as_hard_voxels(o, M, B, grid):
    return hard_voxel_ops.HardVoxels(o.get('voxels'), o['voxel_coords'], o['voxel_num_points'], o['slot_rows'], M, B, tuple(grid))


def mean_bound(ref, key, points):
    """(M, C): n 2^-23 max|v| per voxel and column"""
    slots, num = ref[f'{key}.slot_rows'], ref[f'{key}.voxel_num_points']
    big = np.abs(expected_voxels(points, slots)).astype(np.float64).max(1)
    return num[:, None] * 2.0 ** -23 * big


@pytest.mark.parametrize("tag, C_, cap", CASES, ids=CASE_IDS)
def test_voxelize_equals_the_fixture_exactly(ref, arena, dev, tag, C_, cap):
    geo, B, T = geo_of(ref, tag)
    key, points = f'{tag}.m{cap}.c{C_}', ref[f'{tag}.c{C_}.points']
    arena.reset()
    _, o, M, unsorted = raw_voxelize(arena, dev, points, geo, B, T, cap)
    assert unsorted == 0 and M == len(ref[f'{key}.voxel_num_points'])
    for name in ('slot_rows', 'voxel_coords', 'voxel_num_points'):
        assert np.array_equal(o[name].cpu().numpy(), ref[f'{key}.{name}']), name
    want = expected_voxels(points, ref[f'{key}.slot_rows'])
    assert np.array_equal(o['voxels'].cpu().numpy().view(np.int32), want.view(np.int32))           # bit for bit, padding zeros included
    # a second run into other views, without the padded tensor: the same bits, and nothing written anywhere else
    _, o2, M2, _ = raw_voxelize(arena, dev, points, geo, B, T, cap, with_voxels=False)
    assert M2 == M and all(torch.equal(o[name], o2[name]) for name in ('slot_rows', 'voxel_coords', 'voxel_num_points'))
    # materialize on its own equals the in-call tensor
    out = arena.carve((M, T, C_), torch.float32, 4)
    _native.call("pdm_hard_voxel_materialize", _native.stream(dev), M, T, C_ + 1, arena.put(points, 4, poison=float('nan')).data_ptr(),
                 o2['slot_rows'].data_ptr(), out.data_ptr())
    torch.cuda.synchronize()
    arena.check()
    assert torch.equal(out.view(torch.int32), o['voxels'].view(torch.int32))
    if tag == 'h1':
        per_sample = [int((o['voxel_coords'][:, 0] == b).sum()) for b in range(B)]
        assert per_sample[1] == 0 and (per_sample == [50, 0, 50]) == (cap == 50) and int(o['voxel_num_points'].max()) == T
    if tag == 'h3':
        assert int((o['voxel_coords'][:, 0] == 31).sum()) > 20


def test_the_module_level_voxelize_reads_the_host_once_and_slices(ref, arena, dev):
    geo, B, T = geo_of(ref, 'h1')
    arena.reset()
    pts = arena.put(ref['h1.c4.points'], 4, poison=float('nan'))
    before = hard_voxel_ops.HOST_READS
    hv = hard_voxel_ops.voxelize(pts, B, max_points_per_voxel=T, max_voxels=50, materialize=True, **geo)
    assert hard_voxel_ops.HOST_READS - before == 1 and hv.num_voxels == 100 and hv.voxels.shape == (100, T, 4) and hv.slot_rows.shape == (100, T)
    assert np.array_equal(hv.slot_rows.cpu().numpy(), ref['h1.m50.c4.slot_rows']) and hv.voxel_coords.dtype == torch.int32
    assert torch.equal(hard_voxel_ops.materialize(pts, hv), hv.voxels) and hard_voxel_ops.HOST_READS - before == 1
    assert hard_voxel_ops.voxelize(pts, B, max_points_per_voxel=T, max_voxels=50, **geo).voxels is None
    arena.check()


@pytest.mark.parametrize("how", ['swapped_samples', 'one_row_back', 'nan'])
def test_unsorted_rows_raise_and_write_nowhere_else(ref, arena, dev, how):
    geo, B, T = geo_of(ref, 'h1')
    p = ref['h1.c4.points'].copy()
    if how == 'swapped_samples':
        p = p[::-1].copy()
    elif how == 'one_row_back':
        p[len(p) // 2, 0] = 0.0                # a row of sample 0 in the middle of sample 2
    else:
        p[7, 0] = np.nan
    arena.reset()
    _, o, M, unsorted = raw_voxelize(arena, dev, p, geo, B, T, 50)          # checks the red zones
    assert unsorted == 1 and M == 0
    pts = arena.put(p, 4, poison=float('nan'))
    with pytest.raises(ValueError, match='samples ascending'):
        hard_voxel_ops.voxelize(pts, B, max_points_per_voxel=T, max_voxels=50, **geo)
    arena.check()


def test_no_points_and_no_kept_points_give_no_voxels(ref, arena, dev):
    geo, B, T = geo_of(ref, 'h1')
    hv = hard_voxel_ops.voxelize(torch.zeros((0, 5), device=dev), B, max_points_per_voxel=T, max_voxels=50, materialize=True, **geo)
    assert hv.num_voxels == 0 and hv.voxels.shape == (0, T, 4) and hv.slot_rows.shape == (0, T) and hv.voxel_coords.shape == (0, 4)
    assert hard_voxel_ops.voxel_mean(torch.zeros((0, 5), device=dev), hv).shape == (0, 4)
    outside = np.array([[-1, 3.0, 0.0, 0, 0.5], [0, 25.0, 0, 0, 0.5], [0, 3.0, 0.0, 9.0, 0.5], [1, -0.5, 0, 0, 0.1], [2, 3.0, -7.0, 0, 0.5],
                        [5, 3.0, 0.0, 0, 0.5]], dtype=np.float32)
    arena.reset()
    _, o, M, unsorted = raw_voxelize(arena, dev, outside, geo, B, T, 50)
    assert M == 0 and unsorted == 0


@pytest.mark.parametrize("tag, C_, cap", CASES, ids=CASE_IDS)
def test_voxel_mean_stays_within_the_summation_bound(ref, arena, dev, tag, C_, cap):
    geo, B, T = geo_of(ref, tag)
    key, points = f'{tag}.m{cap}.c{C_}', ref[f'{tag}.c{C_}.points']
    arena.reset()
    pts = arena.put(points, 4, poison=float('nan'))
    slots = arena.put(ref[f'{key}.slot_rows'], 4, poison=0)
    num = arena.put(ref[f'{key}.voxel_num_points'], 4, poison=T)
    M = len(num)
    outs = []
    for _ in range(2):
        out = arena.carve((M, C_), torch.float32, 4)
        _native.call("pdm_hard_voxel_mean", _native.stream(dev), M, T, C_ + 1, pts.data_ptr(), slots.data_ptr(), num.data_ptr(), out.data_ptr())
        torch.cuda.synchronize()
        arena.check()
        outs.append(out)
    assert torch.equal(outs[0], outs[1])
    bound = mean_bound(ref, key, points)
    err = np.abs(outs[0].cpu().numpy().astype(np.float64) - ref[f'{key}.voxel_mean64'])
    print(f'{key}: voxel_mean worst error {err.max():.3g}, worst error / bound {(err / np.maximum(bound, 1e-300)).max():.3g}')
    assert (err <= bound).all()
    # the module: on the device's own voxelization, and on a batch that already holds the reference's voxels
    from pdm_ssd_amd.vfe import MeanVFE
    cfg = cfg_from_dict({'MAX_POINTS_PER_VOXEL': T, 'MAX_NUMBER_OF_VOXELS': {'train': 1, 'test': cap}})
    vfe = MeanVFE(model_cfg=cfg, num_point_features=C_, **geo).eval()
    before = hard_voxel_ops.HOST_READS
    bd = vfe({'points': pts, 'batch_size': B})
    assert hard_voxel_ops.HOST_READS - before == 1
    assert torch.equal(bd['voxel_features'], outs[0]) and np.array_equal(bd['voxel_coords'].cpu().numpy(), ref[f'{key}.voxel_coords'])
    assert np.array_equal(bd['voxel_num_points'].cpu().numpy(), ref[f'{key}.voxel_num_points'])
    given = {'voxels': torch.from_numpy(expected_voxels(points, ref[f'{key}.slot_rows'])).to(dev), 'voxel_num_points': num,
             'voxel_coords': torch.from_numpy(ref[f'{key}.voxel_coords']).to(dev)}
    got = vfe(dict(given))['voxel_features']
    assert hard_voxel_ops.HOST_READS - before == 1
    for name, t in (('given voxels', got), ('the reference MeanVFE', torch.from_numpy(ref[f'{key}.mean_vfe']))):
        err = np.abs(t.cpu().numpy().astype(np.float64) - ref[f'{key}.voxel_mean64'])
        assert (err <= bound).all(), name


def build_vfe(ref, pfn, name, C_, kw, dev, cap=2000):
    from pdm_ssd_amd.vfe import PillarVFE
    geo, B, T = geo_of(ref, 'h1')
    cfg = {'USE_NORM': kw.get('use_norm', True), 'WITH_DISTANCE': kw.get('with_distance', False), 'USE_ABSLOTE_XYZ': kw.get('use_absolute_xyz', True),
           'NUM_FILTERS': list(kw.get('num_filters', [64])), 'MAX_POINTS_PER_VOXEL': T, 'MAX_NUMBER_OF_VOXELS': cap}
    vfe = PillarVFE(model_cfg=cfg_from_dict(cfg), num_point_features=C_, **geo)
    vfe.load_state_dict({k[len(f'{name}.state.'):]: torch.from_numpy(v) for k, v in pfn.items() if k.startswith(f'{name}.state.')})
    return vfe.to(dev).eval(), geo, B, T


def run_ids():
    with open(os.path.join(GOLDEN, "ref_hard_voxel_manifest.json")) as f:
        return [r[0] for r in json.load(f)['runs']]


@pytest.mark.parametrize("index", range(9), ids=run_ids())
def test_features_and_pfn_outputs_equal_the_reference(ref, pfn, runs, arena, dev, index):
    """every recorded configuration: the composed path's (M, T, F) feature rows against the fixture's (f_cluster within the
    summation bound, every other column exactly), and the (M, K) outputs of the module (fused for one layer), of the fused
    operator on arena views and of the composed formulation at 1e-4 absolute"""
    name, key, C_, kw = runs[index]
    cap = int(key.split('.')[1][1:])
    vfe, geo, B, T = build_vfe(ref, pfn, name, C_, kw, dev, cap)
    points = ref[f'h1.c{C_}.points']
    arena.reset()
    pts = arena.put(points, 4, poison=float('nan'))
    want = torch.from_numpy(pfn[f'{name}.pillar_features']).to(dev)
    with torch.no_grad():
        before = hard_voxel_ops.HOST_READS
        bd = vfe({'points': pts, 'batch_size': B})
        assert hard_voxel_ops.HOST_READS - before == 1
        again = vfe({'points': pts, 'batch_size': B})
        hv = hard_voxel_ops.voxelize(pts, B, max_points_per_voxel=T, max_voxels=cap, materialize=True, **geo)
        feats = vfe.features_of(hv.voxels, hv.voxel_num_points, hv.voxel_coords)
        composed = vfe.composed(hv.voxels, hv.voxel_num_points, hv.voxel_coords)
        given = vfe({'voxels': hv.voxels, 'voxel_num_points': hv.voxel_num_points, 'voxel_coords': hv.voxel_coords})['pillar_features']
    arena.check()
    assert np.array_equal(bd['voxel_coords'].cpu().numpy(), ref[f'{key}.voxel_coords']) and bd['pillar_features'] is bd['voxel_features']
    assert torch.equal(bd['pillar_features'], again['pillar_features']) and 'pillar_cell_table' not in bd
    # feature rows
    got, ref_rows = feats.cpu().numpy(), ref[f'{name}.features']
    assert got.shape == ref_rows.shape
    abs_xyz = kw.get('use_absolute_xyz', True)
    c0 = C_ if abs_xyz else C_ - 3
    exact = [c for c in range(got.shape[2]) if not c0 <= c < c0 + 3]
    assert np.array_equal(got[:, :, exact], ref_rows[:, :, exact]), [c for c in exact if not np.array_equal(got[:, :, c], ref_rows[:, :, c])]
    slots, num = ref[f'{key}.slot_rows'], ref[f'{key}.voxel_num_points']
    vox = expected_voxels(points, slots)
    real = (np.arange(T)[None, :] < num[:, None])[:, :, None]
    cluster64 = np.where(real, vox[:, :, :3].astype(np.float64) - ref[f'{key}.voxel_mean64'][:, None, :3], 0.0)
    bound = mean_bound(ref, key, points)[:, None, :3]
    err = np.abs(got[:, :, c0:c0 + 3].astype(np.float64) - cluster64)
    print(f'{name}: f_cluster worst error {err.max():.3g}, worst error / bound {(err / np.maximum(bound, 1e-300)).max():.3g}')
    assert (err <= bound).all()
    # outputs
    errs = {'module': float((bd['pillar_features'] - want).abs().max()), 'composed': float((composed - want).abs().max()),
            'given voxels': float((given - want).abs().max())}
    if len(vfe.pfn_layers) == 1:
        w, sc, sh = (arena.put(t.detach().cpu(), 4, poison=float('nan')) for t in vfe.pfn_layers[0].folded())
        fused = hard_voxel_ops.fused_pfn(pts, hv, vfe.geometry, w, sc, sh, vfe.use_absolute_xyz, vfe.with_distance)
        arena.check()
        assert torch.equal(fused, bd['pillar_features'])        # the module took the fused operator
        errs['fused'] = float((fused - want).abs().max())
        pad = torch.relu(sh)[None, :].expand_as(want)
        at = (hv.voxel_num_points[:, None] < T) & ((want - pad).abs() <= 1e-6) & (pad > 0)
        assert int(at.sum()) > 0                                  # voxels whose maximum IS the padding rows' value
        print(f'{name}: {int(at.sum())} (voxel, channel) pairs hold the padding value; worst error there {float((fused - want)[at].abs().max()):.3g}')
    print(f'{name}: PFN worst error ' + ', '.join(f'{k} {v:.3g}' for k, v in errs.items()))
    assert bd['pillar_features'].shape == want.shape and all(v <= 1e-4 for v in errs.values()), errs


def reference_formulation(vfe, voxels, num, coords):
    """The reference PillarVFE's arithmetic, written out here on the layers of `vfe`: what the module's composed path must equal."""
    g = vfe.geometry
    xyz = voxels[:, :, :3]
    mean = xyz.sum(1, keepdim=True) / num.float().view(-1, 1, 1)
    centre = torch.stack([coords[:, 3].float() * g.vx + g.x_offset, coords[:, 2].float() * g.vy + g.y_offset,
                          coords[:, 1].float() * g.vz + g.z_offset], 1)[:, None, :]
    cols = [voxels if vfe.use_absolute_xyz else voxels[:, :, 3:], xyz - mean, xyz - centre]
    if vfe.with_distance:
        cols.append(xyz.norm(dim=2, keepdim=True))
    x = torch.cat(cols, 2) * (torch.arange(voxels.shape[1], device=voxels.device)[None, :] < num[:, None]).float()[:, :, None]
    for layer in vfe.pfn_layers:
        y = layer.linear(x)
        if layer.use_norm:        # batch statistics over all M * T rows, the zero-masked padding included
            y = layer.norm(y.reshape(-1, y.shape[2])).reshape(y.shape)
        y = torch.relu(y)
        top = y.max(1, keepdim=True)[0]
        x = top if layer.last_vfe else torch.cat([y, top.expand(-1, y.shape[1], -1)], 2)
    return x[:, 0, :]


@pytest.mark.parametrize("filters", [[64], [32, 64]])
def test_vfe_training_step_equals_the_reference_formulation(ref, dev, filters):
    """forward in training mode and backward to linear.weight and the norm parameters, against the reference's formulation in
    torch on the same padded tensor: rtol = atol = 1e-4"""
    from pdm_ssd_amd.vfe import PillarVFE
    geo, B, T = geo_of(ref, 'h1')
    torch.manual_seed(11)
    cfg = cfg_from_dict({'USE_NORM': True, 'WITH_DISTANCE': False, 'USE_ABSLOTE_XYZ': True, 'NUM_FILTERS': filters, 'MAX_POINTS_PER_VOXEL': T,
                         'MAX_NUMBER_OF_VOXELS': {'train': 2000, 'test': 50}})
    mine = PillarVFE(model_cfg=cfg, num_point_features=4, **geo).to(dev).train()
    other = copy.deepcopy(mine)
    pts = torch.from_numpy(ref['h1.c4.points']).to(dev)
    key = 'h1.m2000.c4'
    voxels = torch.from_numpy(expected_voxels(ref['h1.c4.points'], ref[f'{key}.slot_rows'])).to(dev)
    proj = torch.randn((64,), device=dev, generator=torch.Generator(device=dev).manual_seed(3))
    a = mine({'points': pts, 'batch_size': B})['pillar_features']
    b = reference_formulation(other, voxels, torch.from_numpy(ref[f'{key}.voxel_num_points']).to(dev), torch.from_numpy(ref[f'{key}.voxel_coords']).to(dev))
    assert a.shape == b.shape == (len(ref[f'{key}.voxel_num_points']), 64) and a.requires_grad
    torch.testing.assert_close(a, b, rtol=1e-4, atol=1e-4)
    ((a * proj).sum() / a.shape[0]).backward()
    ((b * proj).sum() / b.shape[0]).backward()
    names = [n for n, _ in mine.named_parameters()]
    assert 'pfn_layers.0.linear.weight' in names and 'pfn_layers.0.norm.weight' in names and 'pfn_layers.0.norm.bias' in names
    for (n, p), (_, q) in zip(mine.named_parameters(), other.named_parameters()):
        assert p.grad is not None and torch.isfinite(p.grad).all() and float(p.grad.abs().max()) > 0, n
        torch.testing.assert_close(p.grad, q.grad, rtol=1e-4, atol=1e-4, msg=lambda m: f'{n}: {m}')
    for (n, p), (_, q) in zip(mine.named_buffers(), other.named_buffers()):      # the running statistics moved alike
        torch.testing.assert_close(p.float(), q.float(), rtol=1e-4, atol=1e-4, msg=lambda m: f'{n}: {m}')


GT = np.zeros((3, 3, 8), dtype=np.float32)
GT[0, 0] = [6.0, 1.0, -1.0, 3.9, 1.6, 1.5, 0.3, 1]
GT[0, 1] = [12.0, -3.0, -0.8, 0.8, 0.6, 1.7, -1.2, 2]
GT[1, 0] = [5.0, -2.2, -0.9, 1.7, 0.6, 1.7, 2.1, 3]
GT[2, 0] = [15.7, -2.2, -0.9, 1.7, 0.6, 1.7, 2.1, 3]


def run_detector(model, batch, B, dev):
    """eval, then one training step; hard_voxel_ops reads the host once per forward"""
    model.eval()
    with torch.no_grad():
        before = hard_voxel_ops.HOST_READS
        pred, recall = model(dict(batch))
        assert hard_voxel_ops.HOST_READS - before == 1
    assert len(pred) == B
    for p in pred:
        assert p['pred_boxes'].shape[1] == 7 and torch.isfinite(p['pred_boxes']).all() and torch.isfinite(p['pred_scores']).all()
    model.train()
    before = hard_voxel_ops.HOST_READS
    ret, tb, _ = model(dict(batch))
    ret['loss'].backward()
    assert hard_voxel_ops.HOST_READS - before == 1 and torch.isfinite(ret['loss'])
    for n, p in model.named_parameters():
        if p.requires_grad:
            assert p.grad is not None and torch.isfinite(p.grad).all(), n


def test_point_pillar_on_hard_voxels_runs_eval_and_a_training_step(ref, dev):
    from pdm_ssd_amd import detector_config as dc
    geo, B, T = geo_of(ref, 'h1')
    torch.manual_seed(2)
    cfg = copy.deepcopy(dc.POINT_PILLAR_HARD_CFG)
    cfg['VFE'].update(MAX_POINTS_PER_VOXEL=T, MAX_NUMBER_OF_VOXELS={'train': 200, 'test': 2000})
    cfg['BACKBONE_2D'] = {'NAME': 'BaseBEVBackbone', 'LAYER_NUMS': [1], 'LAYER_STRIDES': [2], 'NUM_FILTERS': [32], 'UPSAMPLE_STRIDES': [1],
                          'NUM_UPSAMPLE_FILTERS': [32]}        # one block: the 20 x 12 map the anchors' stride 2 expects
    model = dc.build_point_pillar(cfg, dataset=dc.pillar_dataset(4, **geo)).to(dev)
    assert [type(m).__name__ for m in model.module_list] == ['PillarVFE', 'PointPillarScatter', 'BaseBEVBackbone', 'AnchorHeadSingle']
    batch = {'batch_size': B, 'points': torch.from_numpy(ref['h1.c4.points']).to(dev), 'gt_boxes': torch.from_numpy(GT).to(dev)}
    run_detector(model, batch, B, dev)
    assert float(model.vfe.pfn_layers[0].linear.weight.grad.abs().max()) > 0


def test_second_on_hard_voxels_runs_eval_and_a_training_step(ref, dev):
    """H2's range and its 16 x 16 cells in x and y; 40 cells of 0.1 m in z, because VoxelBackBone8x and the 256-channel
    HeightCompression need the KITTI depth (H2's 8 cells leave the last strided convolution no output)"""
    from pdm_ssd_amd import detector_config as dc
    geo, B, T = geo_of(ref, 'h2')
    geo = dict(geo, voxel_size=[0.5, 0.5, 0.1], grid_size=[16, 16, 40])
    torch.manual_seed(5)
    cfg = copy.deepcopy(dc.SECOND_HARD_CFG)
    cfg['VFE'].update(MAX_NUMBER_OF_VOXELS={'train': 300, 'test': 5000})
    model = dc.build_second(cfg, dataset=dc.voxel_dataset(4, **geo)).to(dev)
    assert [type(m).__name__ for m in model.module_list] == ['MeanVFE', 'VoxelBackBone8x', 'HeightCompression', 'BaseBEVBackbone', 'AnchorHeadSingle']
    gt = GT[:B].copy()
    gt[:, :, 0] *= 0.4
    batch = {'batch_size': B, 'points': torch.from_numpy(ref['h2.c4.points']).to(dev), 'gt_boxes': torch.from_numpy(gt).to(dev)}
    run_detector(model, batch, B, dev)
    assert bool(model.backbone_3d.conv_input[0].weight.grad.any())

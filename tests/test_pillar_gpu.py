"""The pillar path's device operators (csrc/pillar.hip) against the reference's own results (tests/golden/ref_pillar*.npz,
written by gen_pillar_fixtures.py from the reference's DynamicPillarVFE / PointPillarScatter) and, for gradients, against
the torch formulation.  Shapes G1 - G3 are described in the generator.  Inputs and outputs are carved from a poisoned
Arena: the points sit 4 bytes off a 16-byte boundary between NaN red zones, index inputs between in-range values.

Exact: kept_idx, unq_inv, voxel_coords, pillar_count, cell_table, every feature column but f_cluster, the canvas, the
scatter and segment-max gradients, and two runs of everything.
Bounded: pillar_mean and f_cluster against a float64 mean, |err| <= n 2^-23 max|coordinate in the pillar| + 2^-20 (n the
pillar's count: twice the first-order worst case of any fp32 summation order, plus the fixed-point step); the PFN outputs
against the fixture at 1e-4 absolute (the generator asserts n_in 2^-24 max sum |w x| |scale| <= 1e-4 on these inputs).
"""
import copy
import os

import numpy as np
import pytest
import torch

from arena import Arena
from pdm_ssd_amd import _native, pillar_ops
from pdm_ssd_amd.config import cfg_from_dict

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# (fixture name, shape tag, C, config overrides)
CONFIGS = [('g1.c4', 'g1', 4, {}), ('g1.c4.abs1.dist1', 'g1', 4, dict(WITH_DISTANCE=True)),
           ('g1.c4.abs0.dist1', 'g1', 4, dict(USE_ABSLOTE_XYZ=False, WITH_DISTANCE=True)),
           ('g1.c4.abs0.dist0', 'g1', 4, dict(USE_ABSLOTE_XYZ=False)), ('g1.c5', 'g1', 5, {}),
           ('g1.c4.f32_64', 'g1', 4, dict(NUM_FILTERS=[32, 64])), ('g1.c4.nonorm', 'g1', 4, dict(USE_NORM=False)),
           ('g1.c5.dist.nonorm', 'g1', 5, dict(USE_NORM=False, WITH_DISTANCE=True)), ('g2.c4', 'g2', 4, {}), ('g3.c4', 'g3', 4, {})]
IDS = [c[0] for c in CONFIGS]
SHAPES = [('g1', 4), ('g1', 5), ('g2', 4), ('g3', 4)]


@pytest.fixture(scope="module")
def ref():
    z = np.load(os.path.join(GOLDEN, "ref_pillar.npz"))
    return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def pfn():
    z = np.load(os.path.join(GOLDEN, "ref_pillar_pfn.npz"))
    return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def arena(dev):
    return Arena(dev)


def geo_of(ref, tag):
    return dict(point_cloud_range=[float(v) for v in ref[f'{tag}.range']], voxel_size=[float(v) for v in ref[f'{tag}.voxel']],
                grid_size=[int(v) for v in ref[f'{tag}.grid']]), int(ref[f'{tag}.B'])


def vfe_cfg(**kw):
    return cfg_from_dict(dict({'USE_NORM': True, 'WITH_DISTANCE': False, 'USE_ABSLOTE_XYZ': True, 'NUM_FILTERS': [64]}, **kw))


def raw_assign(arena, dev, points_np, geo, B):
    """pdm_pillar_assign on arena views -> (points view, dict of the sliced outputs)"""
    nx, ny, nz = geo['grid_size']
    N, C1 = points_np.shape
    ncell = B * nx * ny
    cap = min(N, ncell)
    pts = arena.put(points_np, misalign_bytes=4, poison=float('nan'))
    i32 = torch.int32
    o = {'kept_idx': arena.carve(N, i32, 4), 'unq_inv': arena.carve(N, i32, 8), 'voxel_coords': arena.carve((cap, 4), i32, 12),
         'pillar_count': arena.carve(cap, i32, 4), 'pillar_mean': arena.carve((cap, 3), torch.float32, 4), 'cell_table': arena.carve(ncell, i32, 4),
         'seg_start': arena.carve(cap + 1, i32, 12), 'seg_rows': arena.carve(N, i32, 4), 'record': arena.carve(2, i32, 8)}
    nbytes = _native.lib().pdm_pillar_assign_workspace_bytes(N, B, nx, ny)
    ws = arena.carve(max(nbytes, 8), torch.uint8, 8)
    r, v = geo['point_cloud_range'], geo['voxel_size']
    _native.call("pdm_pillar_assign", _native.stream(dev), N, C1, pts.data_ptr(), B, nx, ny, nz, r[0], r[1], v[0], v[1],
                 *[o[k].data_ptr() for k in ('kept_idx', 'unq_inv', 'voxel_coords', 'pillar_count', 'pillar_mean', 'cell_table', 'seg_start',
                                             'seg_rows', 'record')], ws.data_ptr(), nbytes)
    torch.cuda.synchronize()
    arena.check()
    n_kept, P = o['record'].tolist()
    out = {'kept_idx': o['kept_idx'][:n_kept], 'unq_inv': o['unq_inv'][:n_kept], 'voxel_coords': o['voxel_coords'][:P],
           'pillar_count': o['pillar_count'][:P], 'pillar_mean': o['pillar_mean'][:P], 'cell_table': o['cell_table'],
           'seg_start': o['seg_start'][:P + 1], 'seg_rows': o['seg_rows'][:n_kept], 'num_kept': n_kept, 'num_pillars': P}
    return pts, out


def as_pillars(o, B, grid):
    return pillar_ops.Pillars(o['kept_idx'], o['unq_inv'], o['voxel_coords'], o['pillar_count'], o['pillar_mean'], o['cell_table'],
                              o['seg_start'], o['seg_rows'], o['num_kept'], o['num_pillars'], B, tuple(grid))


def mean_bound(ref, key):
    """(P, 1): n 2^-23 max|coordinate in the pillar| + 2^-20"""
    pts, kept, inv, cnt = ref[f'{key}.points'], ref[f'{key}.kept_idx'], ref[f'{key}.unq_inv'], ref[f'{key}.pillar_count']
    big = np.zeros(len(cnt))
    np.maximum.at(big, inv, np.abs(pts[kept][:, 1:4]).max(1).astype(np.float64))
    return (cnt * 2.0 ** -23 * big + 2.0 ** -20)[:, None]


def sorted_segments(o):
    """the CSR with every segment's rows sorted: what does not depend on the slot order"""
    rows, start = o['seg_rows'].cpu().numpy(), o['seg_start'].cpu().numpy()
    return np.concatenate([np.sort(rows[a:b]) for a, b in zip(start[:-1], start[1:])] + [np.zeros(0, dtype=rows.dtype)])


@pytest.mark.parametrize("tag, C_", SHAPES)
def test_assign_equals_the_reference_exactly(ref, arena, dev, tag, C_):
    geo, B = geo_of(ref, tag)
    key = f'{tag}.c{C_}'
    arena.reset()
    _, o = raw_assign(arena, dev, ref[f'{key}.points'], geo, B)
    for name in ('kept_idx', 'unq_inv', 'voxel_coords', 'pillar_count'):
        assert np.array_equal(o[name].cpu().numpy(), ref[f'{key}.{name}']), name
    P, nx, ny = o['num_pillars'], geo['grid_size'][0], geo['grid_size'][1]
    assert nx != ny and P == len(ref[f'{key}.keys'])
    table = np.full(B * nx * ny, -1, dtype=np.int32)
    table[ref[f'{key}.keys']] = np.arange(P, dtype=np.int32)
    assert np.array_equal(o['cell_table'].cpu().numpy(), table)
    err = np.abs(o['pillar_mean'].cpu().numpy().astype(np.float64) - ref[f'{key}.pillar_mean64'])
    bound = mean_bound(ref, key)
    print(f'{key}: pillar_mean worst error {err.max():.3g}, worst error / bound {(err / bound).max():.3g}')
    assert (err <= bound).all()
    # the CSR: segment p holds exactly the rows of pillar p
    start = o['seg_start'].cpu().numpy()
    assert start[0] == 0 and start[-1] == o['num_kept'] and np.array_equal(np.diff(start), ref[f'{key}.pillar_count'])
    assert np.array_equal(sorted_segments(o), np.argsort(ref[f'{key}.unq_inv'], kind='stable'))
    # a second run into other views: the same bits
    _, o2 = raw_assign(arena, dev, ref[f'{key}.points'], geo, B)
    for name in ('kept_idx', 'unq_inv', 'voxel_coords', 'pillar_count', 'pillar_mean', 'cell_table', 'seg_start'):
        assert torch.equal(o[name], o2[name]), name
    assert np.array_equal(sorted_segments(o), sorted_segments(o2))
    if tag == 'g1':     # the edge rows, by what the issue says of them
        pts = ref[f'{key}.points']
        kept = set(o['kept_idx'].tolist())
        where = {tuple(np.float32(v) for v in row): i for i, row in enumerate(pts[:, 1:4])}
        f = np.float32
        assert where[(f(20.0), f(0.3), f(0.0))] not in kept and where[(f(-1e-7), f(1.0), f(0.0))] not in kept
        assert where[(f(3.0), f(6.0), f(0.0))] not in kept and where[(f(5.2), f(-1.3), f(9.0))] in kept
        first, last = where[(f(0.0), f(-6.0), f(0.0))], where[(np.nextafter(f(20), f(0)), f(5.9), f(0.25))]
        inv = dict(zip(o['kept_idx'].tolist(), o['unq_inv'].tolist()))
        vc = o['voxel_coords'].cpu().numpy()
        assert vc[inv[first]].tolist() == [0, 0, 0, 0] and vc[inv[last]].tolist() == [2, 0, 23, 39]
        # y = nextafter(6, 0) lies inside the range, but the reference's fp32 y - (-6) rounds up to 12.0: cell 24, dropped
        assert where[(np.nextafter(f(20), f(0)), np.nextafter(f(6), f(0)), f(0.5))] not in kept
        assert not (ref[f'{key}.points'][:, 0] == 1).any() and int(o['pillar_count'].max()) > 1024


@pytest.mark.parametrize("name, tag, C_, kw", CONFIGS, ids=IDS)
def test_features_equal_the_reference(ref, arena, dev, name, tag, C_, kw):
    geo, B = geo_of(ref, tag)
    key = f'{tag}.c{C_}'
    arena.reset()
    pts, o = raw_assign(arena, dev, ref[f'{key}.points'], geo, B)
    g = pillar_ops.geometry(geo['point_cloud_range'], geo['voxel_size'])
    abs_xyz, dist = kw.get('USE_ABSLOTE_XYZ', True), kw.get('WITH_DISTANCE', False)
    want = ref[f'{name}.features']
    n, F = want.shape
    assert n == o['num_kept'] and F == pillar_ops.num_features(C_, abs_xyz, dist)
    outs = []
    for _ in range(2):
        out = arena.carve((n, F), torch.float32, 4)
        _native.call("pdm_pillar_features", _native.stream(dev), n, C_ + 1, pts.data_ptr(), o['kept_idx'].data_ptr(), o['unq_inv'].data_ptr(),
                     o['voxel_coords'].data_ptr(), o['pillar_mean'].data_ptr(), *pillar_ops._feature_args(g, abs_xyz, dist), out.data_ptr())
        torch.cuda.synchronize()
        arena.check()
        outs.append(out)
    assert torch.equal(outs[0], outs[1])
    got = outs[0].cpu().numpy()
    c0 = C_ if abs_xyz else C_ - 3                      # first f_cluster column
    exact = [c for c in range(F) if not c0 <= c < c0 + 3]
    assert np.array_equal(got[:, exact], want[:, exact]), [c for c in exact if not np.array_equal(got[:, c], want[:, c])]
    xyz = ref[f'{key}.points'][ref[f'{key}.kept_idx']][:, 1:4].astype(np.float64)
    inv = ref[f'{key}.unq_inv']
    err = np.abs(got[:, c0:c0 + 3].astype(np.float64) - (xyz - ref[f'{key}.pillar_mean64'][inv]))
    bound = mean_bound(ref, key)[inv]
    print(f'{name}: f_cluster worst error {err.max():.3g}, worst error / bound {(err / bound).max():.3g}')
    assert (err <= bound).all()


def torch_segment_max(x, inv, P):
    """(x_max, arg): amax per pillar and the lowest row that holds it"""
    idx = inv.long()[:, None].expand_as(x)
    x_max = torch.zeros((P, x.shape[1]), dtype=x.dtype, device=x.device).scatter_reduce(0, idx, x, 'amax', include_self=False)
    rows = torch.arange(x.shape[0], device=x.device, dtype=torch.float32)[:, None].expand_as(x)      # exact below 2^24
    cand = torch.where(x == x_max[inv.long()], rows, torch.full_like(rows, float(x.shape[0])))
    arg = torch.full((P, x.shape[1]), float(x.shape[0]), device=x.device).scatter_reduce(0, idx, cand, 'amin', include_self=True).long()
    return x_max, arg


@pytest.mark.parametrize("tag, K", [('g1', 64), ('g1', 5), ('g2', 32), ('g3', 7)])
def test_segment_max_and_its_gradient_equal_the_torch_formulation(ref, arena, dev, tag, K):
    geo, B = geo_of(ref, tag)
    key = f'{tag}.c4'
    arena.reset()
    _, o = raw_assign(arena, dev, ref[f'{key}.points'], geo, B)
    n, P = o['num_kept'], o['num_pillars']
    gen = torch.Generator().manual_seed(K)
    x_host = torch.randint(-3, 4, (n, K), generator=gen).float() * 0.25           # few values: ties in every pillar of two rows or more
    x = arena.put(x_host, 4, poison=float('inf'))
    inv = arena.put(o['unq_inv'].cpu(), 4, poison=0)
    start = arena.put(o['seg_start'].cpu(), 4, poison=0)
    rows = arena.put(o['seg_rows'].cpu(), 4, poison=0)
    g_host = torch.randn((P, K), generator=gen)
    gmax = arena.put(g_host, 4, poison=float('nan'))
    res = []
    for _ in range(2):
        x_max, arg, gx = arena.carve((P, K), torch.float32, 4), arena.carve((P, K), torch.int32, 4), arena.carve((n, K), torch.float32, 4)
        _native.call("pdm_pillar_segment_max", _native.stream(dev), P, K, x.data_ptr(), start.data_ptr(), rows.data_ptr(), x_max.data_ptr(),
                     arg.data_ptr())
        _native.call("pdm_pillar_segment_max_grad", _native.stream(dev), n, K, gmax.data_ptr(), arg.data_ptr(), inv.data_ptr(), gx.data_ptr())
        torch.cuda.synchronize()
        arena.check()
        res.append((x_max, arg, gx))
    for a, b in zip(*res):
        assert torch.equal(a, b)
    x_max, arg, gx = res[0]
    want_max, want_arg = torch_segment_max(x, inv, P)
    assert torch.equal(x_max, want_max) and torch.equal(arg.long(), want_arg)
    cols = torch.arange(K, device=dev)[None, :].expand(P, K)
    want_gx = torch.zeros((n, K), device=dev)
    want_gx[want_arg, cols] = gmax
    assert torch.equal(gx, want_gx)
    # and through autograd
    xa = x.clone().requires_grad_(True)
    ya, _ = pillar_ops.segment_max(xa, as_pillars(dict(o, unq_inv=inv, seg_start=start, seg_rows=rows), B, geo['grid_size']))
    ya.backward(gmax)
    assert torch.equal(ya.detach(), want_max) and torch.equal(xa.grad, want_gx)


def build_vfe(ref, pfn, name, tag, C_, kw, dev):
    from pdm_ssd_amd.vfe import DynamicPillarVFE
    geo, B = geo_of(ref, tag)
    vfe = DynamicPillarVFE(model_cfg=vfe_cfg(**kw), num_point_features=C_, **geo)
    vfe.load_state_dict({k[len(f'{name}.state.'):]: torch.from_numpy(v) for k, v in pfn.items() if k.startswith(f'{name}.state.')})
    return vfe.to(dev).eval(), geo, B


@pytest.mark.parametrize("name, tag, C_, kw", CONFIGS, ids=IDS)
def test_pfn_outputs_fused_and_unfused_equal_the_reference(ref, pfn, arena, dev, name, tag, C_, kw):
    """1e-4 absolute on the (P, K) pillar features, both through the fused operator (one PFN layer) and through features +
    nn.Linear + BatchNorm1d + segment_max; the points come from the arena, 4 bytes off alignment between NaN red zones"""
    vfe, geo, B = build_vfe(ref, pfn, name, tag, C_, kw, dev)
    arena.reset()
    pts = arena.put(ref[f'{tag}.c{C_}.points'], 4, poison=float('nan'))
    want = torch.from_numpy(pfn[f'{name}.pillar_features']).to(dev)
    with torch.no_grad():
        bd = vfe({'points': pts, 'batch_size': B})
        again = vfe({'points': pts, 'batch_size': B})
        pillars = pillar_ops.assign(pts, B, **geo)
        x = pillar_ops.features(pts, pillars, vfe.geometry, vfe.use_absolute_xyz, vfe.with_distance)
        for layer in vfe.pfn_layers:
            x = layer(x, pillars)
    arena.check()
    assert np.array_equal(bd['voxel_coords'].cpu().numpy(), ref[f'{tag}.c{C_}.voxel_coords']) and bd['voxel_coords'].dtype == torch.int32
    assert bd['pillar_features'] is bd['voxel_features'] and bd['pillar_cell_table'].numel() == B * geo['grid_size'][0] * geo['grid_size'][1]
    assert torch.equal(bd['pillar_features'], again['pillar_features'])
    err_module, err_unfused = float((bd['pillar_features'] - want).abs().max()), float((x - want).abs().max())
    print(f'{name}: PFN worst error, module path {err_module:.3g}, unfused {err_unfused:.3g}')
    assert bd['pillar_features'].shape == want.shape and err_module <= 1e-4 and err_unfused <= 1e-4
    if len(vfe.pfn_layers) == 1:            # the module took the fused operator: call it on arena views too
        w, sc, sh = (arena.put(t.detach().cpu(), 4, poison=float('nan')) for t in vfe.pfn_layers[0].folded())
        out = pillar_ops.fused_pfn(pts, pillars, vfe.geometry, w, sc, sh, vfe.use_absolute_xyz, vfe.with_distance)
        arena.check()
        assert torch.equal(out, bd['pillar_features'])


@pytest.mark.parametrize("name, tag", [('g1.c4', 'g1'), ('g1.c5', 'g1'), ('g2.c4', 'g2'), ('g3.c4', 'g3')])
@pytest.mark.parametrize("own_table", [True, False])
def test_scatter_equals_the_reference_canvas_and_its_gradient_the_torch_gather(ref, pfn, arena, dev, name, tag, own_table):
    geo, B = geo_of(ref, tag)
    nx, ny, _ = geo['grid_size']
    key = name
    arena.reset()
    vc_host = torch.from_numpy(ref[f'{key}.voxel_coords'])
    vc = arena.put(vc_host, 4, poison=0)
    feats = arena.put(np.ascontiguousarray(pfn[f'{name}.pillar_features'][:, :8]), 4, poison=float('nan'))
    P, C_ = feats.shape
    if own_table:       # no table from the VFE: built from voxel_coords
        table = arena.carve(B * nx * ny, torch.int32, 4)
        _native.call("pdm_pillar_cell_table", _native.stream(dev), P, vc.data_ptr(), B, nx, ny, 1, table.data_ptr())
    else:
        host = np.full(B * nx * ny, -1, dtype=np.int32)
        host[ref[f'{key}.keys']] = np.arange(P, dtype=np.int32)
        table = arena.put(host, 4, poison=0)
    gen = torch.Generator().manual_seed(5)
    gcan = arena.put(torch.randn((B, C_, ny, nx), generator=gen), 4, poison=float('nan'))
    res = []
    for _ in range(2):
        canvas, gf = arena.carve((B, C_, ny, nx), torch.float32, 4), arena.carve((P, C_), torch.float32, 4)
        _native.call("pdm_pillar_scatter", _native.stream(dev), P, C_, feats.data_ptr(), table.data_ptr(), B, nx, ny, 1, canvas.data_ptr())
        _native.call("pdm_pillar_scatter_grad", _native.stream(dev), P, C_, gcan.data_ptr(), vc.data_ptr(), B, nx, ny, 1, gf.data_ptr())
        torch.cuda.synchronize()
        arena.check()
        res.append((canvas, gf))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
    canvas, gf = res[0]
    assert np.array_equal(canvas.cpu().numpy(), ref[f'{name}.canvas'])
    b, cy, cx = (vc[:, i].long() for i in (0, 2, 3))
    assert torch.equal(gf, gcan[b, :, cy, cx])
    # the module, through autograd
    from pdm_ssd_amd.backbones_2d.map_to_bev import PointPillarScatter
    fa = feats.clone().requires_grad_(True)
    bd = {'pillar_features': fa, 'voxel_coords': vc, 'batch_size': B}
    if not own_table:
        bd['pillar_cell_table'] = table
    out = PointPillarScatter(model_cfg=cfg_from_dict({'NUM_BEV_FEATURES': 8}), grid_size=geo['grid_size'])(bd)['spatial_features']
    out.backward(gcan)
    assert torch.equal(out.detach(), canvas) and torch.equal(fa.grad, gf)


@pytest.mark.parametrize("case", ["no_points", "all_outside"])
def test_empty_inputs_give_empty_outputs(ref, arena, dev, case):
    geo, B = geo_of(ref, 'g1')
    nx, ny, _ = geo['grid_size']
    pts_np = np.zeros((0, 5), dtype=np.float32) if case == "no_points" else \
        np.array([[0, 25.0, 0, 0, 0.5], [2, 3.0, -7.0, 0, 0.5], [1, -0.5, 0, 0, 0.1], [5, 3.0, 0.0, 0, 0.5], [-1, 3.0, 0.0, 0, 0.5]], dtype=np.float32)
    arena.reset()
    if case == "no_points":         # (an arena view needs at least one element)
        pts = torch.from_numpy(pts_np).to(dev)
    else:
        pts, o = raw_assign(arena, dev, pts_np, geo, B)
        assert o['num_kept'] == 0 and o['num_pillars'] == 0 and o['seg_start'].tolist() == [0]
        assert bool((o['cell_table'] == -1).all())
    pillars = pillar_ops.assign(pts, B, **geo)
    assert pillars.seg_start.tolist() == [0] and pillars.cell_table.numel() == B * nx * ny and bool((pillars.cell_table == -1).all())
    assert pillars.num_kept == 0 and pillars.num_pillars == 0 and pillars.voxel_coords.shape == (0, 4)
    g = pillar_ops.geometry(geo['point_cloud_range'], geo['voxel_size'])
    f = pillar_ops.features(pts, pillars, g)
    assert f.shape == (0, 10)
    x_max, arg = pillar_ops.segment_max(torch.zeros((0, 64), device=dev), pillars)
    assert x_max.shape == (0, 64) and arg.shape == (0, 64)
    out = pillar_ops.fused_pfn(pts, pillars, g, torch.zeros((64, 10), device=dev), torch.ones(64, device=dev), torch.zeros(64, device=dev))
    assert out.shape == (0, 64)
    canvas = pillar_ops.scatter(out, pillars.cell_table, pillars.voxel_coords, B, geo['grid_size'])
    torch.cuda.synchronize()
    arena.check()
    assert canvas.shape == (B, 64, ny, nx) and not bool(canvas.any())


class TorchPillarVFE(torch.nn.Module):
    """The torch formulation of the encoder on the SAME PFN layers: boolean mask, torch.unique, index_add_ mean,
    scatter_reduce('amax') with the gradient on the lowest winning row (torch_scatter's one-winner rule)."""

    def __init__(self, vfe):
        super().__init__()
        self.vfe = vfe

    def forward(self, points):
        v = self.vfe
        r, s, g = (torch.tensor(t, device=points.device) for t in (v.point_cloud_range, v.voxel_size, v.grid_size))
        pc = torch.floor((points[:, [1, 2]] - r[[0, 1]]) / s[[0, 1]]).int()
        mask = ((pc >= 0) & (pc < g[[0, 1]])).all(dim=1)
        points, pc = points[mask], pc[mask]
        xyz = points[:, 1:4].contiguous()
        merge = points[:, 0].int() * (v.grid_size[0] * v.grid_size[1]) + pc[:, 0] * v.grid_size[1] + pc[:, 1]
        unq, inv, cnt = torch.unique(merge, return_inverse=True, return_counts=True, dim=0)
        mean = torch.zeros((len(unq), 3), device=points.device).index_add_(0, inv, xyz) / cnt[:, None]
        geom = v.geometry
        centre = torch.stack([pc[:, 0].float() * geom.vx + geom.x_offset, pc[:, 1].float() * geom.vy + geom.y_offset,
                              torch.full_like(xyz[:, 2], geom.z_offset)], 1)
        feats = [points[:, 1:] if v.use_absolute_xyz else points[:, 4:], xyz - mean[inv], xyz - centre]
        if v.with_distance:
            feats.append(torch.norm(xyz, 2, dim=1, keepdim=True))
        x = torch.cat(feats, dim=-1)
        for layer in v.pfn_layers:
            y = layer.relu(layer.norm(layer.linear(x)) if layer.use_norm else layer.linear(x))
            with torch.no_grad():
                _, arg = torch_segment_max(y, inv, len(unq))
            y_max = y.gather(0, arg)
            x = y_max if layer.last_vfe else torch.cat([y, y_max[inv]], dim=1)
        return x


@pytest.mark.parametrize("filters", [[64], [32, 64]])
def test_vfe_training_step_equals_the_torch_formulation(ref, dev, filters):
    """forward in training mode (batch statistics over the N' kept points) and backward to linear.weight and the norm
    parameters, against the same layers on the torch formulation: rtol = atol = 1e-4"""
    from pdm_ssd_amd.vfe import DynamicPillarVFE
    geo, B = geo_of(ref, 'g1')
    torch.manual_seed(11)
    mine = DynamicPillarVFE(model_cfg=vfe_cfg(NUM_FILTERS=filters), num_point_features=4, **geo).to(dev).train()
    other = copy.deepcopy(mine)
    plain = TorchPillarVFE(other)
    pts = torch.from_numpy(ref['g1.c4.points']).to(dev)
    proj = torch.randn((64,), device=dev, generator=torch.Generator(device=dev).manual_seed(3))
    a = mine({'points': pts, 'batch_size': B})['pillar_features']
    b = plain(pts)
    assert a.shape == b.shape == (len(ref['g1.c4.keys']), 64)
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


def small_center_pillar(ref):
    from pdm_ssd_amd.detector_config import CENTER_PILLAR_CFG, build_center_pillar, pillar_dataset
    geo, B = geo_of(ref, 'g1')
    cfg = copy.deepcopy(CENTER_PILLAR_CFG)
    cfg['BACKBONE_2D'] = {'NAME': 'BaseBEVBackbone', 'LAYER_NUMS': [1], 'LAYER_STRIDES': [1], 'NUM_FILTERS': [32], 'UPSAMPLE_STRIDES': [1],
                          'NUM_UPSAMPLE_FILTERS': [32]}
    cfg['DENSE_HEAD']['SHARED_CONV_CHANNEL'] = 32
    cfg['DENSE_HEAD']['TARGET_ASSIGNER_CONFIG'].update(FEATURE_MAP_STRIDE=1, NUM_MAX_OBJS=20)
    cfg['DENSE_HEAD']['POST_PROCESSING'].update(MAX_OBJ_PER_SAMPLE=100, POST_CENTER_LIMIT_RANGE=[-1, -7, -4, 21, 7, 3])
    return build_center_pillar(cfg, dataset=pillar_dataset(4, geo['point_cloud_range'], geo['voxel_size'], geo['grid_size'])), B


def test_center_pillar_detector_runs_eval_and_a_training_step_with_one_host_read(ref, dev):
    torch.manual_seed(2)
    model, B = small_center_pillar(ref)
    model = model.to(dev)
    assert [type(m).__name__ for m in model.module_list] == ['DynamicPillarVFE', 'PointPillarScatter', 'BaseBEVBackbone', 'CenterHead']
    pts = torch.from_numpy(ref['g1.c4.points']).to(dev)
    gt = np.zeros((B, 3, 8), dtype=np.float32)
    gt[0, 0] = [6.0, 1.0, -1.0, 3.9, 1.6, 1.5, 0.3, 1]
    gt[0, 1] = [12.0, -3.0, -0.8, 0.8, 0.6, 1.7, -1.2, 2]
    gt[2, 0] = [15.7, -2.2, -0.9, 1.7, 0.6, 1.7, 2.1, 3]
    batch = {'batch_size': B, 'points': pts, 'gt_boxes': torch.from_numpy(gt).to(dev)}
    model.eval()
    with torch.no_grad():
        for head in model.dense_head.heads_list:
            head.hm[-1].bias.fill_(-1.0)
        before = pillar_ops.HOST_READS
        pred, recall = model(dict(batch))
        assert pillar_ops.HOST_READS - before == 1
    assert len(pred) == B and recall['gt'] == 3
    for p in pred:
        assert p['pred_boxes'].shape[1] == 7 and torch.isfinite(p['pred_boxes']).all() and torch.isfinite(p['pred_scores']).all()
    model.train()
    params = [p for p in model.parameters() if p.requires_grad]
    before = pillar_ops.HOST_READS
    ret, tb, _ = model(dict(batch))
    ret['loss'].backward()
    assert pillar_ops.HOST_READS - before == 1
    assert torch.isfinite(ret['loss']) and float(tb['loc_loss_head_0']) > 0
    for n, p in model.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), n
    assert float(model.vfe.pfn_layers[0].linear.weight.grad.abs().max()) > 0 and params

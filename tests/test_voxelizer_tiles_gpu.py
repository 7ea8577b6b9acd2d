"""The three point-to-cell front ends (csrc/pillar.hip, csrc/sparse_conv.hip, csrc/hard_voxel.hip) at the sizes where their
tiled scans (csrc/common.h tile_reduce / tile_scan, tiles of 2048 items) can go wrong and no other exact test reaches: row
counts on either side of one and two tiles, two tiles of pillar cells, and an occupancy bitmap of more than one tile of
groups.  The references are the numpy restatements of sparse_conv_reference.py and hard_voxel_reference.py, computed once a
case; every test first asserts that its reference answer is not a degenerate one.  Inputs and outputs are arena views.

Points are drawn with a fixed seed, uniform over the range, plus a dozen rows just outside each face of the range and two NaN
rows (in x and in y, which every operator tests); rows are sorted by sample, which the hard voxelizer needs.

Exact: every index output.  Bounded: the means against a float64 mean, |err| <= n 2^-23 max|v in the cell| + 2^-20 (n the
cell's count), the bound of test_sparse_conv_gpu.py and test_pillar_gpu.py.  Bit-equal: the pillars' mean and the voxels' on
the same nz = 1 grid (one key rule, one fixed-point mean).
"""
import functools

import numpy as np
import pytest
import torch

import hard_voxel_reference as hvr
import sparse_conv_reference as scr
from arena import Arena
from pdm_ssd_amd import _native

pytestmark = pytest.mark.gpu

ROWS = [0, 1, 2047, 2048, 2049, 4097]
TILE = 2048
DRAW = [0.0, -4.0, -2.0, 8.0, 4.0, 2.0]            # the points' own range; GRID3 is this range
GRID3 = dict(range=DRAW, voxel=[0.5, 0.5, 0.5], grid=[16, 16, 8], B=2)
# 3840 cells; its x and y extents are DRAW's, its one z cell holds every point
GRID2 = dict(range=[0.0, -4.0, -100.0, 8.0, 4.0, 100.0], voxel=[8.0 / 48, 0.2, 200.0], grid=[48, 40, 1], B=2)
T = 5
FACE_ROWS = 12
I32 = torch.int32


@pytest.fixture(scope="module")
def arena(dev):
    return Arena(dev)


def put(arena, src, misalign_bytes=0, poison=None):
    """arena.put, or a plain empty tensor: an Arena hands out no view of zero elements"""
    src = torch.as_tensor(src)
    return arena.put(src, misalign_bytes, poison) if src.numel() else src.to(arena.buf.device)


def carve(arena, shape, dtype, misalign_bytes=0):
    return arena.carve(shape, dtype, misalign_bytes) if int(np.prod(shape)) else torch.empty(shape, dtype=dtype, device=arena.buf.device)


@functools.lru_cache(maxsize=None)
def points_of(N):
    """-> (points (N, 5) rows (b, x, y, z, intensity), {(axis, side): rows just outside that face}); 70 % of the rows are sample 0"""
    rng = np.random.default_rng(1000 + N)
    f32 = np.float32
    lo, hi = np.asarray(DRAW[:3], dtype=f32), np.asarray(DRAW[3:], dtype=f32)
    xyz = rng.uniform(lo, hi, (N, 3)).astype(f32)
    faces = {}
    if N >= 6 * FACE_ROWS + 2:
        at = rng.permutation(N)[:6 * FACE_ROWS + 2]
        half = FACE_ROWS // 2
        for axis in range(3):
            below = np.concatenate([np.full(half, np.nextafter(lo[axis], f32(-np.inf))), lo[axis] - rng.uniform(0.01, 1.0, half)])
            above = np.concatenate([np.full(half // 2, hi[axis]), np.full(half - half // 2, np.nextafter(hi[axis], f32(np.inf))),
                                    hi[axis] + rng.uniform(0.01, 1.0, half)])
            for side, values in enumerate((below, above)):
                rows = at[(2 * axis + side) * FACE_ROWS:(2 * axis + side + 1) * FACE_ROWS]
                xyz[rows, axis] = values.astype(f32)
                faces[(axis, side)] = rows
        xyz[at[-2], 0] = np.nan
        xyz[at[-1], 1] = np.nan
    b = (np.arange(N) >= int(0.7 * N)).astype(f32)
    return np.concatenate([b[:, None], xyz, rng.uniform(0, 1, (N, 1)).astype(f32)], 1), faces


@functools.lru_cache(maxsize=None)
def assign_reference(N, flat):
    """the numpy voxel_assign on GRID2 (flat) or GRID3; asserts what makes a large case worth running"""
    geo = GRID2 if flat else GRID3
    p, faces = points_of(N)
    want = scr.voxel_assign(p, geo['B'], geo['range'], geo['voxel'], geo['grid'])
    if N >= TILE - 1:
        kept = set(want['kept_idx'].tolist())
        for (axis, side), rows in faces.items():
            tested = not (flat and axis == 2)                   # the flat grid's z cell holds every point
            assert all((int(r) in kept) != tested for r in rows), (axis, side)
        assert int(want['voxel_count'].max()) > 1 and len(want['voxel_count']) > 256
        assert len(kept) < N - 2 and set(want['voxel_coords'][:, 0].tolist()) == {0, 1}
    return want


@functools.lru_cache(maxsize=None)
def hard_reference(N):
    """-> (max_voxels, the numpy voxelize_batch on GRID3); max_voxels lies between the two samples' occupied cells"""
    p, _ = points_of(N)
    cells = assign_reference(N, False)['voxel_coords'][:, 0]
    per_sample = [int((cells == b).sum()) for b in range(GRID3['B'])]
    max_voxels = max(1, sum(per_sample) // 2)
    want = hvr.voxelize_batch(p, GRID3['B'], GRID3['range'], GRID3['voxel'], GRID3['grid'], T, max_voxels)
    if N >= TILE - 1:
        got = [int((want['voxel_coords'][:, 0] == b).sum()) for b in range(GRID3['B'])]
        assert per_sample[1] < max_voxels < per_sample[0] and got == [max_voxels, per_sample[1]], (per_sample, max_voxels, got)
        assert int(want['voxel_num_points'].max()) == T and int(want['voxel_num_points'].min()) == 1
    return max_voxels, want


def mean_bound(p, got, count, C):
    """(P, 1): n 2^-23 max|v in the cell| + 2^-20 over the first C columns behind batch_idx"""
    big = np.zeros(len(count))
    np.maximum.at(big, got['unq_inv'], np.abs(p[got['kept_idx'], 1:1 + C]).max(1).astype(np.float64))
    return (count * 2.0 ** -23 * big + 2.0 ** -20)[:, None]


# ---- the raw operators on arena views ----------------------------------------------------------------------------------------
def raw_voxel_assign(arena, p, geo):
    arena.reset()
    nx, ny, nz = geo['grid']
    N, C1 = p.shape
    cap = min(N, geo['B'] * nx * ny * nz)
    pts = put(arena, p, 4, poison=float('nan'))
    o = {'kept_idx': carve(arena, N, I32, 4), 'unq_inv': carve(arena, N, I32, 8), 'voxel_coords': carve(arena, (cap, 4), I32, 12),
         'voxel_count': carve(arena, cap, I32, 4), 'voxel_mean': carve(arena, (cap, C1 - 1), torch.float32, 4), 'record': carve(arena, 2, I32, 8)}
    nbytes = _native.lib().pdm_voxel_assign_workspace_bytes(N, C1, geo['B'], nx, ny, nz)
    assert nbytes > 0
    ws = carve(arena, nbytes, torch.uint8, 8)
    _native.call("pdm_voxel_assign", _native.stream(ws), N, C1, pts.data_ptr(), geo['B'], nx, ny, nz, *geo['range'][:3], *geo['voxel'],
                 *[o[k].data_ptr() for k in ('kept_idx', 'unq_inv', 'voxel_coords', 'voxel_count', 'voxel_mean', 'record')], ws.data_ptr(), nbytes)
    torch.cuda.synchronize()
    arena.check()
    n_kept, P = o['record'].tolist()
    return {k: o[k][:n_kept if k in ('kept_idx', 'unq_inv') else P].cpu().numpy() for k in o if k != 'record'}


def raw_pillar_assign(arena, p, geo):
    arena.reset()
    nx, ny, nz = geo['grid']
    N, C1 = p.shape
    ncell = geo['B'] * nx * ny
    cap = min(N, ncell)
    pts = put(arena, p, 4, poison=float('nan'))
    o = {'kept_idx': carve(arena, N, I32, 4), 'unq_inv': carve(arena, N, I32, 8), 'voxel_coords': carve(arena, (cap, 4), I32, 12),
         'pillar_count': carve(arena, cap, I32, 4), 'pillar_mean': carve(arena, (cap, 3), torch.float32, 4), 'cell_table': carve(arena, ncell, I32, 4),
         'seg_start': carve(arena, cap + 1, I32, 12), 'seg_rows': carve(arena, N, I32, 4), 'record': carve(arena, 2, I32, 8)}
    nbytes = _native.lib().pdm_pillar_assign_workspace_bytes(N, geo['B'], nx, ny)
    assert nbytes > 0
    ws = carve(arena, nbytes, torch.uint8, 8)
    r, v = geo['range'], geo['voxel']
    _native.call("pdm_pillar_assign", _native.stream(ws), N, C1, pts.data_ptr(), geo['B'], nx, ny, nz, r[0], r[1], v[0], v[1],
                 *[o[k].data_ptr() for k in ('kept_idx', 'unq_inv', 'voxel_coords', 'pillar_count', 'pillar_mean', 'cell_table', 'seg_start',
                                             'seg_rows', 'record')], ws.data_ptr(), nbytes)
    torch.cuda.synchronize()
    arena.check()
    n_kept, P = o['record'].tolist()
    size = {'kept_idx': n_kept, 'unq_inv': n_kept, 'seg_rows': n_kept, 'seg_start': P + 1, 'cell_table': ncell}
    return {k: o[k][:size.get(k, P)].cpu().numpy() for k in o if k != 'record'}


def raw_hard_voxelize(arena, p, geo, max_voxels):
    arena.reset()
    nx, ny, nz = geo['grid']
    N, C1 = p.shape
    cap = min(N, geo['B'] * max_voxels, geo['B'] * nx * ny * nz)
    pts = put(arena, p, 4, poison=float('nan'))
    o = {'slot_rows': carve(arena, (cap, T), I32, 4), 'voxel_coords': carve(arena, (cap, 4), I32, 12), 'voxel_num_points': carve(arena, cap, I32, 8),
         'record': carve(arena, 2, I32, 8)}
    nbytes = _native.lib().pdm_hard_voxelize_workspace_bytes(N, geo['B'], nx, ny, nz)
    assert nbytes > 0
    ws = carve(arena, nbytes, torch.uint8, 8)
    _native.call("pdm_hard_voxelize", _native.stream(ws), N, C1, pts.data_ptr(), geo['B'], nx, ny, nz, *geo['range'][:3], *geo['voxel'], T, max_voxels,
                 o['slot_rows'].data_ptr(), o['voxel_coords'].data_ptr(), o['voxel_num_points'].data_ptr(), None, o['record'].data_ptr(),
                 ws.data_ptr(), nbytes)
    torch.cuda.synchronize()
    arena.check()
    M, unsorted = o['record'].tolist()
    assert unsorted == 0
    return {k: o[k][:M].cpu().numpy() for k in o if k != 'record'}


# ---- rows on either side of one and two tiles --------------------------------------------------------------------------------
@pytest.mark.parametrize("N", ROWS)
def test_voxel_assign_across_row_tiles(arena, N):
    p, _ = points_of(N)
    want = assign_reference(N, False)
    got = raw_voxel_assign(arena, p, GRID3)
    for k in ('kept_idx', 'unq_inv', 'voxel_coords', 'voxel_count'):
        assert np.array_equal(got[k], want[k].reshape(got[k].shape)), k
    err = np.abs(got['voxel_mean'] - want['mean64'])
    assert (err <= mean_bound(p, got, got['voxel_count'], 4)).all()


@pytest.mark.parametrize("N", ROWS)
def test_hard_voxelize_across_row_and_cell_tiles(arena, N):
    p, _ = points_of(N)
    max_voxels, want = hard_reference(N)
    got = raw_hard_voxelize(arena, p, GRID3, max_voxels)
    for k in ('slot_rows', 'voxel_coords', 'voxel_num_points'):
        assert np.array_equal(got[k], want[k].reshape(got[k].shape)), k


@pytest.mark.parametrize("N", ROWS)
def test_pillar_assign_across_row_tiles_and_two_cell_tiles(arena, N):
    """the voxel reference on the one-cell-deep grid: its keys are the pillars' keys and its (b, 0, cy, cx) their coordinates"""
    p, _ = points_of(N)
    want = assign_reference(N, True)
    ncell = GRID2['B'] * GRID2['grid'][0] * GRID2['grid'][1]
    assert TILE < ncell <= 2 * TILE
    got = raw_pillar_assign(arena, p, GRID2)
    for k, w in (('kept_idx', 'kept_idx'), ('unq_inv', 'unq_inv'), ('voxel_coords', 'voxel_coords'), ('pillar_count', 'voxel_count')):
        assert np.array_equal(got[k], want[w].reshape(got[k].shape)), k
    P = len(want['keys'])
    table = np.full(ncell, -1, dtype=np.int32)
    table[want['keys']] = np.arange(P, dtype=np.int32)
    assert np.array_equal(got['cell_table'], table)
    if N >= TILE - 1:
        assert (want['keys'] < TILE).any() and (want['keys'] >= TILE).any()
    start = got['seg_start']
    assert start[0] == 0 and start[-1] == len(want['kept_idx']) and np.array_equal(np.diff(start), want['voxel_count'])
    segments = [np.sort(got['seg_rows'][a:b]) for a, b in zip(start[:-1], start[1:])]
    assert np.array_equal(np.concatenate(segments + [np.zeros(0, dtype=np.int32)]), np.argsort(want['unq_inv'], kind='stable'))
    err = np.abs(got['pillar_mean'] - want['mean64'][:, :3])
    assert (err <= mean_bound(p, got, got['pillar_count'], 3)).all()


# ---- one key rule and one fixed-point mean, from both ends ---------------------------------------------------------------------
def test_pillars_and_voxels_agree_on_a_one_cell_deep_grid(arena):
    p, _ = points_of(ROWS[-1])
    assert int(assign_reference(ROWS[-1], True)['voxel_count'].max()) > 1
    pillars = raw_pillar_assign(arena, p, GRID2)
    voxels = raw_voxel_assign(arena, p, GRID2)
    for k, w in (('kept_idx', 'kept_idx'), ('unq_inv', 'unq_inv'), ('voxel_coords', 'voxel_coords'), ('pillar_count', 'voxel_count')):
        assert np.array_equal(pillars[k], voxels[w]), k
    assert len(pillars['pillar_count']) > 256
    assert np.array_equal(pillars['pillar_mean'].view(np.int32), np.ascontiguousarray(voxels['voxel_mean'][:, :3]).view(np.int32))


# ---- bitmap groups across a scan tile ------------------------------------------------------------------------------------------
BIG_B, BIG_SHAPE = 2, (8, 200, 176)                # (D, H, W): 563 200 cells, 2200 groups of 256: more than one tile of 2048 groups


@functools.lru_cache(maxsize=None)
def big_sites():
    """about 3000 distinct sites (b, z, y, x) in shuffled row order, a few hundred of them in the second tile of groups"""
    rng = np.random.default_rng(77)
    D, H, W = BIG_SHAPE
    key = rng.choice(BIG_B * D * H * W, 3000, replace=False).astype(np.int64)
    idx = np.stack([key // (D * H * W), key % D, (key // D) % H, (key // (D * H)) % W], 1).astype(np.int32)
    assert np.array_equal(scr.site_key(idx, BIG_SHAPE), key)
    beyond = int((key >= TILE * 256).sum())
    assert 100 <= beyond <= 500 and BIG_B * D * H * W > TILE * 256, beyond
    return idx, key


def test_site_index_and_rulebook_with_groups_in_two_scan_tiles(arena):
    """the site index as test_voxel_rcnn_gpu.py checks it (every row returned, nothing else set, the group prefixes the popcounts
    in front of each group), and a submanifold rulebook on the same sites against the numpy restatement"""
    idx_np, key = big_sites()
    D, H, W = BIG_SHAPE
    P, ncell = len(idx_np), BIG_B * D * H * W
    lib = _native.lib()
    arena.reset()
    idx = arena.put(idx_np, 4, poison=[0, 1, 1, 1])
    nbytes = lib.pdm_sparse_index_workspace_bytes(P, BIG_B, D, H, W)
    assert nbytes > 0
    ws = arena.carve(nbytes, torch.uint8, 8)
    _native.call("pdm_sparse_index", _native.stream(ws), P, idx.data_ptr(), BIG_B, D, H, W, ws.data_ptr(), nbytes)
    torch.cuda.synchronize()
    arena.check()
    a256 = lambda v: (v + 255) & ~255      # noqa: E731      (the layout of csrc/sc_index.h)
    ngroups = (ncell + 255) // 256
    nwords, ntiles = 8 * ngroups, (ngroups + TILE - 1) // TILE
    assert ntiles == 2
    at_prefix = a256(4 * nwords)
    at_rows = at_prefix + a256(4 * ngroups) + a256(4 * ntiles)
    raw = ws.cpu().numpy()
    words = raw[:4 * nwords].view(np.uint32)
    bits = ((words[:, None] >> np.arange(32, dtype=np.uint32)) & 1).astype(bool).reshape(-1)
    gprefix, row_of_rank = raw[at_prefix:at_prefix + 4 * ngroups].view(np.int32), raw[at_rows:at_rows + 4 * P].view(np.int32)
    assert bits[key].all() and int(bits.sum()) == P and not bits[ncell:].any()
    before = np.concatenate([[0], np.cumsum(bits)])            # set cells in front of every cell
    assert np.array_equal(row_of_rank[before[key]], np.arange(P))
    assert np.array_equal(gprefix, before[np.arange(ngroups) * 256]) and gprefix[TILE] > 0

    want = scr.rulebook(idx_np, BIG_B, BIG_SHAPE, *scr.GEOMETRIES['subm3'])[1]
    assert int((want >= 0).sum()) > P                           # some sites have neighbours
    g = (BIG_B, D, H, W, 3, 3, 3, 1, 1, 1, 1, 1, 1, 1)
    nbytes = lib.pdm_sparse_rulebook_workspace_bytes(P, *g)
    assert nbytes > 0
    ws = arena.carve(nbytes, torch.uint8, 8)
    record = arena.carve(1, I32, 4)
    nbr = arena.carve((P, 27), I32, 4)
    _native.call("pdm_sparse_sites", _native.stream(ws), P, idx.data_ptr(), *g, record.data_ptr(), ws.data_ptr(), nbytes)
    _native.call("pdm_sparse_rulebook", _native.stream(ws), P, idx.data_ptr(), P, *g, None, nbr.data_ptr(), ws.data_ptr(), nbytes)
    torch.cuda.synchronize()
    arena.check()
    assert int(record.cpu()) == P and np.array_equal(nbr.cpu().numpy(), want)

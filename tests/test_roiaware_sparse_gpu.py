"""pdm_roiaware_pool_sparse (csrc/roiaware_sparse.hip): the head's two RoI-aware poolings for the whole batch, straight to sparse
rows, against the composed formulation of this tree: per sample RoIAwarePool3d 'avg' on the part features and 'max' on the rpn
features, the activity rule on the pooled part channels (their fp32 sum in ascending channel order is non-zero), nonzero, gather.
Every output is compared with torch.equal.

The scene: B = 3 samples of N = 5 boxes, max_pts_each_voxel = 2 (one point a cell is kept: the cap bites wherever two points share
a cell).  Sample 0 holds the points: boxes 0 and 1 overlap and share points, box 2 is rotated, box 3 stands alone and has one cell
whose points all carry zero part features (occupied, inactive), box 4 is empty.  Sample 1 has no point.  Sample 2 has points, all
outside its boxes.  Points are reject-sampled: none within 1e-4 of the box size of a box face or of a cell boundary.
"""
import numpy as np
import pytest
import torch

import part_a2_reference as par
import roi_pool_reference as rpr
from arena import Arena
from pdm_ssd_amd import _native, sparse_conv_ops
from pdm_ssd_amd.roiaware_pool3d.roiaware_pool3d_utils import RoIAwarePool3d, roiaware_pool_sparse, sparse_list_capacity

pytestmark = pytest.mark.gpu
F = np.float32
B, N, MAX_PTS = 3, 5, 2
ROIS0 = F([[10.0, 2.0, -1.0, 4.0, 1.8, 1.6, 0.0],         # 0 and 1 overlap
           [10.8, 2.3, -0.9, 3.8, 1.7, 1.5, 0.2],
           [20.0, -5.0, -1.0, 4.2, 1.9, 1.7, 0.9],        # rotated
           [30.0, 6.0, -0.8, 3.6, 1.6, 1.5, 0.0],         # alone; one occupied cell is inactive
           [60.0, 0.0, -1.0, 4.0, 1.8, 1.6, -0.4]])       # empty: past every point
SIZES = [(3, 3, 3), (2, 3, 4)]


@pytest.fixture(scope="module")
def arena(dev):
    return Arena(dev)


def make_scene(out, C):
    """-> dict of numpy arrays; the same scene for every C (the rpn features' leading columns agree)"""
    rois = np.stack([ROIS0, ROIS0 + F([0, 40, 0, 0, 0, 0, 0]), ROIS0 + F([0, -40, 0, 0, 0, 0, 0])]).astype(F)
    seed = 5
    while True:
        rng = np.random.default_rng(seed)
        seed += 1
        per_box = [rng.normal(ROIS0[k, :3], [1.2, 0.7, 0.5], (60, 3)) for k in range(4)]
        p0 = np.concatenate(per_box + [np.stack([rng.uniform(0, 45, 80), rng.uniform(-8, 8, 80), rng.uniform(-2, 0, 80)], -1)]).astype(F)
        p0 = p0[rng.permutation(len(p0))]
        p2 = np.stack([rng.uniform(0, 45, 70), rng.uniform(-8, 8, 70), rng.uniform(-2, 0, 70)], -1).astype(F)   # far from sample 2's boxes
        big = float(ROIS0[:, 3:6].max())
        if all(rpr.face_clearance(p, r) > 1e-4 * big and rpr.voxel_clearance(p, r, out) > 1e-4 * max(out)
               for p, r in ((p0, rois[0]), (p2, rois[2]))):
            break
    pts = np.concatenate([p0, p2])
    counts = np.array([len(p0), 0, len(p2)], dtype=np.int32)
    part = rng.uniform(0.05, 1.0, (len(pts), 4)).astype(F) * rng.choice([-1, 1], (len(pts), 4)).astype(F)
    rpn = rng.standard_normal((len(pts), 16)).astype(F)[:, :C].copy()
    # box 3 of sample 0: the points of the cell of its first point carry zero part features
    inside = np.nonzero(rpr.in_box_mask(p0, rois[0, 3]))[0]
    xi, yi, zi = rpr.voxel_indices(p0, rois[0, 3], out)
    cell = (xi[inside[0]], yi[inside[0]], zi[inside[0]])
    quiet = [p for p in inside if (xi[p], yi[p], zi[p]) == cell]
    part[quiet] = 0
    return dict(rois=rois, pts=pts, counts=counts, part=part, rpn=rpn, quiet_cell=(3, *cell), out=out,
                shared=int((rpr.in_box_mask(p0, rois[0, 0]) & rpr.in_box_mask(p0, rois[0, 1])).sum()),
                in_sample2=int(sum(rpr.in_box_mask(p2, r).sum() for r in rois[2])))


def composed(dev, sc):
    """the formulation already in the tree -> coords (Q, 4) int32, part (Q, 4), rpn (Q, C), and the dense part pooling"""
    pool = RoIAwarePool3d(sc['out'], MAX_PTS)
    pts, part, rpn = (torch.from_numpy(sc[k]).to(dev) for k in ('pts', 'part', 'rpn'))
    starts = np.concatenate([[0], np.cumsum(sc['counts'])])
    pp, pr = [], []
    for b in range(B):
        sl = slice(int(starts[b]), int(starts[b + 1]))
        rois = torch.from_numpy(sc['rois'][b]).to(dev)
        pp.append(pool(rois, pts[sl], part[sl], pool_method='avg'))
        pr.append(pool(rois, pts[sl], rpn[sl], pool_method='max'))
    pp, pr = torch.cat(pp), torch.cat(pr)
    active = ((pp[..., 0] + pp[..., 1]) + pp[..., 2]) + pp[..., 3] != 0       # fp32, ascending channels
    idx = active.nonzero()
    return idx.int(), pp[idx[:, 0], idx[:, 1], idx[:, 2], idx[:, 3]], pr[idx[:, 0], idx[:, 1], idx[:, 2], idx[:, 3]], pp


@pytest.fixture(scope="module", params=SIZES, ids=lambda s: 'x'.join(map(str, s)))
def scene(request):
    return make_scene(request.param, 16)


@pytest.mark.parametrize("C", [1, 16])
def test_sparse_pool_equals_the_composed_formulation(dev, scene, C):
    sc = dict(scene, rpn=np.ascontiguousarray(scene['rpn'][:, :C]))
    assert sc['shared'] > 0 and sc['in_sample2'] == 0
    want_c, want_p, want_r, dense_part = composed(dev, sc)
    t = {k: torch.from_numpy(sc[k]).to(dev) for k in ('rois', 'pts', 'counts', 'part', 'rpn')}
    before = sparse_conv_ops.HOST_READS
    got = roiaware_pool_sparse(t['rois'], t['pts'], t['counts'], t['part'], t['rpn'], sc['out'], MAX_PTS)
    assert sparse_conv_ops.HOST_READS == before + 1
    again = roiaware_pool_sparse(t['rois'], t['pts'], t['counts'], t['part'], t['rpn'], sc['out'], MAX_PTS)
    Q = want_c.shape[0]
    print(sc['out'], 'C', C, 'Q', Q, 'of', B * N * int(np.prod(sc['out'])), 'cells; shared points', sc['shared'])
    assert Q >= 3
    assert torch.equal(got[0], want_c) and torch.equal(got[1], want_p) and torch.equal(got[2], want_r)
    assert all(torch.equal(a, b) for a, b in zip(got, again)), 'two runs differ'
    # the numpy restatement of the activity rule and the row order agrees
    assert np.array_equal(par.active_cells(dense_part.cpu().numpy()), want_c.cpu().numpy())
    rows = set(map(tuple, want_c.cpu().tolist()))
    # the scene holds what it claims: the cap bites, a cell is occupied but inactive, boxes of every sample but 0 are empty
    assert sc['quiet_cell'] not in rows
    assert {r for r, *_ in rows} == {0, 1, 2, 3}
    starts = np.concatenate([[0], np.cumsum(sc['counts'])])
    p0 = sc['pts'][: starts[1]]
    per_cell = {}
    for k in range(4):
        m = rpr.in_box_mask(p0, sc['rois'][0, k])
        xi, yi, zi = rpr.voxel_indices(p0, sc['rois'][0, k], sc['out'])
        for p in np.nonzero(m)[0]:
            per_cell[(k, xi[p], yi[p], zi[p])] = per_cell.get((k, xi[p], yi[p], zi[p]), 0) + 1
    assert max(per_cell.values()) > MAX_PTS - 1 and len(per_cell) == Q + 1


def test_sparse_pool_writes_inside_its_outputs_only(dev, arena, scene):
    """the two entry points on arena views: rows and columns 4 bytes off a 16-byte boundary, NaN around the inputs"""
    sc = scene
    C = 16
    want_c, want_p, want_r, _ = composed(dev, sc)
    Q = want_c.shape[0]
    arena.reset()
    rois = arena.put(sc['rois'], 4, poison=float('nan'))
    pts = arena.put(sc['pts'], 4, poison=float('nan'))
    counts = arena.put(sc['counts'], 4, poison=1 << 20)
    part = arena.put(sc['part'], 4, poison=float('nan'))
    rpn = arena.put(sc['rpn'], 4, poison=float('nan'))
    ox, oy, oz = sc['out']
    L = sparse_list_capacity(B * N, len(sc['pts']), ox * oy * oz, MAX_PTS)
    nbytes = _native.lib().pdm_roiaware_pool_sparse_workspace_bytes(B, N, ox, oy, oz, L)
    ws = arena.carve(nbytes, torch.uint8, 8)
    record = arena.carve(2, torch.int32, 4)
    coords = arena.carve((Q, 4), torch.int32, 4)
    out_p = arena.carve((Q, 4), torch.float32, 8)
    out_r = arena.carve((Q, C), torch.float32, 12)
    st = _native.stream(dev)
    _native.call("pdm_roiaware_pool_sparse_index", st, B, N, len(sc['pts']), MAX_PTS, ox, oy, oz, rois.data_ptr(), pts.data_ptr(),
                 counts.data_ptr(), part.data_ptr(), L, record.data_ptr(), ws.data_ptr(), nbytes)
    assert record.cpu().tolist() == [Q, 0]
    _native.call("pdm_roiaware_pool_sparse_emit", st, B, N, len(sc['pts']), C, ox, oy, oz, part.data_ptr(), rpn.data_ptr(), L, Q,
                 ws.data_ptr(), nbytes, coords.data_ptr(), out_p.data_ptr(), out_r.data_ptr())
    torch.cuda.synchronize()
    arena.check()
    assert torch.equal(coords, want_c) and torch.equal(out_p, want_p) and torch.equal(out_r, want_r)


def test_sparse_pool_without_an_active_cell_and_with_too_small_a_list(dev, scene):
    sc = scene
    t = {k: torch.from_numpy(sc[k]).to(dev) for k in ('rois', 'pts', 'counts', 'part', 'rpn')}
    # sample 2 alone (as a batch of one): points, but none in a box
    n0 = int(sc['counts'][0])
    one = torch.tensor([int(sc['counts'][2])], dtype=torch.int32, device=dev)
    got = roiaware_pool_sparse(t['rois'][2:], t['pts'][n0:], one, t['part'][n0:], t['rpn'][n0:], sc['out'], MAX_PTS)
    assert [tuple(g.shape) for g in got] == [(0, 4), (0, 4), (0, 16)] and got[0].dtype == torch.int32
    # all part features zero: cells are occupied, none is active
    got = roiaware_pool_sparse(t['rois'], t['pts'], t['counts'], torch.zeros_like(t['part']), t['rpn'], sc['out'], MAX_PTS)
    assert got[0].shape[0] == 0
    # no points, no boxes: no launch and no host read
    before = sparse_conv_ops.HOST_READS
    got = roiaware_pool_sparse(t['rois'], t['pts'][:0], torch.zeros(B, dtype=torch.int32, device=dev), t['part'][:0], t['rpn'][:0], sc['out'], MAX_PTS)
    assert got[0].shape[0] == 0 and sparse_conv_ops.HOST_READS == before
    # a list too small for the boxes' points is refused, not truncated
    with pytest.raises(RuntimeError, match='list_capacity'):
        roiaware_pool_sparse(t['rois'], t['pts'], t['counts'], t['part'], t['rpn'], sc['out'], MAX_PTS, list_capacity=3)

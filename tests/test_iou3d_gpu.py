"""Rotated-box IoU / NMS / points-in-boxes: the HIP kernels through the reference-shaped
python API against (a) areas known by hand, (b) an exact float64 polygon clip, (c) oracle/iou3d_oracle.c and (d) NMS
keep lists known by construction.  No comparison here has an escape clause: every condition a comparison needs (no pair
IoU near the threshold, few corners in inside_box's margin band, few points near a face) is a property of the scene
alone and is proved on the CPU by tests/test_box_geometry_host.py, which builds the same scenes from the tables below."""
import functools

import numpy as np
import pytest
import torch

import box_geometry_cases as bg
from pdm_ssd_amd.iou3d_nms import iou3d_nms_utils as iu

pytestmark = pytest.mark.gpu

TABLE_TOL = 2e-6        # the oracle's own bound against the hand-derived areas (test_box_geometry_host.py; 1.1e-6 measured)
EXACT_F = 4.0           # kernel error <= EXACT_F x the oracle's error against the exact clip
TIE_BAND = 1e-4         # |oracle IoU - thresh| below this: the device's own IoU decides the pair (hybrid reference)
MIN_HALF_GAP = 5e-5     # exact NMS scenes: no pair IoU this close to the threshold (30 x the oracle's 1.7e-6 error)

# offsets of the exact-area scenes: around the origin, and the far range of KITTI, nuScenes and Waymo
OFFSETS = [(0.0, 0.0), (70.0, 40.0), (150.0, -150.0)]

# exact NMS scenes (n, spread, nominal threshold, normal): every block-boundary size, dense enough to suppress
NMS_EXACT = [(n, 3.0 + (n % 2), nominal, normal)
             for normal in (False, True) for nominal in (0.1, 0.3, 0.5) for n in (63, 64, 65, 127, 128, 129, 200)] + \
            [(1000, 12.0, nominal, normal) for normal in (False, True) for nominal in (0.1, 0.3, 0.5)]

# the large cases that were here before (n, thresh, normal), boxes at spread 12
NMS_LARGE = [(500, 0.1, False), (3000, 0.01, False), (1000, 0.5, False), (700, 0.3, True),
             (65, 0.25, False), (1, 0.5, False), (0, 0.5, False)]

POINT_CASES = [(3, 40, 5000), (1, 300, 1000), (2, 0, 64), (2, 5, 0)]
CHUNK_CASES = [(T, M) for T in (127, 128, 129, 257) for M in (255, 256, 257)]


def random_boxes(n, seed, spread=20.0):
    rng = np.random.default_rng(seed)
    xy = rng.uniform(-spread, spread, (n, 2))
    z = rng.uniform(-1, 1, (n, 1))
    dims = np.stack([rng.uniform(1.5, 5.0, n), rng.uniform(1.0, 2.5, n), rng.uniform(1.0, 2.0, n)], 1)
    heading = rng.uniform(-np.pi, np.pi, (n, 1))
    return np.concatenate([xy, z, dims, heading], 1).astype(np.float32)


def T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


T_ = T


# ---- scenes shared with tests/test_box_geometry_host.py ----------------------------------------------------------------
def exact_scene(offset):
    """60 x 60 pairs at spread 5 moved to `offset`."""
    a, b = random_boxes(60, 3, spread=5.0), random_boxes(60, 4, spread=5.0)
    shift = np.asarray(offset, np.float32)
    a[:, :2] += shift; b[:, :2] += shift
    return a, b


@functools.lru_cache(maxsize=None)
def exact_scene_reference(offset):
    """-> (a, b, exact areas (60, 60) float64, bool (60, 60): the pair is outside the margin band)."""
    a, b = exact_scene(offset)
    return a, b, bg.clip_area64_matrix(a, b), ~bg.margin_band_matrix(a, b)


def nms_scene(n, spread):
    """boxes and distinct scores; -> (boxes, scores, order = the boxes by descending score)."""
    boxes = random_boxes(n, 10 + n, spread=spread)
    scores = np.random.default_rng(n).uniform(0, 1, n).astype(np.float32)
    assert np.unique(scores).size == n
    return boxes, scores, np.argsort(-scores, kind="stable")


def scene_iou(oracle, sorted_boxes, normal):
    return bg.iou_normal_np(sorted_boxes, sorted_boxes) if normal else oracle.boxes_iou_bev(sorted_boxes, sorted_boxes)


def point_scene(B, T, M):
    rng = np.random.default_rng(B * 100 + T)
    boxes = np.stack([random_boxes(T, 50 + b, spread=10.0) for b in range(B)]) if T else np.zeros((B, 0, 7), np.float32)
    pts = np.concatenate([rng.uniform(-12, 12, (B, M, 2)), rng.uniform(-2, 2, (B, M, 1))], 2).astype(np.float32)
    if T and M:
        pts[:, :T] = boxes[:, :T, :3][:, :M]                    # box centres: inside (possibly several boxes: first wins)
        boxes[:, -1] = boxes[:, 0]                              # a duplicate box later in the list never wins
    return pts, boxes


def chunk_scene(T, M):
    """Boxes on an 8 m lattice (sizes up to 5 x 2.5: disjoint), so that no box contains another's centre, and points
    at the centres of the LAST min(T, M, 200) boxes (the other points are anywhere): point k sits in box T - 1 - k,
    which lies in the second or third 128-box LDS chunk whenever T > 128.  With T > 130, box 130 is moved into box 3 and a point is put inside both.
    -> (pts (1, M, 3), boxes (1, T, 7), expected (M) with -2 = whatever the oracle says)."""
    rng = np.random.default_rng(1000 * T + M)
    boxes = random_boxes(T, 70 + T, spread=1.0)
    side = int(np.ceil(np.sqrt(T)))
    cell = rng.permutation(side * side)[:T]
    boxes[:, 0] = (cell % side - (side - 1) / 2) * 8.0
    boxes[:, 1] = (cell // side - (side - 1) / 2) * 8.0
    span = side * 4.0
    pts = np.concatenate([rng.uniform(-span, span, (M, 2)), rng.uniform(-2, 2, (M, 1))], 1).astype(np.float32)
    expected = np.full(M, -2, np.int32)
    if T > 130:
        boxes[130] = boxes[3]
        boxes[130, 6] += 0.5
        boxes[130, :2] += np.float32(0.05)
    k = min(T, M, 200)
    pts[:k] = boxes[T - 1 - np.arange(k), :3]
    expected[:k] = T - 1 - np.arange(k)
    if T > 130:
        expected[T - 1 - 130] = 3                               # box 130's centre lies in box 3 as well: the first wins
        pts[k - 1] = boxes[3, :3] + np.float32([0.1, -0.05, 0.0])
        expected[k - 1] = 3                                     # inside box 3 and box 130, at neither's centre
    return pts[None], boxes[None], expected


def all_point_scenes():
    for B, T, M in POINT_CASES:
        if T and M:
            yield (B, T, M), point_scene(B, T, M)
    for T, M in CHUNK_CASES:
        pts, boxes, _ = chunk_scene(T, M)
        yield (1, T, M), (pts, boxes)


def near_face_mask(pts, boxes):
    return np.stack([bg.near_face(pts[b], boxes[b]) for b in range(pts.shape[0])])


# ---- areas -------------------------------------------------------------------------------------------------------------
def _iou3d(ov, a, b, h):
    """3-D IoU of pairs with a common height overlap h from BEV overlaps, float64."""
    o3 = ov * h
    va, vb = np.prod(a[..., 3:6].astype(np.float64), -1), np.prod(b[..., 3:6].astype(np.float64), -1)
    return o3 / np.clip(va + vb - o3, 1e-6, None)


@pytest.mark.parametrize("swap", [False, True])
def test_closed_form_areas_through_every_entry(dev, swap):
    """Every row of CLOSED_FORM through the five public entries, both argument orders, to the oracle's own bound.
    All boxes share z = 0 and dz = 1.5, so the height overlap is 1.5; the aligned entries see row i against row i, the
    pairwise ones take the diagonal of the full (R, R) matrix (16 x 16 tiles with unused rows)."""
    a, b, area, kinds = bg.closed_form_arrays()
    if swap:
        a, b = b, a
    R = len(area)
    ta, tb = T(a, dev), T(b, dev)
    ov = iu.boxes_overlap_bev(ta, tb).cpu().numpy().astype(np.float64)
    iou = iu.boxes_iou_bev(ta, tb).cpu().numpy().astype(np.float64)
    al = iu._aligned_overlap(ta, tb)[2].cpu().numpy().astype(np.float64)[:, 0]     # boxes_aligned_overlap_bev
    i3 = iu.boxes_iou3d_gpu(ta, tb).cpu().numpy().astype(np.float64)
    pr = iu.paired_boxes_iou3d_gpu(ta, tb).cpu().numpy().astype(np.float64)
    al3 = iu.boxes_aligned_iou3d_gpu(ta, tb).cpu().numpy().astype(np.float64)[:, 0]
    sa, sb = (a[:, 3] * a[:, 4]).astype(np.float64), (b[:, 3] * b[:, 4]).astype(np.float64)
    # d IoU / d area = S / (S - area)^2 <= 1 in every row (S = sa + sb), so the area's bound holds for the IoUs too
    want_iou = area / np.maximum(sa + sb - area, 1e-8)
    want_3d = _iou3d(area, a, b, 1.5)
    for r in range(R):
        name = bg.CLOSED_FORM[r][0]
        print("%-44s area %.9g  overlap %.9g  aligned %.9g  iou %.9g  iou3d %.9g"
              % (name, area[r], ov[r, r], al[r], iou[r, r], i3[r, r]))
        assert abs(ov[r, r] - area[r]) <= TABLE_TOL, name
        assert abs(al[r] - area[r]) <= TABLE_TOL, name
        assert abs(iou[r, r] - want_iou[r]) <= TABLE_TOL, name
        assert abs(i3[r, r] - want_3d[r]) <= TABLE_TOL, name
        assert abs(pr[r] - want_3d[r]) <= TABLE_TOL, name
        assert abs(al3[r] - want_3d[r]) <= TABLE_TOL, name


@pytest.mark.parametrize("na,nb", [(37, 53), (1, 1), (200, 16), (0, 5), (15, 17), (16, 16), (17, 33), (33, 15)])
def test_pairwise_overlap_and_iou_match_oracle(oracle, dev, na, nb):
    a, b = random_boxes(na, 1, spread=6.0), random_boxes(nb, 2, spread=6.0)
    if na and nb:
        b[0] = a[0]                                   # identical boxes (coincident edges)
        b[1 % nb, :2] = a[0, :2]; b[1 % nb, 6] = a[0, 6] + np.pi / 2
    ov = iu.boxes_overlap_bev(T(a, dev).view(-1, 7), T(b, dev).view(-1, 7)).cpu().numpy()
    iou = iu.boxes_iou_bev(T(a, dev).view(-1, 7), T(b, dev).view(-1, 7)).cpu().numpy()
    np.testing.assert_allclose(ov, oracle.boxes_overlap_bev(a, b), rtol=1e-4, atol=1e-4)
    np.testing.assert_allclose(iou, oracle.boxes_iou_bev(a, b), rtol=1e-4, atol=1e-5)
    assert ov.shape == (na, nb) and (iou >= 0).all() and (iou <= 1.0 + 1e-4).all()
    if na and nb:
        assert (ov > 0).any()


def test_iou3d_and_aligned_variants(oracle, dev):
    a, b = random_boxes(64, 3, spread=5.0), random_boxes(64, 4, spread=5.0)
    ov = oracle.boxes_overlap_bev(a, b)
    h = np.clip(np.minimum(a[:, None, 2] + a[:, None, 5] / 2, b[None, :, 2] + b[None, :, 5] / 2) -
                np.maximum(a[:, None, 2] - a[:, None, 5] / 2, b[None, :, 2] - b[None, :, 5] / 2), 0, None)
    o3 = ov * h
    ref = o3 / np.clip(np.prod(a[:, 3:6], 1)[:, None] + np.prod(b[:, 3:6], 1)[None] - o3, 1e-6, None)
    got = iu.boxes_iou3d_gpu(T(a, dev), T(b, dev)).cpu().numpy()
    np.testing.assert_allclose(got, ref, rtol=1e-4, atol=1e-5)
    al = iu.boxes_aligned_iou3d_gpu(T(a, dev), T(b, dev)).cpu().numpy()
    pr = iu.paired_boxes_iou3d_gpu(T(a, dev), T(b, dev)).cpu().numpy()
    np.testing.assert_allclose(al[:, 0], np.diag(ref), rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(pr, np.diag(ref), rtol=1e-4, atol=1e-5)


@pytest.mark.parametrize("offset", OFFSETS)
def test_overlap_against_exact_clip_at_range(oracle, dev, offset):
    """Outside inside_box's margin band the kernels' algorithm computes the true intersection area: measured against
    the float64 polygon clip, the kernel may be EXACT_F times as far off as the oracle (same fp32 operations, other
    cosf / sinf / atan2f) and no further.  Measured on the MI355X: ratios 0.962, 1.000 and 1.000."""
    a, b, exact, clear = exact_scene_reference(offset)
    got = iu.boxes_overlap_bev(T(a, dev), T(b, dev)).cpu().numpy().astype(np.float64)
    ref = oracle.boxes_overlap_bev(a, b).astype(np.float64)
    err_kernel = float(np.abs(got - exact)[clear].max())
    err_oracle = float(np.abs(ref - exact)[clear].max())
    print("offset %s: %d pairs compared, err_kernel %.3e, err_oracle %.3e, ratio %.3f"
          % (offset, int(clear.sum()), err_kernel, err_oracle, err_kernel / err_oracle))
    assert err_kernel <= EXACT_F * err_oracle


# ---- NMS ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,spread,nominal,normal", NMS_EXACT)
def test_nms_equals_oracle_exactly(oracle, dev, n, spread, nominal, normal):
    """The threshold sits in the middle of the widest gap of the scene's pair IoUs (at least MIN_HALF_GAP to either
    side, proved on the CPU): the keep list is the oracle's, with nothing excused."""
    boxes, scores, order = nms_scene(n, spread)
    thresh, half = bg.gap_threshold(scene_iou(oracle, boxes[order], normal), nominal)
    assert half >= MIN_HALF_GAP
    fn = iu.nms_normal_gpu if normal else iu.nms_gpu
    sel, _ = fn(T(boxes, dev), T(scores, dev), thresh)
    ref = order[oracle.nms(boxes[order], thresh, normal=normal)]
    assert sel.dtype == torch.int64
    assert np.array_equal(sel.cpu().numpy(), ref)
    assert 0 < len(ref) < n


def hybrid_keep(oracle, dev, sorted_boxes, thresh, normal):
    """bg.hybrid_keep of boxes in score order: the oracle's decisions, the device's own IoU within TIE_BAND"""
    if sorted_boxes.shape[0] == 0:
        return np.zeros(0, np.int64)
    if normal:
        ref_iou = own_iou = bg.iou_normal_np(sorted_boxes, sorted_boxes)     # iou_normal restated: fp32 + - * / only, one value
    else:
        ref_iou = oracle.boxes_iou_bev(sorted_boxes, sorted_boxes)
        t = T(sorted_boxes, dev)
        own_iou = iu.boxes_iou_bev(t, t).cpu().numpy()
    return bg.hybrid_keep(ref_iou, own_iou, thresh, TIE_BAND)


@pytest.mark.parametrize("n,thresh,normal", NMS_LARGE)
def test_nms_matches_oracle(oracle, dev, n, thresh, normal):
    boxes, scores, order = nms_scene(n, 12.0)
    fn = iu.nms_normal_gpu if normal else iu.nms_gpu
    sel, _ = fn(T(boxes, dev).view(-1, 7), T(scores, dev), thresh)
    # torch's sort and numpy's agree when scores are distinct (they are); greedy NMS over the sorted boxes
    ref = order[hybrid_keep(oracle, dev, boxes[order], thresh, normal)]
    got = sel.cpu().numpy()
    assert sel.dtype == torch.int64
    assert np.array_equal(got, ref)
    if n:
        assert got[0] == order[0]                     # the best-scored box always survives


def test_nms_more_than_16384_boxes(dev):
    """The reference's nms_gpu takes any N (iou3d_nms_utils.py:120-136); beyond 16384 boxes the suppression walk keeps
    its bitmap in LDS.  Checked against a greedy walk over the IoU matrix of the same kernels' BEV IoU."""
    n, thresh = 17000, 0.3
    boxes, scores = random_boxes(n, 21, spread=60.0), np.random.default_rng(21).uniform(0, 1, n).astype(np.float32)
    b, sc = T(boxes, dev).view(-1, 7), T(scores, dev)
    sel, _ = iu.nms_gpu(b, sc, thresh)
    order = sc.sort(0, descending=True)[1]
    sup = iu.boxes_iou_bev(b[order].contiguous(), b[order].contiguous()) > thresh
    removed = torch.zeros(n, dtype=torch.bool, device=dev)
    later = torch.arange(n, device=dev)
    keep = []
    for i in range(n):   # host loop, device state
        if bool(removed[i]):
            continue
        keep.append(i)
        removed |= sup[i] & (later > i)
    ref = order[torch.tensor(keep, device=dev)]
    assert torch.equal(sel, ref)                      # both sides evaluate the same iou_bev: nothing to excuse
    assert 0 < len(keep) < n


@pytest.mark.parametrize("n,b_last", [(4095, False), (4096, False), (4097, False), (8200, False), (16383, False),
                                      (16384, False), (16384, True), (16385, False), (16385, True)])
def test_nms_every_slot_of_the_walk(dev, n, b_last):
    """chain_scene: the keep list is known by construction (A and C of every site stay, B goes; every decision at
    least 0.12 from the threshold), and the members of a site lie in different 64-box blocks and, from 12288 boxes on,
    in different 4096-box slots of nms_walk's four `removed` words per lane.  16385 boxes take the LDS walk."""
    boxes, scores, order, keep = bg.chain_scene_of(n, seed=n, b_last=b_last)
    assert boxes.shape[0] == n
    sel, _ = iu.nms_gpu(T(boxes, dev), T(scores, dev), 0.3)
    assert np.array_equal(sel.cpu().numpy(), keep)


def test_nms_pre_maxsize_and_self_consistency(dev):
    """Kept boxes do not suppress each other, every dropped box is suppressed by a kept one of higher score."""
    boxes, scores = random_boxes(800, 5, spread=8.0), np.random.default_rng(5).uniform(0, 1, 800).astype(np.float32)
    sel, none = iu.nms_gpu(T(boxes, dev), T(scores, dev), 0.2, pre_maxsize=300)
    assert none is None
    sel = sel.cpu().numpy()
    top = np.argsort(-scores, kind="stable")[:300]
    assert set(sel.tolist()) <= set(top.tolist())
    iou = iu.boxes_iou_bev(T(boxes, dev), T(boxes, dev)).cpu().numpy()
    kept = iou[np.ix_(sel, sel)] - np.eye(len(sel))
    assert (kept <= 0.2 + 1e-4).all()
    dropped = np.setdiff1d(top, sel)
    for d in dropped:
        better = sel[scores[sel] > scores[d]]
        assert (iou[better, d] > 0.2 - 1e-4).any()


# ---- points in boxes ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,T,M", POINT_CASES)
def test_points_in_boxes_matches_oracle(oracle, dev, B, T, M):
    pts, boxes = point_scene(B, T, M)
    ref = oracle.points_in_boxes(pts, boxes)
    got = iu.points_in_boxes_gpu(T_(pts, dev), T_(boxes, dev)).cpu().numpy()
    assert got.shape == (B, M) and got.dtype == np.int32
    if T and M:
        decided = ~near_face_mask(pts, boxes)         # device vs libm sin/cos: only a point within 1e-4 of a face may differ
        assert decided.mean() >= 0.995
        assert np.array_equal(got[decided], ref[decided])
        assert (ref >= 0).any() and (ref == -1).any() and (ref != T - 1).all()
    else:
        assert np.array_equal(got, ref)


@pytest.mark.parametrize("T,M", CHUNK_CASES)
def test_points_in_boxes_every_lds_chunk(oracle, dev, T, M):
    """Boxes are staged 128 at a time: the deciding box of a point in the first, second and third chunk, a point
    inside a box of the first chunk and one of the second (the first wins), T and M at and around 128 and 256."""
    pts, boxes, expected = chunk_scene(T, M)
    got = iu.points_in_boxes_gpu(T_(pts, dev), T_(boxes, dev)).cpu().numpy()
    known = expected != -2
    assert known.sum() == min(T, M, 200)
    assert np.array_equal(got[0, known], expected[known])
    if T > 128:
        assert (expected[known] >= 128).any()
    if T > 256:
        assert (expected[known] >= 256).any()
    ref = oracle.points_in_boxes(pts, boxes)
    assert np.array_equal(ref[0, known], expected[known])
    decided = ~near_face_mask(pts, boxes)
    assert decided.mean() >= 0.995
    assert np.array_equal(got[decided], ref[decided])
    assert (ref == -1).any()


def test_points_in_boxes_exact_faces(dev):
    """Heading 0 and exactly representable values: cosf(-0) = 1 and sinf(-0) = -0 exactly, so the local coordinates
    are the shifts themselves.  |z - cz| = dz / 2 is inside (the height test rejects with >); |lx| = dx / 2 is inside
    (the test is < dx / 2 + 1e-5); dx / 2 + 2e-5 is outside."""
    box = np.array([[[1.0, 2.0, 0.5, 4.0, 2.0, 1.5, 0.0]]], np.float32)
    e, up = np.float32(2e-5), np.float32(1.25) + np.spacing(np.float32(1.25))
    rows = [([1.0, 2.0, 1.25], 0), ([1.0, 2.0, -0.25], 0), ([1.0, 2.0, up], -1),
            ([3.0, 2.0, 0.5], 0), ([-1.0, 2.0, 0.5], 0), ([1.0, 3.0, 0.5], 0), ([1.0, 1.0, 0.5], 0),
            ([3.0, 3.0, 1.25], 0),
            ([np.float32(3.0) + e, 2.0, 0.5], -1), ([np.float32(-1.0) - e, 2.0, 0.5], -1),
            ([1.0, np.float32(3.0) + e, 0.5], -1), ([1.0, np.float32(1.0) - e, 0.5], -1)]
    pts = np.array([[r[0] for r in rows]], np.float32)
    assert float(pts[0, 8, 0]) - 3.0 > 1.5e-5 and 3.0 - float(pts[0, 11, 1]) - 2.0 > 1.5e-5
    got = iu.points_in_boxes_gpu(T_(pts, dev), T_(box, dev)).cpu().numpy()
    assert got[0].tolist() == [r[1] for r in rows]

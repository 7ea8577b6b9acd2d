"""Cases and exact references for the rotated-box operators (box_geometry.h, nms.h): numpy only, no GPU, no test.

  clip_area64     the intersection area of two rotated rectangles in float64 by polygon clipping: nothing of the
                  kernels' algorithm (edge intersections + contained corners with a 1e-2 margin + atan2 sort + fan)
  margin_band     the pairs on which that algorithm differs from exact geometry ON PURPOSE (inside_box's margin)
  CLOSED_FORM     pairs whose area is known by hand
  gap_threshold   an NMS threshold that no pair IoU of a scene comes near
  hybrid_keep     the reference's NMS keep list, with the pairs at the threshold left to the implementation
  chain_scene     an NMS scene whose keep list is known by construction, laid out over the blocks and slots of nms_walk
  near_face       the points within eps of a face plane of a box that can decide them

Boxes are 7 numbers [x, y, z, dx, dy, dz, heading]; the float32 values a kernel receives are the inputs, every
reference here starts from exactly those values widened to float64.
"""
import math

import numpy as np

F = np.float32


# ---- exact intersection area --------------------------------------------------------------------------------------
def _clip_axis(poly, axis, sign, lim):
    """Sutherland-Hodgman against the half-plane sign * p[axis] <= lim."""
    out = []
    for k in range(len(poly)):
        p, q = poly[k - 1], poly[k]
        dp, dq = sign * p[axis] - lim, sign * q[axis] - lim
        if dp <= 0:
            out.append(p)
        if (dp < 0 < dq) or (dq < 0 < dp):
            t = dp / (dp - dq)
            out.append((p[0] + t * (q[0] - p[0]), p[1] + t * (q[1] - p[1])))
    return out


def clip_area64(a, b):
    """Exact (float64) intersection area of the BEV footprints of boxes a and b: a's corners in b's frame, clipped
    against b's four half-planes, shoelace.  No margin."""
    a = [float(v) for v in np.asarray(a, dtype=np.float64)]
    b = [float(v) for v in np.asarray(b, dtype=np.float64)]
    ca, sa = math.cos(a[6]), math.sin(a[6])
    cb, sb = math.cos(b[6]), math.sin(b[6])
    poly = []
    for ux, uy in ((-0.5, -0.5), (0.5, -0.5), (0.5, 0.5), (-0.5, 0.5)):
        lx, ly = ux * a[3], uy * a[4]
        wx, wy = a[0] + lx * ca - ly * sa - b[0], a[1] + lx * sa + ly * ca - b[1]
        poly.append((wx * cb + wy * sb, -wx * sb + wy * cb))
    for axis, sign, lim in ((0, 1.0, b[3] / 2), (0, -1.0, b[3] / 2), (1, 1.0, b[4] / 2), (1, -1.0, b[4] / 2)):
        poly = _clip_axis(poly, axis, sign, lim)
        if len(poly) < 3:
            return 0.0
    s = 0.0
    for k in range(len(poly)):
        p, q = poly[k - 1], poly[k]
        s += p[0] * q[1] - q[0] * p[1]
    return abs(s) / 2


def clip_area64_matrix(a, b):
    return np.array([[clip_area64(x, y) for y in b] for x in a], dtype=np.float64).reshape(len(a), len(b))


def _corner_depth(box, other):
    """(...) largest signed Chebyshev distance, in box's frame, of the four corners of `other` to box's boundary
    (negative inside) and the smallest; both in float64, broadcasting over leading axes."""
    box, other = np.asarray(box, dtype=np.float64), np.asarray(other, dtype=np.float64)
    c, s = np.cos(other[..., 6]), np.sin(other[..., 6])
    cb, sb = np.cos(box[..., 6]), np.sin(box[..., 6])
    d = []
    for ux, uy in ((-0.5, -0.5), (0.5, -0.5), (0.5, 0.5), (-0.5, 0.5)):
        lx, ly = ux * other[..., 3], uy * other[..., 4]
        wx, wy = other[..., 0] + lx * c - ly * s - box[..., 0], other[..., 1] + lx * s + ly * c - box[..., 1]
        rx, ry = wx * cb + wy * sb, -wx * sb + wy * cb
        d.append(np.maximum(np.abs(rx) - box[..., 3] / 2, np.abs(ry) - box[..., 4] / 2))
    return np.stack(d, -1)


def margin_band(a, b, inside=1e-3, outside=2e-2):
    """True where a corner of one box lies between `inside` inside and `outside` outside the other's boundary
    (Chebyshev distance in the box frame, float64): there inside_box's 1e-2 margin may count a corner that exact
    geometry does not, so the kernels' algorithm and the exact area differ by design.  Broadcasts: a (..., 7), b (..., 7)."""
    da, db = _corner_depth(a, b), _corner_depth(b, a)
    return (((da >= -inside) & (da <= outside)) | ((db >= -inside) & (db <= outside))).any(-1)


def margin_band_matrix(a, b):
    return margin_band(np.asarray(a)[:, None, :], np.asarray(b)[None, :, :])


# ---- areas known by hand ------------------------------------------------------------------------------------------
def _box(x, y, dx, dy, h, z=0.0, dz=1.5):
    return np.array([x, y, z, dx, dy, dz, h], dtype=F)


def _turned_area(w, h, delta):
    """a w x h rectangle against itself turned by a small angle delta about the common centre: the rectangle less four
    corner triangles, w h - tan|delta| ((h/2 - w/2 t)^2 + (w/2 - h/2 t)^2), t = tan(|delta| / 2)."""
    d = abs(delta)
    t = math.tan(d / 2)
    return w * h - math.tan(d) * ((h / 2 - w / 2 * t) ** 2 + (w / 2 - h / 2 * t) ** 2)


def _closed_form():
    """-> list of (name, box a, box b, area, kind); kind 'exact' (geometry), 'quirk' (the algorithm's own, pinned) or
    'nan'.  Areas are those of the float32 values stored in the boxes: where a heading or a size is rounded on the way
    to float32, the area follows the rounded value."""
    rows = []

    def add(name, a, b, area, kind='exact'):
        rows.append((name, a, b, float(area), kind))

    f64 = lambda v: float(F(v))
    add('identical h=0', _box(0, 0, 4, 2, 0), _box(0, 0, 4, 2, 0), 8)
    add('identical h=0.7', _box(0, 0, 4, 2, 0.7), _box(0, 0, 4, 2, 0.7), 8)
    add('identical at (70, -40)', _box(70, -40, 4, 2, 0.7), _box(70, -40, 4, 2, 0.7), 8)
    # float32(pi) and float32(0.7 + pi / 2) are not pi and 0.7 + pi / 2: the second box is turned by the rounding error
    hp = F(np.pi)
    add('same footprint, heading + pi', _box(0, 0, 4, 2, 0), _box(0, 0, 4, 2, hp), _turned_area(4, 2, float(hp) - math.pi))
    hq = F(0.7) + F(np.pi / 2)
    add('same footprint, (dy, dx) at heading + pi/2', _box(0, 0, 4, 2, 0.7), _box(0, 0, 2, 4, hq),
        _turned_area(4, 2, float(hq) - f64(0.7) - math.pi / 2))
    add('nested, axis-aligned', _box(0, 0, 4, 2, 0), _box(0.5, 0.25, 1, 0.5, 0), 0.5)
    add('nested, rotated', _box(3, 5, 4, 2, 0.7), _box(3.25, 5.25, 1, 0.5, -0.4), 0.5)
    add('cross 6 x 1, axis-aligned', _box(2, 1, 6, 1, 0), _box(2, 1, 1, 6, 0), 1)
    add('cross 6 x 1, h=0.4', _box(2, 1, 6, 1, 0.4), _box(2, 1, 1, 6, 0.4), 1)
    # the diamond's corners reach the square's edge mid-points to within 5e-8: what pokes out is below 1e-14
    add('sqrt2 diamond in a 2-square', _box(0, 0, 2, 2, 0), _box(0, 0, np.sqrt(2), np.sqrt(2), np.pi / 4), f64(np.sqrt(2)) ** 2)
    # the octagon's area is stationary at 45 degrees: float32(pi/4)'s 2e-8 moves it by 1e-15
    add('2-squares 45 degrees apart', _box(0, 0, 2, 2, 0), _box(0, 0, 2, 2, np.pi / 4), 8 * (math.sqrt(2) - 1))
    add('half shift', _box(0, 0, 4, 2, 0), _box(2, 0, 4, 2, 0), 4)
    add('shared edge', _box(0, 0, 4, 2, 0), _box(4, 0, 4, 2, 0), 0)
    add('shared corner', _box(0, 0, 4, 2, 0), _box(4, 2, 4, 2, 0), 0)
    add('gap of 0.02', _box(0, 0, 4, 2, 0), _box(4.02, 0, 4, 2, 0), 0)
    add('far apart', _box(0, 0, 4, 2, 0.3), _box(50, -30, 4, 2, -1.0), 0)
    add('zero-size box', _box(0, 0, 4, 2, 0.3), _box(0.5, 0.2, 0, 0, 0), 0)
    add('both zero-size', _box(1, 1, 0, 0, 0), _box(1, 1, 0, 0, 0.5), 0)
    add('NaN centre', _box(0, 0, 4, 2, 0), _box(np.nan, 0, 4, 2, 0), 0, 'nan')
    hw = F(100.0 - 32 * np.pi)
    add('heading 100 against 100 - 32 pi', _box(1, -2, 4, 2, 100.0), _box(1, -2, 4, 2, hw),
        _turned_area(4, 2, (100.0 - float(hw)) - 32 * math.pi))
    add('slivers 10 x 0.05 at +-0.3', _box(0, 0, 10, 0.05, 0.3), _box(0, 0, 10, 0.05, -0.3),
        f64(0.05) ** 2 / math.sin(2 * f64(0.3)))
    # inside_box's margin: across an axis-aligned gap of 0.005 each box's two facing corners count as inside the
    # other, and the fan over those four corners is the gap's own rectangle, 0.005 x 2.  Pinned, not geometry.
    add('quirk: gap of 0.005', _box(0, 0, 4, 2, 0), _box(4.005, 0, 4, 2, 0), 0.01, 'quirk')
    return rows


CLOSED_FORM = _closed_form()


def closed_form_arrays():
    """-> boxes a (R, 7), boxes b (R, 7) float32, areas (R) float64, kinds (list)."""
    return (np.stack([r[1] for r in CLOSED_FORM]), np.stack([r[2] for r in CLOSED_FORM]),
            np.array([r[3] for r in CLOSED_FORM]), [r[4] for r in CLOSED_FORM])


# ---- NMS thresholds away from every pair ------------------------------------------------------------------------------
def iou_normal_np(a, b):
    """box_geometry.h's iou_normal (axis-aligned footprints, headings ignored) in float32, operation for operation."""
    a, b = np.asarray(a, dtype=F)[:, None, :], np.asarray(b, dtype=F)[None, :, :]
    two, zero = F(2), F(0)
    left, right = np.maximum(a[..., 0] - a[..., 3] / two, b[..., 0] - b[..., 3] / two), np.minimum(a[..., 0] + a[..., 3] / two, b[..., 0] + b[..., 3] / two)
    top, bottom = np.maximum(a[..., 1] - a[..., 4] / two, b[..., 1] - b[..., 4] / two), np.minimum(a[..., 1] + a[..., 4] / two, b[..., 1] + b[..., 4] / two)
    inter = np.maximum(right - left, zero) * np.maximum(bottom - top, zero)
    return (inter / np.maximum(a[..., 3] * a[..., 4] + b[..., 3] * b[..., 4] - inter, F(1e-8))).astype(F)


def gap_threshold(iou, nominal):
    """iou (n, n): the pair IoUs of a scene.  -> (threshold, half-gap): the float32 mid-point of the widest interval
    free of pair IoUs inside nominal +- 25 %, and the distance from it to the nearest pair IoU (or end of the range)."""
    iou = np.asarray(iou, dtype=np.float64)
    v = iou[np.triu_indices(iou.shape[0], 1)]
    lo, hi = 0.75 * nominal, 1.25 * nominal
    v = np.sort(np.concatenate([[lo, hi], v[(v > lo) & (v < hi)]]))
    k = int(np.argmax(np.diff(v)))
    t = float(F((v[k] + v[k + 1]) / 2))
    return t, min(t - v[k], v[k + 1] - t)


def greedy_keep(sup):
    """the NMS walk over a suppression matrix in score order: sup[i, j] (j > i) = box i, if kept, removes box j."""
    sup = np.asarray(sup, dtype=bool)
    n = sup.shape[0]
    removed = np.zeros(n, dtype=bool)
    keep = []
    for i in range(n):
        if removed[i]:
            continue
        keep.append(i)
        removed[i + 1:] |= sup[i, i + 1:]
    return np.asarray(keep, dtype=np.int64)


def hybrid_keep(ref_iou, own_iou, thresh, band=1e-4):
    """The keep list (positions in score order) of a greedy walk over the reference's decisions ref_iou > thresh, except
    for the pairs whose reference IoU is within `band` of the threshold: those, and only those, are decided by the
    implementation's own IoU of that pair (a last-bit cosf may fall either side).  thresh is compared as float32."""
    ref_iou, own_iou, thresh = np.asarray(ref_iou, dtype=F), np.asarray(own_iou, dtype=F), F(thresh)
    tie = np.abs(ref_iou.astype(np.float64) - float(thresh)) < band
    return greedy_keep(np.where(tie, own_iou > thresh, ref_iou > thresh))


# ---- an NMS scene with a keep list known by construction ------------------------------------------------------------
def chain_scene(nsites, seed, pitch=8.0, extra=0, b_last=False):
    """Sites on a square lattice of `pitch` metres, three boxes per site: A (3-4 x 1.5-2, any heading), B = A moved
    along its own x axis by 0.4 dx, C = A moved by 0.8 dx.  IoU(A, B) = IoU(B, C) = 0.6 / 1.4 = 0.4286, IoU(A, C) =
    0.2 / 1.8 (a little more with inside_box's margin, at most 0.154), boxes of different sites are at least 0.3 m
    apart: IoU exactly 0.  At a threshold of 0.3 every decision is at least 0.12 away.
    extra = 1, 2: one more site holding only A, or only A and B (so that any box count can be reached).

    The score order ranks all A's, then all B's, then all C's: A is kept, B is suppressed by A, and C is kept because
    a suppressed box does not itself suppress.  One permutation of the sites orders all three groups, so a site's
    members are nsites (+ 1) ranks apart: in different 64-box blocks from 64 sites on, and in different 4096-box slots
    of nms_walk from 4096 sites on (below that, for every site whose members straddle a slot boundary).
    b_last: all A's, all C's, then all B's: the same keep set, with the suppressed boxes in the last blocks and slots.

    -> boxes (n, 7) float32 in storage order (shuffled), scores (n) float32 distinct in (0.15, 0.95], order (n) = the
    boxes by descending score, keep = the expected keep list (indices into boxes, in score order)."""
    assert extra in (0, 1, 2)
    rng = np.random.default_rng(seed)
    ns = nsites + (1 if extra else 0)
    side = int(math.ceil(math.sqrt(ns)))
    site = np.arange(ns)
    cx, cy = (site % side - (side - 1) / 2) * pitch, (site // side - (side - 1) / 2) * pitch
    dx, dy, dz = rng.uniform(3, 4, ns), rng.uniform(1.5, 2, ns), rng.uniform(1, 2, ns)
    h = -rng.uniform(-np.pi, np.pi, ns)                        # (-pi, pi]
    z = rng.uniform(-1, 1, ns)
    members = []
    for shift in (-0.4, 0.0, 0.4):                             # B sits on the lattice point
        members.append(np.stack([cx + shift * dx * np.cos(h), cy + shift * dx * np.sin(h), z, dx, dy, dz, h], 1))
    perm = rng.permutation(ns)
    role_rows = [perm, perm[perm < nsites + (extra == 2)], perm[perm < nsites]]     # sites holding an A, a B, a C
    groups = [(0, role_rows[0]), (2, role_rows[2]), (1, role_rows[1])] if b_last else [(r, role_rows[r]) for r in range(3)]
    ranked = np.concatenate([members[r][rows] for r, rows in groups]).astype(F)
    kept_rank = np.concatenate([np.full(len(rows), r != 1) for r, rows in groups])
    n = ranked.shape[0]
    store = rng.permutation(n)                                  # storage position of the box of each rank
    boxes, scores = np.zeros((n, 7), F), np.zeros(n, F)
    boxes[store] = ranked
    scores[store] = (0.15 + 0.8 * (n - np.arange(n)) / n).astype(F)
    assert np.unique(scores).size == n
    return boxes, scores, store.astype(np.int64), store[kept_rank].astype(np.int64)


def chain_scene_of(n, seed, **kw):
    """chain_scene with exactly n boxes."""
    return chain_scene(n // 3, seed, extra=n % 3, **kw)


# ---- points a last-bit difference in cosf / sinf could move across a face ---------------------------------------------
def near_face(pts, boxes, eps=1e-4):
    """pts (M, 3), boxes (T, 7) -> bool (M): the point lies within eps of a face plane of a box that can decide it:
    one whose BEV bounding circle + 0.1 m holds the point and with |z - cz| < dz / 2 + 0.1.  float64; the clearance
    arithmetic is roi_pool_reference's."""
    from roi_pool_reference import point_face_clearance
    pts, boxes = np.asarray(pts, dtype=np.float64), np.asarray(boxes, dtype=np.float64)
    near = np.zeros(pts.shape[0], dtype=bool)
    for bx in boxes:
        clear, (lx, ly, lz) = point_face_clearance(pts, bx)
        reach = 0.5 * math.hypot(bx[3], bx[4]) + 0.1
        decides = (lx * lx + ly * ly < reach * reach) & (np.abs(lz) < bx[5] / 2 + 0.1)
        near |= decides & (clear < eps)
    return near

"""The rotated BEV RoI crop of SECOND-IoU's head in numpy float64, its error bound, and the cases the crop tests share.
A helper module like pv_rcnn_reference.py: no fixtures here.

crop64 restates what SECONDHead.roi_grid_pool computes per RoI (theta, the corner-aligned G x G lattice, the pixel position, the
bilinear blend with zero padding) in float64, from the fp32 inputs as the operator sees them.

The bound.  Bilinear sampling with zero padding is continuous in the position, so per output element
    |got - want64| <= delta (Lx_c + Ly_c) + 8 2^-24 T
with Lx_c, Ly_c the largest absolute differences of horizontally and vertically adjacent cells of that sample's channel c, the
map padded with one ring of zeros; T the blend's sum of |weight * corner|; delta the position error in cells:
    delta = DELTA_UNITS 2^-24 max(H, W).
DELTA_UNITS is 4 x the largest deviation, in those units, of the reference's own fp32 output grid (its theta through torch's
affine_grid and grid_sample's un-normalisation, on the CPU) from float64 over CASES below, as tests/golden/
gen_second_iou_fixtures.py measured it (ref_second_iou.npz: 'delta.units.<case>'): the factor 4 because the operator's order of
operations differs from torch's batched matmul.  tests/test_second_iou_host.py asserts that the constant is 4 x the fixture's
figure and that the reference's own pooled output lies within the bound.
"""
import numpy as np

U = 2.0 ** -24
MEASURED_UNITS = 3.4        # gen_second_iou_fixtures.py: the largest 'delta.units.<case>', rounded up to one decimal
DELTA_UNITS = 4 * MEASURED_UNITS

# geometry of the crop cases: cells of 0.4 m (VOXEL_SIZE 0.05 * DOWNSAMPLE_RATIO 8), the map's corner at (X0, Y0)
VOXEL, RATIO, X0, Y0 = [0.05, 0.05, 0.1], 8, 0.0, -2.6
CELL = np.float32(VOXEL[0] * RATIO)
CASES = {'small': (13, 9), 'kitti': (200, 176)}         # (H, W)


SHAPES = [(1, 1, 7), (3, 37, 9), (1, 37, 7), (3, 1, 9)]     # (B, n, roi_stride)


def crop_cases():
    """the crop cases of tests/test_bev_roi_crop_gpu.py, which the fixture generator measures delta over:
    (name, C, G, B, n, roi_stride, seed)"""
    return [(name, C, G, B, n, stride, 17 * k + C + G) for name in CASES for C in (1, 5, 64) for G in (2, 7)
            for k, (B, n, stride) in enumerate(SHAPES)]


def pc_range(H, W):
    return [X0, Y0, -3.0, X0 + float(CELL) * W, Y0 + float(CELL) * H, 1.0]


def make_rois(H, W, B, n, roi_stride, seed):
    """(B, n, roi_stride) fp32 rois on an H x W map of CELL-sized cells: in turn a roi inside the map, one across each of the four
    borders, one wholly outside (every sample position more than a cell off the map), at headings 0, pi / 2 and arbitrary in
    turn; the last row of every sample with n > 1 is the all-zero padding proposal_layer leaves.  -> (rois, outside (B, n) bool)"""
    rng = np.random.default_rng(seed)
    cell = float(CELL)
    wx, wy = W * cell, H * cell
    rois = np.zeros((B, n, roi_stride), dtype=np.float32)
    outside = np.zeros((B, n), dtype=bool)
    k = 0
    for b in range(B):
        for r in range(n):
            if n > 1 and r == n - 1:
                continue                                    # the padding row
            kind = k % 6
            size = rng.uniform(1.0, 4.5, 2) if min(H, W) > 20 else rng.uniform(0.6, 2.0, 2)
            centre = np.array([X0 + rng.uniform(0.3, 0.7) * wx, Y0 + rng.uniform(0.3, 0.7) * wy])
            if kind == 1:
                centre[0] = X0 + rng.uniform(-0.2, 0.2) * size[0]
            elif kind == 2:
                centre[0] = X0 + wx + rng.uniform(-0.2, 0.2) * size[0]
            elif kind == 3:
                centre[1] = Y0 + rng.uniform(-0.2, 0.2) * size[1]
            elif kind == 4:
                centre[1] = Y0 + wy + rng.uniform(-0.2, 0.2) * size[1]
            elif kind == 5:
                far = float(np.hypot(size[0], size[1])) + 2 * cell
                centre = [(X0 - far, centre[1]), (X0 + wx + far, centre[1]), (centre[0], Y0 - far), (centre[0], Y0 + wy + far)][(k // 6) % 4]
                outside[b, r] = True
            heading = [0.0, np.pi / 2, rng.uniform(-np.pi, np.pi)][(k // 2) % 3]
            rois[b, r, :7] = [centre[0], centre[1], rng.uniform(-1, 0), size[0], size[1], 1.5, heading]
            if roi_stride > 7:
                rois[b, r, 7:] = rng.standard_normal(roi_stride - 7)
            k += 1
    return rois, outside


def make_map(B, C, H, W, seed):
    """a smooth field plus noise: neighbouring cells differ by less than the values' spread, as a backbone's map does"""
    rng = np.random.default_rng(seed)
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing='ij')
    phase = rng.uniform(0, 2 * np.pi, (B, C, 1, 1))
    freq = rng.uniform(0.05, 0.6, (B, C, 1, 1))
    return (np.sin(freq * xx + phase) * np.cos(0.7 * freq * yy - phase) + 0.1 * rng.standard_normal((B, C, H, W))).astype(np.float32)


def positions64(rois, H, W, x0, y0, cell_x, cell_y, G, transpose_ij=False):
    """pixel positions (R, G, G) of every RoI's lattice, [i][j], in float64 from the fp32 inputs: the reference's theta,
    affine_grid(align_corners=True) and grid_sample's un-normalisation"""
    r = rois.reshape(-1, rois.shape[-1]).astype(np.float64)
    x0, y0, cell_x, cell_y = (float(np.float32(v)) for v in (x0, y0, cell_x, cell_y))
    x1, x2 = (r[:, 0] - r[:, 3] / 2 - x0) / cell_x, (r[:, 0] + r[:, 3] / 2 - x0) / cell_x
    y1, y2 = (r[:, 1] - r[:, 4] / 2 - y0) / cell_y, (r[:, 1] + r[:, 4] / 2 - y0) / cell_y
    cosa, sina = np.cos(r[:, 6]), np.sin(r[:, 6])
    t = [(x2 - x1) / (W - 1) * cosa, (x2 - x1) / (W - 1) * -sina, (x1 + x2 - W + 1) / (W - 1),
         (y2 - y1) / (H - 1) * sina, (y2 - y1) / (H - 1) * cosa, (y1 + y2 - H + 1) / (H - 1)]
    t = [v[:, None, None] for v in t]
    lat = -1 + 2 * np.arange(G) / (G - 1)
    u, v = lat[None, None, :], lat[None, :, None]
    if transpose_ij:
        u, v = v, u
    px = ((t[0] * u + t[1] * v + t[2]) + 1) / 2 * (W - 1)
    py = ((t[3] * u + t[4] * v + t[5]) + 1) / 2 * (H - 1)
    return px, py


def blend64(feat, sample_of_roi, px, py):
    """feat (B, C, H, W), positions (R, G, G) -> (want (R, C, G, G), T (R, C, G, G)): the bilinear blend with zero padding and the
    sum of |weight * corner|, float64"""
    f = feat.astype(np.float64)
    B, C, H, W = f.shape
    fx0, fy0 = np.floor(px), np.floor(py)
    fx, fy = px - fx0, py - fy0
    want = np.zeros((px.shape[0], C) + px.shape[1:])
    T = np.zeros_like(want)
    for dx, dy, w in ((0, 0, (1 - fx) * (1 - fy)), (1, 0, fx * (1 - fy)), (0, 1, (1 - fx) * fy), (1, 1, fx * fy)):
        x, y = fx0 + dx, fy0 + dy
        on = (x >= 0) & (x < W) & (y >= 0) & (y < H)
        xi, yi = np.clip(x, 0, W - 1).astype(np.int64), np.clip(y, 0, H - 1).astype(np.int64)
        val = f[sample_of_roi[:, None, None, None], np.arange(C)[None, :, None, None], yi[:, None], xi[:, None]]
        val = np.where(on[:, None], val, 0.0)
        want += val * w[:, None]
        T += np.abs(val * w[:, None])
    return want, T


def crop64(rois, feat, x0, y0, cell_x, cell_y, G, transpose_ij=False, swap_xy=False):
    """-> (want, T), both (B n, C, G, G) float64.  transpose_ij: cell (i, j) sampled where (j, i) belongs; swap_xy: the RoI's x
    and y (and dx, dy) exchanged: the two mistakes the tests must be able to see."""
    B, n = rois.shape[0], rois.shape[1]
    if swap_xy:
        rois = rois.copy()
        rois[..., [0, 1]] = rois[..., [1, 0]]
        rois[..., [3, 4]] = rois[..., [4, 3]]
    px, py = positions64(rois, feat.shape[2], feat.shape[3], x0, y0, cell_x, cell_y, G, transpose_ij)
    return blend64(feat, np.repeat(np.arange(B), n), px, py)


def lipschitz(feat):
    """(Lx, Ly), each (B, C): the largest |difference| of horizontally / vertically adjacent cells of the zero-padded maps"""
    p = np.pad(feat.astype(np.float64), ((0, 0), (0, 0), (1, 1), (1, 1)))
    return np.abs(np.diff(p, axis=3)).max(axis=(2, 3)), np.abs(np.diff(p, axis=2)).max(axis=(2, 3))


def delta(H, W, units=DELTA_UNITS):
    return units * U * max(H, W)


def crop_bound(feat, n, T, units=DELTA_UNITS):
    """the bound of every element of a (B n, C, G, G) crop"""
    Lx, Ly = lipschitz(feat)
    L = np.repeat(Lx + Ly, n, axis=0)[:, :, None, None]
    return delta(feat.shape[2], feat.shape[3], units) * L + 8 * U * T

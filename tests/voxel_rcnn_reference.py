"""What the Voxel R-CNN tests share (a helper module like sparse_conv_reference.py: no tests, no fixtures, nothing from
pdm_ssd_amd): a numpy restatement of the RoI-grid pooling specified in DESIGN.md 7t, voxels found through a dictionary keyed
by coordinate.

  grid_points   local = (i + 0.5) / G size - size / 2, nonzero()'s order (x index slowest), turned by the heading, plus the centre;
                fp32, one rounding per operation
  cells         floor(floor((p - p0) / voxel) / stride) per axis (floor, not truncation, for negative cells)
  centres       (float(c) + 0.5) (float(voxel) stride) + p0: three fp32 roundings
  hit_sets      the window walked z outermost and x innermost, cells outside the grid and unset cells skipped, a set cell kept
                unless sqdist(centre - p) > radius^2, the FIRST nsample kept cells
  pool          max over the group of relu(f + fma(dot(Wp, centre - p), scale_p, shift_p)); relu(shift_p) for an empty group;
                out = relu((Wout pooled) scale_o + shift_o).  In float64, with the same expression on absolute values (the `A` of
                the tests' bound).
The host tests hold it to the reference's own NeighborVoxelSAModuleMSG (tests/golden/ref_voxel_rcnn.npz); the GPU tests hold the
device to it.
"""
import numpy as np

f32 = np.float32


def grid_points(rois, G):
    """rois (R, 7 + C) -> (R G^3, 3) fp32 grid points, rows r G^3 + (ix G + iy) G + iz"""
    rois = np.asarray(rois, dtype=f32).reshape(-1, np.shape(rois)[-1])
    idx = np.stack(np.meshgrid(np.arange(G), np.arange(G), np.arange(G), indexing='ij'), -1).reshape(-1, 3).astype(f32)     # x slowest
    size = rois[:, None, 3:6]
    local = ((idx[None] + f32(0.5)) / f32(G)) * size - size / f32(2)
    c, s = np.cos(rois[:, 6]).astype(f32)[:, None], np.sin(rois[:, 6]).astype(f32)[:, None]
    x = local[..., 0] * c - local[..., 1] * s
    y = local[..., 0] * s + local[..., 1] * c
    out = np.stack([x, y, local[..., 2]], -1).astype(f32) + rois[:, None, 0:3]
    return out.reshape(-1, 3).astype(f32)


def cell_coordinate(points, point_cloud_range, voxel_size):
    """the fp32 quotient (p - p0) / voxel whose floor is the base cell (the generator keeps it away from the cell boundaries)"""
    return (np.asarray(points, dtype=f32) - np.asarray(point_cloud_range[:3], dtype=f32)) / np.asarray(voxel_size, dtype=f32)


def cells(points, point_cloud_range, voxel_size, stride):
    """-> (M, 3) int64 (x, y, z) cells at the level of `stride`"""
    with np.errstate(invalid='ignore', over='ignore'):
        c0 = np.floor(cell_coordinate(points, point_cloud_range, voxel_size))
    c0 = np.where(np.isfinite(c0) & (np.abs(c0) < 1e9), c0, -2.0 ** 30)
    return np.floor_divide(c0.astype(np.int64), int(stride))


def centres(zyx, stride, voxel_size, point_cloud_range):
    """(N, 3) (z, y, x) indices of a level -> (N, 3) fp32 centres (x, y, z)"""
    c = np.asarray(zyx)[:, [2, 1, 0]].astype(f32)
    v = np.asarray(voxel_size, dtype=f32) * f32(stride)
    return ((c + f32(0.5)) * v + np.asarray(point_cloud_range[:3], dtype=f32)).astype(f32)


def sqdist(d):
    """fma(dz, dz, fma(dy, dy, rn(dx dx))) in fp32 (products of fp32 values are exact in float64)"""
    d = np.asarray(d, dtype=f32).astype(np.float64)
    t = f32(d[..., 0] * d[..., 0]).astype(np.float64)
    t = f32(d[..., 1] * d[..., 1] + t).astype(np.float64)
    return f32(d[..., 2] * d[..., 2] + t)


def hit_sets(points, sample, cell, indices, shape, stride, voxel_size, point_cloud_range, query_range, radius, nsample):
    """-> (hits: per grid point the list of rows, offsets: per grid point (len, 3) fp32 centre - p, margin: the smallest
    |sqrt(d2) - radius| / radius over every tested voxel)"""
    idx = np.asarray(indices, dtype=np.int64).reshape(-1, 4)
    where = {tuple(c): i for i, c in enumerate(idx.tolist())}
    D, H, W = shape
    rz, ry, rx = query_range
    r2 = f32(f32(radius) * f32(radius))
    cen = centres(idx[:, 1:4], stride, voxel_size, point_cloud_range) if len(idx) else np.zeros((0, 3), f32)
    hits, offsets, margin = [], [], np.inf
    for p, b, (cx, cy, cz) in zip(np.asarray(points, dtype=f32), sample, np.asarray(cell).tolist()):
        rows, offs = [], []
        for dz in range(-rz, rz + 1):
            for dy in range(-ry, ry + 1):
                for dx in range(-rx, rx + 1):
                    z, y, x = cz + dz, cy + dy, cx + dx
                    if not (0 <= z < D and 0 <= y < H and 0 <= x < W):
                        continue
                    row = where.get((int(b), z, y, x))
                    if row is None:
                        continue
                    d = cen[row] - p
                    d2 = sqdist(d)
                    if radius > 0:
                        margin = min(margin, abs(float(np.sqrt(np.float64(d2))) - float(radius)) / float(radius))
                    if d2 > r2:
                        continue
                    if len(rows) < nsample:
                        rows.append(row)
                        offs.append(d)
        hits.append(rows)
        offsets.append(np.array(offs, dtype=f32).reshape(-1, 3))
    return hits, offsets, margin


def pool(features_in, hits, offsets, wp, scale_p, shift_p, wout, scale_o, shift_o):
    """-> (out (M, C2) float64, A (M, C2) float64: the same expression on absolute values, pooled (M, C1) float64)"""
    f = np.asarray(features_in, dtype=np.float64)
    wp, sp, hp = (np.asarray(t, dtype=np.float64) for t in (wp, scale_p, shift_p))
    wo, so, ho = (np.asarray(t, dtype=np.float64) for t in (wout, scale_o, shift_o))
    M, C1 = len(hits), wp.shape[0]
    pooled, pooled_abs = np.zeros((M, C1)), np.zeros((M, C1))
    for m, (rows, d) in enumerate(zip(hits, offsets)):
        if not rows:
            pooled[m], pooled_abs[m] = np.maximum(hp, 0), np.abs(hp)
            continue
        d = d.astype(np.float64)
        pos = (d @ wp.T) * sp + hp                                  # (len, C1)
        pooled[m] = np.maximum(f[rows] + pos, 0).max(0)
        pooled_abs[m] = (np.abs(f[rows]) + (np.abs(d) @ np.abs(wp).T) * np.abs(sp) + np.abs(hp)).max(0)
    out = np.maximum((pooled @ wo.T) * so + ho, 0)
    A = (pooled_abs @ np.abs(wo).T) * np.abs(so) + np.abs(ho)
    return out, A, pooled


def fold(weight, bias, mean, var, eps=1e-5):
    """eval BatchNorm -> (scale, shift) in float64"""
    scale = np.asarray(weight, np.float64) / np.sqrt(np.asarray(var, np.float64) + eps)
    return scale, np.asarray(bias, np.float64) - np.asarray(mean, np.float64) * scale


def module_forward(state, prefix, k, rois, G, indices, features, shape, stride, voxel_size, point_cloud_range, query_range, radius, nsample,
                   with_bound=False):
    """scale k of a NeighborVoxelSAModuleMSG from its state_dict arrays (state[prefix + 'mlps_in.k.0.weight'], ...), in float64
    behind the fp32 geometry -> (out (M, C2), hits), and with_bound: (out, hits, A, C1)"""
    def bn(name):
        p = f'{prefix}{name}.{k}.1.'
        return fold(state[p + 'weight'], state[p + 'bias'], state[p + 'running_mean'], state[p + 'running_var'])
    w_in = np.asarray(state[f'{prefix}mlps_in.{k}.0.weight'], np.float64).reshape(-1, np.shape(features)[1])
    w_pos = np.asarray(state[f'{prefix}mlps_pos.{k}.0.weight'], np.float64).reshape(-1, 3)
    w_out = np.asarray(state[f'{prefix}mlps_out.{k}.0.weight'], np.float64).reshape(-1, w_in.shape[0])
    s_in, h_in = bn('mlps_in')
    s_pos, h_pos = bn('mlps_pos')
    s_out, h_out = bn('mlps_out')
    f_in = (np.asarray(features, np.float64) @ w_in.T) * s_in + h_in
    rois = np.asarray(rois, dtype=f32)
    B, n = rois.shape[0], rois.shape[1]
    pts = grid_points(rois, G)
    sample = np.repeat(np.arange(B), n * G ** 3)
    cell = cells(pts, point_cloud_range, voxel_size, stride)
    hits, offs, _ = hit_sets(pts, sample, cell, indices, shape, stride, voxel_size, point_cloud_range, query_range, radius, nsample)
    out, A, _ = pool(f_in, hits, offs, w_pos, s_pos, h_pos, w_out, s_out, h_out)
    return (out, hits, A, w_in.shape[0]) if with_bound else (out, hits)

"""What the PV-RCNN tests share (a helper module like voxel_rcnn_reference.py: no tests, no fixtures, nothing from pdm_ssd_amd): a
numpy restatement of the keypoint path specified in DESIGN.md 7w.

  fps              farthest point sampling as the kernels run it: temp = 1e10, pick 0 first, fp32 pinned squared distances, the
                   first index on a tie
  keypoint_rows    per sample min(N, K) picks, slot j reads pick j mod that count (the reference's repeat rule)
  bev_interpolate  bilinear_interpolate_torch in fp32, one rounding per operation, the weights from the clamped corners
  ball_query       stack_ball_query_kernel's rows (strict <, first nsample by index, padding with the first hit, empty balls zero
                   rows and flagged) plus the smallest relative clearance |d^2 - r^2| / r^2 seen
  sa_msg           StackSAModuleMSG in eval mode, float64 behind the fp32 geometry
  linear_bn_relu   a Linear / Conv1d(k=1) + BatchNorm (eval) + ReLU stack in float64
The host tests hold it to the reference's own modules (tests/golden/ref_pv_rcnn.npz); the GPU tests hold the device to the fixture.
"""
import numpy as np

from voxel_rcnn_reference import grid_points, sqdist  # noqa: F401  (the lattice and the pinned distance are Voxel R-CNN's)

f32 = np.float32
EPS = 1e-5


def fps(xyz, npoint):
    xyz = np.asarray(xyz, dtype=f32)
    temp = np.full(len(xyz), 1e10, dtype=f32)
    out = np.zeros(npoint, dtype=np.int64)
    for j in range(1, npoint):
        temp = np.minimum(sqdist(xyz - xyz[out[j - 1]]), temp)
        out[j] = int(np.argmax(temp))
    return out


def keypoint_rows(points, counts, num_keypoints):
    """-> (B, K) rows of `points`"""
    rows, start = [], 0
    for n in counts:
        picks = fps(points[start:start + n, 1:4], min(n, num_keypoints))
        rows.append(start + picks[np.arange(num_keypoints) % len(picks)])
        start += n
    return np.stack(rows)


def bev_interpolate(keypoints, bev, point_cloud_range, voxel_size, stride):
    """keypoints (K, 4) rows (b, x, y, z), bev (B, C, H, W) -> (K, C) fp32"""
    kp = np.asarray(keypoints, dtype=f32)
    H, W = bev.shape[2], bev.shape[3]
    x = (kp[:, 1] - f32(point_cloud_range[0])) / f32(voxel_size[0]) / f32(stride)
    y = (kp[:, 2] - f32(point_cloud_range[1])) / f32(voxel_size[1]) / f32(stride)
    fx, fy = np.floor(x).astype(np.int64), np.floor(y).astype(np.int64)
    x0, x1 = np.clip(fx, 0, W - 1), np.clip(fx + 1, 0, W - 1)
    y0, y1 = np.clip(fy, 0, H - 1), np.clip(fy + 1, 0, H - 1)
    b = kp[:, 0].astype(np.int64)
    Ia, Ib, Ic, Id = bev[b, :, y0, x0], bev[b, :, y1, x0], bev[b, :, y0, x1], bev[b, :, y1, x1]
    wa = (x1.astype(f32) - x) * (y1.astype(f32) - y)
    wb = (x1.astype(f32) - x) * (y - y0.astype(f32))
    wc = (x - x0.astype(f32)) * (y1.astype(f32) - y)
    wd = (x - x0.astype(f32)) * (y - y0.astype(f32))
    return (((Ia * wa[:, None] + Ib * wb[:, None]).astype(f32) + Ic * wc[:, None]).astype(f32) + Id * wd[:, None]).astype(f32)


def ball_query(radius, nsample, xyz, xyz_cnt, new_xyz, new_cnt):
    """-> idx (M, nsample) int32 LOCAL to the sample, empty (M,) bool, the sizes of the balls before the cut (M,), clearance"""
    xyz, new_xyz = np.asarray(xyz, dtype=f32), np.asarray(new_xyz, dtype=f32)
    r2 = f32(radius) * f32(radius)
    M = len(new_xyz)
    idx = np.zeros((M, nsample), dtype=np.int32)
    empty = np.zeros(M, dtype=bool)
    sizes = np.zeros(M, dtype=np.int64)
    clearance = np.inf
    xs, ns = np.concatenate([[0], np.cumsum(xyz_cnt)]), np.concatenate([[0], np.cumsum(new_cnt)])
    for b in range(len(xyz_cnt)):
        src = xyz[xs[b]:xs[b + 1]]
        for m in range(ns[b], ns[b + 1]):
            d = sqdist(new_xyz[m] - src) if len(src) else np.zeros(0, f32)
            if len(d):
                clearance = min(clearance, float(np.abs(d.astype(np.float64) - float(r2)).min() / float(r2)))
            hits = np.nonzero(d < r2)[0]
            sizes[m] = len(hits)
            if len(hits) == 0:
                empty[m] = True
                continue
            idx[m] = hits[0]
            idx[m, :min(len(hits), nsample)] = hits[:nsample]
    return idx, empty, sizes, clearance


def _bn(x, state, prefix):
    return (x - state[prefix + 'running_mean']) / np.sqrt(state[prefix + 'running_var'].astype(np.float64) + EPS) * state[prefix + 'weight'] \
        + state[prefix + 'bias']


def linear_bn_relu(x, state, prefix, first=0):
    """the children first, first + 1, ... of a Sequential: weight (C', C[, 1]) without bias + BatchNorm + ReLU per block (a
    Dropout child is skipped), a trailing biased layer without them; x (rows, C) -> (rows, C') float64"""
    x = np.asarray(x, dtype=np.float64)
    k = first
    while f'{prefix}{k}.weight' in state or f'{prefix}{k + 1}.weight' in state:
        if f'{prefix}{k}.weight' not in state:      # a Dropout
            k += 1
            continue
        w = state[f'{prefix}{k}.weight'].astype(np.float64)
        x = x @ w.reshape(w.shape[0], -1).T
        if f'{prefix}{k}.bias' in state:
            return x + state[f'{prefix}{k}.bias']
        x = np.maximum(_bn(x, state, f'{prefix}{k + 1}.'), 0)
        k += 3
    return x


def sa_msg(state, prefix, radii, nsamples, xyz, xyz_cnt, new_xyz, new_cnt, features):
    """-> ((M, sum of widths) float64, [idx per scale], [empty per scale], [sizes per scale], clearance)"""
    xyz, new_xyz = np.asarray(xyz, dtype=f32), np.asarray(new_xyz, dtype=f32)
    starts = np.repeat(np.concatenate([[0], np.cumsum(xyz_cnt)])[:-1], new_cnt)
    cols, idxs, empties, sizes, clearance = [], [], [], [], np.inf
    for k, (radius, nsample) in enumerate(zip(radii, nsamples)):
        idx, empty, size, c = ball_query(radius, nsample, xyz, xyz_cnt, new_xyz, new_cnt)
        clearance = min(clearance, c)
        g = idx + starts[:, None]
        rel = (xyz[g] - new_xyz[:, None, :]).astype(f32)                                        # (M, ns, 3)
        grouped = rel if features is None else np.concatenate([rel, np.asarray(features, dtype=f32)[g]], -1)
        grouped = np.where(empty[:, None, None], 0, grouped).astype(np.float64)
        M, ns, C = grouped.shape
        y = linear_bn_relu(grouped.reshape(M * ns, C), state, f'{prefix}mlps.{k}.')
        cols.append(y.reshape(M, ns, -1).max(1))
        idxs.append(idx); empties.append(empty); sizes.append(size)
    return np.concatenate(cols, 1), idxs, empties, sizes, clearance

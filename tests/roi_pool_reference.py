"""Numpy restatement of the three launchers of the reference's RoI pooling extensions, written from
pcdet/ops/roipoint_pool3d/src/roipoint_pool3d_kernel.cu:22-134 (roipool3dLauncher) and
pcdet/ops/roiaware_pool3d/src/roiaware_pool3d_kernel.cu:39-233 (roiaware_pool3d_launcher), :236-307
(roiaware_pool3d_backward_launcher).  fp32 operation for operation where the kernels compute in fp32 (local coordinates,
voxel indices with the clamp on `unsigned`, the average's adds and its one divide), outputs updated in place over what
the caller passed (the reference's callers zero-fill), the maximum a strict > from -inf.

The in-box mask is oracle.cpu_oracle.points_in_boxes with one-box lists: one definition of check_pt_in_box3d's margin
rule on the test side.  Used by tests/golden/gen_roi_fixtures.py (as the stubbed native extensions under the reference's
own Python) and by tests/test_roi_pool_host.py / test_roi_pool_gpu.py.
"""
import numpy as np

from oracle import cpu_oracle as o

F = np.float32


def in_box_mask(pts, box):
    """pts (N, 3), box (7) -> bool (N): check_pt_in_box3d."""
    pts = np.ascontiguousarray(pts, dtype=F)
    if pts.shape[0] == 0:
        return np.zeros((0,), dtype=bool)
    return o.points_in_boxes(pts[None], np.ascontiguousarray(box, dtype=F)[None, None, :7])[0] == 0


def local_xy(pts, box):
    """lidar_to_local_coords in fp32, one rounding per operation."""
    pts, box = np.asarray(pts, dtype=F), np.asarray(box, dtype=F)
    sx, sy = pts[:, 0] - box[0], pts[:, 1] - box[1]
    c, s = np.cos(-box[6], dtype=F), np.sin(-box[6], dtype=F)
    return sx * c + sy * (-s), sx * s + sy * c


def pooled_indices(xyz, box, S):
    """get_pooled_idx for one box: (indices (S) or None for an empty box, in-box count capped at S)."""
    hits = np.nonzero(in_box_mask(xyz, box))[0][:S]
    cnt = len(hits)
    if cnt == 0:
        return None, 0
    return hits[np.arange(S) % cnt] if cnt < S else hits, cnt


def roipoint_pool3d(xyz, boxes, feats, pooled, empty_flag):
    """xyz (B, N, 3), boxes (B, M, 7) already enlarged, feats (B, N, C); pooled (B, M, S, 3 + C) and empty_flag (B, M) are
    updated IN PLACE: an empty box sets its flag to 1 and leaves its rows; other flags are left as passed."""
    B, M, S = pooled.shape[0], pooled.shape[1], pooled.shape[2]
    for b in range(B):
        for m in range(M):
            idx, cnt = pooled_indices(xyz[b], boxes[b, m], S)
            if idx is None:
                empty_flag[b, m] = 1
                continue
            pooled[b, m, :, 0:3] = xyz[b, idx]
            pooled[b, m, :, 3:] = feats[b, idx]


def voxel_indices(pts, box, out):
    """generate_pts_mask_for_box3d's three indices (N) for every point (meaningful for the in-box ones)."""
    pts, box = np.asarray(pts, dtype=F), np.asarray(box, dtype=F)
    lx, ly = local_xy(pts, box)
    lz = pts[:, 2] - box[2]
    res = []
    with np.errstate(all='ignore'):
        for local, d, n in zip((lx, ly, lz), box[3:6], out):
            r = d / F(n)
            q = np.nan_to_num(np.trunc((local + d / F(2)) / r), nan=0.0, posinf=2.0 ** 31 - 1, neginf=-2.0 ** 31)
            u = np.clip(q, -2.0 ** 31, 2.0 ** 31 - 1).astype(np.int64) & 0xFFFFFFFF      # int(...) stored in an unsigned
            res.append(np.minimum(u, n - 1).astype(np.int64))                            # min(max(u, 0), out - 1) on unsigned
    return res


def roiaware_pool3d_forward(rois, pts, feats, argmax, pts_idx_of_voxels, pooled, pool_method):
    """rois (K, 7), pts (P, 3), feats (P, C); pts_idx_of_voxels (K, ox, oy, oz, max_pts) (zeros on entry, as the
    reference's caller passes it), argmax / pooled (K, ox, oy, oz, C) updated IN PLACE.  pool_method 0 max, 1 avg."""
    K, ox, oy, oz, max_pts = pts_idx_of_voxels.shape
    feats = np.asarray(feats, dtype=F)
    for k in range(K):
        mask = in_box_mask(pts, rois[k])
        xi, yi, zi = voxel_indices(pts, rois[k], (ox, oy, oz))
        for p in np.nonzero(mask)[0]:
            cell = pts_idx_of_voxels[k, xi[p], yi[p], zi[p]]
            if cell[0] < max_pts - 1:
                cell[cell[0] + 1] = p
                cell[0] += 1
        for x in range(ox):
            for y in range(oy):
                for z in range(oz):
                    cell = pts_idx_of_voxels[k, x, y, z]
                    idxs = cell[1:1 + cell[0]]
                    if pool_method == 0:
                        best = np.full(feats.shape[1], -np.inf, dtype=F)
                        arg = np.full(feats.shape[1], -1, dtype=np.int32)
                        for i in idxs:
                            win = feats[i] > best
                            best[win] = feats[i][win]
                            arg[win] = i
                        pooled[k, x, y, z][arg != -1] = best[arg != -1]
                        argmax[k, x, y, z] = arg
                    else:
                        total = np.zeros(feats.shape[1], dtype=F)
                        for i in idxs:
                            total = total + feats[i]
                        if len(idxs) > 0:
                            pooled[k, x, y, z] = total / F(len(idxs))


def roiaware_pool3d_backward(pts_idx_of_voxels, argmax, grad_out, grad_in, pool_method):
    """grad_in (P, C) accumulated IN PLACE (any float dtype: pass float64 for an order-free reference).  Returns the sum
    of the absolute terms per element, the scale an fp32 accumulation's error is measured against."""
    K, ox, oy, oz, max_pts = pts_idx_of_voxels.shape
    C = grad_out.shape[-1]
    abs_sum = np.zeros(grad_in.shape, dtype=np.float64)
    g = np.asarray(grad_out, dtype=F).reshape(K, -1, C)
    lists = pts_idx_of_voxels.reshape(K, -1, max_pts)
    am = None if argmax is None else argmax.reshape(K, -1, C)
    for k in range(K):
        for v in range(g.shape[1]):
            if pool_method == 0:
                for ch in range(C):
                    if am[k, v, ch] != -1:
                        grad_in[am[k, v, ch], ch] += g[k, v, ch]
                        abs_sum[am[k, v, ch], ch] += abs(float(g[k, v, ch]))
            else:
                n = lists[k, v, 0]
                term = g[k, v] * (F(1) / max(F(n), F(1)))
                for i in lists[k, v, 1:1 + n]:
                    grad_in[i] += term
                    abs_sum[i] += np.abs(term.astype(np.float64))
    return abs_sum


# ---- reject sampling: how close a case comes to a decision that a last-ulp difference in cosf could flip -------------
def point_face_clearance(pts, bx):
    """pts (N, 3), one box (7), float64 -> (per point: distance to the nearest face plane of the box, axis by axis;
    the local coordinates lx, ly, lz)."""
    c, s = np.cos(-bx[6]), np.sin(-bx[6])
    sx, sy = pts[:, 0] - bx[0], pts[:, 1] - bx[1]
    lx, ly, lz = sx * c - sy * s, sx * s + sy * c, pts[:, 2] - bx[2]
    near = np.full(pts.shape[0], np.inf)
    for local, d in ((lx, bx[3]), (ly, bx[4]), (lz, bx[5])):
        near = np.minimum(near, np.abs(np.abs(local) - d / 2))
    return near, (lx, ly, lz)


def face_clearance(pts, boxes):
    """smallest distance (float64) of any point to any face plane of any box, axis by axis (conservative: the planes, not
    the faces)."""
    pts, boxes = np.asarray(pts, dtype=np.float64), np.asarray(boxes, dtype=np.float64)
    best = np.inf
    for bx in boxes:
        best = min(best, float(np.min(point_face_clearance(pts, bx)[0])))
    return best


def voxel_clearance(pts, boxes, out):
    """smallest distance (float64) of an in-box point's fractional voxel coordinate to an integer."""
    best = np.inf
    for bx in boxes:
        m = in_box_mask(pts, bx)
        p, b = np.asarray(pts, dtype=np.float64)[m], np.asarray(bx, dtype=np.float64)
        if len(p) == 0:
            continue
        c, s = np.cos(-b[6]), np.sin(-b[6])
        sx, sy = p[:, 0] - b[0], p[:, 1] - b[1]
        for local, d, k in ((sx * c - sy * s, b[3], out[0]), (sx * s + sy * c, b[4], out[1]), (p[:, 2] - b[2], b[5], out[2])):
            q = (local + d / 2) / (d / k)
            best = min(best, float(np.min(np.abs(q - np.round(q)))))
    return best

"""The hard voxel generator's semantics (DESIGN.md "Hard voxels"), restated in numpy for this project's tests and fixture
generator.  `voxelize_loop` is the sequential loop of spconv's CPU generator (Point2VoxelCPU3d, which the reference's
VoxelGeneratorWrapper wraps), written from knowledge of it: spconv is on no machine of this project.  `voxelize_closed_form`
is what the device builds: appearance ranks and the T smallest rows.  `voxelize_batch` is the reference's collate over the
samples of a batch.
"""
import numpy as np

F32 = np.float32


def cells_of(points_xyz, point_cloud_range, voxel_size):
    """(n, 3) float cells (x, y, z) = floor((p - range_min) / voxel) in fp32, an IEEE subtraction then an IEEE division"""
    r, v = np.asarray(point_cloud_range, dtype=F32), np.asarray(voxel_size, dtype=F32)
    return np.floor(((points_xyz.astype(F32) - r[None, :3]).astype(F32) / v[None, :]).astype(F32))


def inside(cells, grid_size):
    """compared as floats: a NaN is outside"""
    g = np.asarray(grid_size, dtype=F32)
    with np.errstate(invalid='ignore'):
        return ((cells >= 0) & (cells < g[None, :])).all(axis=1)


def voxelize_loop(rows, point_cloud_range, voxel_size, grid_size, T, max_voxels):
    """One sample.  rows (n, C) = (x, y, z, ...).  -> (slot_rows (M, T) row numbers or -1, coords (M, 3) = (cz, cy, cx), num (M))"""
    cells = cells_of(rows[:, :3], point_cloud_range, voxel_size)
    ok = inside(cells, grid_size)
    voxel_of, slot_rows, coords, num = {}, [], [], []
    for i in range(len(rows)):
        if not ok[i]:
            continue
        c = tuple(int(x) for x in cells[i])
        v = voxel_of.get(c)
        if v is None:
            if len(coords) >= max_voxels:
                continue                    # the row is skipped; later rows of accepted cells are still taken
            v = voxel_of[c] = len(coords)
            coords.append((c[2], c[1], c[0]))
            slot_rows.append([-1] * T)
            num.append(0)
        if num[v] < T:
            slot_rows[v][num[v]] = i
            num[v] += 1
    return (np.asarray(slot_rows, dtype=np.int32).reshape(-1, T), np.asarray(coords, dtype=np.int32).reshape(-1, 3),
            np.asarray(num, dtype=np.int32))


def voxelize_closed_form(rows, point_cloud_range, voxel_size, grid_size, T, max_voxels):
    """The same result without the loop's state: a cell's appearance rank is the rank of its first row among the first rows of
    all occupied cells; rank < max_voxels makes it voxel `rank`; a voxel keeps the T smallest rows of its cell, ascending."""
    cells = cells_of(rows[:, :3], point_cloud_range, voxel_size)
    kept = np.nonzero(inside(cells, grid_size))[0]
    c = cells[kept].astype(np.int64)
    nx, ny, nz = (int(g) for g in grid_size)
    key = (c[:, 0] * ny + c[:, 1]) * nz + c[:, 2]
    uniq, first, inv = np.unique(key, return_index=True, return_inverse=True)
    order = np.argsort(first, kind='stable')                 # cells in the order their first rows appear
    rank = np.empty(len(uniq), dtype=np.int64)
    rank[order] = np.arange(len(uniq))
    M = min(len(uniq), max_voxels)
    slot_rows = np.full((M, T), -1, dtype=np.int32)
    coords = np.zeros((M, 3), dtype=np.int32)
    num = np.zeros(M, dtype=np.int32)
    for u in order[:M]:
        members = np.sort(kept[inv.reshape(-1) == u])[:T]
        v = rank[u]
        slot_rows[v, :len(members)] = members
        num[v] = len(members)
        cx, rest = divmod(int(uniq[u]), ny * nz)
        coords[v] = (rest % nz, rest // nz, cx)
    return slot_rows, coords, num


def voxelize_batch(points, batch_size, point_cloud_range, voxel_size, grid_size, T, max_voxels, voxelize=voxelize_loop):
    """points (N, 1 + C) rows (batch_idx, x, y, z, ...), the rows of a sample contiguous and samples ascending; rows whose
    batch_idx is outside [0, B) are dropped.  -> dict: slot_rows (M, T) rows of `points`, voxel_coords (M, 4) = (b, cz, cy, cx),
    voxel_num_points (M), voxels (M, T, C) with zero padding"""
    with np.errstate(invalid='ignore'):
        assert (points[:-1, 0] <= points[1:, 0]).all(), 'rows are not grouped by sample'
    slot_rows, coords, num = [], [], []
    for b in range(batch_size):
        idx = np.nonzero((points[:, 0] >= b) & (points[:, 0] < b + 1))[0]
        s, c, n = voxelize(points[idx, 1:], point_cloud_range, voxel_size, grid_size, T, max_voxels)
        slot_rows.append(np.where(s >= 0, idx[np.maximum(s, 0)] if len(idx) else s, -1).astype(np.int32).reshape(-1, T))
        coords.append(np.concatenate([np.full((len(c), 1), b, dtype=np.int32), c], axis=1))
        num.append(n)
    slot_rows, coords, num = np.concatenate(slot_rows), np.concatenate(coords), np.concatenate(num)
    voxels = np.where(slot_rows[:, :, None] >= 0, points[np.maximum(slot_rows, 0)][:, :, 1:], F32(0)).astype(F32)
    return {'slot_rows': slot_rows, 'voxel_coords': coords.astype(np.int32), 'voxel_num_points': num.astype(np.int32), 'voxels': voxels}

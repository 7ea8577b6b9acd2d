"""What the voxel path's tests share (a helper module like detector_case.py: no tests, no fixtures, nothing from pdm_ssd_amd):

  * voxel_assign / rulebook: a numpy restatement of pdm_voxel_assign and of pdm_sparse_sites + pdm_sparse_rulebook, the
    neighbours found through a dictionary keyed by coordinate.  The host tests hold it to the fixture
    (tests/golden/ref_sparse_conv.npz), the GPU tests hold the device to it row for row.
  * conv_reference: F.conv3d in float64 at the active sites, on each site's dense receptive field.
  * the test shapes V1 / R1 / B1 and the seeded parameters of the backbones (the fixture holds no weights: two backbones'
    would be 10 MB; the generator and the tests fill them from the same seeds, and the fixture holds check sums).
"""
import numpy as np
import torch

GEOMETRIES = {              # the four layer geometries of the backbones: (kernel, stride, padding, subm)
    'subm3': ((3, 3, 3), (1, 1, 1), (1, 1, 1), True),
    'k3s2p1': ((3, 3, 3), (2, 2, 2), (1, 1, 1), False),
    'k3s2p011': ((3, 3, 3), (2, 2, 2), (0, 1, 1), False),
    'k311s211p0': ((3, 1, 1), (2, 1, 1), (0, 0, 0), False),
}


# ---- a. points -> voxels ------------------------------------------------------------------------------------------------
def voxel_assign(points, batch_size, point_cloud_range, voxel_size, grid_size):
    """-> dict(kept_idx, unq_inv, voxel_coords (b, cz, cy, cx), voxel_count, mean64 (P, C) float64, keys int64)"""
    p = np.asarray(points, dtype=np.float32)
    r0, v = np.asarray(point_cloud_range[:3], dtype=np.float32), np.asarray(voxel_size, dtype=np.float32)
    g = np.asarray(grid_size, dtype=np.int64)
    with np.errstate(invalid='ignore', over='ignore'):
        cell = np.floor((p[:, 1:4] - r0) / v)                  # fp32 subtraction, fp32 IEEE division
        keep = ((cell >= 0) & (cell < g.astype(np.float32))).all(1) & (p[:, 0] >= 0) & (p[:, 0] < np.float32(batch_size))
    kept = np.nonzero(keep)[0]
    c = cell[kept].astype(np.int64)
    b = p[kept, 0].astype(np.int64)
    keys = ((b * g[0] + c[:, 0]) * g[1] + c[:, 1]) * g[2] + c[:, 2]
    unq, inv, cnt = np.unique(keys, return_inverse=True, return_counts=True)
    inv = inv.reshape(-1)
    mean = np.zeros((len(unq), p.shape[1] - 1))
    np.add.at(mean, inv, p[kept, 1:].astype(np.float64))
    mean /= np.maximum(cnt, 1)[:, None]
    coords = np.stack([unq // (g[0] * g[1] * g[2]), unq % g[2], (unq // g[2]) % g[1], (unq // (g[1] * g[2])) % g[0]], 1)
    return dict(kept_idx=kept.astype(np.int32), unq_inv=inv.astype(np.int32), voxel_coords=coords.astype(np.int32),
                voxel_count=cnt.astype(np.int32), mean64=mean, keys=unq)


# ---- b. rulebook --------------------------------------------------------------------------------------------------------
def out_shape(spatial_shape, kernel, stride, padding, subm):
    if subm:
        return tuple(int(v) for v in spatial_shape)
    return tuple((int(n) + 2 * padding[d] - kernel[d]) // stride[d] + 1 for d, n in enumerate(spatial_shape))


def site_key(idx, shape):
    """((b W + x) H + y) D + z of rows (b, z, y, x) on the grid shape = (D, H, W)"""
    idx = np.asarray(idx, dtype=np.int64).reshape(-1, 4)
    D, H, W = shape
    return ((idx[:, 0] * W + idx[:, 3]) * H + idx[:, 2]) * D + idx[:, 1]


def rulebook(indices, batch_size, spatial_shape, kernel, stride, padding, subm):
    """indices (P, 4) (b, z, y, x) in any row order -> (out_indices (P_out, 4) int32, nbr (P_out, kvol) int32, out_shape)"""
    idx = np.asarray(indices, dtype=np.int64).reshape(-1, 4)
    where = {tuple(c): i for i, c in enumerate(idx.tolist())}
    oshape = out_shape(spatial_shape, kernel, stride, padding, subm)
    offsets = [(kz, ky, kx) for kz in range(kernel[0]) for ky in range(kernel[1]) for kx in range(kernel[2])]
    if subm:
        out = idx
    else:
        sites = set()
        for b, z, y, x in idx.tolist():
            for k in offsets:
                o = []
                for d, v in enumerate((z, y, x)):
                    t = v + padding[d] - k[d]
                    if t < 0 or t % stride[d] or t // stride[d] >= oshape[d]:
                        break
                    o.append(t // stride[d])
                else:
                    sites.add((b, *o))
        out = np.array(sorted(sites), dtype=np.int64).reshape(-1, 4)
        out = out[np.argsort(site_key(out, oshape), kind='stable')]
    nbr = np.full((len(out), len(offsets)), -1, dtype=np.int32)
    for i, (b, z, y, x) in enumerate(out.tolist()):
        for j, k in enumerate(offsets):
            if subm:
                c = (b, z + k[0] - kernel[0] // 2, y + k[1] - kernel[1] // 2, x + k[2] - kernel[2] // 2)
            else:
                c = (b, z * stride[0] - padding[0] + k[0], y * stride[1] - padding[1] + k[1], x * stride[2] - padding[2] + k[2])
            nbr[i, j] = where.get(c, -1)
    return out.astype(np.int32), nbr, oshape


# ---- c. the dense-convolution identity ---------------------------------------------------------------------------------
def conv_reference(x, indices, batch_size, spatial_shape, weight, kernel, stride, padding, subm, out_indices):
    """F.conv3d in float64 at the sites out_indices: x (P, Cin), indices (P, 4), weight (Cout, kz, ky, kx, Cin) -> (P_out, Cout)
    float64.  Each site's dense receptive field (zeros where no input is active) is cut from the dense input and convolved."""
    x = torch.as_tensor(np.asarray(x)).double()
    idx = torch.as_tensor(np.asarray(indices)).long().reshape(-1, 4)
    out_idx = torch.as_tensor(np.asarray(out_indices)).long().reshape(-1, 4)
    w = torch.as_tensor(np.asarray(weight)).double().permute(0, 4, 1, 2, 3).contiguous()       # (Cout, Cin, kz, ky, kx)
    D, H, W = spatial_shape
    pad = [max(kernel[d], padding[d]) for d in range(3)]
    dense = torch.zeros((int(batch_size), D + 2 * pad[0], H + 2 * pad[1], W + 2 * pad[2], x.shape[1]), dtype=torch.float64)
    dense[idx[:, 0], idx[:, 1] + pad[0], idx[:, 2] + pad[1], idx[:, 3] + pad[2]] = x
    first = [out_idx[:, 1 + d] - kernel[d] // 2 if subm else out_idx[:, 1 + d] * stride[d] - padding[d] for d in range(3)]
    rng = [torch.arange(kernel[d]) for d in range(3)]
    Z = (first[0] + pad[0])[:, None, None, None] + rng[0][None, :, None, None]
    Y = (first[1] + pad[1])[:, None, None, None] + rng[1][None, None, :, None]
    X = (first[2] + pad[2])[:, None, None, None] + rng[2][None, None, None, :]
    patches = dense[out_idx[:, 0][:, None, None, None], Z, Y, X]                              # (P_out, kz, ky, kx, Cin)
    if len(out_idx) == 0:
        return np.zeros((0, w.shape[0]))
    y = torch.nn.functional.conv3d(patches.permute(0, 4, 1, 2, 3).contiguous(), w)           # (P_out, Cout, 1, 1, 1)
    return y.reshape(len(out_idx), -1).numpy()


# ---- shapes ---------------------------------------------------------------------------------------------------------------
V1 = dict(range=[0.0, -4.0, -3.0, 10.5, 4.0, 1.0], voxel=[0.5, 0.5, 0.1], grid=[21, 16, 40], B=3)
V2 = dict(range=[0.0, -1.28, -0.8, 3.2, 1.28, 0.8], voxel=[0.16, 0.16, 0.16], grid=[20, 16, 10], B=1)      # voxel 0.16 on all axes
R1_SHAPE, R1_B = (41, 16, 21), 3           # (D, H, W) of grid [21, 16, 41]
B1_GRID, B1_B = [21, 16, 40], 3
D1 = dict(range=[0.0, -4.0, -3.0, 16.0, 4.0, 1.0], voxel=[0.5, 0.5, 0.1], grid=[32, 16, 40], B=2)


def ulp_neighbours(v):
    v = np.asarray(v, dtype=np.float32)
    return np.concatenate([np.nextafter(v, np.float32(-np.inf)), v, np.nextafter(v, np.float32(np.inf))])


def v1_points():
    """(N, 6) rows (b, x, y, z, intensity, fifth): sample 1 owns no point, rows shuffled across samples; one voxel with 1100
    points, single-point voxels, twin rows, points on every face of the range and one ulp to either side on all three axes,
    NaN and +-inf rows"""
    rng = np.random.default_rng(31)
    f32 = np.float32
    rows = [np.stack([rng.choice([0, 2], 600), rng.uniform(-0.5, 11.0, 600), rng.uniform(-4.4, 4.4, 600), rng.uniform(-3.3, 1.3, 600)], 1),
            np.stack([np.full(1100, 2), rng.uniform(7.5, 8.0, 1100), rng.uniform(-1.5, -1.0, 1100), rng.uniform(-0.5, -0.4, 1100)], 1),
            np.stack([rng.choice([0, 2], 200), rng.uniform(0, 10.5, 200), rng.uniform(-4, 4, 200), rng.uniform(-3, 1, 200)], 1),
            np.array([[0, 3.3125, 1.4375, -0.25]] * 2)]
    mid = [5.2, 0.3, -1.05]
    lo, hi = V1['range'][:3], V1['range'][3:]
    for axis in range(3):           # both faces of every axis, and one ulp to either side
        for face in (lo[axis], hi[axis]):
            for v in ulp_neighbours([f32(face)]):
                row = [0.0] + mid
                row[1 + axis] = v
                rows.append(np.array([row]))
    bad = np.array([[0, np.nan, 0.3, 0.0], [2, 1.0, np.nan, 0.0], [0, 1.0, 0.3, np.nan], [0, np.inf, 0.3, 0.0], [2, 1.0, -np.inf, 0.0],
                    [0, 1.0, 0.3, np.inf], [3, 1.0, 0.3, 0.0], [-1, 1.0, 0.3, 0.0]])
    rows.append(bad)
    p = np.concatenate(rows).astype(f32)
    p = np.concatenate([p, rng.uniform(0, 1, (len(p), 2)).astype(f32)], 1)
    return p[rng.permutation(len(p))]


def v2_points():
    """voxel 0.16: points at float32(k * 0.16) and one ulp to either side on x, y and z: what tells a division from a reciprocal
    multiply (the pillar tests' G2)"""
    rng = np.random.default_rng(7)
    xs = ulp_neighbours([np.float32(k * 0.16) for k in range(0, 21)])
    ys = ulp_neighbours([np.float32(k * 0.16) for k in range(-8, 9)])
    zs = ulp_neighbours([np.float32(k * 0.16) for k in range(-5, 6)])
    a = np.stack([np.zeros_like(xs), xs, np.full_like(xs, 0.4), np.full_like(xs, 0.1)], 1)
    b = np.stack([np.zeros_like(ys), np.full_like(ys, 1.0), ys, np.full_like(ys, 0.1)], 1)
    c = np.stack([np.zeros_like(zs), np.full_like(zs, 1.0), np.full_like(zs, 0.4), zs], 1)
    p = np.concatenate([a, b, c]).astype(np.float32)
    p = np.concatenate([p, rng.uniform(0, 1, (len(p), 2)).astype(np.float32)], 1)
    return p[rng.permutation(len(p))]


def r1_indices(P=None):
    """Active sites (b, z, y, x) on R1_SHAPE in shuffled row order, sample 1 empty: a full 3 x 3 x 3 block, isolated voxels, all
    eight corners and a voxel on every face, a voxel at x = W - 1 beside x = 0 of the next grid row and of the next sample
    (which must not be neighbours), the same coordinates in samples 0 and 2, filled up with random sites to about 400.
    P: the first P rows of that list (0, 1, 63, 64, 65), or all of it."""
    D, H, W = R1_SHAPE
    rng = np.random.default_rng(5)
    s = []
    s += [(0, 10 + dz, 5 + dy, 8 + dx) for dz in range(3) for dy in range(3) for dx in range(3)]
    s += [(0, 30, 12, 3), (0, 20, 2, 17), (2, 35, 9, 11)]
    s += [(b, z, y, x) for b in (0, 2) for z in (0, D - 1) for y in (0, H - 1) for x in (0, W - 1)]
    s += [(0, 0, 7, 9), (0, D - 1, 7, 9), (0, 17, 0, 9), (0, 17, H - 1, 9), (0, 17, 7, 0), (0, 17, 7, W - 1)]
    s += [(0, 22, 6, W - 1), (0, 22, 7, 0), (0, 22, H - 1, W - 1), (2, 22, 0, 0), (0, D - 1, H - 1, W - 1), (2, 0, 0, 0)]
    s += [(0, 5, 3, 4), (2, 5, 3, 4), (0, 6, 3, 4), (2, 5, 4, 5)]
    seen, sites = set(), []
    for c in s:
        if c not in seen:
            seen.add(c)
            sites.append(c)
    while len(sites) < 400:         # clusters, so that strided levels keep several inputs per site
        b, z0, y0, x0 = int(rng.choice([0, 2])), int(rng.integers(0, D)), int(rng.integers(0, H)), int(rng.integers(0, W))
        for _ in range(12):
            c = (b, int(np.clip(z0 + rng.integers(-2, 3), 0, D - 1)), int(np.clip(y0 + rng.integers(-2, 3), 0, H - 1)),
                 int(np.clip(x0 + rng.integers(-2, 3), 0, W - 1)))
            if c not in seen:
                seen.add(c)
                sites.append(c)
    idx = np.array(sites, dtype=np.int32)
    idx = idx[rng.permutation(len(idx))]
    return idx if P is None else idx[:P].reshape(-1, 4)


def b1_voxels(C=4):
    """about 400 voxels in clusters on B1_GRID (so that the last level is not empty), some at z = 0 and z = 39, sample 1 empty, in
    ascending key order as the VFE leaves them: (coords (P, 4) int32 (b, z, y, x), features (P, C) fp32)"""
    nx, ny, nz = B1_GRID
    rng = np.random.default_rng(11)
    seen = set()
    for b in (0, 2):
        for x in (2, 9, 15):
            for z in (0, nz - 1):
                seen.add((b, z, 5, x))
    while len(seen) < 400:
        b, z0, y0, x0 = int(rng.choice([0, 2])), int(rng.integers(0, nz)), int(rng.integers(0, ny)), int(rng.integers(0, nx))
        for _ in range(25):
            seen.add((b, int(np.clip(z0 + rng.integers(-3, 4), 0, nz - 1)), int(np.clip(y0 + rng.integers(-2, 3), 0, ny - 1)),
                      int(np.clip(x0 + rng.integers(-2, 3), 0, nx - 1))))
    idx = np.array(sorted(seen), dtype=np.int32)
    idx = idx[np.argsort(site_key(idx, (nz, ny, nx)), kind='stable')]
    feats = rng.uniform(-1, 1, (len(idx), C)).astype(np.float32)
    return idx, feats


def fill_backbone(net, seed, gain=1.0):
    """Seeded parameters of a voxel backbone (the generator and the tests call this with the same seed): convolution weights
    uniform within +-gain sqrt(3 / (9 Cin)) (about a third of the offsets are present around a site; the residual backbone takes a
    smaller gain, or its identity branches grow the activations level after level), BatchNorm with set running
    statistics: gamma in [0.8, 1.2], var in [0.5, 1.5], beta in [0, 0.4], mean in [-0.2, 0.2].  -> check sum (float)."""
    g = torch.Generator().manual_seed(seed)
    total = 0.0
    with torch.no_grad():
        for name, t in sorted(net.state_dict().items()):
            if name.endswith('num_batches_tracked'):
                continue
            if name.endswith('running_var'):
                v = torch.rand(t.shape, generator=g) + 0.5
            elif name.endswith('running_mean'):
                v = torch.rand(t.shape, generator=g) * 0.4 - 0.2
            elif t.dim() == 5:
                v = (torch.rand(t.shape, generator=g) * 2 - 1) * float(gain * np.sqrt(3.0 / (9 * t.shape[-1])))
            elif '.bn' in name or name.split('.')[-2].isdigit():       # BatchNorm weight / bias (conv biases are below)
                v = torch.rand(t.shape, generator=g) * 0.4 + (0.8 if name.endswith('weight') else 0.0)
            else:
                v = torch.rand(t.shape, generator=g) * 0.2 - 0.1
            t.copy_(v.to(t.dtype))
            total += float(v.double().abs().sum())
    return total

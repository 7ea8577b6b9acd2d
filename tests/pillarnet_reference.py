"""What the tests of the wide sparse convolution and of the 2-D pillar path share (a helper module like sparse_conv_reference.py:
no tests, no fixtures, nothing from pdm_ssd_amd's device code):

  * the depth-1 test geometries: sites (b, 0, y, x) of a (1, H, W) grid, the two layer geometries of the 2-D pillar backbones as
    the 3-D operators take them (1 x 3 x 3 submanifold; 1 x 3 x 3 stride (1, 2, 2) padding (0, 1, 1)), their rulebooks by
    sparse_conv_reference.rulebook;
  * conv_case / grad_case: fp32 inputs of one convolution with its float64 references and the absolute-value companions that
    bound the rounding error of any fp32 summation order (sparse_conv_reference.conv_reference, sparse_conv_grad_reference.grads);
  * conv2d_reference: torch.nn.functional.conv2d in float64 on the densified input, read at the output sites.
"""
import numpy as np
import torch

import sparse_conv_grad_reference as sgr
import sparse_conv_reference as scr

GEOMETRIES_2D = {           # (kernel, stride, padding, subm) on a depth-1 grid
    'subm133': ((1, 3, 3), (1, 1, 1), (0, 1, 1), True),
    'k133s122p011': ((1, 3, 3), (1, 2, 2), (0, 1, 1), False),
}
P2_SHAPE, P2_B = (1, 24, 20), 3             # the operator tests' grid: sample 1 owns no site
CHUNK_SHAPE = (1, 48, 40)                   # holds one weight-gradient chunk (1024 rows) and a row


def p2_indices(P=None):
    """About 180 active sites (b, 0, y, x) on P2_SHAPE in shuffled row order, sample 1 empty: a full 3 x 3 block, isolated sites,
    the four corners of samples 0 and 2, a site at x = W - 1 beside x = 0 of the next grid row and of the next sample (no
    neighbours), clusters up to 180.  P: the first P rows of the list, or all of it."""
    _, H, W = P2_SHAPE
    rng = np.random.default_rng(52)
    s = [(0, 0, 5 + dy, 8 + dx) for dy in range(3) for dx in range(3)]
    s += [(0, 0, 20, 3), (2, 0, 2, 17), (2, 0, 13, 11)]
    s += [(b, 0, y, x) for b in (0, 2) for y in (0, H - 1) for x in (0, W - 1)]
    s += [(0, 0, 6, W - 1), (0, 0, 7, 0), (2, 0, 0, 1)]
    seen, sites = set(), []
    for c in s:
        if c not in seen:
            seen.add(c)
            sites.append(c)
    while len(sites) < 180:
        b, y0, x0 = int(rng.choice([0, 2])), int(rng.integers(0, H)), int(rng.integers(0, W))
        for _ in range(10):
            c = (b, 0, int(np.clip(y0 + rng.integers(-2, 3), 0, H - 1)), int(np.clip(x0 + rng.integers(-2, 3), 0, W - 1)))
            if c not in seen:
                seen.add(c)
                sites.append(c)
    idx = np.array(sites, dtype=np.int32)
    idx = idx[rng.permutation(len(idx))]
    return idx if P is None else idx[:P].reshape(-1, 4)


def chunk_indices(P):
    """P seeded random distinct sites (0, 0, y, x) of CHUNK_SHAPE, one sample"""
    _, H, W = CHUNK_SHAPE
    cells = np.random.default_rng(43).choice(H * W, size=P, replace=False)
    return np.stack([np.zeros_like(cells), np.zeros_like(cells), cells // W, cells % W], 1).astype(np.int32)


def book(idx, name, batch_size=P2_B, shape=P2_SHAPE):
    """(out_indices, nbr, out_shape) of the numpy restatement"""
    return scr.rulebook(idx, batch_size, shape, *GEOMETRIES_2D[name])


def conv_case(idx, rulebook, name, cin, cout, seed, batch_size=P2_B, shape=P2_SHAPE):
    """fp32 inputs of one convolution and its float64 references: y = F.conv3d at the output sites, A = the same convolution of
    |x| with |w| (test_sparse_conv_gpu.conv_case on another grid)"""
    rng = np.random.default_rng(seed)
    kernel, stride, padding, subm = GEOMETRIES_2D[name]
    out_idx, nbr, _ = rulebook
    n = kernel[0] * kernel[1] * kernel[2] * cin
    x = rng.uniform(-1, 1, (len(idx), cin)).astype(np.float32)
    w = (rng.uniform(-1, 1, (cout, *kernel, cin)) / np.sqrt(n)).astype(np.float32)
    y = scr.conv_reference(x, idx, batch_size, shape, w, kernel, stride, padding, subm, out_idx)
    A = scr.conv_reference(np.abs(x), idx, batch_size, shape, np.abs(w), kernel, stride, padding, subm, out_idx)
    return dict(x=x, w=w, y=y, A=A, n=n, nbr=np.ascontiguousarray(nbr), cin=cin, cout=cout,
                scale=rng.uniform(0.5, 1.5, cout).astype(np.float32) * rng.choice([-1, 1], cout).astype(np.float32),
                shift=rng.uniform(-0.5, 0.5, cout).astype(np.float32), res=rng.uniform(-1, 1, (len(out_idx), cout)).astype(np.float32))


def grad_case(num_in, nbr, kernel, cin, cout, seed):
    """test_sparse_conv_grad_gpu.grad_case: x, w, dy in fp32 and dx64, A_dx, dW64, A_dW, n_k of sparse_conv_grad_reference.grads"""
    rng = np.random.default_rng(seed)
    n = kernel[0] * kernel[1] * kernel[2] * cin
    c = dict(x=rng.uniform(-1, 1, (num_in, cin)).astype(np.float32), w=(rng.uniform(-1, 1, (cout, *kernel, cin)) / np.sqrt(n)).astype(np.float32),
             dy=rng.uniform(-1, 1, (len(nbr), cout)).astype(np.float32), nbr=np.ascontiguousarray(nbr), kernel=kernel, cin=cin, cout=cout)
    c.update(sgr.grads(c['x'], c['w'], c['dy'], nbr))
    return c


def conv2d_reference(x, idx3, batch_size, shape_hw, weight, stride, padding, out_idx3):
    """x (P, Cin), idx3 (P, 3) (b, y, x), weight (Cout, kh, kw, Cin) -> (y, A) float64 (P_out, Cout): F.conv2d of the densified
    input, and of |x| with |w|, read at out_idx3"""
    H, W = shape_hw
    i = torch.as_tensor(np.asarray(idx3)).long()
    o = torch.as_tensor(np.asarray(out_idx3)).long()
    w = torch.as_tensor(np.asarray(weight)).double().permute(0, 3, 1, 2).contiguous()
    out = []
    for xs, ws in ((torch.as_tensor(np.asarray(x)).double(), w), (torch.as_tensor(np.abs(np.asarray(x))).double(), w.abs())):
        dense = torch.zeros((int(batch_size), xs.shape[1], H, W), dtype=torch.float64)
        dense[i[:, 0], :, i[:, 1], i[:, 2]] = xs
        y = torch.nn.functional.conv2d(dense, ws, stride=stride, padding=padding)
        out.append(y[o[:, 0], :, o[:, 1], o[:, 2]].numpy())
    return out


# ---- the pillar path's fixture shape (tests/golden/gen_pillarnet_fixtures.py) -----------------------------------------------------
# 48 x 32 pillars (ny = 48, nx = 32): the backbone's levels are 48 x 32 -> 24 x 16 -> 12 x 8 -> 6 x 4, conv5 gives 3 x 2.  Every
# level is even down to x_conv4, or BaseBEVBackboneV1 could not concatenate the stride-2 upsampled x_conv5 with x_conv4 (a 6 x 5
# level gives 3 x 3, which comes back as 6 x 6).
PN = dict(range=[0.0, -12.0, -3.0, 16.0, 12.0, 1.0], voxel=[0.5, 0.5, 4.0], grid=[32, 48, 1], B=3)
VFE_CONFIGS = {         # tag -> the encoder's config; 'a' is PILLARNET_CFG's
    'a': {'USE_NORM': True, 'WITH_DISTANCE': False, 'USE_ABSLOTE_XYZ': True, 'NUM_FILTERS': [32]},
    'b': {'USE_NORM': True, 'WITH_DISTANCE': True, 'USE_ABSLOTE_XYZ': False, 'NUM_FILTERS': [32]},
    'c': {'USE_NORM': False, 'WITH_DISTANCE': True, 'USE_ABSLOTE_XYZ': True, 'NUM_FILTERS': [16, 32]},
}


def pn_points():
    """(N, 5) rows (b, x, y, z, intensity), sample 1 empty, rows shuffled: clusters that fill about 300 pillars, a crowded pillar,
    rows outside in x, in y (dropped) and in z only (kept), rows on the faces of the range"""
    rng = np.random.default_rng(77)
    rows = []
    for _ in range(12):
        b, c = int(rng.choice([0, 2])), rng.uniform([1.0, -11.0], [15.0, 11.0])
        n = int(rng.integers(20, 60))
        rows.append(np.concatenate([np.full((n, 1), b), c + rng.normal(0, 0.7, (n, 2)), rng.uniform(-3, 1, (n, 1))], 1))
    rows.append(np.stack([np.full(300, 2), rng.uniform(7.5, 8.0, 300), rng.uniform(-1.5, -1.0, 300), rng.uniform(-3, 1, 300)], 1))
    rows.append(np.array([[0, 16.0, 0.3, 0.0], [0, 0.0, -12.0, 0.0], [2, -1e-7, 1.0, 0.0], [0, 3.0, 12.0, 0.0], [0, 5.2, -1.3, 9.0],
                          [2, np.nextafter(np.float32(16), np.float32(0)), 11.9, 0.25], [0, 17.0, 0.0, 0.0], [2, 4.0, -12.5, 0.0]]))
    p = np.concatenate(rows).astype(np.float32)
    p = np.concatenate([p, rng.uniform(0, 1, (len(p), 1)).astype(np.float32)], 1)
    return p[rng.permutation(len(p))]


def vfe_features(points, geo, use_absolute_xyz, with_distance):
    """numpy restatement of DynamicPillarVFESimple2D up to its first PFN layer -> dict: kept_idx (N') the rows inside the grid in x
    and y in input order, unq_inv (N'), pillar_coords (P, 3) int32 (b, cy, cx) ascending in b nx ny + cx ny + cy, features (N', F)
    fp32 = [x - (float(cx) vx + x_offset), y - (float(cy) vy + y_offset), z - z_offset | points[:, 1:] or [:, 4:] | |xyz|], every
    operation rounded to fp32 as the reference's torch expressions round it"""
    f32 = np.float32
    p = np.asarray(points, dtype=f32)
    r0, v = np.asarray(geo['range'][:3], dtype=f32), np.asarray(geo['voxel'], dtype=f32)
    nx, ny = int(geo['grid'][0]), int(geo['grid'][1])
    cell = np.floor((p[:, 1:3] - r0[:2]) / v[:2])
    keep = (cell[:, 0] >= 0) & (cell[:, 0] < nx) & (cell[:, 1] >= 0) & (cell[:, 1] < ny)
    kept = np.nonzero(keep)[0]
    c = cell[kept].astype(np.int64)
    q = p[kept]
    key = q[:, 0].astype(np.int64) * nx * ny + c[:, 0] * ny + c[:, 1]
    unq, inv = np.unique(key, return_inverse=True)
    coords = np.stack([unq // (nx * ny), unq % ny, (unq % (nx * ny)) // ny], 1).astype(np.int32)
    off = [f32(float(geo['voxel'][d]) / 2 + float(geo['range'][d])) for d in range(3)]
    fc = np.stack([q[:, 1] - (c[:, 0].astype(f32) * v[0] + off[0]), q[:, 2] - (c[:, 1].astype(f32) * v[1] + off[1]), q[:, 3] - off[2]], 1)
    cols = [fc.astype(f32), q[:, 1:] if use_absolute_xyz else q[:, 4:]]
    if with_distance:
        # torch.norm's CPU kernel: sqrt(fma(z, z, fma(y, y, x * x))) in fp32 (a product of two fp32 values is exact in float64)
        x64, y64, z64 = (q[:, d].astype(np.float64) for d in (1, 2, 3))
        s = (q[:, 1] * q[:, 1]).astype(f32)
        s = (y64 * y64 + s.astype(np.float64)).astype(f32)
        s = (z64 * z64 + s.astype(np.float64)).astype(f32)
        cols.append(np.sqrt(s).astype(f32)[:, None])
    return dict(kept_idx=kept.astype(np.int32), unq_inv=inv.reshape(-1).astype(np.int32), pillar_coords=coords,
                features=np.concatenate(cols, 1).astype(f32))


def fill_vfe(net, seed):
    """Seeded parameters of a pillar encoder (the generator and the tests call this with the same seed): linear weights within
    +-0.3, biases within +-0.1, BatchNorm with gamma in [0.8, 1.2], var in [1, 2] (so |gamma / sqrt(var + eps)| <= 1.2), beta in
    [0, 0.4], mean in [-0.2, 0.2].  -> check sum (float)."""
    g = torch.Generator().manual_seed(seed)
    total = 0.0
    with torch.no_grad():
        for name, t in sorted(net.state_dict().items()):
            if name.endswith('num_batches_tracked'):
                continue
            if name.endswith('running_var'):
                v = torch.rand(t.shape, generator=g) + 1.0
            elif name.endswith('running_mean'):
                v = torch.rand(t.shape, generator=g) * 0.4 - 0.2
            elif t.dim() == 2:
                v = torch.rand(t.shape, generator=g) * 0.6 - 0.3
            elif '.norm.' in name:
                v = torch.rand(t.shape, generator=g) * 0.4 + (0.8 if name.endswith('weight') else 0.0)
            else:
                v = torch.rand(t.shape, generator=g) * 0.2 - 0.1
            t.copy_(v.to(t.dtype))
            total += float(v.double().abs().sum())
    return total


def fill_pillarnet(net, seed, gain=1.0):
    """sparse_conv_reference.fill_backbone's sibling for the 2-D modules (sparse 2-D backbones, BaseBEVBackboneV1): every 4-D
    weight, sparse (Cout, kh, kw, Cin) or dense (Cout, Cin, kh, kw), uniform within +-gain sqrt(3 / fan) with fan = numel / shape[0];
    BatchNorm with set running statistics: gamma in [0.8, 1.2], var in [0.5, 1.5], beta in [0, 0.4], mean in [-0.2, 0.2]; convolution
    biases within +-0.1.  -> check sum (float)."""
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
            elif t.dim() == 4:
                v = (torch.rand(t.shape, generator=g) * 2 - 1) * float(gain * np.sqrt(3.0 * t.shape[0] / t.numel()))
            elif '.bn' in name or name.split('.')[-2].isdigit():       # BatchNorm weight / bias (conv biases are below)
                v = torch.rand(t.shape, generator=g) * 0.4 + (0.8 if name.endswith('weight') else 0.0)
            else:
                v = torch.rand(t.shape, generator=g) * 0.2 - 0.1
            t.copy_(v.to(t.dtype))
            total += float(v.double().abs().sum())
    return total


# ---- the torch formulation of a 2-D backbone's training step ----------------------------------------------------------------------
def backbone2d_step(net, features, coords, batch_size, books, proj4, proj5, dtype):
    """sparse_conv_grad_reference.backbone_step for the sparse 2-D backbones: a copy of `net` in `dtype` on the CPU in training mode
    over the device's rulebooks `books` (indice_key -> (out_indices, nbr) as CPU tensors, 'out_shape' = (H, W) of x_conv4): conv1 to
    conv4 by per offset index_select -> mm -> index_add_, BatchNorm1d and ReLU, the dense x_conv4 by torch indexing, conv5 as it is;
    loss = (x_conv4 * proj4).sum() / numel + (x_conv5 * proj5).sum() / numel, backward.  -> dict: 'x_conv4', 'x_conv5', 'loss',
    'grad.<parameter>', 'stat.<running statistic>' as float64 numpy arrays."""
    import copy
    ref = copy.deepcopy(net).cpu().to(dtype).train()
    for p in ref.parameters():
        p.grad = None
    x = (torch.as_tensor(features).to(dtype), torch.as_tensor(coords))
    for name in ('conv1', 'conv2', 'conv3', 'conv4'):
        x = sgr._run(getattr(ref, name), x, books)
    f, idx = x
    H, W = books['out_shape']
    i = idx.long()
    dense = torch.zeros((batch_size, H, W, f.shape[1]), dtype=dtype).index_put((i[:, 0], i[:, -2], i[:, -1]), f).permute(0, 3, 1, 2)
    x5 = ref.conv5(dense)
    loss = (dense * torch.as_tensor(proj4).to(dtype)).sum() / dense.numel() + (x5 * torch.as_tensor(proj5).to(dtype)).sum() / x5.numel()
    loss.backward()
    out = {'x_conv4': dense.detach().double().numpy(), 'x_conv5': x5.detach().double().numpy(), 'loss': loss.detach().double().numpy()}
    for n, p in ref.named_parameters():
        out['grad.' + n] = p.grad.double().numpy()
    for n, b in ref.named_buffers():
        if n.endswith('running_mean') or n.endswith('running_var'):
            out['stat.' + n] = b.double().numpy()
    return out

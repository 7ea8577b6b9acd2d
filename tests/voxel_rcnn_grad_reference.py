"""What the Voxel R-CNN training tests share (a helper module like voxel_rcnn_reference.py: no tests, no fixtures, nothing from
pdm_ssd_amd): the training form of the RoI-grid pooling restated twice.

  * In torch on the CPU, the way the reference computes it: the groups of voxel_rcnn_reference.hit_sets, the padded (M, S)
    tensors materialised (a partly filled group repeats its first hit, an empty one is zeros), nn.BatchNorm1d / BatchNorm2d in
    training mode, the maximum over the slots, autograd (scale_modules, train_forward).  float64 by default; float32 gives
    the `e` of the device tests' bound.
  * In numpy float64 over kept groups (rows with -1 in unused slots), the way the device computes it: the pooled value and the
    winning slot (pool_train), the gradients as plain sums (pool_grad), the nine moments of the padded offsets (moments) and
    the position BatchNorm formed from them (position_norm_from_moments).
"""
import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

import voxel_rcnn_case as case
import voxel_rcnn_reference as vr


def level_groups(rois, G, lv, query_range, radius, nsample, voxel=None, rng0=None):
    """-> (hits: per grid point the rows, offsets: per grid point (len, 3) fp32 centre - p)"""
    rois = np.asarray(rois, np.float32)
    voxel, rng0 = case.VOXEL if voxel is None else voxel, case.RANGE if rng0 is None else rng0
    pts = vr.grid_points(rois, G)
    sample = np.repeat(np.arange(rois.shape[0]), rois.shape[1] * G ** 3)
    cell = vr.cells(pts, rng0, voxel, lv['stride'])
    hits, offs, _ = vr.hit_sets(pts, sample, cell, lv['indices'], lv['shape'], lv['stride'], voxel, rng0, query_range, radius, nsample)
    return hits, offs


def kept(hits, offs, S):
    """-> (rows (M, S) int32 with -1 in unused slots, offsets (M, S, 3) fp32 with 0 there, counts (M)): what the query keeps"""
    M = len(hits)
    rows, d = np.full((M, S), -1, np.int32), np.zeros((M, S, 3), np.float32)
    for m, (h, o) in enumerate(zip(hits, offs)):
        rows[m, :len(h)], d[m, :len(h)] = h, o
    return rows, d, (rows >= 0).sum(1)


def padded(rows, d):
    """kept groups -> the reference's padded tensors: idx (M, S) int64 (the first hit in unused slots, 0 for an empty group), offsets
    (M, S, 3) float64 (the first hit's, zeros for an empty group)"""
    unused = rows < 0
    idx = np.where(unused, np.maximum(rows[:, :1], 0), rows).astype(np.int64)
    dd = np.where(unused[..., None], d[:, :1], d).astype(np.float64)
    dd[rows[:, 0] < 0] = 0
    return idx, dd


def moments(dd):
    """padded offsets (M, S, 3) float64 -> the nine sums [x, y, z, xx, xy, xz, yy, yz, zz]"""
    x = np.asarray(dd, np.float64).reshape(-1, 3)
    return np.array([x[:, 0].sum(), x[:, 1].sum(), x[:, 2].sum(), (x[:, 0] * x[:, 0]).sum(), (x[:, 0] * x[:, 1]).sum(), (x[:, 0] * x[:, 2]).sum(),
                     (x[:, 1] * x[:, 1]).sum(), (x[:, 1] * x[:, 2]).sum(), (x[:, 2] * x[:, 2]).sum()])


def position_norm_from_moments(weight, gamma, beta, eps, mom, num_slots):
    """The moment identity in torch float64: Conv2d(3 -> C1, no bias) + training BatchNorm2d over N = num_slots offsets is
    dot(W[c], d) scale[c] + shift[c] with mean_c = W[c] . m, var_c = W[c]^T Cov W[c] (biased), m and Cov from the nine sums.
    weight (C1, 3), gamma, beta (C1) may require grad -> (scale, shift, mean, unbiased variance)"""
    m = torch.as_tensor(np.asarray(mom), dtype=torch.float64) / num_slots
    second = torch.stack([m[3], m[4], m[5], m[4], m[6], m[7], m[5], m[7], m[8]]).view(3, 3)
    cov = second - m[:3].view(3, 1) * m[:3].view(1, 3)
    mean = weight @ m[:3]
    var = ((weight @ cov) * weight).sum(1)
    scale = gamma * torch.rsqrt(var + eps)
    return scale, beta - mean * scale, mean, var * (num_slots / (num_slots - 1.0))


def scale_modules(state, prefix, k, dtype=torch.float64):
    """scale k of a NeighborVoxelSAModuleMSG rebuilt from state_dict arrays, in training mode -> {'mlps_in', 'mlps_pos', 'mlps_out'}"""
    get = lambda key: torch.as_tensor(np.asarray(state[prefix + key]))      # noqa: E731
    c1, cin = get(f'mlps_in.{k}.0.weight').shape[:2]
    c2 = get(f'mlps_out.{k}.0.weight').shape[0]
    mods = {'mlps_in': nn.Sequential(nn.Conv1d(cin, c1, 1, bias=False), nn.BatchNorm1d(c1)),
            'mlps_pos': nn.Sequential(nn.Conv2d(3, c1, 1, bias=False), nn.BatchNorm2d(c1)),
            'mlps_out': nn.Sequential(nn.Conv1d(c1, c2, 1, bias=False), nn.BatchNorm1d(c2), nn.ReLU())}
    for name, m in mods.items():
        m.load_state_dict({key: get(f'{name}.{k}.{key}').clone() for key in m.state_dict()})
        m.to(dtype).train()
    return mods


def train_forward(mods, features, rows, d):
    """the reference's formulation over materialised padded tensors: features (P, C) torch (may require grad), kept groups ->
    (out (M, C2), pooled (M, C1), x (C1, M, S): the slots' values behind the ReLU)"""
    dtype = features.dtype
    idx, dd = padded(rows, d)
    f_in = mods['mlps_in'](features.t().unsqueeze(0)).squeeze(0).t()
    empty = torch.from_numpy(rows[:, 0] < 0).view(-1, 1, 1)
    grouped = f_in[torch.from_numpy(idx)].masked_fill(empty, 0).permute(2, 0, 1).unsqueeze(0)       # (1, C1, M, S)
    pos = mods['mlps_pos'](torch.from_numpy(dd).to(dtype).permute(2, 0, 1).unsqueeze(0))
    x = torch.relu(grouped + pos)
    pooled = F.max_pool2d(x, kernel_size=[1, x.size(3)]).squeeze(-1)
    out = mods['mlps_out'](pooled).squeeze(0).t()
    return out, pooled.squeeze(0).t(), x.squeeze(0)


def named_parameters(mods):
    return {f'{name}.{key}': p for name, m in mods.items() for key, p in m.named_parameters()}


def running_stats(mods):
    return {f'{name}.1.{key}': getattr(m[1], key).detach().clone() for name, m in mods.items() for key in ('running_mean', 'running_var', 'num_batches_tracked')}


def winner_margins(x, scale):
    """x (C1, M, S) the slots' values of the padded tensor; rows' distinct slots are those that differ, so the margin is taken over
    distinct VALUES: -> (the smallest gap between the best and the next distinct value of an (m, c) with a positive maximum,
    the smallest positive maximum), both relative to `scale`"""
    v = np.sort(np.asarray(x.detach() if torch.is_tensor(x) else x, np.float64), axis=-1)[..., ::-1]
    best = v[..., 0]
    gap = np.where(v[..., 1:] < best[..., None], best[..., None] - v[..., 1:], np.inf).min(-1)
    pos = best > 0
    return (float(gap[pos].min()) / scale if pos.any() else np.inf), (float(best[pos].min()) / scale if pos.any() else np.inf)


# ---- the device's formulation over kept groups, numpy float64 ------------------------------------------------------------------
def pool_train(f_in, rows, d, wp, sp, hp):
    """-> (pooled (M, C1), arg (M, C1) uint8, A (M, C1): the winning expression on absolute values, gap: the smallest distance of a
    positive maximum to the next slot's value or to zero)"""
    f, wp, sp, hp, d = (np.asarray(t, np.float64) for t in (f_in, wp, sp, hp, d))
    used = rows >= 0
    safe = np.maximum(rows, 0)
    t = f[safe] + (d @ wp.T) * sp + hp                                      # (M, S, C1)
    a = np.abs(f[safe]) + (np.abs(d) @ np.abs(wp).T) * np.abs(sp) + np.abs(hp)
    empty = ~used[:, 0]
    t[empty, 0], a[empty, 0] = hp, np.abs(hp)
    used = used.copy()
    used[empty, 0] = True
    t = np.where(used[..., None], t, -np.inf)
    best, arg = t.max(1), t.argmax(1)
    pooled = np.maximum(best, 0)
    A = np.where(used[..., None], a, 0).max(1)
    order = np.sort(t, axis=1)[:, ::-1]
    second = order[:, 1] if t.shape[1] > 1 else np.full_like(best, -np.inf)
    pos = best > 0
    gap = float(np.minimum(best - np.maximum(second, 0), best)[pos].min()) if pos.any() else np.inf
    return pooled, np.where(pos, arg, 255).astype(np.uint8), A, gap


def pool_grad(g, arg, rows, d, wp, sp, num_rows):
    """-> dict: dfeat (P, C1), dwp (C1, 3), dscale, dshift (C1) as float64 sums, with the sums of the addends' absolute values
    (abs_dwp, abs_dscale, abs_dshift) and cnt (P, C1), the addends of every features' element"""
    g, wp, sp, d = (np.asarray(t, np.float64) for t in (g, wp, sp, d))
    M, C1 = g.shape
    m_i, c_i = np.nonzero(arg != 255)
    s = arg[m_i, c_i].astype(np.int64)
    gv = g[m_i, c_i]
    row = rows[m_i, s]
    ne = row >= 0
    out = {k: np.zeros((num_rows, C1)) for k in ('dfeat', 'cnt')}
    np.add.at(out['dfeat'], (row[ne], c_i[ne]), gv[ne])
    np.add.at(out['cnt'], (row[ne], c_i[ne]), 1)
    off = d[m_i, s]                                                         # (K, 3)
    dot = (off * wp[c_i]).sum(1)
    for name, add in (('dshift', gv), ('dscale', np.where(ne, gv * dot, 0)), ('dwp', np.where(ne[:, None], (gv * sp[c_i])[:, None] * off, 0))):
        total, absum = np.zeros((C1,) + add.shape[1:]), np.zeros((C1,) + add.shape[1:])
        np.add.at(total, c_i, add)
        np.add.at(absum, c_i, np.abs(add))
        out[name], out['abs_' + name] = total, absum
    return out

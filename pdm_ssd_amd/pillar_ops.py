"""The pillar front end's device operators (csrc/pillar.hip): points -> dynamic pillars (assign), the per-point pillar
features, the per-pillar max with its gradient, the fused single-layer PFN of eval mode and the BEV canvas scatter with
its gradient.  count -> scan -> fill on the device: no host loop, no sort, no float atomics, so every result is a
function of the input alone and two runs give the same bits.

ONE host read per batch: assign() copies the two ints {N', P} (kept rows, pillars) to the host to slice its
capacity-sized outputs.  Nothing else in this module, in vfe/ or in backbones_2d/map_to_bev reads the device, in eval
and in training alike; HOST_READS counts the copies so that a test can assert it.

The torch formulations these replace (boolean-mask indexing, torch.unique, index_add_, scatter_reduce('amax') and the
per-sample scatter loop) are what the tests and tools/pillar_rate.py compare with.
"""
import ctypes
from collections import namedtuple

import numpy as np
import torch
from torch.autograd import Function

from . import _native

MAX_FUSED_FEATURES = 16     # input columns of the fused PFN layer (PL_MAXF)
HOST_READS = 0              # device-to-host copies this module has made (one per assign())

Pillars = namedtuple('Pillars', ['kept_idx', 'unq_inv', 'voxel_coords', 'pillar_count', 'pillar_mean', 'cell_table',
                                 'seg_start', 'seg_rows', 'num_kept', 'num_pillars', 'batch_size', 'grid_size'])
PillarGeometry = namedtuple('PillarGeometry', ['vx', 'vy', 'x_offset', 'y_offset', 'z_offset'])


def geometry(point_cloud_range, voxel_size):
    """The reference's cell-centre offsets: voxel / 2 + range start in double on the host, rounded to fp32 where used."""
    vx, vy, vz = (float(v) for v in voxel_size[:3])
    return PillarGeometry(vx, vy, vx / 2 + float(point_cloud_range[0]), vy / 2 + float(point_cloud_range[1]),
                          vz / 2 + float(point_cloud_range[2]))


def _check_points(points):
    assert points.is_cuda and points.dtype == torch.float32 and points.dim() == 2 and points.shape[1] >= 4, \
        'points: fp32 (N, 1 + C) rows (batch_idx, x, y, z, ...) on the GPU'
    return points if points.is_contiguous() else points.contiguous()


@torch.no_grad()
def assign(points, batch_size, point_cloud_range, voxel_size, grid_size):
    """points (N, 1 + C) fp32 rows (batch_idx, x, y, z, ...) in any row order -> Pillars (pdm_pillar_assign):
      kept_idx (N') int32     the rows inside the grid in x and y (z is not tested), in input order: the reference's points[mask]
      unq_inv (N') int32      the pillar of each kept row
      voxel_coords (P, 4)     int32 (b, 0, cy, cx); pillars ascend in b nx ny + cx ny + cy (torch.unique's order, x-major)
      pillar_count (P) int32, pillar_mean (P, 3) = float(double(sum of llrint(x 2^20)) 2^-20 / count)
      cell_table (B nx ny)    int32 pillar id or -1, in key order
      seg_start (P + 1), seg_rows (N')   the kept rows of every pillar (slot order unspecified)
    cell = floor((x - x0) / vx) in fp32 with an IEEE division.  The outputs are allocated at capacity and sliced after
    ONE device-to-host copy of {N', P}: the only host read of the pillar path per batch, in eval and in training."""
    global HOST_READS
    points = _check_points(points)
    nx, ny, nz = (int(v) for v in grid_size)
    N, C1, B, dev = points.shape[0], points.shape[1], int(batch_size), points.device
    ncell = B * nx * ny
    if ncell > 0x7fffffff:      # the call below rejects it; nothing is allocated for it
        ncell = N = 0
    cap = min(N, ncell)
    i32 = dict(dtype=torch.int32, device=dev)
    kept_idx, unq_inv, seg_rows = (torch.empty(N, **i32) for _ in range(3))
    voxel_coords = torch.empty((cap, 4), **i32)
    pillar_count = torch.empty(cap, **i32)
    pillar_mean = torch.empty((cap, 3), dtype=torch.float32, device=dev)
    cell_table = torch.empty(ncell, **i32)
    seg_start = torch.empty(cap + 1, **i32)
    record = torch.empty(2, **i32)
    nbytes = _native.lib().pdm_pillar_assign_workspace_bytes(N, B, nx, ny)
    ws = torch.empty(max(nbytes, 8), dtype=torch.uint8, device=dev)
    _native.call("pdm_pillar_assign", _native.stream(dev), points.shape[0], C1, points.data_ptr(), B, nx, ny, nz, float(point_cloud_range[0]),
                 float(point_cloud_range[1]), float(voxel_size[0]), float(voxel_size[1]), kept_idx.data_ptr(), unq_inv.data_ptr(),
                 voxel_coords.data_ptr(), pillar_count.data_ptr(), pillar_mean.data_ptr(), cell_table.data_ptr(), seg_start.data_ptr(),
                 seg_rows.data_ptr(), record.data_ptr(), ws.data_ptr(), nbytes)
    HOST_READS += 1
    n_kept, P = (int(v) for v in record.cpu().tolist())
    return Pillars(kept_idx[:n_kept], unq_inv[:n_kept], voxel_coords[:P], pillar_count[:P], pillar_mean[:P], cell_table,
                   seg_start[:P + 1], seg_rows[:n_kept], n_kept, P, B, (nx, ny, nz))


def num_features(num_point_features, use_absolute_xyz=True, with_distance=False):
    """columns of features() for rows of 1 + num_point_features floats"""
    return (num_point_features if use_absolute_xyz else num_point_features - 3) + 6 + (1 if with_distance else 0)


def _feature_args(geom, use_absolute_xyz, with_distance):
    return (1 if use_absolute_xyz else 0, 1 if with_distance else 0, geom.vx, geom.vy,
            float(np.float32(geom.x_offset)), float(np.float32(geom.y_offset)), float(np.float32(geom.z_offset)))


@torch.no_grad()
def features(points, pillars, geom, use_absolute_xyz=True, with_distance=False):
    """-> (N', F) rows in the reference's column order: points[:, 1:] (or [:, 4:]), f_cluster = xyz - pillar mean,
    f_center = xyz - (float(cell) * voxel + offset) with the product and the sum rounded separately, and the norm of xyz
    when with_distance (pdm_pillar_features).  No gradient: points are data.  No host read."""
    points = _check_points(points)
    F = num_features(points.shape[1] - 1, use_absolute_xyz, with_distance)
    out = torch.empty((pillars.num_kept, F), dtype=torch.float32, device=points.device)
    _native.call("pdm_pillar_features", _native.stream(points), pillars.num_kept, points.shape[1], points.data_ptr(),
                 pillars.kept_idx.data_ptr(), pillars.unq_inv.data_ptr(), pillars.voxel_coords.data_ptr(), pillars.pillar_mean.data_ptr(),
                 *_feature_args(geom, use_absolute_xyz, with_distance), out.data_ptr())
    return out


class _SegmentMax(Function):
    @staticmethod
    def forward(ctx, x, unq_inv, seg_start, seg_rows):
        assert x.is_cuda and x.dtype == torch.float32 and x.dim() == 2 and x.shape[0] == unq_inv.shape[0] == seg_rows.shape[0]
        x = x.contiguous()
        P, K = seg_start.shape[0] - 1, x.shape[1]
        x_max = torch.empty((P, K), dtype=torch.float32, device=x.device)
        arg = torch.empty((P, K), dtype=torch.int32, device=x.device)
        _native.call("pdm_pillar_segment_max", _native.stream(x), P, K, x.data_ptr(), seg_start.data_ptr(), seg_rows.data_ptr(),
                     x_max.data_ptr(), arg.data_ptr())
        ctx.save_for_backward(arg, unq_inv)
        ctx.mark_non_differentiable(arg)
        return x_max, arg

    @staticmethod
    def backward(ctx, g, _g_arg):
        arg, unq_inv = ctx.saved_tensors
        g = g.contiguous().float()
        n, K = unq_inv.shape[0], g.shape[1]
        gx = torch.empty((n, K), dtype=torch.float32, device=g.device)
        _native.call("pdm_pillar_segment_max_grad", _native.stream(g), n, K, g.data_ptr(), arg.data_ptr(), unq_inv.data_ptr(), gx.data_ptr())
        return gx, None, None, None


def segment_max(x, pillars):
    """x (N', K) fp32 -> (x_max (P, K), arg (P, K) int32): the maximum over each pillar's rows and the row that holds it,
    ties to the lower row (pdm_pillar_segment_max).  The gradient goes to the winning row alone, written without atomics
    (a row belongs to one pillar).  No host read."""
    return _SegmentMax.apply(x, pillars.unq_inv, pillars.seg_start, pillars.seg_rows)


@torch.no_grad()
def fused_pfn(points, pillars, geom, weight, scale, shift, use_absolute_xyz=True, with_distance=False):
    """One PFN layer in eval mode in one launch: features -> weight (K, F) -> * scale (K) + shift (K) (the folded
    BatchNorm, or 1 and the bias) -> ReLU -> max per pillar: (P, K).  The (N', K) activations never reach memory
    (pdm_pillar_fused_pfn).  No host read."""
    points = _check_points(points)
    F = num_features(points.shape[1] - 1, use_absolute_xyz, with_distance)
    K = weight.shape[0]
    assert weight.shape == (K, F) and scale.shape == (K,) and shift.shape == (K,), (tuple(weight.shape), F)
    if F > MAX_FUSED_FEATURES:
        raise ValueError(f'fused_pfn: at most {MAX_FUSED_FEATURES} feature columns (got {F})')
    weight, scale, shift = (t.detach().float().contiguous() for t in (weight, scale, shift))
    out = torch.empty((pillars.num_pillars, K), dtype=torch.float32, device=points.device)
    _native.call("pdm_pillar_fused_pfn", _native.stream(points), pillars.num_pillars, K, points.shape[1], points.data_ptr(),
                 pillars.kept_idx.data_ptr(), pillars.voxel_coords.data_ptr(), pillars.pillar_mean.data_ptr(), pillars.seg_start.data_ptr(),
                 pillars.seg_rows.data_ptr(), *_feature_args(geom, use_absolute_xyz, with_distance), weight.data_ptr(), scale.data_ptr(),
                 shift.data_ptr(), out.data_ptr())
    return out


@torch.no_grad()
def cell_table_from_coords(voxel_coords, batch_size, grid_size):
    """voxel_coords (P, 4) (b, 0, cy, cx), any integer dtype -> cell_table (B nx ny) int32, pillar id or -1, for a caller
    whose VFE left none (pdm_pillar_cell_table).  No host read."""
    nx, ny, nz = (int(v) for v in grid_size)
    vc = voxel_coords.to(torch.int32).contiguous()
    table = torch.empty(int(batch_size) * nx * ny, dtype=torch.int32, device=vc.device)
    _native.call("pdm_pillar_cell_table", _native.stream(vc), vc.shape[0], vc.data_ptr(), int(batch_size), nx, ny, nz, table.data_ptr())
    return table


class _Scatter(Function):
    @staticmethod
    def forward(ctx, feats, cell_table, voxel_coords, B, nx, ny):
        assert feats.is_cuda and feats.dtype == torch.float32 and feats.dim() == 2 and feats.shape[0] == voxel_coords.shape[0]
        assert cell_table.dtype == torch.int32 and cell_table.numel() == B * nx * ny and voxel_coords.dtype == torch.int32
        feats, voxel_coords = feats.contiguous(), voxel_coords.contiguous()
        P, C = feats.shape
        out = torch.empty((B, C, ny, nx), dtype=torch.float32, device=feats.device)
        _native.call("pdm_pillar_scatter", _native.stream(feats), P, C, feats.data_ptr(), cell_table.data_ptr(), B, nx, ny, 1, out.data_ptr())
        ctx.save_for_backward(voxel_coords)
        ctx.dims = (B, nx, ny)
        return out

    @staticmethod
    def backward(ctx, g):
        voxel_coords, = ctx.saved_tensors
        B, nx, ny = ctx.dims
        g = g.contiguous().float()
        P, C = voxel_coords.shape[0], g.shape[1]
        gf = torch.empty((P, C), dtype=torch.float32, device=g.device)
        _native.call("pdm_pillar_scatter_grad", _native.stream(g), P, C, g.data_ptr(), voxel_coords.data_ptr(), B, nx, ny, 1, gf.data_ptr())
        return gf, None, None, None, None, None


def scatter(pillar_features, cell_table, voxel_coords, batch_size, grid_size):
    """pillar_features (P, C) fp32, cell_table (B nx ny) int32, voxel_coords (P, 4) int32 -> the BEV canvas
    (B, C, ny, nx): one pass writes every element, zeros included (pdm_pillar_scatter).  The gradient is a gather of the
    canvas gradient at the pillar cells (pdm_pillar_scatter_grad).  No host read."""
    nx, ny, nz = (int(v) for v in grid_size)
    assert nz == 1
    return _Scatter.apply(pillar_features, cell_table, voxel_coords, int(batch_size), nx, ny)

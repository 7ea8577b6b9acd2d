"""Hard voxelization and its two encoders on the device (csrc/hard_voxel.hip, DESIGN.md "Hard voxels"): the reference's
`transform_points_to_voxels` step (spconv's CPU voxel generator, a sequential loop over one frame) as its closed form, for
the whole batch, with no host loop, no sort and no float atomic.  Every result is a function of the input alone: two runs
give the same bits.

  voxelize      points -> HardVoxels: at most T points a voxel, at most max_voxels voxels a sample, voxels numbered in the
                order their first point appears, samples ascending (the reference's collate)
  materialize   the reference's padded (M, T, C) `voxels` tensor, for the paths that run its formulation under autograd
  voxel_mean    MeanVFE without the padded tensor
  fused_pfn     PillarVFE with one PFN layer in eval mode in one launch, without the (M, T, F) and (M, T, K) tensors

ONE host read per voxelize(): the two ints {M, unsorted}, to slice the capacity-sized outputs and to refuse rows that are
not grouped by sample.  HOST_READS counts the copies so that a test can assert it.  Nothing here has a gradient: points
are data.
"""
from collections import namedtuple

import numpy as np
import torch

from . import _native
from .pillar_ops import MAX_FUSED_FEATURES, num_features

HOST_READS = 0              # device-to-host copies this module has made (one per voxelize())

HardVoxels = namedtuple('HardVoxels', ['voxels', 'voxel_coords', 'voxel_num_points', 'slot_rows', 'num_voxels', 'batch_size',
                                       'grid_size'])
VoxelGeometry = namedtuple('VoxelGeometry', ['vx', 'vy', 'vz', 'x_offset', 'y_offset', 'z_offset'])


def max_points_per_voxel():
    """the largest T the kernels take (pdm_hard_voxel_max_points)"""
    return int(_native.lib().pdm_hard_voxel_max_points())


def geometry(point_cloud_range, voxel_size):
    """The reference's cell-centre offsets: voxel / 2 + range start in double on the host, rounded to fp32 where used."""
    vx, vy, vz = (float(v) for v in voxel_size[:3])
    return VoxelGeometry(vx, vy, vz, vx / 2 + float(point_cloud_range[0]), vy / 2 + float(point_cloud_range[1]),
                         vz / 2 + float(point_cloud_range[2]))


def _check_points(points):
    assert points.is_cuda and points.dtype == torch.float32 and points.dim() == 2 and points.shape[1] >= 4, \
        'points: fp32 (N, 1 + C) rows (batch_idx, x, y, z, ...) on the GPU'
    return points if points.is_contiguous() else points.contiguous()


@torch.no_grad()
def voxelize(points, batch_size, point_cloud_range, voxel_size, grid_size, max_points_per_voxel, max_voxels, materialize=False):
    """points (N, 1 + C) fp32 rows (batch_idx, x, y, z, ...), the rows of a sample contiguous and samples ascending ->
    HardVoxels (pdm_hard_voxelize):
      voxel_coords (M, 4) int32    (b, cz, cy, cx); per sample in the order the voxels' first points appear
      voxel_num_points (M) int32   min(points of the cell, T)
      slot_rows (M, T) int32       the input row of every slot, ascending, -1 for padding
      voxels (M, T, C) or None     with materialize: bit copies of the rows past batch_idx, zero padding
    cell = floor((v - v0) / size) in fp32 with an IEEE division on x, y and z (z is tested on a pillar grid too).  A cell
    past the sample's first max_voxels is refused and its rows dropped; later rows of accepted cells are still taken.
    Raises ValueError when batch_idx is not non-decreasing over the rows."""
    global HOST_READS
    points = _check_points(points)
    nx, ny, nz = (int(v) for v in grid_size)
    N, C1, B, dev = points.shape[0], points.shape[1], int(batch_size), points.device
    T, cap_per_sample = int(max_points_per_voxel), int(max_voxels)
    nbytes = _native.lib().pdm_hard_voxelize_workspace_bytes(N, B, nx, ny, nz)
    cap = min(N, B * max(cap_per_sample, 0), B * nx * ny * nz) if nbytes and 1 <= T <= 1024 else 0    # a bad call is rejected below
    i32 = dict(dtype=torch.int32, device=dev)
    slot_rows = torch.empty((cap, T if cap else 0), **i32)
    voxel_coords = torch.empty((cap, 4), **i32)
    num = torch.empty(cap, **i32)
    voxels = torch.empty((cap, T, C1 - 1), dtype=torch.float32, device=dev) if materialize and cap else None
    record = torch.empty(2, **i32)
    ws = torch.empty(max(nbytes, 8), dtype=torch.uint8, device=dev)
    r, v = point_cloud_range, voxel_size
    _native.call("pdm_hard_voxelize", _native.stream(dev), N, C1, points.data_ptr(), B, nx, ny, nz, float(r[0]), float(r[1]), float(r[2]),
                 float(v[0]), float(v[1]), float(v[2]), T, cap_per_sample, slot_rows.data_ptr(), voxel_coords.data_ptr(), num.data_ptr(),
                 None if voxels is None else voxels.data_ptr(), record.data_ptr(), ws.data_ptr(), nbytes)
    HOST_READS += 1
    M, unsorted = (int(x) for x in record.cpu().tolist())
    if unsorted:
        raise ValueError('voxelize: the rows of a sample must be contiguous with samples ascending (batch_idx decreases, or is NaN, '
                         'somewhere along the rows)')
    if materialize:
        voxels = voxels[:M] if voxels is not None else torch.zeros((0, T, C1 - 1), dtype=torch.float32, device=dev)
    return HardVoxels(voxels, voxel_coords[:M], num[:M], slot_rows[:M].reshape(M, T), M, B, (nx, ny, nz))


@torch.no_grad()
def materialize(points, hv):
    """-> voxels (M, T, C) fp32: the slots' rows past batch_idx, zeros in the padding, every element written
    (pdm_hard_voxel_materialize).  No host read."""
    points = _check_points(points)
    M, T = hv.slot_rows.shape
    out = torch.empty((M, T, points.shape[1] - 1), dtype=torch.float32, device=points.device)
    _native.call("pdm_hard_voxel_materialize", _native.stream(points), M, T, points.shape[1], points.data_ptr(), hv.slot_rows.data_ptr(),
                 out.data_ptr())
    return out


@torch.no_grad()
def voxel_mean(points, hv):
    """-> (M, C): the fp32 sum of every voxel's slots in slot order, then one IEEE division by max(num, 1): MeanVFE
    (pdm_hard_voxel_mean).  No host read."""
    points = _check_points(points)
    M, T = hv.slot_rows.shape
    out = torch.empty((M, points.shape[1] - 1), dtype=torch.float32, device=points.device)
    _native.call("pdm_hard_voxel_mean", _native.stream(points), M, T, points.shape[1], points.data_ptr(), hv.slot_rows.data_ptr(),
                 hv.voxel_num_points.data_ptr(), out.data_ptr())
    return out


@torch.no_grad()
def fused_pfn(points, hv, geom, weight, scale, shift, use_absolute_xyz=True, with_distance=False):
    """The reference's PillarVFE with ONE PFN layer in eval mode in one launch (pdm_hard_pillar_pfn): columns in the
    reference's order -> weight (K, F) -> * scale (K) + shift (K) (the folded BatchNorm, or 1 and the bias) -> ReLU -> max
    over the voxel's slots, a voxel with fewer than T points also taking relu(shift), what its zero-masked padding rows
    give: (M, K).  Neither (M, T, F) nor (M, T, K) reaches memory.  No host read."""
    points = _check_points(points)
    F = num_features(points.shape[1] - 1, use_absolute_xyz, with_distance)
    K = weight.shape[0]
    assert weight.shape == (K, F) and scale.shape == (K,) and shift.shape == (K,), (tuple(weight.shape), F)
    if F > MAX_FUSED_FEATURES:
        raise ValueError(f'fused_pfn: at most {MAX_FUSED_FEATURES} feature columns (got {F})')
    weight, scale, shift = (t.detach().float().contiguous() for t in (weight, scale, shift))
    M, T = hv.slot_rows.shape
    out = torch.empty((M, K), dtype=torch.float32, device=points.device)
    _native.call("pdm_hard_pillar_pfn", _native.stream(points), M, K, T, points.shape[1], points.data_ptr(), hv.slot_rows.data_ptr(),
                 hv.voxel_num_points.data_ptr(), hv.voxel_coords.data_ptr(), 1 if use_absolute_xyz else 0, 1 if with_distance else 0,
                 geom.vx, geom.vy, geom.vz, float(np.float32(geom.x_offset)), float(np.float32(geom.y_offset)),
                 float(np.float32(geom.z_offset)), weight.data_ptr(), scale.data_ptr(), shift.data_ptr(), out.data_ptr())
    return out

"""PV-RCNN's two operators (csrc/pv_rcnn.hip): the batch form of the BEV interpolation at the keypoints and the
query half of the RoI-grid pooling over the keypoints.  Both are one launch, read nothing on the host and can be captured in a
graph; there is no torch fallback here: the callers keep the composed formulations as checkers.
"""
import torch

from . import _native


def sample_counts(batch_idx, batch_size):
    """rows per sample, int32 (B,), from the batch column: an integer scatter-add on the device (torch.bincount reads the
    largest index on the host)"""
    counts = torch.zeros((batch_size,), dtype=torch.int32, device=batch_idx.device)
    return counts.scatter_add_(0, batch_idx.long(), torch.ones_like(batch_idx, dtype=torch.int32))


def bev_interpolate(keypoints, spatial_features, point_cloud_range, voxel_size, bev_stride, out=None, col0=0):
    """keypoints (K, 4) fp32 rows (b, x, y, z) of all samples; spatial_features (B, C, H, W) fp32 as HeightCompression leaves it
    (no transposed copy is made) -> columns [col0, col0 + C) of the rows of `out` (K, ld >= col0 + C; a fresh (K, C) when None),
    bit for bit the reference's bilinear_interpolate_torch of every sample (pdm_bev_interpolate)."""
    assert keypoints.is_cuda and keypoints.dtype == torch.float32 and keypoints.dim() == 2 and keypoints.shape[1] == 4, 'keypoints: fp32 (K, 4) on the GPU'
    assert spatial_features.is_cuda and spatial_features.dtype == torch.float32 and spatial_features.dim() == 4, 'spatial_features: fp32 (B, C, H, W)'
    keypoints, spatial_features = keypoints.contiguous(), spatial_features.contiguous()
    K = keypoints.shape[0]
    B, C, H, W = spatial_features.shape
    if out is None:
        out = torch.empty((K, C), dtype=torch.float32, device=keypoints.device)
    assert out.is_cuda and out.dtype == torch.float32 and out.dim() == 2 and out.shape[0] == K and out.stride(1) == 1, 'out: fp32 (K, ld) rows'
    assert 0 <= col0 and col0 + C <= out.shape[1], f'out: columns [{col0}, {col0 + C}) do not fit its {out.shape[1]} columns'
    _native.call("pdm_bev_interpolate", _native.stream(keypoints), K, keypoints.data_ptr(), B, C, H, W, spatial_features.data_ptr(),
                 float(point_cloud_range[0]), float(point_cloud_range[1]), float(voxel_size[0]), float(voxel_size[1]), int(bev_stride),
                 out.data_ptr(), out.stride(0), int(col0))
    return out


def roi_keypoint_query_cap():
    """the most keypoints a sample may hold for roi_keypoint_query to serve it"""
    return int(_native.lib().pdm_roi_keypoint_query_cap())


def roi_keypoint_query(rois, grid_size, xyz, xyz_batch_cnt, max_per_sample, radii, nsamples):
    """rois (B, n, 7 + C) fp32, xyz (K, 3) fp32 keypoints of all samples stacked, xyz_batch_cnt (B) int32 on the device,
    max_per_sample the caller's (host) bound on those counts, one or two scales ->
    (grid_points (B n G^3, 3), [idx (B n G^3, nsample) int32 GLOBAL rows per scale], [empty (B n G^3) bool per scale]):
    pointnet2_stack.ball_query's rows plus the sample starts, on the grid points of Voxel R-CNN's lattice, all scales in one
    launch (pdm_roi_keypoint_query).  Raises NativeLibraryError when max_per_sample is above roi_keypoint_query_cap()."""
    assert rois.is_cuda and rois.dtype == torch.float32 and rois.dim() == 3 and rois.shape[2] >= 7, 'rois: fp32 (B, n, 7 + C) on the GPU'
    assert xyz.is_cuda and xyz.dtype == torch.float32 and xyz.dim() == 2 and xyz.shape[1] == 3, 'xyz: fp32 (K, 3)'
    assert xyz_batch_cnt.is_cuda and xyz_batch_cnt.dtype == torch.int32 and xyz_batch_cnt.numel() == rois.shape[0], 'xyz_batch_cnt: int32 (B)'
    assert len(radii) == len(nsamples) and 1 <= len(radii) <= 2, 'one or two scales'
    rois, xyz, xyz_batch_cnt = rois.contiguous(), xyz.contiguous(), xyz_batch_cnt.contiguous()
    B, n = rois.shape[0], rois.shape[1]
    M = B * n * int(grid_size) ** 3
    dev = rois.device
    grid = torch.empty((M, 3), dtype=torch.float32, device=dev)
    idx = [torch.empty((M, int(ns)), dtype=torch.int32, device=dev) for ns in nsamples]
    empty = [torch.empty((M,), dtype=torch.bool, device=dev) for _ in nsamples]
    two = len(radii) == 2
    _native.call("pdm_roi_keypoint_query", _native.stream(rois), B, n, rois.shape[2], rois.data_ptr(), int(grid_size), xyz.shape[0],
                 xyz.data_ptr(), xyz_batch_cnt.data_ptr(), int(max_per_sample), len(radii), float(radii[0]), int(nsamples[0]),
                 float(radii[1]) if two else 0.0, int(nsamples[1]) if two else 0, grid.data_ptr(), idx[0].data_ptr(), empty[0].data_ptr(),
                 idx[1].data_ptr() if two else 0, empty[1].data_ptr() if two else 0)
    return grid, idx, empty

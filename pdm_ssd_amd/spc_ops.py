"""PV-RCNN++'s proposal-centric sampling on the device (csrc/spc.hip): the reference's sample_points_with_roi and
sector_fps (voxel_set_abstraction.py:45-121) for the whole batch, without the per-sample loops, the (points x rois) matrix, the
boolean-mask indexing or the per-sector .item() reads.  There is no torch fallback here: the encoder keeps the composed formulation
as the checker.

An EMPTY sample (no points) has no answer in the reference; here it yields nothing and every count of it is 0.  A sample whose
kept points ALL have sector index S (exactly on the negative x axis; the fallback point alone is the likely case) yields no
keypoint: the reference's `len(xyz_batch_cnt) == 0` branch, which samples num_keypoints of those points, is not restated.
"""
import torch

from . import _native
from .pointnet2_stack import pointnet2_stack_hip


def max_rois():
    """the most rois a sample may carry for spc_partition to serve it"""
    return int(_native.lib().pdm_spc_partition_max_rois())


def spc_partition(xyz, xyz_batch_cnt, rois, radius, num_sectors, num_keypoints, fallback=True, want_mask=False):
    """xyz (N, 3) fp32 sample-major stacked rows, xyz_batch_cnt (B) int32 on the device, rois (B, n, 7 + C) fp32 ->
    dict(seg_xyz (N, 3), seg_row (N) int32: valid up to seg_cnt.sum(), sample-major, sector ascending, source order inside a sector;
         seg_cnt (B max(S, 1)), seg_take (B S, None when S = 0), kept_cnt (B), mask (N) bool or None).
    Reads nothing on the host; can be captured in a graph (pdm_spc_partition: the rules are in include/pdmssd_hip.h)."""
    assert xyz.is_cuda and xyz.dtype == torch.float32 and xyz.dim() == 2 and xyz.shape[1] == 3, 'xyz: fp32 (N, 3) on the GPU'
    assert rois.is_cuda and rois.dtype == torch.float32 and rois.dim() == 3 and rois.shape[2] >= 7, 'rois: fp32 (B, n, 7 + C) on the GPU'
    assert xyz_batch_cnt.is_cuda and xyz_batch_cnt.dtype == torch.int32 and xyz_batch_cnt.numel() == rois.shape[0], 'xyz_batch_cnt: int32 (B)'
    xyz, rois, xyz_batch_cnt = xyz.contiguous(), rois.contiguous(), xyz_batch_cnt.contiguous()
    N, (B, n), S, dev = xyz.shape[0], rois.shape[:2], int(num_sectors), xyz.device
    nseg = max(S, 1)
    out = dict(seg_xyz=torch.empty((N, 3), dtype=torch.float32, device=dev), seg_row=torch.empty((N,), dtype=torch.int32, device=dev),
               seg_cnt=torch.empty((B * nseg,), dtype=torch.int32, device=dev),
               seg_take=torch.empty((B * S,), dtype=torch.int32, device=dev) if S > 0 else None,
               kept_cnt=torch.empty((B,), dtype=torch.int32, device=dev),
               mask=torch.zeros((N,), dtype=torch.bool, device=dev) if want_mask else None)
    return spc_partition_into(xyz, xyz_batch_cnt, rois, radius, S, num_keypoints, fallback, out)


def spc_partition_into(xyz, xyz_batch_cnt, rois, radius, num_sectors, num_keypoints, fallback, out, workspace=None):
    """spc_partition into the caller's tensors (contiguous, sized as spc_partition's); workspace: uint8, 8-byte aligned"""
    N, (B, n) = xyz.shape[0], rois.shape[:2]
    need = int(_native.lib().pdm_spc_partition_ws_bytes(N, B, int(num_sectors)))
    if workspace is None:
        workspace = torch.empty((max(need, 8),), dtype=torch.uint8, device=xyz.device)
    ptr = lambda t: t.data_ptr() if t is not None else 0       # noqa: E731
    _native.call("pdm_spc_partition", _native.stream(xyz), N, xyz.data_ptr(), B, xyz_batch_cnt.data_ptr(), n, rois.shape[2], rois.data_ptr(),
                 float(radius), int(num_sectors), int(num_keypoints), 1 if fallback else 0, out['seg_xyz'].data_ptr(), out['seg_row'].data_ptr(),
                 out['seg_cnt'].data_ptr(), ptr(out.get('seg_take')), out['kept_cnt'].data_ptr(), ptr(out.get('mask')), workspace.data_ptr(),
                 workspace.numel())
    return out


def roi_point_filter(xyz, xyz_batch_cnt, rois, radius, fallback=False, want_mask=False):
    """the S = 0 form: the rows of every sample within `radius` of a roi, compacted in source order -> the same dict, seg_cnt (B) the
    per-sample counts.  fallback=False is what FILTER_NEIGHBOR_WITH_ROI does in the reference (it indexes with the mask itself);
    fallback=True is sample_points_with_roi's first return value."""
    return spc_partition(xyz, xyz_batch_cnt, rois, radius, 0, 1, fallback=fallback, want_mask=want_mask)


def sector_fps_batch(xyz, xyz_batch_cnt, rois, radius, num_sectors, num_keypoints):
    """sectorized_proposal_centric_sampling of every sample at once: the partition, then ONE stack FPS call over its B S segments ->
    (keypoints (M, 3), rows (M) int64 of xyz, counts (B) int32 on the device, host_counts: the same as a python list).  A sample
    yields at most num_keypoints + num_sectors keypoints, sector after sector.  ONE host read: the stack FPS wrapper's (both count
    arrays at once), which also tells M."""
    S, K = int(num_sectors), int(num_keypoints)
    assert S >= 1, 'sector_fps_batch: at least one sector'
    p = spc_partition(xyz, xyz_batch_cnt, rois, radius, S, K)
    B = rois.shape[0]
    idx = torch.zeros((B * (K + S),), dtype=torch.int32, device=xyz.device)
    temp = torch.full((xyz.shape[0],), 1e10, dtype=torch.float32, device=xyz.device)
    host = pointnet2_stack_hip.stack_farthest_point_sampling_counts(p['seg_xyz'], temp, p['seg_cnt'], idx, p['seg_take'])
    per = host[1].view(B, S).sum(1)
    M = int(per.sum())
    picks = idx[:M].long()
    return p['seg_xyz'][picks], p['seg_row'][picks].long(), p['seg_take'].view(B, S).sum(1, dtype=torch.int32), per.tolist()

"""PV-RCNN++'s voxel set abstraction: the reference's pcdet/models/backbones_3d/pfe/voxel_set_abstraction.py (VoxelSetAbstraction)
with everything the plain VoxelSetAbstraction of this package refuses: SAMPLE_METHOD 'SPC' (sectorized proposal-centric sampling)
besides 'FPS', POINT_SOURCE 'voxel_centers' besides 'raw_points', FILTER_NEIGHBOR_WITH_ROI / RADIUS_OF_NEIGHBOR_WITH_ROI per source,
and both layer kinds of build_local_aggregation_module (StackSAModuleMSG, VectorPoolAggregationModuleMSG).  Constructor signature,
config keys and state_dict keys are the reference class's; it is registered as 'VoxelSetAbstractionSPC' because the plain class
keeps its refusals.  Eval mode only.  It reads batch_dict['rois'] (B, n, 7 + C): the detector runs the proposal layer first.

`use_fused_spc` (default on) selects the mechanism:
  on   the keypoints of the whole batch come from spc_ops.sector_fps_batch: ONE pdm_spc_partition call (keep rule, sectors, take
       counts, compaction in the reference's order) and ONE stack FPS call over its B S segments; every filtered source is ONE
       pdm_spc_partition call with S = 0, its features follow by index_select on the source rows
  off  the reference's formulation under the reference's names, on the device: sample_points_with_roi, sector_fps,
       sectorized_proposal_centric_sampling and the per-sample loops with their (points x rois) matrix, boolean masks and per-sector
       .item() reads.  The on-device checker.

The keypoints are RAGGED: a sample yields sum over its sectors of min(c, ceil(c / N' K)) <= NUM_KEYPOINTS + NUM_SECTORS of them.
new_xyz_batch_cnt is that count per sample; batch_dict gets point_coords_max_per_sample = NUM_KEYPOINTS + NUM_SECTORS,
keypoint_indices (the flat rows of the sample-major point source) and keypoint_batch_cnt.  (With SAMPLE_METHOD 'FPS' the counts
are NUM_KEYPOINTS each and keypoint_indices is the flat form of the plain class's.)

HOST READS of the fused path, a batch: at most TWO of its own, (1) the stack FPS wrapper's read of both count arrays, which also
tells the number of keypoints, (2) the kept totals of ALL filtered sources in one copy; plus those inside the existing VectorPool
wrappers: one per VectorPool scale, the total of its neighbour count pass, which sizes the stacked index exactly.  At PV_RCNN_PP_CFG
(bev + three filtered two-scale local_interpolation sources) that is 2 + 6 = 8 reads a batch (host_reads_per_batch(), asserted in
tests/test_pv_rcnn_pp_gpu.py).

An EMPTY sample has no answer in the reference; here it yields no keypoint and every count of it is 0.  A sample whose fallback
point (the first point, when none is near a roi) has sector index NUM_SECTORS (a point on the negative x axis) yields no keypoint
either.  That is the reference's `len(xyz_batch_cnt) == 0` branch, reached when EVERY kept point of a sample has sector index
NUM_SECTORS (all of them exactly on the negative x axis; the fallback point alone is the likely case): the reference then samples
NUM_KEYPOINTS of those points, here (both paths) the sample yields no keypoint.
"""
import math

import numpy as np
import torch

from ... import pv_rcnn_ops, spc_ops
from ...config import cfg_get as _get
from ...pointnet2_stack import pointnet2_modules as pointnet2_stack_modules
from ...pointnet2_stack import pointnet2_utils as pointnet2_stack_utils
from ...pv_rcnn_ops import sample_counts
from ...utils import common_utils
from .voxel_set_abstraction import VoxelSetAbstraction, sa_into


def sample_points_with_roi(rois, points, sample_radius_with_roi, num_max_points_of_part=200000):
    """rois (M, 7 + C), points (N, 3) of one sample -> (sampled_points (N_out, 3), point_mask (N)): the reference's function of
    this name (ref :45-75), the (N, M) distance matrix in parts of num_max_points_of_part rows"""
    masks = []
    for start in range(0, max(points.shape[0], 1), num_max_points_of_part):
        part = points[start:start + num_max_points_of_part]
        distance = (part[:, None, :] - rois[None, :, 0:3]).norm(dim=-1)
        min_dis, min_dis_roi_idx = distance.min(dim=-1)
        roi_max_dim = (rois[min_dis_roi_idx, 3:6] / 2).norm(dim=-1)
        masks.append(min_dis < roi_max_dim + sample_radius_with_roi)
    point_mask = torch.cat(masks, dim=0)
    sampled_points = points[:1] if point_mask.sum() == 0 else points[point_mask, :]
    return sampled_points, point_mask


def sector_fps(points, num_sampled_points, num_sectors):
    """points (N, 3) -> (N_out, 3): the reference's function of this name (ref :78-121).  The angle is divided by a TENSOR: on the
    device torch turns a division by a python number into a multiplication by its reciprocal, and the sector is defined by the IEEE
    quotient.  When no point has a sector (every point exactly on the negative x axis, where the reference samples num_sampled_points
    of them all) nothing is sampled."""
    sector_size = points.new_tensor(np.pi * 2 / num_sectors)
    point_angles = torch.atan2(points[:, 1], points[:, 0]) + np.pi
    sector_idx = (point_angles / sector_size).floor().clamp(min=0, max=num_sectors)
    xyz_points_list, xyz_batch_cnt, num_sampled_points_list = [], [], []
    for k in range(num_sectors):
        mask = (sector_idx == k)
        cur_num_points = mask.sum().item()
        if cur_num_points > 0:
            xyz_points_list.append(points[mask])
            xyz_batch_cnt.append(cur_num_points)
            ratio = cur_num_points / points.shape[0]
            num_sampled_points_list.append(min(cur_num_points, math.ceil(ratio * num_sampled_points)))
    if len(xyz_batch_cnt) == 0:
        return points[:0]
    xyz = torch.cat(xyz_points_list, dim=0)
    xyz_batch_cnt = torch.tensor(xyz_batch_cnt, device=points.device).int()
    sampled_points_batch_cnt = torch.tensor(num_sampled_points_list, device=points.device).int()
    sampled_pt_idxs = pointnet2_stack_utils.stack_farthest_point_sample(xyz.contiguous(), xyz_batch_cnt, sampled_points_batch_cnt).long()
    return xyz[sampled_pt_idxs]


class VoxelSetAbstractionSPC(VoxelSetAbstraction):
    def __init__(self, model_cfg, voxel_size, point_cloud_range, num_bev_features=None, num_rawpoint_features=None, **kwargs):
        super().__init__(model_cfg, voxel_size, point_cloud_range, num_bev_features=num_bev_features,
                         num_rawpoint_features=num_rawpoint_features, **kwargs)
        self.use_fused_spc = True

    def _check_config(self, model_cfg):
        if _get(model_cfg, 'POINT_SOURCE') not in ('raw_points', 'voxel_centers'):
            raise NotImplementedError(f"VoxelSetAbstractionSPC: POINT_SOURCE = {_get(model_cfg, 'POINT_SOURCE')!r} ('raw_points' or 'voxel_centers')")
        if _get(model_cfg, 'SAMPLE_METHOD') not in ('FPS', 'SPC'):
            raise NotImplementedError(f"VoxelSetAbstractionSPC: SAMPLE_METHOD = {_get(model_cfg, 'SAMPLE_METHOD')!r} ('FPS' or 'SPC')")
        if _get(model_cfg, 'SAMPLE_METHOD') == 'SPC':
            spc = _get(model_cfg, 'SPC_SAMPLING')
            assert int(_get(spc, 'NUM_SECTORS')) >= 1 and float(_get(spc, 'SAMPLE_RADIUS_WITH_ROI')) >= 0.0
        for src_name in _get(model_cfg, 'FEATURES_SOURCE'):
            if src_name == 'bev':
                continue
            cfg = _get(_get(model_cfg, 'SA_LAYER'), src_name)
            if _get(cfg, 'FILTER_NEIGHBOR_WITH_ROI', False):
                assert _get(cfg, 'RADIUS_OF_NEIGHBOR_WITH_ROI', None) is not None, f'SA_LAYER.{src_name}: RADIUS_OF_NEIGHBOR_WITH_ROI is missing'

    def host_reads_per_batch(self):
        """what the fused path reads on the host a batch: the stack FPS wrapper's counts, the kept totals of the filtered sources (one
        copy for all of them), and one total per VectorPool scale (its neighbour count pass)"""
        SA_cfg = _get(self.model_cfg, 'SA_LAYER')
        names = [n for n in _get(self.model_cfg, 'FEATURES_SOURCE') if n != 'bev']
        filtered = any(_get(_get(SA_cfg, n), 'FILTER_NEIGHBOR_WITH_ROI', False) for n in names)
        scales = sum(int(_get(_get(SA_cfg, n), 'NUM_GROUPS')) for n in names if _get(_get(SA_cfg, n), 'NAME', '') == 'VectorPoolAggregationModuleMSG')
        return 1 + int(filtered) + scales

    # ------------------------------------------------------------------ keypoints

    def sectorized_proposal_centric_sampling(self, roi_boxes, points):
        """roi_boxes (M, 7 + C), points (N, 3) of one sample -> (N_out, 3) (ref :206-225)"""
        spc = _get(self.model_cfg, 'SPC_SAMPLING')
        sampled_points, _ = sample_points_with_roi(rois=roi_boxes, points=points, sample_radius_with_roi=_get(spc, 'SAMPLE_RADIUS_WITH_ROI'),
                                                  num_max_points_of_part=_get(spc, 'NUM_POINTS_OF_EACH_SAMPLE_PART', 200000))
        return sector_fps(points=sampled_points, num_sampled_points=_get(self.model_cfg, 'NUM_KEYPOINTS'),
                          num_sectors=_get(spc, 'NUM_SECTORS'))

    def _point_source(self, batch_dict):
        """-> (N, 4) rows (b, x, y, z) of the keypoint source, sample-major in their own order"""
        if _get(self.model_cfg, 'POINT_SOURCE') == 'raw_points':
            src = batch_dict['points'][:, 0:4].float()
        else:
            coords = batch_dict['voxel_coords']
            centres = common_utils.get_voxel_centers(coords[:, 1:4], downsample_times=1, voxel_size=self.voxel_size,
                                                     point_cloud_range=self.point_cloud_range)
            src = torch.cat((coords[:, 0:1].float(), centres), dim=1)
        return src[torch.argsort(src[:, 0], stable=True)]

    def get_sampled_points(self, batch_dict, points=None):
        """-> keypoints (N1 + N2 + ..., 4) rows (b, x, y, z); batch_dict gets keypoint_indices (flat rows of the sample-major
        source), keypoint_batch_cnt (B) int32 on the device and point_coords_max_per_sample"""
        B, K = int(batch_dict['batch_size']), int(_get(self.model_cfg, 'NUM_KEYPOINTS'))
        src = self._point_source(batch_dict) if points is None else points[:, 0:4].float()
        dev = src.device
        if _get(self.model_cfg, 'SAMPLE_METHOD') == 'FPS':
            keypoints = super().get_sampled_points(batch_dict, src)
            batch_dict['keypoint_indices'] = batch_dict['keypoint_indices'].view(-1)
            batch_dict['keypoint_batch_cnt'] = torch.full((B,), K, dtype=torch.int32, device=dev)
            batch_dict['point_coords_max_per_sample'] = K
            return keypoints
        spc = _get(self.model_cfg, 'SPC_SAMPLING')
        S, radius = int(_get(spc, 'NUM_SECTORS')), float(_get(spc, 'SAMPLE_RADIUS_WITH_ROI'))
        rois = batch_dict['rois'].float()
        xyz = src[:, 1:4].contiguous()
        batch_dict['point_coords_max_per_sample'] = K + S
        if self.use_fused_spc and xyz.is_cuda:
            kp, rows, per, per_host = spc_ops.sector_fps_batch(xyz, sample_counts(src[:, 0], B), rois, radius, S, K)
            batch_col = torch.repeat_interleave(torch.arange(B, device=dev, dtype=torch.float32), per.long(), output_size=kp.shape[0])
            batch_dict['keypoint_indices'], batch_dict['keypoint_batch_cnt'] = rows, per
            return torch.cat((batch_col[:, None], kp), dim=1)
        # the reference's loop (ref :250-276); the rows are found again by position: a kept point is its own row
        keypoints_list, per = [], []
        for bs_idx in range(B):
            sampled_points = xyz[src[:, 0] == bs_idx]
            cur = self.sectorized_proposal_centric_sampling(roi_boxes=rois[bs_idx], points=sampled_points) if sampled_points.shape[0] else xyz[:0]
            keypoints_list.append(torch.cat((cur.new_ones(cur.shape[0], 1) * bs_idx, cur), dim=1))
            per.append(cur.shape[0])
        batch_dict['keypoint_indices'] = None
        batch_dict['keypoint_batch_cnt'] = torch.tensor(per, dtype=torch.int32, device=dev)
        return torch.cat(keypoints_list, dim=0)

    # ------------------------------------------------------------------ sources

    def _filter_composed(self, xyz, feats, bs_idxs, rois, radius, B):
        """the reference's loop (ref :305-320): per sample the mask of sample_points_with_roi itself (no fallback point)"""
        xs, fs, cnt = [], [], []
        for bs_idx in range(B):
            bs_mask = bs_idxs == bs_idx
            _, valid = sample_points_with_roi(rois=rois[bs_idx], points=xyz[bs_mask], sample_radius_with_roi=radius)
            xs.append(xyz[bs_mask][valid])
            fs.append(feats[bs_mask][valid] if feats is not None else None)
            cnt.append(int(valid.sum()))
        feats = torch.cat(fs).contiguous() if feats is not None else None
        return torch.cat(xs).contiguous(), feats, torch.tensor(cnt, dtype=torch.int32, device=xyz.device)

    def _layer_into(self, layer, xyz, cnt, new_xyz, new_cnt, feats, rows, coff):
        if isinstance(layer, pointnet2_stack_modules.StackSAModuleMSG):
            return sa_into(layer, xyz, cnt, new_xyz, new_cnt, feats, rows, coff)
        _, pooled = layer(xyz=xyz, xyz_batch_cnt=cnt, new_xyz=new_xyz, new_xyz_batch_cnt=new_cnt, features=feats)
        rows[:, coff:coff + pooled.shape[1]] = pooled
        return coff + pooled.shape[1]

    def _forward(self, batch_dict):
        B = int(batch_dict['batch_size'])
        sources = list(_get(self.model_cfg, 'FEATURES_SOURCE'))
        SA_cfg = _get(self.model_cfg, 'SA_LAYER')
        keypoints = self.get_sampled_points(batch_dict)
        dev = keypoints.device
        M = keypoints.shape[0]
        new_xyz = keypoints[:, 1:4].contiguous()
        new_cnt = batch_dict['keypoint_batch_cnt']
        before = torch.zeros((M, self.num_point_features_before_fusion), dtype=torch.float32, device=dev)
        coff = 0
        if 'bev' in sources:
            bev, stride = batch_dict['spatial_features'], batch_dict['spatial_features_stride']
            assert bev.shape[1] == self.num_bev_features, f'spatial_features: {bev.shape[1]} channels, built for {self.num_bev_features}'
            if self.use_fused_bev and bev.is_cuda:
                pv_rcnn_ops.bev_interpolate(keypoints, bev.float(), self.point_cloud_range, self.voxel_size, stride, out=before, col0=coff)
            else:
                before[:, coff:coff + bev.shape[1]] = self.interpolate_from_bev_features(keypoints, bev, B, stride)
            coff += bev.shape[1]

        # every source sample-major: (name, layer, xyz, batch column, features), in the reference's column order
        jobs = []
        if 'raw_points' in sources:
            raw = batch_dict['points']
            raw = raw[torch.argsort(raw[:, 0], stable=True)]
            jobs.append(('raw_points', self.SA_rawpoints, raw[:, 1:4].float().contiguous(), raw[:, 0],
                         raw[:, 4:].float().contiguous() if raw.shape[1] > 4 else None))
        for k, src_name in enumerate(self.SA_layer_names):
            level = batch_dict['multi_scale_3d_features'][src_name]
            coords = level.indices
            xyz = common_utils.get_voxel_centers(coords[:, 1:4], downsample_times=self.downsample_times_map[src_name],
                                                 voxel_size=self.voxel_size, point_cloud_range=self.point_cloud_range)
            jobs.append((src_name, self.SA_layers[k], xyz.contiguous(), coords[:, 0], level.features.float().contiguous()))

        fused = self.use_fused_spc and new_xyz.is_cuda
        rois = batch_dict['rois'].float() if 'rois' in batch_dict else None
        radius_of = {name: _get(_get(SA_cfg, name), 'RADIUS_OF_NEIGHBOR_WITH_ROI', None) for name, *_ in jobs
                     if _get(_get(SA_cfg, name), 'FILTER_NEIGHBOR_WITH_ROI', False)}
        parts = {}
        if fused and radius_of:
            for name, _, xyz, bcol, _ in jobs:
                if name in radius_of:
                    parts[name] = spc_ops.roi_point_filter(xyz, sample_counts(bcol, B), rois, float(radius_of[name]))
            # the kept totals of every filtered source: one copy to the host
            totals = torch.stack([parts[name]['seg_cnt'].sum() for name in parts]).cpu().tolist()
            totals = dict(zip(parts, totals))
        for name, layer, xyz, bcol, feats in jobs:
            if name not in radius_of:
                cnt = sample_counts(bcol, B)
            elif fused:
                p, T = parts[name], int(totals[name])
                xyz, cnt = p['seg_xyz'][:T], p['seg_cnt']
                feats = feats.index_select(0, p['seg_row'][:T].long()) if feats is not None else None
            else:
                xyz, feats, cnt = self._filter_composed(xyz, feats, bcol, rois, float(radius_of[name]), B)
            coff = self._layer_into(layer, xyz, cnt, new_xyz, new_cnt, feats, before, coff)
        assert coff == before.shape[1]
        batch_dict['point_features_before_fusion'] = before
        batch_dict['point_features'] = self._fusion(before)
        batch_dict['point_coords'] = keypoints
        return batch_dict

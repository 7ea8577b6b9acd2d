"""PV-RCNN's voxel set abstraction: behaviour, constructor signature, config keys and state_dict keys of the reference's
pcdet/models/backbones_3d/pfe/voxel_set_abstraction.py (VoxelSetAbstraction), restated for POINT_SOURCE 'raw_points' and
SAMPLE_METHOD 'FPS' in eval mode.

NUM_KEYPOINTS keypoints per sample by farthest point sampling of the raw points; per keypoint the features of every
FEATURES_SOURCE side by side: 'bev' (the BEV map, bilinearly), 'raw_points' and 'x_conv1..4' (StackSAModuleMSG over the raw
points / over the voxel centres of a level of the sparse backbone); vsa_point_feature_fusion on top.

What differs from the reference is mechanism only:
  * the keypoints of the whole batch come from ONE stack FPS call (each sample asked for min(its points, NUM_KEYPOINTS)); the
    reference's rule for a sample with fewer points than NUM_KEYPOINTS (repeat the sampled indices) is index arithmetic on the
    device, slot j of a sample reads pick j mod its count;
  * 'bev' is one launch of pdm_bev_interpolate on the NCHW map as it is (`use_fused_bev`, default on; the reference's
    per-sample loop, interpolate_from_bev_features, stays as the checker);
  * per-sample counts are an integer scatter-add on the device, not a loop of .sum() reads, and every source's columns are
    written in place into one point_features_before_fusion buffer (no torch.cat).
HOST READS: one per batch, inside the stack FPS wrapper (the per-sample point counts, which choose its instantiation).

An empty sample has no answer in the reference (it divides by the point count).  Here its NUM_KEYPOINTS keypoints copy a point
of another sample (the row the clamped index lands on) under the empty sample's batch index; every query in it finds nothing,
so its set-abstraction columns are the layers' response to an empty ball.

Refused with NotImplementedError: SAMPLE_METHOD 'SPC', POINT_SOURCE 'voxel_centers', FILTER_NEIGHBOR_WITH_ROI and the
VectorPoolAggregationModuleMSG layers (PV-RCNN++: VoxelSetAbstractionSPC in voxel_set_abstraction_spc.py serves them, under its own
registry NAME), and training mode.
"""
import torch
import torch.nn as nn

from ... import fused, pv_rcnn_ops
from ...config import cfg_get as _get
from ...dense_heads.point_head_box import _fc_layers
from ...pointnet2_stack import pointnet2_modules as pointnet2_stack_modules
from ...pointnet2_stack import pointnet2_stack_hip
from ...pv_rcnn_ops import sample_counts
from ...utils import common_utils


def bilinear_interpolate_torch(im, x, y):
    """im (H, W, C), x (N), y (N) -> (N, C): the reference's function of this name, operation for operation"""
    x0 = torch.floor(x).long()
    x1 = x0 + 1
    y0 = torch.floor(y).long()
    y1 = y0 + 1
    x0 = torch.clamp(x0, 0, im.shape[1] - 1)
    x1 = torch.clamp(x1, 0, im.shape[1] - 1)
    y0 = torch.clamp(y0, 0, im.shape[0] - 1)
    y1 = torch.clamp(y1, 0, im.shape[0] - 1)
    Ia, Ib, Ic, Id = im[y0, x0], im[y1, x0], im[y0, x1], im[y1, x1]
    wa = (x1.type_as(x) - x) * (y1.type_as(y) - y)
    wb = (x1.type_as(x) - x) * (y - y0.type_as(y))
    wc = (x - x0.type_as(x)) * (y1.type_as(y) - y)
    wd = (x - x0.type_as(x)) * (y - y0.type_as(y))
    return torch.t(torch.t(Ia) * wa) + torch.t(torch.t(Ib) * wb) + torch.t(torch.t(Ic) * wc) + torch.t(torch.t(Id) * wd)


def sa_into(layer, xyz, xyz_batch_cnt, new_xyz, new_xyz_batch_cnt, features, rows, coff, queries=None):
    """the columns of one StackSAModuleMSG written at column `coff` of `rows` (M, ld): in place by the fused kernels where they
    serve the module (ld and coff multiples of 4, as in the published widths; a copy otherwise), else the module's plain forward
    and a copy.  Returns the next free column."""
    if layer._fused_ok(xyz, features):
        in_place = rows.shape[1] % 4 == 0 and coff % 4 == 0     # the fused kernels store 16-byte groups
        got = layer._forward_fused(xyz, xyz_batch_cnt, new_xyz, new_xyz_batch_cnt, features, queries=queries,
                                   dest=(rows, coff) if in_place else None)
        if got is not None:
            width = sum(mlp[-3].out_channels for mlp in layer.mlps)
            if not in_place:
                rows[:, coff:coff + width] = got
            return coff + width
    _, pooled = layer(xyz=xyz, xyz_batch_cnt=xyz_batch_cnt, new_xyz=new_xyz, new_xyz_batch_cnt=new_xyz_batch_cnt, features=features)
    rows[:, coff:coff + pooled.shape[1]] = pooled
    return coff + pooled.shape[1]


class VoxelSetAbstraction(nn.Module):
    def __init__(self, model_cfg, voxel_size, point_cloud_range, num_bev_features=None, num_rawpoint_features=None, **kwargs):
        super().__init__()
        self.model_cfg = model_cfg
        self.voxel_size = [float(v) for v in voxel_size]
        self.point_cloud_range = [float(v) for v in point_cloud_range]
        self.use_fused_bev = True
        self._check_config(model_cfg)
        SA_cfg = _get(model_cfg, 'SA_LAYER')
        sources = list(_get(model_cfg, 'FEATURES_SOURCE'))

        self.SA_layers = nn.ModuleList()
        self.SA_layer_names = []
        self.downsample_times_map = {}
        c_in = 0
        for src_name in sources:
            if src_name in ['bev', 'raw_points']:
                continue
            cfg = _get(SA_cfg, src_name)
            self.downsample_times_map[src_name] = _get(cfg, 'DOWNSAMPLE_FACTOR')
            if _get(cfg, 'INPUT_CHANNELS', None) is None:
                first = _get(cfg, 'MLPS')[0]
                input_channels = first[0] if isinstance(first, (list, tuple)) else first
            else:
                input_channels = _get(cfg, 'INPUT_CHANNELS')
            cur_layer, cur_num_c_out = pointnet2_stack_modules.build_local_aggregation_module(input_channels=input_channels, config=cfg)
            self.SA_layers.append(cur_layer)
            self.SA_layer_names.append(src_name)
            c_in += cur_num_c_out
        if 'bev' in sources:
            c_in += num_bev_features
        if 'raw_points' in sources:
            self.SA_rawpoints, cur_num_c_out = pointnet2_stack_modules.build_local_aggregation_module(
                input_channels=num_rawpoint_features - 3, config=_get(SA_cfg, 'raw_points'))
            c_in += cur_num_c_out
        self.num_bev_features = num_bev_features
        width = _get(model_cfg, 'NUM_OUTPUT_FEATURES')
        self.vsa_point_feature_fusion = nn.Sequential(nn.Linear(c_in, width, bias=False), nn.BatchNorm1d(width), nn.ReLU())
        self.num_point_features = width
        self.num_point_features_before_fusion = c_in

    def _check_config(self, model_cfg):
        """what this class refuses (a subclass that serves more overrides it: VoxelSetAbstractionSPC)"""
        see = '; see VoxelSetAbstractionSPC (voxel_set_abstraction_spc.py)'
        if _get(model_cfg, 'POINT_SOURCE') != 'raw_points':
            raise NotImplementedError(f"VoxelSetAbstraction: POINT_SOURCE = {_get(model_cfg, 'POINT_SOURCE')!r} (only 'raw_points'; "
                                      f"'voxel_centers' is PV-RCNN++{see})")
        if _get(model_cfg, 'SAMPLE_METHOD') != 'FPS':
            raise NotImplementedError(f"VoxelSetAbstraction: SAMPLE_METHOD = {_get(model_cfg, 'SAMPLE_METHOD')!r} (only 'FPS'; 'SPC', the "
                                      f"sectorized proposal-centric sampling, is PV-RCNN++{see})")
        SA_cfg = _get(model_cfg, 'SA_LAYER')
        for src_name in _get(model_cfg, 'FEATURES_SOURCE'):
            if src_name == 'bev':
                continue
            cfg = _get(SA_cfg, src_name)
            if _get(cfg, 'FILTER_NEIGHBOR_WITH_ROI', False):
                raise NotImplementedError(f'VoxelSetAbstraction: SA_LAYER.{src_name}.FILTER_NEIGHBOR_WITH_ROI is PV-RCNN++{see}')
            if _get(cfg, 'NAME', 'StackSAModuleMSG') != 'StackSAModuleMSG':
                raise NotImplementedError(f"VoxelSetAbstraction: SA_LAYER.{src_name}.NAME = {_get(cfg, 'NAME')!r} (the "
                                          f"VectorPoolAggregationModuleMSG layers are PV-RCNN++{see})")

    # ------------------------------------------------------------------ keypoints

    def get_sampled_points(self, batch_dict, points=None):
        """points (N1 + N2 + ..., 1 + 3 + C) sample-major (batch_dict's, when not given) -> keypoints (B NUM_KEYPOINTS, 4) rows
        (b, x, y, z); the rows of `points` they came from are left in batch_dict['keypoint_indices'] (B, NUM_KEYPOINTS) int64."""
        B, K = int(batch_dict['batch_size']), int(_get(self.model_cfg, 'NUM_KEYPOINTS'))
        points = batch_dict['points'] if points is None else points
        assert points.shape[0] > 0, 'VoxelSetAbstraction: a batch without points'
        src = points[:, 1:4].float().contiguous()
        counts = sample_counts(points[:, 0], B)
        take = counts.clamp(max=K)                                  # picks per sample: the reference's first min(N, K) of its K
        packed = torch.zeros((B * K,), dtype=torch.int32, device=src.device)
        temp = torch.full((src.shape[0],), 1e10, dtype=torch.float32, device=src.device)
        pointnet2_stack_hip.stack_farthest_point_sampling_wrapper(src, temp, counts, packed, take)     # (the batch's one host read)
        first = torch.cumsum(take, 0) - take
        slot = first[:, None] + torch.arange(K, device=src.device)[None, :] % take.clamp(min=1)[:, None]   # pick j mod count
        rows = packed[slot.clamp(max=B * K - 1).view(-1)].long().clamp(0, src.shape[0] - 1)
        batch_dict['keypoint_indices'] = rows.view(B, K)
        batch_col = torch.arange(B, device=src.device, dtype=torch.float32).repeat_interleave(K, output_size=B * K)
        return torch.cat((batch_col[:, None], src[rows]), dim=1)

    # ------------------------------------------------------------------ bev

    def interpolate_from_bev_features(self, keypoints, bev_features, batch_size, bev_stride):
        """the reference's per-sample formulation (ref :176-204): the checker of pdm_bev_interpolate.  (The divisions are by
        tensors: on the device torch turns a division by a python number into a multiplication by its reciprocal.)"""
        r0 = keypoints.new_tensor(self.point_cloud_range[0:2])
        vs = keypoints.new_tensor(self.voxel_size[0:2])
        stride = keypoints.new_tensor(float(bev_stride))
        x_idxs = (keypoints[:, 1] - r0[0]) / vs[0] / stride
        y_idxs = (keypoints[:, 2] - r0[1]) / vs[1] / stride
        out = []
        for k in range(batch_size):
            bs_mask = keypoints[:, 0] == k
            out.append(bilinear_interpolate_torch(bev_features[k].permute(1, 2, 0), x_idxs[bs_mask], y_idxs[bs_mask]))
        return torch.cat(out, dim=0)

    # ------------------------------------------------------------------ forward

    def _fusion(self, before):
        if (not torch.is_grad_enabled() and before.is_cuda and before.dtype == torch.float32 and getattr(self, 'use_fused', True)):
            pk = fused.cached_layers(self, 'fusion', self.vsa_point_feature_fusion, lambda: _fc_layers(self.vsa_point_feature_fusion),
                                     before.device)
            if pk is not None:
                width = self.num_point_features
                out = torch.empty((1, before.shape[0], (width + 3) // 4 * 4), dtype=torch.float32, device=before.device)
                fused.rows_forward(pk, before[None], out, relu_last=True)
                return out[0, :, :width]
        return self.vsa_point_feature_fusion(before)

    def forward(self, batch_dict):
        """batch_size, points, spatial_features (+ _stride), multi_scale_3d_features -> point_features (B K, NUM_OUTPUT_FEATURES),
        point_features_before_fusion (B K, sum of the sources' widths), point_coords (B K, 4)"""
        if self.training:
            raise NotImplementedError('VoxelSetAbstraction runs in eval mode only: the gradients of the keypoint path are not built')
        with torch.no_grad():
            return self._forward(batch_dict)

    def _forward(self, batch_dict):
        B, K = int(batch_dict['batch_size']), int(_get(self.model_cfg, 'NUM_KEYPOINTS'))
        sources = list(_get(self.model_cfg, 'FEATURES_SOURCE'))
        # sample-major rows in their own order (a stable sort on the device): what the reference's boolean masks select
        raw = batch_dict['points']
        raw = raw[torch.argsort(raw[:, 0], stable=True)]
        keypoints = self.get_sampled_points(batch_dict, raw)
        dev = keypoints.device
        before = torch.empty((B * K, self.num_point_features_before_fusion), dtype=torch.float32, device=dev)
        coff = 0
        if 'bev' in sources:
            bev = batch_dict['spatial_features']
            stride = batch_dict['spatial_features_stride']
            assert bev.shape[1] == self.num_bev_features, f'spatial_features: {bev.shape[1]} channels, built for {self.num_bev_features}'
            if self.use_fused_bev and bev.is_cuda:
                pv_rcnn_ops.bev_interpolate(keypoints, bev.float(), self.point_cloud_range, self.voxel_size, stride, out=before, col0=coff)
            else:
                before[:, coff:coff + bev.shape[1]] = self.interpolate_from_bev_features(keypoints, bev, B, stride)
            coff += bev.shape[1]

        new_xyz = keypoints[:, 1:4].contiguous()
        new_xyz_batch_cnt = torch.full((B,), K, dtype=torch.int32, device=dev)
        if 'raw_points' in sources:
            coff = sa_into(self.SA_rawpoints, raw[:, 1:4].float().contiguous(), sample_counts(raw[:, 0], B), new_xyz, new_xyz_batch_cnt,
                           raw[:, 4:].float().contiguous() if raw.shape[1] > 4 else None, before, coff)
        for k, src_name in enumerate(self.SA_layer_names):
            level = batch_dict['multi_scale_3d_features'][src_name]
            coords = level.indices
            xyz = common_utils.get_voxel_centers(coords[:, 1:4], downsample_times=self.downsample_times_map[src_name],
                                                 voxel_size=self.voxel_size, point_cloud_range=self.point_cloud_range)
            coff = sa_into(self.SA_layers[k], xyz.contiguous(), sample_counts(coords[:, 0], B), new_xyz, new_xyz_batch_cnt,
                           level.features.float().contiguous(), before, coff)
        assert coff == before.shape[1]
        batch_dict['point_features_before_fusion'] = before
        batch_dict['point_features'] = self._fusion(before)
        batch_dict['point_coords'] = keypoints
        batch_dict['point_coords_max_per_sample'] = K      # (a host number: what the RoI head's query sizes its LDS by)
        return batch_dict

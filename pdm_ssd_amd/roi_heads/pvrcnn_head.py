"""PV-RCNN's second stage: behaviour, constructor signature, config keys and state_dict keys of the reference's
pcdet/models/roi_heads/pvrcnn_head.py (PVRCNNHead), restated, in eval mode.

Per RoI a G x G x G lattice of grid points; per grid point the keypoints of its sample within POOL_RADIUS, the first NSAMPLE of
them, pooled by a StackSAModuleMSG over the keypoint features weighted by point_cls_scores; the flattened (channels x G^3) row
-> shared_fc_layer -> cls_layers / reg_layers (Conv1d stacks).

roi_grid_pool (`use_fused_pool`, default on): ONE launch of pdm_roi_keypoint_query (csrc/pv_rcnn.hip) forms the
grid points and, for all scales at once, the global neighbour rows and empty-ball masks; the existing fused gather -> MLP -> max
kernels then run once per scale on those rows and write their columns of the (B n G^3, sum C) output.  No host read, no
torch.cat, graph-capturable.  More keypoints a sample than the operator's cap, more than two scales, a module the fused
kernels do not serve (a VectorPoolAggregationModuleMSG ROI_GRID_POOL among them) and use_fused_pool = False take the composed path (torch grid points, then ball_query per scale inside
the module): the on-device checker.  `last_pool_path` tells which ran.

Training raises NotImplementedError: eval only.
"""
import torch
import torch.nn as nn

from .. import pv_rcnn_ops
from ..pv_rcnn_ops import sample_counts
from ..pointnet2_stack import pointnet2_modules as pointnet2_stack_modules
from ..utils import common_utils
from .roi_head_template import RoIHeadTemplate, _get


class PVRCNNHead(RoIHeadTemplate):
    def __init__(self, input_channels, model_cfg, num_class=1, **kwargs):
        super().__init__(num_class=num_class, model_cfg=model_cfg)
        self.pool_cfg = _get(model_cfg, 'ROI_GRID_POOL')
        self.roi_grid_pool_layer, num_c_out = pointnet2_stack_modules.build_local_aggregation_module(
            input_channels=input_channels, config=self.pool_cfg)
        self.num_pooled_channels = num_c_out
        self.use_fused_pool = True
        self.last_pool_path = None

        grid_size = int(_get(self.pool_cfg, 'GRID_SIZE'))
        pre_channel = grid_size ** 3 * num_c_out
        drop = _get(model_cfg, 'DP_RATIO')
        widths = list(_get(model_cfg, 'SHARED_FC'))
        shared = []
        for k, width in enumerate(widths):
            shared += [nn.Conv1d(pre_channel, width, kernel_size=1, bias=False), nn.BatchNorm1d(width), nn.ReLU()]
            pre_channel = width
            if k != len(widths) - 1 and drop > 0:       # (holds no parameter but shifts the children behind it: the reference's keys)
                shared.append(nn.Dropout(drop))
        self.shared_fc_layer = nn.Sequential(*shared)
        self.cls_layers = self.make_fc_layers(input_channels=pre_channel, output_channels=self.num_class, fc_list=_get(model_cfg, 'CLS_FC'))
        self.reg_layers = self.make_fc_layers(input_channels=pre_channel, output_channels=self.box_coder.code_size * self.num_class,
                                              fc_list=_get(model_cfg, 'REG_FC'))
        self.init_weights(weight_init='xavier')

    def init_weights(self, weight_init='xavier'):
        init_func = {'kaiming': nn.init.kaiming_normal_, 'xavier': nn.init.xavier_normal_, 'normal': nn.init.normal_}.get(weight_init)
        if init_func is None:
            raise NotImplementedError(weight_init)
        for m in self.modules():
            if isinstance(m, (nn.Conv2d, nn.Conv1d)):
                if weight_init == 'normal':
                    init_func(m.weight, mean=0, std=0.001)
                else:
                    init_func(m.weight)
                if m.bias is not None:
                    nn.init.constant_(m.bias, 0)
        nn.init.normal_(self.reg_layers[-1].weight, mean=0, std=0.001)

    # ------------------------------------------------------------------ pooling

    @torch.no_grad()
    def roi_grid_pool(self, batch_dict):
        """batch_size, rois (B, n, 7 + C), point_coords (K, 4) rows (b, x, y, z) sample-major, point_features (K, C),
        point_cls_scores (K,) -> (B n, G^3, sum of the scales' widths).

        point_coords_max_per_sample (a host int, optional): a bound on the keypoints of any one sample, which the fused query
        sizes its LDS by.  The contract is the caller's: the counts live on the device and are not read back, and a sample that
        holds MORE than the bound is queried over its first `bound` keypoints only, without a signal.  VoxelSetAbstraction leaves
        NUM_KEYPOINTS there, which holds exactly.  Without the key the bound is the total number of keypoints, which is safe
        but, at the published setting with more than one sample (B x 2048 > the cap of 4096), selects the composed path."""
        rois = batch_dict['rois'].float().contiguous()
        B, n = rois.shape[0], rois.shape[1]
        G = int(_get(self.pool_cfg, 'GRID_SIZE'))
        coords = batch_dict['point_coords']
        features = (batch_dict['point_features'] * batch_dict['point_cls_scores'].view(-1, 1)).float().contiguous()
        xyz = coords[:, 1:4].float().contiguous()
        xyz_batch_cnt = sample_counts(coords[:, 0], B)
        layer = self.roi_grid_pool_layer
        M = B * n * G ** 3
        new_cnt = torch.full((B,), n * G ** 3, dtype=torch.int32, device=rois.device)

        bound = int(batch_dict.get('point_coords_max_per_sample', xyz.shape[0]))
        # (a VectorPool ROI_GRID_POOL, PV-RCNN++'s, has no groupers: it pools through the composed path, its own forward)
        if (self.use_fused_pool and rois.is_cuda and hasattr(layer, 'groupers') and len(layer.groupers) <= 2 and 0 < xyz.shape[0] and bound <= pv_rcnn_ops.roi_keypoint_query_cap()
                and self.num_pooled_channels % 4 == 0 and layer._fused_ok(xyz, features)):
            grid, idx, empty = pv_rcnn_ops.roi_keypoint_query(rois, G, xyz, xyz_batch_cnt, bound, [g.radius for g in layer.groupers],
                                                              [g.nsample for g in layer.groupers])
            out = torch.empty((M, self.num_pooled_channels), dtype=torch.float32, device=rois.device)
            if layer._forward_fused(xyz, xyz_batch_cnt, grid, new_cnt, features, queries=list(zip(idx, empty)), dest=(out, 0)) is not None:
                self.last_pool_path = 'fused'
                return out.view(B * n, G ** 3, self.num_pooled_channels)
        self.last_pool_path = 'composed'
        grid, _ = self.get_global_grid_points_of_roi(rois, grid_size=G)
        _, pooled = layer(xyz=xyz, xyz_batch_cnt=xyz_batch_cnt, new_xyz=grid.reshape(-1, 3).contiguous(), new_xyz_batch_cnt=new_cnt,
                          features=features)
        return pooled.view(B * n, G ** 3, pooled.shape[-1])

    def get_global_grid_points_of_roi(self, rois, grid_size):
        rois = rois.view(-1, rois.shape[-1])
        local = self.get_dense_grid_points(rois, rois.shape[0], grid_size)
        points = common_utils.rotate_points_along_z(local.clone(), rois[:, 6])
        points = points + rois[:, 0:3].unsqueeze(dim=1)
        return points, local

    @staticmethod
    def get_dense_grid_points(rois, batch_size_rcnn, grid_size):
        """(R, G^3, 3): (i + 0.5) / G size - size / 2 per axis, the lattice in nonzero()'s order (x index slowest, z fastest)"""
        dense_idx = rois.new_ones((grid_size, grid_size, grid_size)).nonzero()
        dense_idx = dense_idx.repeat(batch_size_rcnn, 1, 1).float()
        size = rois.view(batch_size_rcnn, -1)[:, 3:6]
        return (dense_idx + 0.5) / grid_size * size.unsqueeze(dim=1) - (size.unsqueeze(dim=1) / 2)

    # ------------------------------------------------------------------ forward

    def forward(self, batch_dict):
        """(ref :134-175) proposals (unless rois are given) -> pooled grid features -> rcnn_cls (R, num_class), rcnn_reg
        (R, code_size), batch_cls_preds / batch_box_preds with cls_preds_normalized = False"""
        if self.training:
            raise NotImplementedError('PVRCNNHead runs in eval mode only: proposal targets for it and the gradients of its RoI-grid '
                                      'pooling are not built')
        self.proposal_layer(batch_dict, nms_config=_get(self.model_cfg, 'NMS_CONFIG')['TEST'])
        pooled = self.roi_grid_pool(batch_dict)                         # (R, G^3, C)
        R = pooled.shape[0]
        flat = pooled.permute(0, 2, 1).contiguous().view(R, -1, 1)      # channel-major per RoI, as the reference flattens it
        shared = self.shared_fc_layer(flat)
        rcnn_cls = self.cls_layers(shared).transpose(1, 2).contiguous().squeeze(dim=1)
        rcnn_reg = self.reg_layers(shared).transpose(1, 2).contiguous().squeeze(dim=1)
        cls, boxes = self.generate_predicted_boxes(batch_size=batch_dict['batch_size'], rois=batch_dict['rois'], cls_preds=rcnn_cls,
                                                   box_preds=rcnn_reg)
        batch_dict.update(rcnn_cls=rcnn_cls, rcnn_reg=rcnn_reg, batch_cls_preds=cls, batch_box_preds=boxes, cls_preds_normalized=False)
        return batch_dict

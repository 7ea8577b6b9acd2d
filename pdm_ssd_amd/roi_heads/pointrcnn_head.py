"""PointRCNN's second stage: behaviour, constructor signature, config keys and state_dict keys of
/root/reference/pcdet/models/roi_heads/pointrcnn_head.py, restated.  RoI point pooling and the canonical transformation
are ONE launch of pdm_roipoint_pool3d_canonical (csrc/roi_pool.hip).

Per RoI: 512 pooled points [x, y, z in the RoI's frame, point score, depth, C features] -> the five prefix channels are
lifted by `xyz_up_layer` and merged with the C features by `merge_down_layer` -> PointNet++ set-abstraction levels
(`SA_modules`, the last one grouping all points) -> `cls_layers` and `reg_layers` on the one remaining feature vector.

Training mode (ref :140-179): proposals with NMS_CONFIG.TRAIN -> assign_targets (pdm_proposal_targets) -> the sampled
rois replace the proposals -> pooling under no_grad -> rcnn_cls / rcnn_reg into forward_ret_dict for get_loss().  A head
whose TARGET_CONFIG holds no sampler settings (POINT_RCNN_CFG) has no training half and raises NotImplementedError there.
"""
import torch
import torch.nn as nn

from ..pointnet2_batch.pointnet2_modules import PointnetSAModule
from ..roipoint_pool3d import roipoint_pool3d_utils
from .roi_head_template import RoIHeadTemplate

_WEIGHT_INIT = {'kaiming': nn.init.kaiming_normal_, 'xavier': nn.init.xavier_normal_, 'normal': nn.init.normal_}


def _pointwise_stack(widths, use_bn):
    """Conv2d(1x1) [-> BatchNorm2d] -> ReLU per step of `widths`; the convolution carries the bias when there is no
    BatchNorm (children 0, 2, 4, ... without BatchNorm, 0, 3, 6, ... with it: the reference's keys)."""
    layers = []
    for cin, cout in zip(widths[:-1], widths[1:]):
        layers.append(nn.Conv2d(cin, cout, kernel_size=1, bias=not use_bn))
        if use_bn:
            layers.append(nn.BatchNorm2d(cout))
        layers.append(nn.ReLU())
    return nn.Sequential(*layers)


class PointRCNNHead(RoIHeadTemplate):
    def __init__(self, input_channels, model_cfg, num_class=1, **kwargs):
        super().__init__(num_class=num_class, model_cfg=model_cfg, **kwargs)
        cfg = self.model_cfg
        use_bn = cfg.USE_BN
        self.num_prefix_channels = 3 + 2          # canonical xyz, first-stage score, normalised depth
        lifted = cfg.XYZ_UP_LAYER[-1]
        self.xyz_up_layer = _pointwise_stack([self.num_prefix_channels] + list(cfg.XYZ_UP_LAYER), use_bn)
        self.merge_down_layer = _pointwise_stack([2 * lifted, lifted], use_bn)

        sa = cfg.SA_CONFIG
        self.SA_modules = nn.ModuleList()
        width = input_channels
        for npoint, radius, nsample, mlp in zip(sa.NPOINTS, sa.RADIUS, sa.NSAMPLE, sa.MLPS):
            spec = [width] + list(mlp)            # (the module adds 3 to spec[0] for use_xyz)
            self.SA_modules.append(PointnetSAModule(npoint=None if npoint == -1 else npoint,   # -1: one group of all points
                                                    radius=radius, nsample=nsample, mlp=spec, use_xyz=True, bn=use_bn))
            width = mlp[-1]

        self.cls_layers = self.make_fc_layers(input_channels=width, output_channels=self.num_class, fc_list=cfg.CLS_FC)
        self.reg_layers = self.make_fc_layers(input_channels=width, output_channels=self.box_coder.code_size * self.num_class,
                                              fc_list=cfg.REG_FC)
        pool = cfg.ROI_POINT_POOL
        self.roipoint_pool3d_layer = roipoint_pool3d_utils.RoIPointPool3d(num_sampled_points=pool.NUM_SAMPLED_POINTS,
                                                                          pool_extra_width=pool.POOL_EXTRA_WIDTH)
        self.init_weights(weight_init='xavier')

    def init_weights(self, weight_init='xavier'):
        """Every convolution's weight by `weight_init` ('normal': std 0.001), biases 0; the last regression layer always
        normal with std 0.001, so that the first refinements are close to the proposals."""
        if weight_init not in _WEIGHT_INIT:
            raise NotImplementedError(weight_init)
        for m in self.modules():
            if not isinstance(m, (nn.Conv1d, nn.Conv2d)):
                continue
            if weight_init == 'normal':
                nn.init.normal_(m.weight, mean=0, std=0.001)
            else:
                _WEIGHT_INIT[weight_init](m.weight)
            if m.bias is not None:
                nn.init.zeros_(m.bias)
        nn.init.normal_(self.reg_layers[-1].weight, mean=0, std=0.001)

    @torch.no_grad()
    def roipool3d_gpu(self, batch_dict):
        """batch_size, rois (B, num_rois, 7 + C'), point_coords (num_points, 4) [bs_idx, x, y, z], point_features
        (num_points, C), point_cls_scores (num_points) -> (B * num_rois, num_sampled_points, 3 + 2 + C): per RoI its
        first num_sampled_points points (repeated cyclically when fewer) as [xyz in the RoI's frame, score,
        |xyz| / DEPTH_NORMALIZER - 0.5, features]; zeros for a RoI without points.

        The samples must hold the same number of points, stored sample after sample.  Only what follows from
        batch_size and the row count is checked here (no per-sample count, no host read): a batch whose samples differ
        in size while the total still divides by batch_size is NOT detected and would be pooled across sample
        boundaries.  PointNet2MSG, which produces these rows, checks the per-sample counts itself."""
        num_samples = batch_dict['batch_size']
        xyz = batch_dict['point_coords'][:, 1:4]
        assert xyz.shape[0] % num_samples == 0, 'PointRCNNHead needs the same number of points in every sample'
        depth = xyz.norm(dim=1) / self.model_cfg.ROI_POINT_POOL.DEPTH_NORMALIZER - 0.5
        columns = torch.cat([batch_dict['point_cls_scores'].detach().unsqueeze(1), depth.unsqueeze(1),
                             batch_dict['point_features']], dim=1)
        layer = self.roipoint_pool3d_layer
        pooled, _ = roipoint_pool3d_utils.roipoint_pool3d_canonical(
            xyz.reshape(num_samples, -1, 3), columns.view(num_samples, -1, columns.shape[1]), batch_dict['rois'],
            layer.pool_extra_width, layer.num_sampled_points)
        return pooled.flatten(0, 1)

    def _roi_features(self, pooled):
        """pooled (R, S, 5 + C) -> (R, C_last, 1): prefix lift, merge with the features, the SA levels."""
        k = self.num_prefix_channels
        as_map = pooled.permute(0, 2, 1).unsqueeze(3)                       # (R, 5 + C, S, 1) view
        lifted = self.xyz_up_layer(as_map[:, :k].contiguous())
        merged = self.merge_down_layer(torch.cat([lifted, as_map[:, k:]], dim=1))
        xyz, features = pooled[:, :, 0:3].contiguous(), merged.squeeze(3).contiguous()
        for level in self.SA_modules:
            xyz, features = level(xyz, features)
        return features.contiguous()

    def forward(self, batch_dict):
        """Eval mode (behaviour of ref :132-179): proposals (unless rois are given) -> pooled canonical points -> RoI
        features -> rcnn_cls (R, num_class), rcnn_reg (R, code_size) -> batch_cls_preds / batch_box_preds (refined boxes)
        with cls_preds_normalized = False.
        Training mode: proposals with NMS_CONFIG.TRAIN, the sampled rois and roi_labels of assign_targets replace them in
        batch_dict, and forward_ret_dict = the targets + rcnn_cls / rcnn_reg (fp32) for get_loss(); needs gt_boxes.  A head
        without the sampler's settings raises NotImplementedError."""
        if self.training and not self.has_training_half:
            self._require_training_half('PointRCNNHead')
        self.proposal_layer(batch_dict, nms_config=self.model_cfg.NMS_CONFIG['TRAIN' if self.training else 'TEST'])
        targets_dict = None
        if self.training:
            targets_dict = self.assign_targets(batch_dict)
            batch_dict['rois'] = targets_dict['rois']
            batch_dict['roi_labels'] = targets_dict['roi_labels']
        shared = self._roi_features(self.roipool3d_gpu(batch_dict))
        rcnn_cls = self.cls_layers(shared).squeeze(2)
        rcnn_reg = self.reg_layers(shared).squeeze(2)
        if self.training:
            targets_dict['rcnn_cls'] = rcnn_cls.float()
            targets_dict['rcnn_reg'] = rcnn_reg.float()
            self.forward_ret_dict = targets_dict
            return batch_dict
        cls, boxes = self.generate_predicted_boxes(batch_size=batch_dict['batch_size'], rois=batch_dict['rois'],
                                                   cls_preds=rcnn_cls, box_preds=rcnn_reg)
        batch_dict.update(rcnn_cls=rcnn_cls, rcnn_reg=rcnn_reg, batch_cls_preds=cls, batch_box_preds=boxes,
                          cls_preds_normalized=False)
        return batch_dict

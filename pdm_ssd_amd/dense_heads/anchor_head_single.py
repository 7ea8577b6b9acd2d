"""AnchorHeadSingle: three 1x1 convolutions on the BEV map (class logits, box codes, direction bins) over one anchor table,
the reference's pcdet/models/dense_heads/anchor_head_single.py.  state_dict keys conv_cls, conv_box, conv_dir_cls.

The reference permutes each conv output to (B, H, W, C) and copies it; here the outputs stay as the convolutions leave them
and the loss and decode operators index them by channel (anchor_head_ops.py)."""
import numpy as np
import torch.nn as nn

from .anchor_head_template import AnchorHeadTemplate
from .point_head_template import _get


class AnchorHeadSingle(AnchorHeadTemplate):
    def __init__(self, model_cfg, input_channels, num_class, class_names, grid_size, point_cloud_range,
                 predict_boxes_when_training=True, **kwargs):
        super().__init__(model_cfg=model_cfg, num_class=num_class, class_names=class_names, grid_size=grid_size,
                         point_cloud_range=point_cloud_range, predict_boxes_when_training=predict_boxes_when_training)
        self.num_anchors_per_location = sum(self.num_anchors_per_location)
        self.conv_cls = nn.Conv2d(input_channels, self.num_anchors_per_location * self.num_class, kernel_size=1)
        self.conv_box = nn.Conv2d(input_channels, self.num_anchors_per_location * self.box_coder.code_size, kernel_size=1)
        if _get(self.model_cfg, 'USE_DIRECTION_CLASSIFIER', None) is not None:
            self.conv_dir_cls = nn.Conv2d(input_channels, self.num_anchors_per_location * _get(self.model_cfg, 'NUM_DIR_BINS'), kernel_size=1)
        else:
            self.conv_dir_cls = None
        self.init_weights()

    def init_weights(self, prior=0.01):
        """class logits start at the prior probability 0.01 (bias = logit(prior)); box codes start near zero"""
        nn.init.constant_(self.conv_cls.bias, float(np.log(prior / (1 - prior))))
        nn.init.normal_(self.conv_box.weight, mean=0.0, std=1e-3)

    def forward(self, data_dict):
        spatial_features_2d = data_dict['spatial_features_2d']
        cls_preds = self.conv_cls(spatial_features_2d)               # (B, A_loc * num_class, H, W): kept as it is
        box_preds = self.conv_box(spatial_features_2d)
        dir_cls_preds = self.conv_dir_cls(spatial_features_2d) if self.conv_dir_cls is not None else None
        self.forward_ret_dict['cls_preds'] = cls_preds
        self.forward_ret_dict['box_preds'] = box_preds
        if dir_cls_preds is not None:
            self.forward_ret_dict['dir_cls_preds'] = dir_cls_preds
        else:
            self.forward_ret_dict.pop('dir_cls_preds', None)
        if self.training:
            self.forward_ret_dict.update(self.assign_targets(gt_boxes=data_dict['gt_boxes']))
        if not self.training or self.predict_boxes_when_training:
            batch_cls_preds, batch_box_preds = self.generate_predicted_boxes(
                batch_size=data_dict['batch_size'], cls_preds=cls_preds, box_preds=box_preds, dir_cls_preds=dir_cls_preds)
            data_dict['batch_cls_preds'] = batch_cls_preds
            data_dict['batch_box_preds'] = batch_box_preds
            data_dict['cls_preds_normalized'] = False
        return data_dict

"""Part-A2's point head: constructor signature, config keys (CLS_FC, PART_FC, REG_FC, TARGET_CONFIG.BOX_CODER) and state_dict
keys (`cls_layers.*`, `part_reg_layers.*`, `box_layers.*`) of the reference's pcdet/models/dense_heads/point_intra_part_head.py
(PointIntraPartOffsetHead), the eval forward only: per point (a voxel centre of UNetV2) the foreground score point_cls_scores
(N,), the largest sigmoid over the classes, and the intra-object part location point_part_offset (N, 3) in [0, 1]; with a
BOX_CODER also per-point boxes.  Training (part targets, the part loss) is not built: assign_targets / get_loss raise
NotImplementedError.
"""
import torch

from ..utils import box_coder_utils
from .point_head_template import PointHeadTemplate, _get

NEXT_STEP = ('PointIntraPartOffsetHead runs in eval mode only: the intra-object part targets and the part loss are not built')


class PointIntraPartOffsetHead(PointHeadTemplate):
    def __init__(self, num_class, input_channels, model_cfg, predict_boxes_when_training=False, **kwargs):
        super().__init__(model_cfg=model_cfg, num_class=num_class)
        self.predict_boxes_when_training = predict_boxes_when_training
        self.cls_layers = self.make_fc_layers(fc_cfg=_get(self.model_cfg, 'CLS_FC'), input_channels=input_channels, output_channels=num_class)
        self.part_reg_layers = self.make_fc_layers(fc_cfg=_get(self.model_cfg, 'PART_FC'), input_channels=input_channels, output_channels=3)
        target_cfg = _get(self.model_cfg, 'TARGET_CONFIG')
        if _get(target_cfg, 'BOX_CODER', None) is not None:
            self.box_coder = getattr(box_coder_utils, _get(target_cfg, 'BOX_CODER'))(**_get(target_cfg, 'BOX_CODER_CONFIG'))
            self.box_layers = self.make_fc_layers(fc_cfg=_get(self.model_cfg, 'REG_FC'), input_channels=input_channels,
                                                  output_channels=self.box_coder.code_size)
        else:
            self.box_layers = None

    def assign_targets(self, input_dict):
        raise NotImplementedError(NEXT_STEP)

    def get_loss(self, tb_dict=None):
        raise NotImplementedError(NEXT_STEP)

    def forward(self, batch_dict):
        """point_features (N, C), point_coords (N, 4) -> point_cls_scores (N,), point_part_offset (N, 3)"""
        if self.training:
            raise NotImplementedError(NEXT_STEP)
        point_features = batch_dict['point_features']
        point_cls_preds = self.cls_layers(point_features)
        point_part_preds = self.part_reg_layers(point_features)
        ret_dict = {'point_cls_preds': point_cls_preds, 'point_part_preds': point_part_preds}
        batch_dict['point_cls_scores'] = torch.sigmoid(point_cls_preds).max(dim=-1)[0]
        batch_dict['point_part_offset'] = torch.sigmoid(point_part_preds)
        if self.box_layers is not None:
            ret_dict['point_box_preds'] = self.box_layers(point_features)
            cls, boxes = self.generate_predicted_boxes(points=batch_dict['point_coords'][:, 1:4], point_cls_preds=point_cls_preds,
                                                       point_box_preds=ret_dict['point_box_preds'])
            batch_dict.update(batch_cls_preds=cls, batch_box_preds=boxes, batch_index=batch_dict['point_coords'][:, 0],
                              cls_preds_normalized=False)
        self.forward_ret_dict = ret_dict
        return batch_dict

"""PV-RCNN's keypoint segmentation head: constructor signature, config keys (CLS_FC, USE_POINT_FEATURES_BEFORE_FUSION) and
state_dict keys (`cls_layers.*`) of the reference's pcdet/models/dense_heads/point_head_simple.py (PointHeadSimple), the eval
forward only: point_cls_preds (N, num_class) logits and point_cls_scores (N,), the sigmoid of the largest logit (the
reference takes the largest sigmoid: the same number, the sigmoid being monotonic), which weighs the keypoint features in the
RoI-grid pooling.  In eval mode without autograd the stack runs as one per-row fp32 MFMA launch (pdm_rows_mlp_fused, BatchNorm
folded), as PointHeadBox's does.  Training (point targets and the focal loss on them) is not built: NotImplementedError.
"""
import torch

from .. import fused
from .point_head_box import _fc_layers
from .point_head_template import PointHeadTemplate, _get


class PointHeadSimple(PointHeadTemplate):
    def __init__(self, num_class, input_channels, model_cfg, **kwargs):
        super().__init__(model_cfg=model_cfg, num_class=num_class)
        self.cls_layers = self.make_fc_layers(fc_cfg=_get(self.model_cfg, 'CLS_FC'), input_channels=input_channels,
                                              output_channels=num_class)

    def _cls(self, point_features):
        if (not torch.is_grad_enabled() and point_features.is_cuda and point_features.dtype == torch.float32
                and point_features.dim() == 2 and getattr(self, 'use_fused', True)):
            pk = fused.cached_layers(self, 'cls', self.cls_layers, lambda: _fc_layers(self.cls_layers), point_features.device)
            if pk is not None:
                rows = point_features.contiguous().unsqueeze(0)
                out = torch.empty((1, rows.shape[1], (self.num_class + 3) // 4 * 4), dtype=torch.float32, device=rows.device)
                fused.rows_forward(pk, rows, out, relu_last=False)
                return out[0, :, :self.num_class]
        return self.cls_layers(point_features)

    def forward(self, batch_dict):
        """point_features (N, C) or, with USE_POINT_FEATURES_BEFORE_FUSION, point_features_before_fusion -> point_cls_scores (N,)"""
        if self.training:
            raise NotImplementedError('PointHeadSimple runs in eval mode only: its point targets and loss are not built')
        key = 'point_features_before_fusion' if _get(self.model_cfg, 'USE_POINT_FEATURES_BEFORE_FUSION', False) else 'point_features'
        point_cls_preds = self._cls(batch_dict[key])
        batch_dict['point_cls_scores'] = torch.sigmoid(point_cls_preds.max(dim=-1)[0])
        self.forward_ret_dict = {'point_cls_preds': point_cls_preds}
        return batch_dict

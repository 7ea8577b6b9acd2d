"""Base class of the RoI heads: the inference half of /root/reference/pcdet/models/roi_heads/roi_head_template.py, restated —
make_fc_layers (:29-43), proposal_layer (:45-102) and generate_predicted_boxes (:233-261) with the reference's names,
arguments, batch_dict keys and state_dict keys.  ProposalTargetLayer, the target canonicalisation and the rcnn losses
(:104-231) are not built: a RoI head here runs in eval mode only.
"""
import torch
import torch.nn as nn

from ..iou3d_nms.iou3d_nms_utils import class_agnostic_nms
from ..utils import box_coder_utils
from ..utils.common_utils import rotate_points_along_z


def _get(cfg, key, default=None):
    return cfg.get(key, default) if isinstance(cfg, dict) else getattr(cfg, key, default)


class RoIHeadTemplate(nn.Module):
    def __init__(self, num_class, model_cfg, **kwargs):
        super().__init__()
        self.model_cfg = model_cfg
        self.num_class = num_class
        target_cfg = _get(model_cfg, 'TARGET_CONFIG')
        coder = getattr(box_coder_utils, _get(target_cfg, 'BOX_CODER'))
        self.box_coder = coder(**(_get(target_cfg, 'BOX_CODER_CONFIG', None) or {}))
        self.forward_ret_dict = None

    def make_fc_layers(self, input_channels, output_channels, fc_list):
        """A per-RoI MLP over (rois, channels, 1): [Conv1d(k=1, no bias), BatchNorm1d, ReLU] per width of fc_list, then a
        biased Conv1d to output_channels.  With DP_RATIO >= 0 a Dropout follows the FIRST block; it holds no parameter but
        shifts the indices of the children behind it, and with them the reference's state_dict keys."""
        drop = _get(self.model_cfg, 'DP_RATIO')
        layers, width = [], input_channels
        for depth, hidden in enumerate(fc_list):
            layers += [nn.Conv1d(width, hidden, kernel_size=1, bias=False), nn.BatchNorm1d(hidden), nn.ReLU()]
            if depth == 0 and drop >= 0:
                layers.append(nn.Dropout(drop))
            width = hidden
        layers.append(nn.Conv1d(width, output_channels, kernel_size=1, bias=True))
        return nn.Sequential(*layers)

    @torch.no_grad()
    def proposal_layer(self, batch_dict, nms_config):
        """First-stage predictions -> at most NMS_POST_MAXSIZE proposals per sample.

        Reads batch_cls_preds (B, n, num_class | 1) and batch_box_preds (B, n, 7 + C), or both stacked over the samples,
        (N1 + N2 + ..., ..), with batch_index (N1 + N2 + ...).  Per sample: best class per box, class_agnostic_nms on the
        raw scores (no score threshold), survivors in NMS order.  Writes rois (B, NMS_POST_MAXSIZE, 7 + C), roi_scores
        (B, ..) and roi_labels (B, ..) int64 = best class + 1, with zero rows (label 1, as the reference) behind each
        sample's survivors, has_class_labels = more than one class column, and removes batch_index.  A batch_dict that
        already holds rois is returned untouched.  MULTI_CLASSES_NMS is not implemented, as in the reference."""
        if batch_dict.get('rois', None) is not None:
            return batch_dict
        if _get(nms_config, 'MULTI_CLASSES_NMS'):
            raise NotImplementedError('proposal_layer: MULTI_CLASSES_NMS')
        all_boxes, all_logits = batch_dict['batch_box_preds'], batch_dict['batch_cls_preds']
        sample_of_row = batch_dict.get('batch_index', None)
        stacked = sample_of_row is not None
        assert all_logits.dim() == (2 if stacked else 3)
        num_samples, room = batch_dict['batch_size'], int(_get(nms_config, 'NMS_POST_MAXSIZE'))
        rois = all_boxes.new_zeros((num_samples, room, all_boxes.shape[-1]))
        roi_scores = all_boxes.new_zeros((num_samples, room))
        roi_classes = torch.zeros((num_samples, room), dtype=torch.long, device=all_boxes.device)
        for b in range(num_samples):
            rows = (sample_of_row == b) if stacked else b
            boxes, logits = all_boxes[rows], all_logits[rows]
            best, best_class = logits.max(dim=1)
            kept, _ = class_agnostic_nms(box_scores=best, box_preds=boxes, nms_config=nms_config)
            k = kept.numel()
            rois[b, :k] = boxes[kept]
            roi_scores[b, :k] = best[kept]
            roi_classes[b, :k] = best_class[kept]
        batch_dict.update(rois=rois, roi_scores=roi_scores, roi_labels=roi_classes + 1,
                          has_class_labels=bool(all_logits.shape[-1] > 1))
        batch_dict.pop('batch_index', None)
        return batch_dict

    def generate_predicted_boxes(self, batch_size, rois, cls_preds, box_preds):
        """rois (B, N, 7 [+ C]), cls_preds (B N, num_class | 1), box_preds (B N, code_size) -> batch_cls_preds
        (B, N, num_class | 1), batch_box_preds (B, N, code_size).  The codes are relative to each RoI's own frame: decode
        them against the RoI moved to the origin, turn the result by the RoI's heading about z, move it to the RoI's
        centre."""
        width = self.box_coder.code_size
        at_origin = rois.detach().clone()
        at_origin[..., 0:3] = 0
        local = self.box_coder.decode_torch(box_preds.view(batch_size, -1, width), at_origin).view(-1, 1, width)
        boxes = rotate_points_along_z(local, rois[..., 6].reshape(-1)).view(-1, width)
        boxes[:, 0:3] += rois[..., 0:3].reshape(-1, 3)
        return cls_preds.view(batch_size, -1, cls_preds.shape[-1]), boxes.view(batch_size, -1, width)

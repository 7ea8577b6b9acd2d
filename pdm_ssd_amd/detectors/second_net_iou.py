"""SECONDNetIoU: SECOND's front (dynamic mean VFE -> sparse 3-D backbone -> height compression -> 2-D backbone -> anchor head) and
SECONDHead, which predicts each proposal's IoU with its object from a crop of the 2-D map: the forward and get_training_loss of
the reference's pcdet/models/detectors/second_net_iou.py on this repository's template (as VoxelRCNN's here), and its own
post_processing, restated: the proposals keep their boxes and are re-scored before the final NMS.

POST_PROCESSING.NMS_CONFIG.SCORE_TYPE picks the score the NMS ranks and the threshold cuts:
  None / 'iou'         sigmoid of the head's IoU logit
  'cls'                sigmoid of the first stage's score (roi_scores)
  'weighted_iou_cls'   SCORE_WEIGHTS.iou * iou + SCORE_WEIGHTS.cls * cls
  'score_by_class'     per class NAME 'iou' or 'cls' from NMS_CONFIG.SCORE_BY_CLASS
Two departures from the reference, both on purpose:
  * 'score_by_class' walks all num_class classes.  The reference walks range(torch.unique(labels).shape[0]): with labels {1, 3}
    present it serves classes 1 and 2 and leaves class 3's boxes at score 0, and the unique() costs a host read.
  * 'num_pts_iou_cls' raises NotImplementedError: the reference counts the points in each box on the CPU per sample and its
    interpolation hard-codes a 10 where the configured threshold belongs.
MULTI_CLASSES_NMS and OUTPUT_RAW_SCORE raise NotImplementedError, as in the reference.
"""
import torch

from ..iou3d_nms.iou3d_nms_utils import class_agnostic_nms
from .detector3d_template import Detector3DTemplate, _get


class SECONDNetIoU(Detector3DTemplate):
    def __init__(self, model_cfg, num_class, dataset):
        super().__init__(model_cfg=model_cfg, num_class=num_class, dataset=dataset)
        self.module_list = self.build_networks()

    def forward(self, batch_dict):
        """eval: (pred_dicts, recall_dict); training: ({'loss': loss}, tb_dict, disp_dict)"""
        from .. import fused_bn
        with fused_bn.counter_scope():      # the BatchNorm step counters of every stack: one multi-tensor add
            for cur_module in self.module_list:
                batch_dict = cur_module(batch_dict)
        if self.training:
            loss, tb_dict, disp_dict = self.get_training_loss()
            return {'loss': loss}, tb_dict, disp_dict
        return self.post_processing(batch_dict)

    def get_training_loss(self):
        disp_dict = {}
        loss_rpn, tb_dict = self.dense_head.get_loss()
        loss_rcnn, tb_dict = self.roi_head.get_loss(tb_dict)
        return loss_rpn + loss_rcnn, tb_dict, disp_dict

    @staticmethod
    def set_nms_score_by_class(iou_preds, cls_preds, label_preds, score_by_class, class_names):
        """per box the IoU score or the first stage's score, as SCORE_BY_CLASS says for the class NAME of its label (1-based);
        every class is served whether or not the sample holds a box of it; a label outside 1 .. len(class_names) keeps 0"""
        nms_scores = torch.zeros_like(iou_preds)
        for k, name in enumerate(class_names):
            kind = _get(score_by_class, name)
            if kind not in ('iou', 'cls'):
                raise NotImplementedError(f'SCORE_BY_CLASS[{name!r}] = {kind!r}')
            nms_scores = torch.where(label_preds == k + 1, iou_preds if kind == 'iou' else cls_preds, nms_scores)
        return nms_scores

    @classmethod
    def nms_scores(cls, iou_preds, cls_preds, label_preds, nms_cfg, class_names):
        """the score rule of NMS_CONFIG.SCORE_TYPE (module docstring) on (N,) sigmoid scores and 1-based labels"""
        kind = _get(nms_cfg, 'SCORE_TYPE', None)
        if kind == 'score_by_class' and _get(nms_cfg, 'SCORE_BY_CLASS', None):
            return cls.set_nms_score_by_class(iou_preds, cls_preds, label_preds, _get(nms_cfg, 'SCORE_BY_CLASS'), class_names)
        if kind is None or kind == 'iou':
            return iou_preds
        if kind == 'cls':
            return cls_preds
        if kind == 'weighted_iou_cls':
            weights = _get(nms_cfg, 'SCORE_WEIGHTS')
            return _get(weights, 'iou') * iou_preds + _get(weights, 'cls') * cls_preds
        if kind == 'num_pts_iou_cls':
            raise NotImplementedError("SCORE_TYPE 'num_pts_iou_cls': the reference counts points per box on the CPU and hard-codes "
                                      "one of its thresholds; not restated here")
        raise NotImplementedError(f'SCORE_TYPE {kind!r}')

    def post_processing(self, batch_dict):
        """batch_cls_preds (B, n, 1) IoU logits, batch_box_preds (B, n, 7 + C) = rois, roi_scores (B, n), roi_labels (B, n) ->
        ([{'pred_boxes', 'pred_scores', 'pred_labels', 'pred_cls_scores', 'pred_iou_scores'}] per sample, recall_dict): sigmoid of
        both scores (unless cls_preds_normalized), the label from roi_labels under has_class_labels, the score rule,
        class_agnostic_nms above SCORE_THRESH, recall of the rois and of the kept boxes against gt_boxes when present."""
        cfg = _get(self.model_cfg, 'POST_PROCESSING')
        nms_cfg = _get(cfg, 'NMS_CONFIG')
        if _get(nms_cfg, 'MULTI_CLASSES_NMS', False):
            raise NotImplementedError('SECONDNetIoU.post_processing: MULTI_CLASSES_NMS')
        if _get(cfg, 'OUTPUT_RAW_SCORE', False):
            raise NotImplementedError('SECONDNetIoU.post_processing: OUTPUT_RAW_SCORE')
        recall_dict, pred_dicts = {}, []
        for index in range(batch_dict['batch_size']):
            if batch_dict.get('batch_index', None) is not None:
                assert batch_dict['batch_cls_preds'].dim() == 2
                batch_mask = batch_dict['batch_index'] == index
            else:
                assert batch_dict['batch_cls_preds'].dim() == 3
                batch_mask = index
            box_preds = batch_dict['batch_box_preds'][batch_mask]
            iou_preds = batch_dict['batch_cls_preds'][batch_mask]
            cls_preds = batch_dict['roi_scores'][batch_mask]
            assert iou_preds.shape[1] in [1, self.num_class]
            if not batch_dict['cls_preds_normalized']:
                iou_preds, cls_preds = torch.sigmoid(iou_preds), torch.sigmoid(cls_preds)
            iou_preds, label_preds = torch.max(iou_preds, dim=-1)
            label_preds = batch_dict['roi_labels'][index] if batch_dict.get('has_class_labels', False) else label_preds + 1
            scores = self.nms_scores(iou_preds, cls_preds, label_preds, nms_cfg, self.class_names)
            selected, selected_scores = class_agnostic_nms(box_scores=scores, box_preds=box_preds, nms_config=nms_cfg,
                                                           score_thresh=_get(cfg, 'SCORE_THRESH'))
            final_boxes = box_preds[selected]
            recall_dict = self.generate_recall_record(
                box_preds=final_boxes if 'rois' not in batch_dict else box_preds, recall_dict=recall_dict, batch_index=index,
                data_dict=batch_dict, thresh_list=_get(cfg, 'RECALL_THRESH_LIST'))
            pred_dicts.append({'pred_boxes': final_boxes, 'pred_scores': selected_scores, 'pred_labels': label_preds[selected],
                               'pred_cls_scores': cls_preds[selected], 'pred_iou_scores': iou_preds[selected]})
        return pred_dicts, recall_dict

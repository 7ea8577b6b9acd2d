"""HungarianAssigner3D (the reference's pcdet/models/dense_heads/target_assigner/hungarian_assigner.py): one sample's
one-to-one assignment of ground-truth boxes to TransFusion queries, on transfusion_ops.

The costs are the reference's (transfusion_ops.cost_torch): the focal cost at the gt's class, the L1 distance of the
range-normalised centres and minus the 3-D IoU of overlaps(), which reads z as the box's BOTTOM; each times its weight.
The matching runs where the boxes live: pdm_lsap on the GPU (no host read), the numpy solver lsap_host on the CPU; the
reference copies the cost to the host and calls scipy's linear_sum_assignment.  The two agree wherever the optimum is
unique; equal totals are broken by the lower index here, and a cost that is not finite is read as FLT_MAX, where scipy
raises.  TransFusionHead does not come through here on the GPU: transfusion_ops.assign does the whole batch at once.
"""
import torch

from ... import transfusion_ops


class HungarianAssigner3D:
    def __init__(self, cls_cost, reg_cost, iou_cost):
        self.cls_cost, self.reg_cost, self.iou_cost = dict(cls_cost), dict(reg_cost), dict(iou_cost)

    @torch.no_grad()
    def assign(self, bboxes, gt_bboxes, gt_labels, cls_pred, point_cloud_range):
        """bboxes (P, 7 | 9) decoded queries, gt_bboxes (G, 7 | 9), gt_labels (G) 0-based, cls_pred (1, C, P) logits ->
        assigned_gt_inds (P) int64 (0 = background, g + 1 = box g), max_overlaps (P) (the matched pair's IoU, else 0)"""
        P, G = bboxes.shape[0], gt_bboxes.shape[0]
        assigned = bboxes.new_zeros((P,), dtype=torch.long)
        max_overlaps = bboxes.new_zeros((P,))
        if P == 0 or G == 0:
            return assigned, max_overlaps
        cost, iou = transfusion_ops.cost_torch(bboxes, gt_bboxes, gt_labels.long(), cls_pred[0], point_cloud_range, self.cls_cost,
                                               self.reg_cost, self.iou_cost)
        if cost.is_cuda:
            num_gt = torch.full((1,), G, dtype=torch.int32, device=cost.device)
            gt_of_row = transfusion_ops.lsap(cost[None].float(), num_gt)[0][0].long()
        else:
            gt_of_row = torch.from_numpy(transfusion_ops.lsap_host(cost.numpy())[0]).long()
        pos = gt_of_row >= 0
        assigned[pos] = gt_of_row[pos] + 1
        max_overlaps[pos] = iou[pos, gt_of_row[pos]]
        return assigned, max_overlaps

"""AxisAlignedTargetAssigner: anchors x ground-truth boxes -> labels, regression targets and weights, the rules of the
reference's pcdet/models/dense_heads/target_assigner/axis_aligned_target_assigner.py (DESIGN.md "Anchor head" lists them).

On GPU tensors assign_targets is pdm_anchor_targets (anchor_head_ops.py): one launch chain for the batch, no host read, no
(anchors x boxes) matrix.  On CPU tensors it is the torch formulation below, which follows the reference's algorithm per
sample and anchor set; it is the CPU path and what the tests compare the kernels with.

Refused with NotImplementedError: POS_FRACTION >= 0 (random subsampling), USE_MULTIHEAD, MATCH_HEIGHT (3-D IoU matching).
"""
import torch

from ...utils import box_utils
from .anchor_generator import _get


class AxisAlignedTargetAssigner(object):
    def __init__(self, model_cfg, class_names, box_coder, match_height=False):
        super().__init__()
        anchor_generator_cfg = _get(model_cfg, 'ANCHOR_GENERATOR_CONFIG')
        anchor_target_cfg = _get(model_cfg, 'TARGET_ASSIGNER_CONFIG')
        self.box_coder = box_coder
        self.match_height = match_height
        self.class_names = list(class_names)
        self.anchor_class_names = [_get(config, 'class_name') for config in anchor_generator_cfg]
        pos_fraction = _get(anchor_target_cfg, 'POS_FRACTION', -1.0)
        if pos_fraction is not None and pos_fraction >= 0:
            raise NotImplementedError(f'AxisAlignedTargetAssigner: POS_FRACTION {pos_fraction} >= 0 (random subsampling) is not supported')
        if match_height:
            raise NotImplementedError('AxisAlignedTargetAssigner: MATCH_HEIGHT (3-D IoU matching) is not supported')
        self.use_multihead = _get(model_cfg, 'USE_MULTIHEAD', False)
        if self.use_multihead:
            raise NotImplementedError('AxisAlignedTargetAssigner: USE_MULTIHEAD is not supported')
        assert box_coder.code_size == 7, 'AxisAlignedTargetAssigner: a 7-column ResidualCoder'
        assert len(set(self.anchor_class_names)) == len(self.anchor_class_names), 'one anchor set per class name'
        self.pos_fraction = None
        self.sample_size = _get(anchor_target_cfg, 'SAMPLE_SIZE', 512)
        self.norm_by_num_examples = bool(_get(anchor_target_cfg, 'NORM_BY_NUM_EXAMPLES', False))
        self.matched_thresholds = {_get(c, 'class_name'): _get(c, 'matched_threshold') for c in anchor_generator_cfg}
        self.unmatched_thresholds = {_get(c, 'class_name'): _get(c, 'unmatched_threshold') for c in anchor_generator_cfg}
        self.use_fused = True                       # False: the torch formulation on any device

    # ---- the device operator's tables -----------------------------------------------------------------------------------
    def set_of_class(self):
        """[g] = the anchor set of global class g (1-based; [0] unused) or -1"""
        return [-1] + [self.anchor_class_names.index(n) if n in self.anchor_class_names else -1 for n in self.class_names]

    @staticmethod
    def set_of_slot(all_anchors):
        """the anchor set of each of the anchors of one location, in torch.cat(all_anchors, dim=-3)'s order"""
        return [s for s, anchors in enumerate(all_anchors) for _ in range(anchors.shape[-3] * anchors.shape[-2])]

    def assign_targets(self, all_anchors, gt_boxes_with_classes, flat_anchors=None):
        """all_anchors: per anchor set a (1, ny, nx, #sizes, #rotations, 7) table; gt_boxes_with_classes (B, M, 8), global class
        (1-based, 0 = padding) last, left untouched -> {'box_cls_labels' (B, A) int32, 'box_reg_targets' (B, A, 7),
        'reg_weights' (B, A), 'num_pos' (B) int32 = #labels > 0}; anchors in the order y, x, set, size, rotation.
        flat_anchors: torch.cat(all_anchors, dim=-3).view(-1, 7) where the caller keeps it (the head does), else built here."""
        gt = gt_boxes_with_classes
        if gt.is_cuda and self.use_fused:
            from ... import anchor_head_ops
            flat = flat_anchors if flat_anchors is not None else torch.cat(all_anchors, dim=-3).view(-1, 7)
            flat = flat.to(gt.device)
            thresholds = [[float(t[n]) for n in self.anchor_class_names] for t in (self.matched_thresholds, self.unmatched_thresholds)]
            labels, targets, weights, num_pos = anchor_head_ops.anchor_targets(
                flat, self.set_of_slot(all_anchors), self.set_of_class(), thresholds[0], thresholds[1], gt, self.norm_by_num_examples)
        else:
            per_sample = [self.assign_targets_sample(all_anchors, gt[k].float()) for k in range(gt.shape[0])]
            labels, targets, weights = (torch.stack(x, dim=0) for x in zip(*per_sample))
            num_pos = (labels > 0).sum(dim=1).int()
        return {'box_cls_labels': labels, 'box_reg_targets': targets, 'reg_weights': weights, 'num_pos': num_pos}

    def assign_targets_sample(self, all_anchors, gt):
        """one sample: gt (M, 8).  A box takes part only with a class in 1 .. #classes, against the anchors of its class's set
        (the reference trims trailing zero rows and sends a class-0 row to the last class, where its IoU of 0 with everything
        leaves it inert: same labels)."""
        cls = gt[:, -1].int()
        table = torch.tensor(self.set_of_class(), dtype=torch.int64, device=gt.device)
        valid = (gt[:, -1] >= 1) & (gt[:, -1] < len(self.class_names) + 1)
        set_of_box = torch.where(valid, table[cls.long().clamp(0, len(self.class_names))], torch.full_like(cls, -1, dtype=torch.int64))
        outs = []
        for s, (name, anchors) in enumerate(zip(self.anchor_class_names, all_anchors)):
            shape = anchors.shape[:3]
            mine = set_of_box == s
            single = self.assign_targets_single(anchors.reshape(-1, anchors.shape[-1]).to(gt.device), gt[mine, :7], cls[mine],
                                                self.matched_thresholds[name], self.unmatched_thresholds[name])
            outs.append((single[0].view(*shape, -1), single[1].view(*shape, -1, 7), single[2].view(*shape, -1)))
        return (torch.cat([o[0] for o in outs], dim=-1).view(-1), torch.cat([o[1] for o in outs], dim=-2).view(-1, 7),
                torch.cat([o[2] for o in outs], dim=-1).view(-1))

    def assign_targets_single(self, anchors, gt_boxes, gt_classes, matched_threshold=0.6, unmatched_threshold=0.45):
        """anchors (N, 7) of one set, gt_boxes (n, 7) and gt_classes (n) of its class -> labels (N) int32, targets (N, 7),
        weights (N).  Per anchor the best box (the lowest index among equals); per box the best IoU over the anchors, a best
        of exactly 0 meaning none; an anchor whose IoU with any box equals that box's best is forced positive, with the label
        and target of its OWN best box; otherwise IoU >= matched: positive, < unmatched: 0, else -1."""
        num_anchors, num_gt = anchors.shape[0], gt_boxes.shape[0]
        labels = torch.zeros((num_anchors,), dtype=torch.int32, device=anchors.device)
        targets = anchors.new_zeros((num_anchors, self.box_coder.code_size))
        weights = anchors.new_zeros((num_anchors,))
        if num_gt > 0 and num_anchors > 0:
            overlap = box_utils.boxes3d_nearest_bev_iou(anchors[:, 0:7], gt_boxes[:, 0:7])
            anchor_max, anchor_argmax = overlap.max(dim=1)
            gt_max = overlap.max(dim=0)[0]
            gt_max = torch.where(gt_max == 0, torch.full_like(gt_max, -1.0), gt_max)
            forced = (overlap == gt_max).any(dim=1)
            own = gt_classes[anchor_argmax].int()
            labels = torch.full_like(labels, -1)
            labels = torch.where(anchor_max >= matched_threshold, own, labels)
            labels = torch.where(anchor_max < unmatched_threshold, torch.zeros_like(labels), labels)
            labels = torch.where(forced, own, labels)
            fg = labels > 0
            code = self.box_coder.encode_torch(gt_boxes[anchor_argmax].clone(), anchors.clone())
            targets = torch.where(fg[:, None], code, targets)
        fg = labels > 0
        if self.norm_by_num_examples:
            weights = fg.float() / (labels >= 0).sum().clamp(min=1).float()
        else:
            weights = fg.float()
        return labels, targets, weights

"""ProposalTargetLayer: constructor, config keys, batch_dict keys and the seven result keys of
/root/reference/pcdet/models/roi_heads/target_assigner/proposal_target_layer.py, restated over ONE device operator
(pdm_proposal_targets, csrc/roi_targets.hip) for the whole batch.  The reference loops over the samples and, inside,
over the classes with `.item()` reads, builds a rois x boxes IoU matrix per class, calls nonzero and draws from the
host's numpy and torch RNGs; here there is no host read at all, so the step can be captured in a graph.

What differs from the reference, all of it written down in csrc/roi_targets.hip:
  * the draws are functions of (seed, step, sample, purpose, slot) instead of the global RNGs: `seed` is given at
    construction, the step counter lives on the device and is advanced by every call;
  * a RoI whose best IoU is reached by several ground-truth boxes is assigned the first of them;
  * a sample with neither foreground nor background RoIs (NaN overlaps) does not raise by itself: the operator sets a
    flag on the device and fills the sample's slots with RoI 0.  `check=True` reads the flag after every call (one
    synchronisation) and raises, as the reference does; the default leaves it to `raise_if_failed()`.
Only box code size 7 is built: wider rois or ground truth raise ValueError.
"""
import numpy as np
import torch
import torch.nn as nn

from ... import roi_targets


def _get(cfg, key, default=None):
    return cfg.get(key, default) if isinstance(cfg, dict) else getattr(cfg, key, default)


class ProposalTargetLayer(nn.Module):
    def __init__(self, roi_sampler_cfg, seed=0, check=False):
        super().__init__()
        self.roi_sampler_cfg = roi_sampler_cfg
        self.seed = int(seed)
        self.check = bool(check)
        self._state = None          # int32 [step, error flag] on the device of the first call

    def state(self, device):
        if self._state is None or self._state.device != device:
            self._state = roi_targets.new_state(device)
        return self._state

    def raise_if_failed(self):
        """Synchronises; raises if any call so far met a sample with neither foreground nor background RoIs."""
        if self._state is not None and int(self._state[1].item()) != 0:
            raise NotImplementedError('ProposalTargetLayer: a sample had neither foreground nor background RoIs '
                                      '(NaN overlaps); its sampled RoIs are invalid')

    def forward(self, batch_dict, with_canonical=False):
        """batch_size, rois (B, num_rois, 7), roi_scores (B, num_rois), roi_labels (B, num_rois), gt_boxes (B, N, 7 + 1) ->
        targets_dict: rois (B, M, 7), gt_of_rois (B, M, 8), gt_iou_of_rois, roi_scores, roi_labels, reg_valid_mask,
        rcnn_cls_labels (B, M), M = ROI_PER_IMAGE.  with_canonical (RoIHeadTemplate.assign_targets): gt_of_rois_src
        holds the ground truth as it was and gt_of_rois its canonical form — the operator forms both anyway."""
        cfg = self.roi_sampler_cfg
        rois, gt_boxes = batch_dict['rois'], batch_dict['gt_boxes']
        if rois.shape[-1] != 7 or gt_boxes.shape[-1] != 8:
            raise ValueError(f'ProposalTargetLayer: rois {tuple(rois.shape)}, gt_boxes {tuple(gt_boxes.shape)}: only box code '
                             'size 7 (gt_boxes with the class as the 8th column) is built')
        per_image = int(_get(cfg, 'ROI_PER_IMAGE'))
        out = roi_targets.proposal_targets(
            rois, batch_dict['roi_scores'], batch_dict['roi_labels'], gt_boxes, roi_per_image=per_image,
            fg_per_image=int(np.round(_get(cfg, 'FG_RATIO') * per_image)), by_class=bool(_get(cfg, 'SAMPLE_ROI_BY_EACH_CLASS', False)),
            hard_bg_ratio=_get(cfg, 'HARD_BG_RATIO'), reg_fg_thresh=_get(cfg, 'REG_FG_THRESH'), cls_fg_thresh=_get(cfg, 'CLS_FG_THRESH'),
            cls_bg_thresh=_get(cfg, 'CLS_BG_THRESH'), cls_bg_thresh_lo=_get(cfg, 'CLS_BG_THRESH_LO'),
            cls_score_type=_get(cfg, 'CLS_SCORE_TYPE'), seed=self.seed, state=self.state(rois.device))
        if self.check:
            self.raise_if_failed()
        targets_dict = {'rois': out['rois'], 'gt_of_rois': out['gt_of_rois'] if with_canonical else out['gt_of_rois_src'],
                        'gt_iou_of_rois': out['gt_iou_of_rois'], 'roi_scores': out['roi_scores'], 'roi_labels': out['roi_labels'],
                        'reg_valid_mask': out['reg_valid_mask'], 'rcnn_cls_labels': out['rcnn_cls_labels']}
        if with_canonical:
            targets_dict['gt_of_rois_src'] = out['gt_of_rois_src']
        self.last_sampled_inds, self.last_gt_assignment = out['sampled_inds'], out['gt_assignment']
        return targets_dict

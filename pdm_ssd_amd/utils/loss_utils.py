"""Losses of the hybrid head.

SigmoidFocalClassificationLoss, WeightedSmoothL1Loss: behaviour of /root/reference/pcdet/utils/loss_utils.py:10-74,
76-141 (point head).  FocalLossCenterNet: :266-345 (heat-map head; the CornerNet penalty-reduced focal loss).
get_corner_loss_lidar: :211-234 (the RoI heads' corner regularisation).
Code weights follow the device of the input instead of being moved to the GPU at construction.
"""
import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import box_utils


class SigmoidFocalClassificationLoss(nn.Module):
    """Focal loss on logits: balance(t) * miss(t, p)^gamma * BCE(x, t) per element, where p = sigmoid(x),
    miss = the probability mass on the wrong side, balance = alpha for positives and 1 - alpha for negatives."""

    def __init__(self, gamma: float = 2.0, alpha: float = 0.25):
        super().__init__()
        self.alpha, self.gamma = alpha, gamma

    @staticmethod
    def sigmoid_cross_entropy_with_logits(input, target):
        """Binary cross entropy of logits in its overflow-free form (kept under the reference's name, :26-43)."""
        return F.binary_cross_entropy_with_logits(input, target, reduction='none')

    def forward(self, input, target, weights):
        """input / target (B, #anchors, #classes) logits / one-hot, weights (B, #anchors) -> unreduced loss."""
        if target.dtype != input.dtype:   # mixed dtypes promote, as the reference's arithmetic form does (lerp would raise)
            dt = torch.promote_types(input.dtype, target.dtype)
            input, target = input.to(dt), target.to(dt)
        p = torch.sigmoid(input)
        miss = torch.lerp(p, 1.0 - p, target)                   # t (1 - p) + (1 - t) p
        balance = (1.0 - self.alpha) + target * (2.0 * self.alpha - 1.0)
        per_elem = balance * miss.pow(self.gamma) * self.sigmoid_cross_entropy_with_logits(input, target)
        if weights.dim() + 1 == per_elem.dim():                  # one weight per anchor: broadcast over the classes
            weights = weights[..., None]
        assert weights.dim() == per_elem.dim()
        return per_elem * weights


def sigmoid_focal_cls_loss(input, target, gamma=2.0, alpha=0.25):
    """SigmoidFocalClassificationLoss per element without weights, as a function: what SECONDHead's IOU_LOSS 'focalbce' calls
    (the reference's second_head.py names loss_utils.sigmoid_focal_cls_loss; its own loss_utils does not define it)."""
    return SigmoidFocalClassificationLoss(gamma=gamma, alpha=alpha)(input, target, torch.ones_like(input))


class WeightedSmoothL1Loss(nn.Module):
    """Huber-style regression loss with the knee at beta (default 1/9): quadratic inside, linear outside; residuals are
    scaled per code before the loss and per anchor after it; a NaN target switches its element off."""

    def __init__(self, beta: float = 1.0 / 9.0, code_weights: list = None):
        super().__init__()
        self.beta = beta
        self.code_weights = None if code_weights is None else torch.from_numpy(np.array(code_weights, dtype=np.float32))

    @staticmethod
    def smooth_l1_loss(diff, beta):
        mag = diff.abs()
        if beta < 1e-5:          # degenerate knee: plain L1
            return mag
        return torch.where(mag < beta, mag * mag * (0.5 / beta), mag - 0.5 * beta)

    def forward(self, input, target, weights=None):
        """input / target (B, #anchors, #codes), weights (B, #anchors) -> (B, #anchors, #codes) unreduced."""
        residual = torch.where(torch.isnan(target), torch.zeros_like(input), input - target)
        if self.code_weights is not None:
            self.code_weights = self.code_weights.to(residual.device)
            residual = residual * self.code_weights
        out = self.smooth_l1_loss(residual, self.beta)
        if weights is not None:
            assert weights.shape[:2] == out.shape[:2]
            out = out * weights[..., None]
        return out


class WeightedCrossEntropyLoss(nn.Module):
    """Cross-entropy with one weight per anchor: input (B, #anchors, #classes) logits; target either (B, #anchors) class
    indices or, as the reference passes it (loss_utils.py:183-208), the same shape as input one-hot; weights (B, #anchors)
    -> (B, #anchors) unreduced."""

    def forward(self, input, target, weights):
        index = target if target.dim() == input.dim() - 1 else target.argmax(dim=-1)
        return F.cross_entropy(input.flatten(0, 1), index.flatten().long(), reduction='none').view_as(weights) * weights


def neg_loss_cornernet(pred, gt, mask=None):
    """Penalty-reduced pixel focal loss of the heat-map head.  pred / gt (B, C, H, W) in (0, 1) / [0, 1]: peaks
    (gt == 1) contribute (1-p)^2 log p, every other cell (1-gt)^4 p^2 log(1-p); the sum is negated and divided by the
    number of peaks (by 1 when there is none, which leaves the negative term alone)."""
    peak = gt == 1
    zero = torch.zeros_like(pred)
    at_peaks = torch.where(peak, (1 - pred).square() * pred.log(), zero)
    elsewhere = torch.where(peak, zero, (1 - gt).pow(4) * pred.square() * (1 - pred).log())
    peaks = peak.to(pred.dtype)
    if mask is not None:
        keep = mask[:, None].to(pred.dtype)
        at_peaks, elsewhere, peaks = at_peaks * keep, elsewhere * keep, peaks * keep
    # (the reference branches on the host, `if num_pos == 0`: a device->host sync per step; same value here)
    return -(at_peaks.sum() + elsewhere.sum()) / peaks.sum().clamp(min=1.0)


class FocalLossCenterNet(nn.Module):
    def forward(self, out, target, mask=None):
        return neg_loss_cornernet(out, target, mask=mask)


def get_corner_loss_lidar(pred_bbox3d, gt_bbox3d):
    """pred_bbox3d, gt_bbox3d (N, 7) -> (N): per box the mean over its 8 corners of smooth_l1(distance, beta = 1), the
    distance of a predicted corner being the lesser of those to the ground truth's corner and to the corner of the
    ground truth turned by pi (a box and its half-turn are the same solid)."""
    assert pred_bbox3d.shape[0] == gt_bbox3d.shape[0]
    pred = box_utils.boxes_to_corners_3d(pred_bbox3d)
    turned = gt_bbox3d.clone()
    turned[:, 6] += np.pi
    dist = torch.min(torch.norm(pred - box_utils.boxes_to_corners_3d(gt_bbox3d), dim=2),
                     torch.norm(pred - box_utils.boxes_to_corners_3d(turned), dim=2))
    return WeightedSmoothL1Loss.smooth_l1_loss(dist, beta=1.0).mean(dim=1)


def _reg_loss(regr, gt_regr, mask):
    """L1 regression loss of the centre head (the reference's loss_utils.py:347-376): regr / gt_regr (B, M, D), mask
    (B, M) -> (D): sum over batch and slots of |regr m - gt m| / max(sum(mask), 1), m = mask * !isnan(gt) per element.
    A NaN target element contributes zero (the reference multiplies the NaN by its zero mask, which stays NaN and
    poisons that code's loss; the evident intent, an element left out, is implemented here and in pdm_center_reg_loss)."""
    num = mask.float().sum()
    m = mask.unsqueeze(2).expand_as(gt_regr).float() * (~torch.isnan(gt_regr)).float()
    gt = torch.where(torch.isnan(gt_regr), torch.zeros_like(gt_regr), gt_regr)
    loss = torch.abs(regr * m - gt * m)
    return loss.sum(dim=(0, 1)) / torch.clamp_min(num, min=1.0)


class RegLossCenterNet(nn.Module):
    def forward(self, output, mask, ind=None, target=None):
        """output (B, D, H, W) maps (gathered at ind (B, M) flat cells) or (B, M, D) predictions; mask (B, M);
        target (B, M, D) -> (D) per-code loss."""
        from .centernet_utils import _transpose_and_gather_feat
        pred = output if ind is None else _transpose_and_gather_feat(output, ind)
        return _reg_loss(pred, target, mask)

"""Second-stage training operators (csrc/roi_targets.hip).

proposal_targets: the reference's ProposalTargetLayer.forward + the canonical transformation of
RoIHeadTemplate.assign_targets for the whole batch — no per-sample loop, no host read, no rois x boxes matrix.
rcnn_loss: the rcnn classification, regression and corner losses with their gradients; the forward pass also leaves
d L / d rcnn_cls and d L / d rcnn_reg, and backward() only scales them by the incoming gradients.
"""
import ctypes

import torch
from torch.autograd import Function

from . import _native

MAX_ROIS, MAX_GT = 1024, 256


def new_state(device):
    """The device-resident state of proposal_targets: int32 [step, error flag]."""
    return torch.zeros(2, dtype=torch.int32, device=device)


def proposal_targets(rois, roi_scores, roi_labels, gt_boxes, roi_per_image, fg_per_image, by_class, hard_bg_ratio,
                     reg_fg_thresh, cls_fg_thresh, cls_bg_thresh, cls_bg_thresh_lo, cls_score_type, seed, state):
    """rois (B, R, 7), roi_scores (B, R), roi_labels (B, R) int64, gt_boxes (B, M, 8) on the GPU -> dict of the sampled
    RoIs and their targets (S = roi_per_image): rois (B, S, 7), roi_labels, roi_scores, gt_iou_of_rois (B, S),
    gt_of_rois_src / gt_of_rois (B, S, 8), reg_valid_mask (B, S) int64, rcnn_cls_labels (B, S) int64 ('cls') or float
    ('roi_iou'), sampled_inds / gt_assignment (B, S) int32.  `state` (new_state) is advanced on the device."""
    if rois.dim() != 3 or rois.shape[-1] != 7:
        raise ValueError(f'proposal_targets: rois of shape {tuple(rois.shape)}; only box code size 7 is built')
    if gt_boxes.dim() != 3 or gt_boxes.shape[-1] != 8:
        raise ValueError(f'proposal_targets: gt_boxes of shape {tuple(gt_boxes.shape)}; only (B, M, 7 + 1) is built')
    if cls_score_type not in ('cls', 'roi_iou'):
        raise NotImplementedError(cls_score_type)
    B, R, _ = rois.shape
    M, S = gt_boxes.shape[1], int(roi_per_image)
    assert rois.is_cuda and gt_boxes.shape[0] == B and roi_scores.shape == (B, R) and roi_labels.shape == (B, R)
    assert state.dtype == torch.int32 and state.numel() == 2 and state.device == rois.device
    dev = rois.device
    rois, gt_boxes = rois.detach().float().contiguous(), gt_boxes.detach().float().contiguous()
    roi_scores, roi_labels = roi_scores.detach().float().contiguous(), roi_labels.detach().long().contiguous()
    out = {'rois': torch.empty((B, S, 7), dtype=torch.float32, device=dev),
           'roi_labels': torch.empty((B, S), dtype=torch.int64, device=dev),
           'roi_scores': torch.empty((B, S), dtype=torch.float32, device=dev),
           'gt_iou_of_rois': torch.empty((B, S), dtype=torch.float32, device=dev),
           'gt_of_rois_src': torch.empty((B, S, 8), dtype=torch.float32, device=dev),
           'gt_of_rois': torch.empty((B, S, 8), dtype=torch.float32, device=dev),
           'reg_valid_mask': torch.empty((B, S), dtype=torch.int64, device=dev),
           'rcnn_cls_labels': torch.empty((B, S), dtype=torch.int64 if cls_score_type == 'cls' else torch.float32, device=dev),
           'sampled_inds': torch.empty((B, S), dtype=torch.int32, device=dev),
           'gt_assignment': torch.empty((B, S), dtype=torch.int32, device=dev)}
    _native.call('pdm_proposal_targets', _native.stream(dev), B, R, M, S, rois.data_ptr(),
                 roi_scores.data_ptr(), roi_labels.data_ptr(), gt_boxes.data_ptr(), 1 if by_class else 0, int(fg_per_image),
                 float(hard_bg_ratio), float(reg_fg_thresh), float(cls_fg_thresh), float(cls_bg_thresh), float(cls_bg_thresh_lo),
                 0 if cls_score_type == 'cls' else 1, int(seed) & 0xFFFFFFFF, state.data_ptr(), out['rois'].data_ptr(),
                 out['roi_labels'].data_ptr(), out['roi_scores'].data_ptr(), out['gt_iou_of_rois'].data_ptr(),
                 out['gt_of_rois_src'].data_ptr(), out['gt_of_rois'].data_ptr(), out['reg_valid_mask'].data_ptr(),
                 out['rcnn_cls_labels'].data_ptr(), out['sampled_inds'].data_ptr(), out['gt_assignment'].data_ptr())
    return out


class _RCNNLoss(Function):
    @staticmethod
    def forward(ctx, rcnn_cls, rcnn_reg, rois, gt_of_rois, gt_of_rois_src, reg_valid_mask, cls_labels, spec):
        """rcnn_cls (n, 1) | (n), rcnn_reg (n, 7) fp32; rois (n, 7), gt_of_rois / gt_of_rois_src (n, 8) fp32; reg_valid_mask (n)
        int64; cls_labels (n) int64 or fp32; spec = (code_weights[7], beta, cls_weight, reg_weight, corner_weight, use_corner).
        Returns (loss_cls, loss_reg, loss_corner, fg_count): four 0-dim fp32 tensors, each with storage of its own."""
        code_w, beta, w_cls, w_reg, w_corner, use_corner = spec
        n = rcnn_reg.shape[0]
        assert rcnn_cls.dtype == torch.float32 and rcnn_reg.dtype == torch.float32 and rcnn_cls.numel() == n and rcnn_reg.shape == (n, 7)
        assert rois.shape == (n, 7) and gt_of_rois.shape == (n, 8) and gt_of_rois_src.shape == (n, 8)
        assert reg_valid_mask.dtype == torch.int64 and reg_valid_mask.numel() == n and cls_labels.numel() == n
        assert cls_labels.dtype in (torch.int64, torch.float32)
        dev = rcnn_reg.device
        cls_c, reg_c = rcnn_cls.contiguous(), rcnn_reg.contiguous()
        rois, gt_of_rois, gt_of_rois_src = rois.contiguous(), gt_of_rois.contiguous(), gt_of_rois_src.contiguous()
        reg_valid_mask, cls_labels = reg_valid_mask.contiguous(), cls_labels.contiguous()
        l = _native.lib()
        nbytes = l.pdm_rcnn_loss_workspace_bytes(n)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        dcls = torch.empty(rcnn_cls.shape, dtype=torch.float32, device=dev)
        dreg = torch.empty((n, 7), dtype=torch.float32, device=dev)
        dcorner = torch.empty((n, 7), dtype=torch.float32, device=dev)
        outs = [torch.empty((), dtype=torch.float32, device=dev) for _ in range(4)]
        cw = (ctypes.c_float * 7)(*[float(v) for v in code_w])
        _native.call('pdm_rcnn_loss', _native.stream(dev), n, cls_c.data_ptr(), reg_c.data_ptr(), rois.data_ptr(),
                     gt_of_rois.data_ptr(), gt_of_rois_src.data_ptr(), reg_valid_mask.data_ptr(), cls_labels.data_ptr(),
                     1 if cls_labels.dtype == torch.float32 else 0, cw, beta, w_cls, w_reg, w_corner,
                     1 if use_corner else 0, dcls.data_ptr(), dreg.data_ptr(), dcorner.data_ptr(), outs[0].data_ptr(), outs[1].data_ptr(),
                     outs[2].data_ptr(), outs[3].data_ptr(), ws.data_ptr(), nbytes)
        ctx.save_for_backward(dcls, dreg, dcorner)
        ctx.mark_non_differentiable(outs[3])
        ctx.set_materialize_grads(False)
        return tuple(outs)

    @staticmethod
    def backward(ctx, g_cls, g_reg, g_corner, _g_fg):
        dcls, dreg, dcorner = ctx.saved_tensors
        gc = None if g_cls is None else dcls * g_cls
        gr = None if g_reg is None else dreg * g_reg
        if g_corner is not None:
            gr = dcorner * g_corner if gr is None else torch.addcmul(gr, dcorner, g_corner)
        return gc, gr, None, None, None, None, None, None


def rcnn_loss(rcnn_cls, rcnn_reg, rois, gt_of_rois, gt_of_rois_src, reg_valid_mask, cls_labels, code_weights, beta,
              cls_weight, reg_weight, corner_weight, use_corner):
    return _RCNNLoss.apply(rcnn_cls, rcnn_reg, rois, gt_of_rois, gt_of_rois_src, reg_valid_mask, cls_labels,
                           (list(code_weights), float(beta), float(cls_weight), float(reg_weight), float(corner_weight),
                            bool(use_corner)))

"""The anchor head's three device operators (csrc/anchor_head.hip): target assignment, the loss terms with their gradients
and the box decode — each a short launch chain for the whole batch, no host read, no float atomics on a result, safe to
capture in a torch.cuda.graph after one warm-up call.

The torch formulations they replace stay in dense_heads/target_assigner/axis_aligned_target_assigner.py (assign_targets on
CPU tensors) and dense_heads/anchor_head_template.py (get_cls_layer_loss, get_box_reg_layer_loss, generate_predicted_boxes on
CPU tensors): the CPU path, and what the tests compare with.
"""
import ctypes

import torch
from torch.autograd import Function

from . import _native

MAX_GT = 1024          # boxes of one sample the target kernels hold in LDS; a larger M is refused, never truncated
MAX_SLOTS = 32         # anchors per location
MAX_SETS = 16          # anchor sets
MAX_DIR_BINS = 8


@torch.no_grad()
def anchor_targets(anchors, set_of_slot, set_of_class, matched, unmatched, gt_boxes, norm_by_num_examples=False):
    """anchors (A, 7) fp32 on the GPU in the order y, x, slot; set_of_slot[s] = the anchor set of slot s (len = anchors
    per location); set_of_class[g] = the set of global class g (1-based; [0] unused) or -1; matched / unmatched = the
    sets' thresholds; gt_boxes (B, M, 8) fp32, class last, left untouched ->
    box_cls_labels (B, A) int32, box_reg_targets (B, A, 7), reg_weights (B, A), num_pos (B) int32 (pdm_anchor_targets)."""
    assert anchors.is_cuda and anchors.dim() == 2 and anchors.shape[1] == 7 and anchors.dtype == torch.float32
    assert gt_boxes.dim() == 3 and gt_boxes.shape[2] == 8, f'gt_boxes (B, M, 8): {tuple(gt_boxes.shape)}'
    gt = gt_boxes.detach().float().contiguous()
    anchors = anchors.contiguous()
    B, M, cols = gt.shape
    if M > MAX_GT:
        raise ValueError(f'anchor_targets: at most MAX_GT = {MAX_GT} boxes per sample (M = {M})')
    A, A_loc, S = anchors.shape[0], len(set_of_slot), len(matched)
    assert A % A_loc == 0 and len(unmatched) == S
    dev = gt.device
    labels = torch.empty((B, A), dtype=torch.int32, device=dev)
    targets = torch.empty((B, A, 7), dtype=torch.float32, device=dev)
    weights = torch.empty((B, A), dtype=torch.float32, device=dev)
    num_pos = torch.empty((B,), dtype=torch.int32, device=dev)
    nbytes = _native.lib().pdm_anchor_targets_workspace_bytes(B, M, S)
    ws = torch.empty(max(nbytes, 8), dtype=torch.uint8, device=dev)
    _native.call("pdm_anchor_targets", _native.stream(dev), B, M, cols, A, A_loc, S, len(set_of_class) - 1, anchors.data_ptr(),
                 _native.host_array(ctypes.c_int, set_of_slot), _native.host_array(ctypes.c_int, set_of_class),
                 _native.host_array(ctypes.c_float, matched), _native.host_array(ctypes.c_float, unmatched), gt.data_ptr(),
                 1 if norm_by_num_examples else 0, labels.data_ptr(), targets.data_ptr(), weights.data_ptr(), num_pos.data_ptr(),
                 ws.data_ptr(), nbytes)
    return labels, targets, weights, num_pos


class _AnchorHeadLoss(Function):
    @staticmethod
    def forward(ctx, labels, targets, num_pos, anchor_rot, code_weights, scalars, num_class, num_dir_bins, cls_map, box_map, dir_map):
        B, _, H, W = box_map.shape
        A_loc = len(anchor_rot)
        assert 1 <= A_loc <= MAX_SLOTS and len(code_weights) == 7
        _native.check_map('cls_preds', cls_map, B, H, W, A_loc * num_class)
        _native.check_map('box_preds', box_map, B, H, W, A_loc * 7)
        if dir_map is not None:
            assert 1 <= num_dir_bins <= MAX_DIR_BINS, f'NUM_DIR_BINS {num_dir_bins}: 1 .. {MAX_DIR_BINS}'
            _native.check_map('dir_cls_preds', dir_map, B, H, W, A_loc * num_dir_bins)
        A = H * W * A_loc
        assert labels.shape == (B, A) and labels.dtype == torch.int32 and targets.shape == (B, A, 7) and targets.dtype == torch.float32
        assert num_pos.shape == (B,) and num_pos.dtype == torch.int32
        labels, targets, num_pos = labels.contiguous(), targets.contiguous(), num_pos.contiguous()
        dev = box_map.device
        ptrs, bf, st = _native.map_tables([cls_map, box_map, dir_map], 3)
        out = torch.empty(3, dtype=torch.float32, device=dev)
        g_cls = torch.empty(cls_map.shape, dtype=torch.float32, device=dev)
        g_box = torch.empty(box_map.shape, dtype=torch.float32, device=dev)
        g_dir = None if dir_map is None else torch.empty(dir_map.shape, dtype=torch.float32, device=dev)
        nbytes = _native.lib().pdm_anchor_head_loss_workspace_bytes(B, H, W)
        ws = torch.empty(max(nbytes, 8), dtype=torch.uint8, device=dev)
        cls_w, loc_w, dir_w, dir_offset, beta, alpha, gamma = scalars
        _native.call("pdm_anchor_head_loss", _native.stream(dev), B, H, W, A_loc, int(num_class), int(num_dir_bins), ptrs, bf, st,
                     labels.data_ptr(), targets.data_ptr(), num_pos.data_ptr(), _native.host_array(ctypes.c_float, anchor_rot),
                     _native.host_array(ctypes.c_float, code_weights), cls_w, loc_w, dir_w, dir_offset, beta, alpha, gamma, out.data_ptr(),
                     g_cls.data_ptr(), g_box.data_ptr(), None if g_dir is None else g_dir.data_ptr(), ws.data_ptr(), nbytes)
        ctx.save_for_backward(*([g_cls, g_box] + ([] if g_dir is None else [g_dir])))
        ctx.dtypes = [cls_map.dtype, box_map.dtype, None if dir_map is None else dir_map.dtype]
        return out[0], out[1], out[2]

    @staticmethod
    def backward(ctx, g_cls_loss, g_loc_loss, g_dir_loss):
        saved = ctx.saved_tensors                                     # the maps' gradients were formed in forward(): only scaled here
        grads = [(saved[0] * g_cls_loss.float()).to(ctx.dtypes[0]), (saved[1] * g_loc_loss.float()).to(ctx.dtypes[1]),
                 None if len(saved) < 3 else (saved[2] * g_dir_loss.float()).to(ctx.dtypes[2])]
        return (None,) * 8 + tuple(grads)


def anchor_head_loss(cls_preds, box_preds, dir_cls_preds, labels, targets, num_pos, anchor_rot, code_weights, num_class, num_dir_bins=2,
                     cls_weight=1.0, loc_weight=1.0, dir_weight=1.0, dir_offset=0.0, beta=1.0 / 9.0, alpha=0.25, gamma=2.0):
    """The conv outputs as they leave the convolutions — cls_preds (B, A_loc num_class, H, W), box_preds (B, A_loc 7, H, W),
    dir_cls_preds (B, A_loc num_dir_bins, H, W) or None, fp32 or bf16 with any strides, channel = slot * width + column — with
    anchor_targets' labels, targets and num_pos and the A_loc anchor rotations -> (cls_loss, loc_loss, dir_loss) 0-dim, each
    the reference's weighted term (sigmoid focal loss over labels >= 0; smooth-L1 with the sin-difference on the heading over
    the positives; cross-entropy of the direction bin over the positives; each per sample / max(num_pos, 1), then / B) with
    its gradient on its map (pdm_anchor_head_loss).  Sums are block partials added in a fixed order: two runs give the same
    bits.  dir_loss is an exact 0 without the direction map."""
    scalars = tuple(float(v) for v in (cls_weight, loc_weight, dir_weight, dir_offset, beta, alpha, gamma))
    return _AnchorHeadLoss.apply(labels, targets, num_pos, tuple(float(v) for v in anchor_rot), tuple(float(v) for v in code_weights),
                                 scalars, int(num_class), int(num_dir_bins), cls_preds, box_preds, dir_cls_preds)


@torch.no_grad()
def anchor_decode(box_preds, dir_cls_preds, anchors, num_dir_bins=2, dir_offset=0.0, dir_limit_offset=0.0):
    """box_preds (B, A_loc 7, H, W) and dir_cls_preds (B, A_loc num_dir_bins, H, W) or None as they leave the convolutions,
    anchors (H W A_loc, 7) fp32 -> batch_box_preds (B, H W A_loc, 7) fp32: ResidualCoder.decode_torch, the arg-max direction
    bin (the lower bin on equal logits) and the heading folded into the bin's period, in one launch (pdm_anchor_decode)."""
    B, ch, H, W = box_preds.shape
    assert ch % 7 == 0
    A_loc = ch // 7
    _native.check_map('box_preds', box_preds, B, H, W, A_loc * 7)
    if dir_cls_preds is not None:
        assert 1 <= num_dir_bins <= MAX_DIR_BINS, f'NUM_DIR_BINS {num_dir_bins}: 1 .. {MAX_DIR_BINS}'
        _native.check_map('dir_cls_preds', dir_cls_preds, B, H, W, A_loc * num_dir_bins)
    assert anchors.is_cuda and anchors.dtype == torch.float32 and tuple(anchors.shape) == (H * W * A_loc, 7), tuple(anchors.shape)
    anchors = anchors.contiguous()
    out = torch.empty((B, H * W * A_loc, 7), dtype=torch.float32, device=box_preds.device)
    ptrs, bf, st = _native.map_tables([box_preds.detach(), None if dir_cls_preds is None else dir_cls_preds.detach()], 2)
    _native.call("pdm_anchor_decode", _native.stream(out), B, H, W, A_loc, int(num_dir_bins), ptrs, bf, st, anchors.data_ptr(),
                 float(dir_offset), float(dir_limit_offset), out.data_ptr())
    return out

"""CenterHead's three device operators (csrc/center_head.hip): target assignment, heat-map box decode and the L1
regression loss with its gradient — one launch chain per head for the whole batch, no host read, no float atomics on
results or gradients, safe to capture in a torch.cuda.graph after one warm-up call.

The torch formulations they replace stay in utils/centernet_utils.py (_topk, decode_bbox_from_heatmap), utils/loss_utils.py
(RegLossCenterNet) and dense_heads/center_head.py (assign_targets on the CPU): the CPU path, and what the tests compare with.
"""
import ctypes

import torch
from torch.autograd import Function

from . import _native

MAX_K = 16384          # candidates per sample the decode holds in LDS
MAX_OBJS = 8192        # slots per sample of the regression loss
_HEAD_ORDER = ('center', 'center_z', 'dim', 'rot', 'vel')
_CHANNELS = {'center': 2, 'center_z': 1, 'dim': 3, 'rot': 2, 'vel': 2}


@torch.no_grad()
def center_targets(gt_boxes, local_of, num_head_classes, H, W, x0, y0, vx, vy, stride, num_max_objs, gaussian_overlap,
                   min_radius):
    """gt_boxes (B, M, 7 + E + 1) fp32 on the GPU, global class (1-based, 0 = padding) in the last column, left
    untouched; local_of[g] = the head's 1-based class of global class g (0 = another head's), len = #classes + 1.
    -> heatmap (B, C_head, H, W), target_boxes (B, N, 8 + E), inds (B, N) int64, mask (B, N) int64,
    target_boxes_src (B, N, 7 + E + 1) with the head's class in the last column (pdm_center_targets).
    The gaussian window is the box's own (2 r + 1)^2 cells whatever the radius: nothing is clipped."""
    gt = gt_boxes.detach().float().contiguous()
    B, M, cols = gt.shape
    dev, N = gt.device, int(num_max_objs)
    hm = torch.empty((B, num_head_classes, H, W), dtype=torch.float32, device=dev)
    tb = torch.empty((B, N, cols), dtype=torch.float32, device=dev)
    src = torch.empty((B, N, cols), dtype=torch.float32, device=dev)
    inds = torch.empty((B, N), dtype=torch.int64, device=dev)
    mask = torch.empty((B, N), dtype=torch.int64, device=dev)
    table = _native.host_array(ctypes.c_int, local_of)
    _native.call("pdm_center_targets", _native.stream(dev), B, M, cols, int(num_head_classes), int(H), int(W), gt.data_ptr(),
                 len(local_of) - 1, table, float(x0), float(y0), float(vx), float(vy), float(stride), N, float(gaussian_overlap),
                 int(min_radius), hm.data_ptr(), tb.data_ptr(), inds.data_ptr(), mask.data_ptr(), src.data_ptr())
    return hm, tb, inds, mask, src


@torch.no_grad()
def center_decode(hm, center, center_z, dim, rot, vel, K, score_thresh, post_center_limit_range, x0, y0, vx, vy, stride,
                  global_of):
    """hm (B, C_head, H, W) LOGITS and the raw regression maps (dim before exp; rot = [cos, sin]; vel or None), fp32 or
    bf16 with any strides -> boxes (B, K, 7 | 9), scores (B, K), labels (B, K) int64 (global, 1-based, through
    global_of[c] = 0-based global class of the head's class c), count (B) int32: per sample the K highest sigmoid(hm)
    over (class, y, x), ties by lower flat index, decoded, filtered by the limit range (inclusive) and the score
    threshold (strict) and compacted in rank order; padding rows are zero (pdm_center_decode)."""
    B, C, H, W = hm.shape
    if K > H * W:
        raise RuntimeError(f'center_decode: K = {K} is out of range for a {H} x {W} map (as torch.topk)')
    if K > MAX_K:
        raise ValueError(f'center_decode: at most {MAX_K} candidates per sample (K = {K})')
    maps = [hm, center, center_z, dim, rot] + ([vel] if vel is not None else [])
    for name, t in zip(('hm',) + _HEAD_ORDER, maps):
        _native.check_map(name, t.detach(), B, H, W)
        assert name == 'hm' or t.shape[1] == _CHANNELS[name], f'{name}: {tuple(t.shape)}'
    dev, E = hm.device, 2 if vel is not None else 0
    boxes = torch.empty((B, K, 7 + E), dtype=torch.float32, device=dev)
    scores = torch.empty((B, K), dtype=torch.float32, device=dev)
    labels = torch.empty((B, K), dtype=torch.int64, device=dev)
    count = torch.empty((B,), dtype=torch.int32, device=dev)
    ptrs, bf, st = _native.map_tables(maps, slots=6)
    lim = _native.host_array(ctypes.c_float, post_center_limit_range)
    gl = _native.host_array(ctypes.c_int, global_of)
    assert len(global_of) == C and len(post_center_limit_range) == 6
    _native.call("pdm_center_decode", _native.stream(dev), B, C, H, W, int(K), ptrs, bf, st,
                 float('-inf') if score_thresh is None else float(score_thresh), lim, float(x0), float(y0), float(vx), float(vy),
                 float(stride), gl, boxes.data_ptr(), scores.data_ptr(), labels.data_ptr(), count.data_ptr())
    return boxes, scores, labels, count


class _CenterRegLoss(Function):
    @staticmethod
    def forward(ctx, inds, mask, target, code_weights, loc_weight, *maps):
        """maps: the head's regression maps in code order, (B, c_i, H, W) fp32 or bf16 with any strides, sum c_i = D;
        inds / mask (B, N) int64; target (B, N, D) fp32 -> (loc_loss 0-dim, loss_per_code (D))."""
        B, _, H, W = maps[0].shape
        for i, t in enumerate(maps):
            _native.check_map(f'map {i}', t, B, H, W)
        D = sum(t.shape[1] for t in maps)
        N = inds.shape[1]
        assert inds.shape == (B, N) and mask.shape == (B, N) and inds.dtype == torch.int64 and mask.dtype == torch.int64
        assert target.shape == (B, N, D) and target.dtype == torch.float32 and len(code_weights) == D
        if N > MAX_OBJS:
            raise ValueError(f'center_reg_loss: at most {MAX_OBJS} slots per sample (NUM_MAX_OBJS = {N})')
        inds, mask, target = inds.contiguous(), mask.contiguous(), target.contiguous()
        dev = maps[0].device
        ptrs, bf, st = _native.channel_tables(maps)
        cw = _native.host_array(ctypes.c_float, code_weights)
        nbytes = _native.lib().pdm_center_reg_loss_workspace_bytes(B, D)
        ws = torch.empty(max(nbytes, 8), dtype=torch.uint8, device=dev)
        per_code = torch.empty(D, dtype=torch.float32, device=dev)
        out = torch.empty(3, dtype=torch.float32, device=dev)
        grad = torch.empty((B, D, H, W), dtype=torch.float32, device=dev)
        _native.call("pdm_center_reg_loss", _native.stream(dev), B, N, D, H, W, ptrs, bf, st, inds.data_ptr(), mask.data_ptr(),
                     target.data_ptr(), cw, float(loc_weight), per_code.data_ptr(), out.data_ptr(), grad.data_ptr(), ws.data_ptr(), nbytes)
        ctx.save_for_backward(grad)
        ctx.split = [t.shape[1] for t in maps]
        ctx.dtypes = [t.dtype for t in maps]
        ctx.mark_non_differentiable(per_code)
        return out[0], per_code

    @staticmethod
    def backward(ctx, g, _g_per_code):
        grad, = ctx.saved_tensors
        parts = torch.split(grad * g.float(), ctx.split, dim=1)       # the maps were formed in forward(): only scaled here
        return (None, None, None, None, None) + tuple(p.to(dt) for p, dt in zip(parts, ctx.dtypes))


def center_reg_loss(maps, inds, mask, target, code_weights, loc_weight=1.0):
    """maps: the head's regression maps in code order (HEAD_ORDER) -> (loc_loss, loss_per_code): loss_per_code (D) as
    RegLossCenterNet returns it (detached), loc_loss = loc_weight * sum(loss_per_code * code_weights) with its gradient
    on the maps (pdm_center_reg_loss): slots that share a cell are added in slot order by one thread, so two runs give
    the same bits; cells no slot names get exact zeros.  A NaN target element is left out (utils/loss_utils._reg_loss)."""
    return _CenterRegLoss.apply(inds, mask, target, tuple(float(v) for v in code_weights), float(loc_weight), *maps)

"""Fused multi-head attention (csrc/attention.hip): softmax(q_h k_h^T / sqrt(d)) v_h per head in fp32 on the MFMA,
the keys split into chunks so that few queries against many keys still fill the device; two launches, no host read, no
float atomics, two runs give the same bits, safe to capture in a torch.cuda.graph after one warm-up call.

mha_forward is the inference form.  mha / mha_kv / mha_qkv are differentiable: a forward that also applies the attention
dropout (counter-based draws, csrc/draws.h) and saves each query's (raw maximum, sum), and a key-stationary backward
(csrc/attention_bwd.hip) that recomputes the weights and the mask; the (P, N) weights are never stored.

The torch formulation it replaces is nn.MultiheadAttention between its in- and out-projection (mha_reference, and mha_torch
with an explicit dropout mask): the CPU path, and what the tests compare with.
"""
import math

import numpy as np
import torch

from . import _native


def default_keys_per_chunk():
    return int(_native.lib().pdm_mha_default_keys_per_chunk())


def mha_reference(q, k, v, nheads):
    """(B, P, C), (B, N, C), (B, N, C) -> (B, P, C): the same product by torch operators, in the inputs' dtype"""
    B, P, C = q.shape
    d = C // nheads
    qh, kh, vh = (t.reshape(B, t.shape[1], nheads, d).transpose(1, 2) for t in (q, k, v))
    w = torch.softmax(qh @ kh.transpose(-1, -2) / math.sqrt(d), dim=-1)
    return (w @ vh).transpose(1, 2).reshape(B, P, C)


def _rows(name, t, C):
    """a (B, rows, C) fp32 view whose rows are C contiguous elements and whose samples are `rows` rows on -> its row stride"""
    assert t.is_cuda and t.dtype == torch.float32 and t.dim() == 3 and t.shape[2] == C, f'{name}: fp32 (B, rows, {C}) on the GPU'
    sb, sr, sc = t.stride()
    if (sc != 1 and C > 1) or sr < C or (t.shape[0] > 1 and sb != t.shape[1] * sr):
        raise ValueError(f'{name}: strides {tuple(t.stride())}: rows of contiguous elements, a sample = its rows in a row')
    return sr


@torch.no_grad()
def mha_forward(q, k, v, nheads, keys_per_chunk=0, out=None, workspace=None):
    """q (B, P, C), k (B, N, C), v (B, N, C) fp32 on the GPU, each with its own row stride (k and v may be the halves of one
    (B, N, 2C) tensor) -> out (B, P, C) = softmax(q_h k_h^T / sqrt(d)) v_h, heads concatenated (pdm_mha_forward).
    d = C / nheads in {16, 32}, C <= 256; anything else raises ValueError.  keys_per_chunk = 0: the library's default.
    out / workspace: buffers of the caller's (workspace: uint8, 8-byte aligned, at least the size the library names)."""
    B, P, C = q.shape
    N = k.shape[1]
    nheads, kpc = int(nheads), int(keys_per_chunk)
    if nheads < 1 or C % nheads or C // nheads not in (16, 32) or C > 256 or P < 1 or N < 1 or kpc < 0:
        raise ValueError(f'mha_forward: C = {C}, heads = {nheads}, P = {P}, N = {N}, keys_per_chunk = {kpc}: '
                         'needs C / heads in {16, 32}, C <= 256, P >= 1, N >= 1')
    assert k.shape == (B, N, C) and v.shape == (B, N, C), (q.shape, k.shape, v.shape)
    qs, ks, vs = _rows('q', q, C), _rows('k', k, C), _rows('v', v, C)
    dev = q.device
    if out is None:
        out = torch.empty((B, P, C), dtype=torch.float32, device=dev)
    assert out.shape == (B, P, C) and out.dtype == torch.float32 and out.is_contiguous()
    nbytes = _native.lib().pdm_mha_forward_workspace_bytes(B, P, N, C, nheads, kpc)
    if workspace is None:
        workspace = torch.empty(max(nbytes, 8), dtype=torch.uint8, device=dev)
    _native.call("pdm_mha_forward", _native.stream(dev), B, P, N, C, nheads, q.data_ptr(), qs, k.data_ptr(), ks, v.data_ptr(), vs,
                 kpc, out.data_ptr(), workspace.data_ptr(), workspace.numel())
    return out


# ---- training: dropout draws, the forward that saves the backward's statistics, the backward (csrc/attention_bwd.hip) ----

def _fmix32(h):
    """common.h's fmix32 on uint64 arrays holding 32-bit values"""
    m = np.uint64(0xFFFFFFFF)
    h = h ^ (h >> np.uint64(16))
    h = (h * np.uint64(0x85EBCA6B)) & m
    h = h ^ (h >> np.uint64(13))
    h = (h * np.uint64(0xC2B2AE35)) & m
    return h ^ (h >> np.uint64(16))


def _check_p(p):
    p = float(p)
    if not 0.0 <= p < 1.0:
        raise ValueError(f'attention dropout p = {p}: needs 0 <= p < 1')
    return p


def dropout_scale(p):
    """1.0f / (1.0f - p) as the kernels form it, as a Python float"""
    return float(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))


def dropout_keep_host(seed, step, B, H, P, N, p):
    """The attention dropout's keep mask (B, H, P, N) bool in numpy, a pure function of its arguments (csrc/draws.h):
    weight (b, h, i, j) is kept iff fmix32(draw_key(seed, step, b * H + h, i) ^ j * 0x9E3779B1) >= floor(p * 2^32)."""
    p = _check_p(p)
    if p == 0.0:
        return np.ones((B, H, P, N), dtype=bool)
    m = np.uint64(0xFFFFFFFF)
    u = lambda x: np.asarray(x, dtype=np.uint64)
    k0 = _fmix32(u(int(seed) & 0xFFFFFFFF) ^ ((u(int(step) & 0xFFFFFFFF) * np.uint64(0x85EBCA6B)) & m))
    bh = (u(np.arange(B * H))[:, None] * np.uint64(0x9E3779B1)) & m
    qi = (u(np.arange(P))[None, :] * np.uint64(0x7F4A7C15)) & m
    qkey = _fmix32(k0 ^ bh ^ qi)                                       # (B H, P): draw_key(seed, step, b H + h, i)
    kj = (u(np.arange(N)) * np.uint64(0x9E3779B1)) & m
    draw = _fmix32(qkey[:, :, None] ^ kj[None, None, :])
    return (draw >= np.uint64(math.floor(p * 4294967296.0))).reshape(B, H, P, N)


def _heads(t, nheads):
    B, n, C = t.shape
    return t.reshape(B, n, nheads, C // nheads).transpose(1, 2)


def mha_torch(q, k, v, nheads, keep=None, p=0.0):
    """mha_reference with an explicit dropout mask: keep (B, H, P, N) bool | None multiplies the softmax weights, kept ones
    scaled by 1 / (1 - p) (the fp32 value, in any dtype).  Differentiable by torch autograd: the CPU path and the tests' reference."""
    B, P, C = q.shape
    d = C // nheads
    qh, kh, vh = _heads(q, nheads), _heads(k, nheads), _heads(v, nheads)
    w = torch.softmax(qh @ kh.transpose(-1, -2) / math.sqrt(d), dim=-1)
    if keep is not None:
        w = w * (keep.to(w.dtype) * dropout_scale(p))
    return (w @ vh).transpose(1, 2).reshape(B, P, C)


def mha_backward_torch(q, k, v, out, dout, nheads, keep=None, p=0.0):
    """(dq, dk, dv) of mha_torch by the formulation the kernels use, in torch operators and the inputs' dtype:
    D = dO . O, dP = r M (dO V^T), dS = P (dP - D), dV = (r M P)^T dO, dK = scale dS^T Q, dQ = scale dS K."""
    B, P, C = q.shape
    N = k.shape[1]
    d = C // nheads
    scale = 1.0 / math.sqrt(d)
    qh, kh, vh, oh, doh = (_heads(t, nheads) for t in (q, k, v, out, dout))
    w = torch.softmax(qh @ kh.transpose(-1, -2) * scale, dim=-1)
    mr = None if keep is None else keep.to(w.dtype) * dropout_scale(p)
    delta = (doh * oh).sum(-1, keepdim=True)
    dp = doh @ vh.transpose(-1, -2)
    if mr is not None:
        dp = dp * mr
    ds = w * (dp - delta)
    dv = (w if mr is None else w * mr).transpose(-1, -2) @ doh
    dk = (ds.transpose(-1, -2) @ qh) * scale
    dq = (ds @ kh) * scale
    return (dq.transpose(1, 2).reshape(B, P, C), dk.transpose(1, 2).reshape(B, N, C), dv.transpose(1, 2).reshape(B, N, C))


class AttentionDraws:
    """The state of one attention's dropout: a seed and a device-resident step counter (one int32 element holding the
    unsigned value) that every training forward with p > 0 advances by one on the device.  Data-parallel ranks must use
    different seeds."""

    def __init__(self, seed, device, step=None):
        self.seed = int(seed) & 0xFFFFFFFF
        self.step = torch.zeros(1, dtype=torch.int32, device=device) if step is None else step
        assert self.step.dtype == torch.int32 and self.step.numel() == 1

    def reset(self, value=0):
        self.step.fill_(int(value))


def _check_shapes(who, q, k, v, nheads, kpc):
    B, P, C = q.shape
    N = k.shape[1]
    if nheads < 1 or C % nheads or C // nheads not in (16, 32) or C > 256 or P < 1 or N < 1 or kpc < 0:
        raise ValueError(f'{who}: C = {C}, heads = {nheads}, P = {P}, N = {N}, keys_per_chunk = {kpc}: '
                         'needs C / heads in {16, 32}, C <= 256, P >= 1, N >= 1')
    assert k.shape == (B, N, C) and v.shape == (B, N, C), (q.shape, k.shape, v.shape)
    return B, P, N, C


def _workspace(name, B, P, N, C, nheads, kpc, workspace, dev):
    nbytes = getattr(_native.lib(), name)(B, P, N, C, nheads, kpc)
    return torch.empty(max(nbytes, 8), dtype=torch.uint8, device=dev) if workspace is None else workspace


@torch.no_grad()
def mha_forward_train(q, k, v, nheads, dropout_p=0.0, draws=None, keys_per_chunk=0, out=None, stats=None, used_step=None,
                      workspace=None):
    """mha_forward plus the attention dropout and the backward's statistics (pdm_mha_forward_train) ->
    (out (B, P, C), stats (B, H, P, 2) = raw score maximum and softmax sum, used_step (1,) int32 | None).
    dropout_p > 0 needs draws (AttentionDraws); the call advances draws.step on the device and used_step holds the value
    it drew with.  With dropout_p == 0 out is mha_forward's bit for bit and no counter is touched."""
    nheads, kpc, p = int(nheads), int(keys_per_chunk), _check_p(dropout_p)
    B, P, N, C = _check_shapes('mha_forward_train', q, k, v, nheads, kpc)
    qs, ks, vs = _rows('q', q, C), _rows('k', k, C), _rows('v', v, C)
    dev = q.device
    if p > 0.0 and draws is None:
        raise ValueError('mha_forward_train: dropout_p > 0 needs draws (AttentionDraws)')
    out = torch.empty((B, P, C), dtype=torch.float32, device=dev) if out is None else out
    stats = torch.empty((B, nheads, P, 2), dtype=torch.float32, device=dev) if stats is None else stats
    assert out.shape == (B, P, C) and out.dtype == torch.float32 and out.is_contiguous()
    assert stats.shape == (B, nheads, P, 2) and stats.dtype == torch.float32 and stats.is_contiguous()
    if p > 0.0:
        used_step = torch.empty(1, dtype=torch.int32, device=dev) if used_step is None else used_step
        assert draws.step.device == dev and used_step.dtype == torch.int32
    else:
        used_step = None
    workspace = _workspace('pdm_mha_forward_train_workspace_bytes', B, P, N, C, nheads, kpc, workspace, dev)
    _native.call("pdm_mha_forward_train", _native.stream(dev), B, P, N, C, nheads, q.data_ptr(), qs, k.data_ptr(), ks,
                 v.data_ptr(), vs, kpc, p, draws.seed if p > 0.0 else 0, draws.step.data_ptr() if p > 0.0 else None,
                 used_step.data_ptr() if p > 0.0 else None, stats.data_ptr(), out.data_ptr(), workspace.data_ptr(), workspace.numel())
    return out, stats, used_step


@torch.no_grad()
def mha_backward(q, k, v, out, dout, stats, nheads, dropout_p=0.0, seed=0, used_step=None, keys_per_chunk=0, dq=None, dk=None,
                 dv=None, workspace=None):
    """(dq, dk, dv) of the fused attention from what mha_forward_train left (pdm_mha_backward).  dq, dk, dv: buffers of the
    caller's, each (B, rows, C) with its own row stride (halves or thirds of one packed buffer); allocated when None."""
    nheads, kpc, p = int(nheads), int(keys_per_chunk), _check_p(dropout_p)
    B, P, N, C = _check_shapes('mha_backward', q, k, v, nheads, kpc)
    qs, ks, vs = _rows('q', q, C), _rows('k', k, C), _rows('v', v, C)
    dev = q.device
    dq = torch.empty((B, P, C), dtype=torch.float32, device=dev) if dq is None else dq
    dk = torch.empty((B, N, C), dtype=torch.float32, device=dev) if dk is None else dk
    dv = torch.empty((B, N, C), dtype=torch.float32, device=dev) if dv is None else dv
    assert dq.shape == (B, P, C) and dk.shape == (B, N, C) and dv.shape == (B, N, C)
    dqs, dks, dvs = _rows('dq', dq, C), _rows('dk', dk, C), _rows('dv', dv, C)
    for name, t in (('out', out), ('dout', dout)):
        assert t.shape == (B, P, C) and t.dtype == torch.float32 and t.is_cuda and t.is_contiguous(), f'{name}: contiguous fp32 (B, P, C)'
    assert stats.shape == (B, nheads, P, 2) and stats.dtype == torch.float32 and stats.is_contiguous()
    if p > 0.0 and used_step is None:
        raise ValueError('mha_backward: dropout_p > 0 needs the used_step of the forward')
    workspace = _workspace('pdm_mha_backward_workspace_bytes', B, P, N, C, nheads, kpc, workspace, dev)
    _native.call("pdm_mha_backward", _native.stream(dev), B, P, N, C, nheads, q.data_ptr(), qs, k.data_ptr(), ks, v.data_ptr(), vs,
                 out.data_ptr(), dout.data_ptr(), stats.data_ptr(), p, int(seed) & 0xFFFFFFFF,
                 used_step.data_ptr() if p > 0.0 else None, kpc, dq.data_ptr(), dqs, dk.data_ptr(), dks, dv.data_ptr(), dvs,
                 workspace.data_ptr(), workspace.numel())
    return dq, dk, dv


@torch.no_grad()
def dropout_keep(seed, step, B, H, P, N, p):
    """The keep mask (B, H, P, N) bool of the step a device counter holds (step: (1,) int32 on the GPU, not advanced), by
    the device function the kernels call (pdm_mha_dropout_keep)."""
    keep = torch.empty((B, H, P, N), dtype=torch.uint8, device=step.device)
    _native.call("pdm_mha_dropout_keep", _native.stream(step.device), B, H, P, N, _check_p(p), int(seed) & 0xFFFFFFFF,
                 step.data_ptr(), keep.data_ptr())
    return keep.bool()


_SEPARATE, _PACKED_KV, _PACKED_QKV = 0, 1, 2


def _unpack(mode, tensors):
    if mode == _SEPARATE:
        return tensors
    if mode == _PACKED_KV:
        q, kv = tensors
        C = q.shape[-1]
        return q, kv[..., :C], kv[..., C:]
    qkv, = tensors
    C = qkv.shape[-1] // 3
    return qkv[..., :C], qkv[..., C:2 * C], qkv[..., 2 * C:]


class _MhaFunction(torch.autograd.Function):
    """saves q, k, v (as they were passed: packed stays packed), out, stats and used_step; never a (P, N) tensor"""

    @staticmethod
    def forward(ctx, mode, nheads, p, draws, kpc, *tensors):
        q, k, v = _unpack(mode, tensors)
        out, stats, used = mha_forward_train(q, k, v, nheads, p, draws, kpc)
        ctx.mode, ctx.nheads, ctx.p, ctx.kpc = mode, nheads, p, kpc
        ctx.seed, ctx.has_step = (draws.seed if p > 0.0 else 0), used is not None
        ctx.save_for_backward(*tensors, out, stats, *([used] if used is not None else []))
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dout):
        saved = ctx.saved_tensors
        used = saved[-1] if ctx.has_step else None
        n = len(saved) - 2 - int(ctx.has_step)
        tensors, out, stats = saved[:n], saved[n], saved[n + 1]
        q, k, v = _unpack(ctx.mode, tensors)
        if ctx.mode == _SEPARATE:
            grads = (torch.empty_like(q, memory_format=torch.contiguous_format), torch.empty_like(k, memory_format=torch.contiguous_format),
                     torch.empty_like(v, memory_format=torch.contiguous_format))
        else:                               # one packed buffer, written through the row strides
            grads = tuple(torch.empty(t.shape, dtype=torch.float32, device=t.device) for t in tensors)
        dq, dk, dv = _unpack(ctx.mode, grads)
        mha_backward(q, k, v, out, dout.contiguous(), stats, ctx.nheads, ctx.p, ctx.seed, used, ctx.kpc, dq=dq, dk=dk, dv=dv)
        return (None, None, None, None, None) + tuple(grads)


def _mha(mode, tensors, nheads, dropout_p, draws, keys_per_chunk):
    nheads, kpc, p = int(nheads), int(keys_per_chunk), _check_p(dropout_p)
    if p > 0.0 and draws is None:
        raise ValueError('mha: dropout_p > 0 needs draws (AttentionDraws)')
    q, k, v = _unpack(mode, tensors)
    if not q.is_cuda:                       # the CPU path: torch operators under torch autograd, the same draws
        keep = None
        if p > 0.0:
            step = int(draws.step.item()) & 0xFFFFFFFF
            keep = torch.from_numpy(dropout_keep_host(draws.seed, step, q.shape[0], nheads, q.shape[1], k.shape[1], p))
            draws.step.add_(1)
        return mha_torch(q, k, v, nheads, keep, p)
    return _MhaFunction.apply(mode, nheads, p, draws, kpc, *tensors)


def mha(q, k, v, nheads, dropout_p=0.0, draws=None, keys_per_chunk=0):
    """Differentiable fused attention: q (B, P, C), k, v (B, N, C) fp32, each in a row layout of its own -> (B, P, C).
    dropout_p is the attention dropout on the softmax weights, drawn from draws (AttentionDraws), whose device counter the
    forward advances.  Autograd keeps q, k, v, out, (B, H, P, 2) statistics and the step; the weights are never stored."""
    return _mha(_SEPARATE, (q, k, v), nheads, dropout_p, draws, keys_per_chunk)


def mha_kv(q, kv, nheads, dropout_p=0.0, draws=None, keys_per_chunk=0):
    """mha with k and v the halves of kv (B, N, 2C); the backward writes one (B, N, 2C) gradient through the row strides"""
    assert kv.dim() == 3 and kv.shape[-1] == 2 * q.shape[-1], (q.shape, kv.shape)
    return _mha(_PACKED_KV, (q, kv), nheads, dropout_p, draws, keys_per_chunk)


def mha_qkv(qkv, nheads, dropout_p=0.0, draws=None, keys_per_chunk=0):
    """self-attention on qkv (B, P, 3C) = [Q; K; V]; the backward writes one (B, P, 3C) gradient"""
    assert qkv.dim() == 3 and qkv.shape[-1] % 3 == 0, qkv.shape
    return _mha(_PACKED_QKV, (qkv,), nheads, dropout_p, draws, keys_per_chunk)

"""Fused multi-head attention forward (csrc/attention.hip): softmax(q_h k_h^T / sqrt(d)) v_h per head in fp32 on the MFMA,
the keys split into chunks so that few queries against many keys still fill the device; two launches, no host read, no
float atomics, two runs give the same bits, safe to capture in a torch.cuda.graph after one warm-up call.  Forward only.

The torch formulation it replaces is nn.MultiheadAttention between its in- and out-projection (mha_reference below): the
CPU path, and what the tests compare with.
"""
import math

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

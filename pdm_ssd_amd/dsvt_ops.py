"""DSVT's two operators (csrc/dsvt.hip) and the torch formulations they replace.

set_partition      the input layer of one stage, both shifts: window ids, in-window coordinates, the rotated set partition
                   (set_voxel_inds, two axes a shift) and its key masks, from an occupancy bitmap and two tiled scans: nine
                   launches and ONE host read (the two set counts) against the reference's four torch.unique, six torch.sort and
                   an atomic counter per (stage, shift).  The partition is a pure function of voxel_coords: two runs give the same
                   bits, and the result equals set_partition_torch exactly.
set_attention      softmax(q_h k_h^T / sqrt(d) + mask) v_h per set and head on per-voxel q, k, v rows gathered through
                   set_voxel_inds, written back at every voxel's row: one launch, nothing of size (S, ss, C) or (S, H, ss, ss) in
                   memory, no atomics, capturable.  Inference only: the operators have no backward (set_attention_torch is
                   differentiable and is what training runs).

set_partition_torch and set_attention_torch are the CPU path and what the tests compare with.
"""
import ctypes
import math
from collections import namedtuple

import torch

from . import _native

HOST_READS = 0      # host reads of set_partition, counted for tools/dsvt_rate.py

SetPartition = namedtuple('SetPartition', 'coors_in_win set_voxel_inds set_voxel_mask')


def _ceil_div(a, b):
    return -(-int(a) // int(b))


def _windows(sparse_shape, window_shape, shift):
    """(sx, sy, sz), (wx, wy, wz), (hx, hy, hz) as ints, the z shift 0 where the window spans z, and the windows per axis with
    the extra one a shift can reach"""
    sx, sy, sz = (int(v) for v in sparse_shape)
    wx, wy, wz = (int(v) for v in window_shape)
    hx, hy, hz = (int(v) for v in shift)
    if sz == wz:
        hz = 0
    return (sx, sy, sz), (wx, wy, wz), (hx, hy, hz), (_ceil_div(sx, wx) + 1, _ceil_div(sy, wy) + 1, _ceil_div(sz, wz) + 1)


@torch.no_grad()
def window_coors(coors, sparse_shape, window_shape, shift):
    """coors (N, 4) integer rows (b, z, y, x) -> (batch_win_inds (N), coors_in_win (N, 3) as (z, y, x)): the id of the window
    a voxel falls into after adding `shift` (x, y, z), ((b MX + X // wx) MY + Y // wy) MZ + Z // wz, and its place inside."""
    _, (wx, wy, wz), (hx, hy, hz), (mx, my, mz) = _windows(sparse_shape, window_shape, shift)
    c = coors.long()
    X, Y, Z = c[:, 3] + hx, c[:, 2] + hy, c[:, 1] + hz
    win = ((c[:, 0] * mx + X // wx) * my + Y // wy) * mz + Z // wz
    return win, torch.stack([Z % wz, Y % wy, X % wx], dim=-1)


@torch.no_grad()
def pooling_index(coors, sparse_shape, window_shape):
    """The pooling between two stages: coors (N, 4) (b, z, y, x) -> (batch_win_inds (N), coors_in_win (N, 3) (z, y, x),
    index_in_win (N) = (ix wy + iy) wz + iz, batch_win_coords (N, 4) (b, z, y, x) of the pooled voxel); no extra window."""
    sx, sy, sz = (int(v) for v in sparse_shape)
    wx, wy, wz = (int(v) for v in window_shape)
    mx, my, mz = _ceil_div(sx, wx), _ceil_div(sy, wy), _ceil_div(sz, wz)
    c = coors.long()
    gx, gy, gz = c[:, 3] // wx, c[:, 2] // wy, c[:, 1] // wz
    ix, iy, iz = c[:, 3] % wx, c[:, 2] % wy, c[:, 1] % wz
    win = ((c[:, 0] * mx + gx) * my + gy) * mz + gz
    return win, torch.stack([iz, iy, ix], dim=-1), (ix * wy + iy) * wz + iz, torch.stack([c[:, 0], gz, gy, gx], dim=-1)


def mask_of(set_voxel_inds):
    """a slot is masked when it holds the voxel of its left neighbour in the set"""
    mask = torch.zeros_like(set_voxel_inds, dtype=torch.bool)
    mask[..., 1:] = set_voxel_inds[..., 1:] == set_voxel_inds[..., :-1]
    return mask


@torch.no_grad()
def _sets_one_shift(coors, sparse_shape, window_shape, shift, set_size):
    win, ciw = window_coors(coors, sparse_shape, window_shape, shift)
    wx, wy, wz = (int(v) for v in window_shape)
    max_voxel, ss, dev = wx * wy * wz, int(set_size), coors.device
    N = coors.shape[0]
    if N == 0:
        return ciw, torch.zeros((2, 0, ss), dtype=torch.long, device=dev)
    _, cwin, count = torch.unique(win, return_inverse=True, return_counts=True)     # ascending window ids
    sets = (count + ss - 1) // ss
    first_set = torch.cumsum(sets, 0) - sets
    first_voxel = torch.cumsum(count, 0) - count
    S = int(sets.sum())
    # every slot: its window, its number k among the window's slots, the number of the voxel it takes
    slot_win = torch.repeat_interleave(torch.arange(len(sets), device=dev), sets * ss)
    k = torch.arange(S * ss, device=dev) - (first_set * ss)[slot_win]
    take = (k * count[slot_win]) // (sets[slot_win] * ss) + first_voxel[slot_win]
    iz, iy, ix = ciw[:, 0], ciw[:, 1], ciw[:, 2]
    out = []
    for key in ((iy * wx + ix) * wz + iz, (ix * wy + iy) * wz + iz):
        order = torch.argsort(cwin * max_voxel + key)           # distinct voxels give distinct keys: the order is determined
        out.append(order[take].reshape(S, ss))
    return ciw, torch.stack(out, 0)


@torch.no_grad()
def set_partition_torch(voxel_coords, sparse_shape, window_shapes, shifts, set_size):
    """The reference's window and set partition of one stage in torch operators, with the in-window numbering fixed by the
    sort keys (the reference's result does not depend on it).  voxel_coords (N, 4) (b, z, y, x) distinct voxels; sparse_shape
    (sx, sy, sz); window_shapes and shifts: one (x, y, z) triple a shift -> SetPartition(coors_in_win (2, N, 3) int64,
    [set_voxel_inds (2, S_shift, set_size) int64 per shift], [bool masks])."""
    ciws, inds = [], []
    for w, h in zip(window_shapes, shifts):
        ciw, ind = _sets_one_shift(voxel_coords, sparse_shape, w, h, set_size)
        ciws.append(ciw)
        inds.append(ind)
    return SetPartition(torch.stack(ciws, 0), inds, [mask_of(i) for i in inds])


@torch.no_grad()
def set_partition(voxel_coords, batch_size, sparse_shape, window_shapes, shifts, set_size, workspace=None):
    """set_partition_torch on the device (pdm_dsvt_partition_count, pdm_dsvt_partition): voxel_coords (N, 4) int32 on the GPU ->
    SetPartition(coors_in_win (2, N, 3) int32, [set_voxel_inds (2, S_shift, set_size) int64], [bool masks]).  ONE host read.
    A coordinate outside the sparse shape, set_size < 1 or a workspace sized for smaller windows raise NativeLibraryError."""
    global HOST_READS
    assert voxel_coords.is_cuda and voxel_coords.dtype == torch.int32 and voxel_coords.dim() == 2 and voxel_coords.shape[1] == 4, \
        'voxel_coords: int32 (N, 4) rows (b, z, y, x) on the GPU'
    coords = voxel_coords if voxel_coords.is_contiguous() else voxel_coords.contiguous()
    assert len(window_shapes) == 2 and len(shifts) == 2
    N, B, ss, dev = coords.shape[0], int(batch_size), int(set_size), coords.device
    sx, sy, sz = (int(v) for v in sparse_shape)
    win = _native.host_array(ctypes.c_int, [v for w in window_shapes for v in w])
    sh = _native.host_array(ctypes.c_int, [v for h in shifts for v in h])
    if workspace is None:
        nbytes = _native.lib().pdm_dsvt_partition_workspace_bytes(N, B, sx, sy, sz, win)
        workspace = torch.empty(max(nbytes, 8), dtype=torch.uint8, device=dev)
    ciw = torch.empty((2, N, 3), dtype=torch.int32, device=dev)
    counts = _native.host_array(ctypes.c_int, [0, 0])
    geom = (N, coords.data_ptr(), B, sx, sy, sz, win, sh, ss)
    _native.call("pdm_dsvt_partition_count", _native.stream(dev), *geom, ciw.data_ptr(), counts, workspace.data_ptr(), workspace.numel())
    HOST_READS += 1
    S = [int(counts[0]), int(counts[1])]
    inds = [torch.empty((2, s, ss), dtype=torch.int64, device=dev) for s in S]
    mask = [torch.empty((2, s, ss), dtype=torch.uint8, device=dev) for s in S]
    _native.call("pdm_dsvt_partition", _native.stream(dev), *geom, S[0], S[1], inds[0].data_ptr(), mask[0].data_ptr(), inds[1].data_ptr(),
                 mask[1].data_ptr(), workspace.data_ptr(), workspace.numel())
    return SetPartition(ciw, inds, [m.view(torch.bool) for m in mask])


def _check_attention(who, q, k, v, set_voxel_inds, nheads):
    N, C = q.shape
    S, ss = set_voxel_inds.shape
    nheads = int(nheads)
    if nheads < 1 or C % nheads or C // nheads not in (16, 24, 32) or C > 256 or not 1 <= ss <= 128:
        raise ValueError(f'{who}: C = {C}, heads = {nheads}, set_size = {ss}: needs C / heads in {{16, 24, 32}}, C <= 256 and '
                         '1 <= set_size <= 128')
    assert k.shape == (N, C) and v.shape == (N, C), (q.shape, k.shape, v.shape)
    return N, C, S, ss, nheads


def set_attention_torch(q, k, v, set_voxel_inds, nheads, dropout_p=0.0, training=False):
    """q, k, v (N, C), set_voxel_inds (S, ss) -> (N, C): what nn.MultiheadAttention computes between its in- and
    out-projection on the gathered sets with the duplicate slots masked as keys, each voxel's row taken from its unmasked slot.
    Torch operators in the inputs' dtype, differentiable; dropout_p acts on the softmax weights when training."""
    N, C, S, ss, nheads = _check_attention('set_attention_torch', q, k, v, set_voxel_inds, nheads)
    d = C // nheads
    mask = mask_of(set_voxel_inds)
    qh, kh, vh = (t[set_voxel_inds].reshape(S, ss, nheads, d).transpose(1, 2) for t in (q, k, v))
    score = qh @ kh.transpose(-1, -2) / math.sqrt(d)
    score = score.masked_fill(mask[:, None, None, :], float('-inf'))
    w = torch.softmax(score, dim=-1)
    if training and dropout_p > 0.0:
        w = torch.nn.functional.dropout(w, dropout_p)
    att = (w @ vh).transpose(1, 2).reshape(S * ss, C)
    live = ~mask.reshape(-1)
    out = q.new_zeros((N, C))
    return out.index_copy(0, set_voxel_inds.reshape(-1)[live], att[live])


def _row_stride(name, t, C):
    assert t.is_cuda and t.dtype == torch.float32 and t.dim() == 2 and t.shape[1] == C, f'{name}: fp32 (N, {C}) on the GPU'
    sr, sc = t.stride()
    if (sc != 1 and C > 1) or sr < C:
        raise ValueError(f'{name}: strides {tuple(t.stride())}: rows of contiguous elements')
    return sr


@torch.no_grad()
def set_attention(q, k, v, set_voxel_inds, nheads, out=None):
    """set_attention_torch fused (pdm_set_attention): q, k, v (N, C) fp32 on the GPU, each with its own row stride (the thirds
    of one (N, 3C) projection serve), set_voxel_inds (S, ss) int64 -> out (N, C).  The mask is derived from the indices.
    d = C / nheads in {16, 24, 32}, C <= 256, 1 <= ss <= 128; anything else raises ValueError.  Rows that no set names keep
    what `out` held (a fresh `out` is zero-filled only when there is no set at all)."""
    N, C, S, ss, nheads = _check_attention('set_attention', q, k, v, set_voxel_inds, nheads)
    qs, ks, vs = _row_stride('q', q, C), _row_stride('k', k, C), _row_stride('v', v, C)
    assert set_voxel_inds.is_cuda and set_voxel_inds.dtype == torch.int64
    inds = set_voxel_inds if set_voxel_inds.is_contiguous() else set_voxel_inds.contiguous()
    if out is None:
        out = torch.empty((N, C), dtype=torch.float32, device=q.device) if S else torch.zeros((N, C), dtype=torch.float32, device=q.device)
    assert out.shape == (N, C) and out.dtype == torch.float32 and out.is_contiguous()
    _native.call("pdm_set_attention", _native.stream(q.device), S, ss, N, C, nheads, q.data_ptr(), qs, k.data_ptr(), ks, v.data_ptr(), vs,
                 inds.data_ptr(), out.data_ptr())
    return out

"""Python side of csrc/train_gemm.hip: the bf16 contractions of the training path on this library's own MFMA kernels.

Rows layout throughout: a channels-last activation tensor IS a (rows, channels) matrix.  No fallback: the calls raise
when the HIP library is missing or an argument does not fit (callers test `usable()` first and otherwise keep torch)."""
import os

import torch

from . import _native


def usable(rows, k, n):
    """shapes the kernels take: channel counts multiples of 8 (16-byte rows)"""
    return rows > 0 and k > 0 and n > 0 and k % 8 == 0 and n % 8 == 0


def row_view(x):
    """(rows, C) view of a bf16 tensor whose storage is rows x C with the channel fastest: a contiguous (R, C) matrix, a
    channels-last (B, C, H, W) tensor or a (B, C, L) tensor stored (B, L, C).  None when the layout is something else."""
    if x.dim() == 2:
        return x if x.stride(1) == 1 and x.stride(0) >= x.shape[1] else None
    if x.dim() >= 3:
        xm = x.movedim(1, -1)
        if xm.is_contiguous():
            return xm.reshape(-1, x.shape[1])
    return None


def pack_weight(w, transposed=False, pad_to=None):
    """fp32 (N, K) parameter -> bf16 (N, ld) copy (round to nearest even), or its transpose (K, ld); ld = the row length
    rounded up to a multiple of 8 (pad_to overrides), pad columns zero."""
    assert w.dim() == 2 and w.is_cuda and w.dtype == torch.float32
    w = w.detach().contiguous()
    N, K = w.shape
    inner = N if transposed else K
    ld = (inner + 7) // 8 * 8 if pad_to is None else pad_to
    out = torch.empty((K if transposed else N, ld), dtype=torch.bfloat16, device=w.device)
    _native.call("pdm_tg_pack_weight", _native.stream(w), N, K, w.data_ptr(), 0 if transposed else out.data_ptr(), 0 if transposed else ld,
                 out.data_ptr() if transposed else 0, ld if transposed else 0)
    return out


def pack_weight_into(w, out, transposed=False):
    """the same into the top-left block of an existing bf16 matrix `out` (rows >= N or K, row stride = out.stride(0)); what
    lies outside the block is left as it is (callers that need zero padding allocate zeros)"""
    assert w.dim() == 2 and w.is_cuda and w.dtype == torch.float32 and out.dtype == torch.bfloat16 and out.stride(1) == 1
    w = w.detach().contiguous()
    N, K = w.shape
    assert out.shape[0] >= (K if transposed else N) and out.shape[1] >= (N if transposed else K)
    ld = out.stride(0)
    # the kernel writes ld columns per row: rows of the block are rewritten whole (pad columns zero)
    _native.call("pdm_tg_pack_weight", _native.stream(w), N, K, w.data_ptr(), 0 if transposed else out.data_ptr(), 0 if transposed else ld,
                 out.data_ptr() if transposed else 0, ld if transposed else 0)
    return out


def _pack_weight_pair_now(w, rows_to, cols_to, buf=None):
    N, K = w.shape
    if buf is None:
        buf = torch.empty((2, rows_to * cols_to), dtype=torch.bfloat16, device=w.device)     # the kernel writes the padding too
    wb, wt = buf[0].view(rows_to, cols_to), buf[1].view(cols_to, rows_to)
    _native.call("pdm_tg_pack_weight_pair", _native.stream(w), N, K, w.data_ptr(), wb.data_ptr(), wt.data_ptr(), rows_to, cols_to)
    return wb, wt


# The packed pairs of a model's parameters are kept between calls and refreshed TOGETHER: a parameter changes once per optimizer
# step, and a training step of the detector packed ~40 of them in 40 launches.  An entry remembers the parameter (weakly), its
# storage address, its version counter (torch bumps it on in-place updates: load_state_dict, copy_, the foreach optimizers) and the
# count of optimizer steps seen so far (the FUSED optimizers move no version counter: _watch_optimizers);
# the first request that finds a stale entry — or that asks for a pair a second time since the last refresh, i.e. at the start of
# every new pass over a model — repacks EVERY live entry in one launch (pdm_tg_pack_weight_many over a job table in device memory,
# rebuilt only when the set of entries changes).  The buffers are persistent: a pair handed out (and saved for a
# backward) is overwritten by the next refresh, i.e. after the parameter itself has been overwritten.  PDM_PACK_CACHE=0: one launch
# per request, fresh buffers.  Not used while a stream is being captured into a graph.  What the cache cannot see — a write through
# `.data` or a raw pointer that is not followed by a new pass over the same layers — needs invalidate_packs().
PACK_CACHE = os.environ.get("PDM_PACK_CACHE", "1") == "1"
_packs = {}                       # (device index, address, N, K, rows_to, cols_to) -> [weakref(parameter), buffer (2, rows_to * cols_to), version, epoch]
_pack_tables = {}                 # device index -> (job table tensor, njobs, total blocks, tuple of keys)
_served = {}                      # device index -> keys handed out since the last refresh
_opt_epoch = [0, False]           # [optimizer steps seen (a global post-step hook), hook registered]


def _note_optimizer_step(*_args, **_kwargs):
    _opt_epoch[0] += 1


def _watch_optimizers():
    """torch's FUSED multi-tensor optimizers (AdamW(fused=True): bench.py's default) update parameters without moving their version
    counters — a cache keyed on the counter alone served the initial weights for a whole run (final loss 250 instead of 25 after 14
    steps).  Every optimizer step therefore also advances an epoch (a global post-step hook) that the entries remember."""
    if not _opt_epoch[1]:
        _opt_epoch[1] = True
        from torch.optim.optimizer import register_optimizer_step_post_hook
        register_optimizer_step_post_hook(_note_optimizer_step)


def _refresh_packs(dev_index, device):
    import weakref  # noqa: F401
    import numpy as np
    live = []
    for key in [k for k in _packs if k[0] == dev_index]:
        ref, buf = _packs[key][0], _packs[key][1]
        base = ref()
        if base is None or base.data_ptr() != key[1]:
            del _packs[key]                           # the parameter is gone (or moved): its pair with it
        else:
            live.append((key, base, buf))
    keys = tuple((k, buf.data_ptr()) for k, _, buf in live)       # the table holds addresses: parameters AND buffers
    table = _pack_tables.get(dev_index)
    if table is None or table[3] != keys:
        rec = np.zeros(len(live), dtype=np.dtype([('W', '<u8'), ('Wb', '<u8'), ('Wt', '<u8'), ('N', '<i4'), ('K', '<i4'), ('rows_to', '<i4'),
                                                   ('cols_to', '<i4'), ('first_block', '<i8')]))
        first = 0
        for j, (key, base, buf) in enumerate(live):
            _, ptr, N, K, rows_to, cols_to = key
            rec[j] = (ptr, buf[0].data_ptr(), buf[1].data_ptr(), N, K, rows_to, cols_to, first)
            first += (rows_to * cols_to + 255) // 256
        host = torch.from_numpy(rec.view(np.uint8).copy())
        table = (host.to(device), len(live), first, keys)
        _pack_tables[dev_index] = table
    if table[1]:
        _native.call("pdm_tg_pack_weight_many", _native.stream(device), table[1], table[0].data_ptr(), table[2])
    for key, base, _ in live:
        _packs[key][2] = base._version
        _packs[key][3] = _opt_epoch[0]


def invalidate_packs():
    """Forget every cached pair (the next requests pack afresh).  For edits the cache cannot see: a write through `.data` or a raw
    pointer between two requests that are not a pass apart."""
    _packs.clear()
    _pack_tables.clear()
    _served.clear()


def pack_weight_pair(w, rows_to, cols_to):
    """fp32 (N, K) parameter -> (wb (rows_to, cols_to), wt (cols_to, rows_to)) bf16: the weight for the forward product and
    its transpose for the data gradient, zero padded (rows_to >= N, cols_to >= K, both multiples of 8), in ONE launch — and, for
    a parameter seen before, no launch at all until the parameter changes (see PACK_CACHE above)."""
    assert w.dim() == 2 and w.is_cuda and w.dtype == torch.float32
    base = w._base if w._base is not None else w
    if not (PACK_CACHE and w.is_contiguous() and base.data_ptr() == w.data_ptr() and not torch.cuda.is_current_stream_capturing()):
        return _pack_weight_pair_now(w.detach().contiguous(), rows_to, cols_to)
    import weakref
    _watch_optimizers()
    N, K = w.shape
    key = (w.device.index, w.data_ptr(), N, K, rows_to, cols_to)
    ent = _packs.get(key)
    served = _served.setdefault(w.device.index, set())
    if ent is not None and ent[0]() is base:
        # stale by the version counter, OR asked for a second time since the last refresh: a new pass over the model has begun, and
        # an edit through `.data` (which moves no version counter) may lie in between — one refresh launch per pass either way
        if ent[2] != base._version or ent[3] != _opt_epoch[0] or key in served:
            _refresh_packs(w.device.index, w.device)
            served.clear()
        served.add(key)
        buf = ent[1]
        return buf[0].view(rows_to, cols_to), buf[1].view(cols_to, rows_to)
    served.add(key)
    if len(_packs) > 4096:                             # models come and go (tests): drop the pairs of dead parameters
        for k in [k for k, e in _packs.items() if e[0]() is None]:
            del _packs[k]
    buf = torch.empty((2, rows_to * cols_to), dtype=torch.bfloat16, device=w.device)
    _packs[key] = [weakref.ref(base), buf, base._version, _opt_epoch[0]]
    return _pack_weight_pair_now(w.detach(), rows_to, cols_to, buf)


def gemm_nt_bs(x, w, bx, bcoef):
    """gemm_nt whose product y (R, N) IS the gradient of relu(bn(bx)) (the data gradient of the layer behind that BatchNorm + ReLU):
    also returns the per-slot sums (parts, N, 2) of g = y [bn(bx) > 0] and g xhat taken in the epilogue — what
    pdm_bn_relu_backward_stats' reduce pass would read y and bx again for (finalize: bn_bwd_finalize).  bx (R, N) bf16 rows, bcoef
    (4, N) fp32 from pdm_bn_finalize_stats."""
    R, K = x.shape
    N = w.shape[0]
    assert x.dtype == torch.bfloat16 and w.dtype == torch.bfloat16 and bx.dtype == torch.bfloat16 and x.stride(1) == 1 and w.stride(1) == 1
    assert bx.shape == (R, N) and bx.stride(1) == 1 and bcoef.shape == (4, N) and bcoef.dtype == torch.float32 and bcoef.is_contiguous()
    y = torch.empty((R, N), dtype=torch.bfloat16, device=x.device)
    st = torch.empty((_native.lib().pdm_tg_stats_parts(R, N), N, 2), dtype=torch.float32, device=x.device)
    _native.call("pdm_tg_gemm_nt_bs", _native.stream(x), R, K, N, x.data_ptr(), x.stride(0), w.data_ptr(), w.stride(0), y.data_ptr(), y.stride(0),
                 bx.data_ptr(), bx.stride(0), bcoef.data_ptr(), st.data_ptr())
    return y, st


def bn_bwd_finalize(rows, coef, partial):
    """grads (4, C) fp32 = [dgamma | dbeta | p | q] of a BatchNorm + ReLU backward from the (parts, C, 2) sums a producing
    contraction took (gemm_nt_bs / gemm_nt_dy(..., bs=...))."""
    C = coef.shape[1]
    assert partial.shape[1:] == (C, 2) and partial.dtype == torch.float32 and partial.is_contiguous()
    grads = torch.empty((4, C), dtype=torch.float32, device=coef.device)
    _native.call("pdm_bn_finalize_bwd_stats", _native.stream(coef), rows, C, coef.data_ptr(), grads.data_ptr(), partial.data_ptr(), partial.shape[0])
    return grads


def gemm_nt(x, w, bias=None, stats=False, out=None, x_bn_coef=None, pool_ns=0):
    """x (R, K) bf16 rows (row stride a multiple of 8), w (N, K') bf16 with K' >= K zero padded -> y (R, N) bf16 =
    x . w^T [+ bias], fp32 accumulation, one rounding.  stats=True also returns the column sums (parts, N, 2) fp32 (sum y,
    sum y^2 of the rounded y, one part per persistent workgroup slot): what pdm_bn_relu_forward_stats takes.
    x_bn_coef (4, K) fp32: x is read through BatchNorm + ReLU with these coefficients (the layer before's, unapplied)."""
    R, K = x.shape
    N = w.shape[0]
    assert x.dtype == torch.bfloat16 and w.dtype == torch.bfloat16 and x.stride(1) == 1 and w.stride(1) == 1
    y = torch.empty((R, N), dtype=torch.bfloat16, device=x.device) if out is None else out
    st = None
    if stats:
        st = torch.empty((_native.lib().pdm_tg_stats_parts(R, N), N, 2), dtype=torch.float32, device=x.device)
    if pool_ns:
        # the product feeds BatchNorm + ReLU + max over groups of pool_ns consecutive rows: the epilogue also leaves each group's max / min
        # per channel and the first index attaining them (pdm_tg_gemm_nt_pool); returns (y, stats, (keep (2, G, N) bf16, idx (2, G, N) uint8))
        assert stats and R % pool_ns == 0
        G = R // pool_ns
        keep = torch.empty((2, G, N), dtype=torch.bfloat16, device=x.device)
        idx = torch.empty((2, G, N), dtype=torch.uint8, device=x.device)
        _native.call("pdm_tg_gemm_nt_pool", _native.stream(x), R, K, N, x.data_ptr(), x.stride(0), w.data_ptr(), w.stride(0), y.data_ptr(), y.stride(0),
                     0 if bias is None else bias.data_ptr(), st.data_ptr(), 0 if x_bn_coef is None else x_bn_coef.data_ptr(), pool_ns,
                     keep[0].data_ptr(), keep[1].data_ptr(), idx[0].data_ptr(), idx[1].data_ptr())
        return y, st, (keep, idx)
    _native.call("pdm_tg_gemm_nt", _native.stream(x), R, K, N, x.data_ptr(), x.stride(0), w.data_ptr(), w.stride(0), y.data_ptr(), y.stride(0),
                 0 if bias is None else bias.data_ptr(), 0 if st is None else st.data_ptr(),
                 0 if x_bn_coef is None else x_bn_coef.data_ptr())
    return (y, st) if stats else y


def gemm_nt_dy(dz, yp, coef, grads, w, bs=None):
    """Data gradient straight behind a BatchNorm + ReLU backward: dz (R, K) bf16 = the gradient of relu(bn(yp)), yp (R, K) bf16 the
    BatchNorm's input, coef / grads (4, K) fp32 from pdm_bn_finalize_stats / pdm_bn_relu_backward_stats, w (N, K) bf16 ->
    (dx (R, N) bf16 = dy . w^T, dy (R, K) bf16) with dy = the BatchNorm + ReLU backward of dz, formed while dz and yp are read
    (bit for bit pdm_bn_relu_backward's dx)."""
    R, K = dz.shape
    N = w.shape[0]
    assert dz.dtype == torch.bfloat16 and yp.dtype == torch.bfloat16 and w.dtype == torch.bfloat16 and yp.shape == dz.shape
    assert dz.stride(1) == 1 and yp.stride(1) == 1 and w.stride(1) == 1 and coef.shape == (4, K) and grads.shape == (4, K)
    dx = torch.empty((R, N), dtype=torch.bfloat16, device=dz.device)
    dy = torch.empty((R, K), dtype=torch.bfloat16, device=dz.device)
    if bs is not None:
        # bs = (bx (R, N) bf16, bcoef (4, N)): dx is itself the gradient of relu(bn(bx)); its statistics leave through the epilogue
        # (see gemm_nt_bs); returns (dx, dy, partial (parts, N, 2))
        bx, bcoef = bs
        assert bx.shape == (R, N) and bx.dtype == torch.bfloat16 and bx.stride(1) == 1 and bcoef.shape == (4, N) and bcoef.is_contiguous()
        st = torch.empty((_native.lib().pdm_tg_dy_stats_parts(R, N), N, 2), dtype=torch.float32, device=dz.device)
        _native.call("pdm_tg_gemm_nt_dy_bs", _native.stream(dz), R, K, N, dz.data_ptr(), dz.stride(0), yp.data_ptr(), yp.stride(0), w.data_ptr(),
                     w.stride(0), dx.data_ptr(), dx.stride(0), dy.data_ptr(), dy.stride(0), coef.data_ptr(), grads.data_ptr(),
                     bx.data_ptr(), bx.stride(0), bcoef.data_ptr(), st.data_ptr())
        return dx, dy, st
    _native.call("pdm_tg_gemm_nt_dy", _native.stream(dz), R, K, N, dz.data_ptr(), dz.stride(0), yp.data_ptr(), yp.stride(0), w.data_ptr(),
                 w.stride(0), dx.data_ptr(), dx.stride(0), dy.data_ptr(), dy.stride(0), coef.data_ptr(), grads.data_ptr())
    return dx, dy


def wgrad(dy, x, out=None, accumulate=False, x_bn_coef=None):
    """dy (R, N) bf16, x (R, K) bf16 -> dW (N, K) fp32 = dy^T . x (fp32 accumulation, deterministic)."""
    R, N = dy.shape
    K = x.shape[1]
    assert dy.dtype == torch.bfloat16 and x.dtype == torch.bfloat16 and x.shape[0] == R and dy.stride(1) == 1 and x.stride(1) == 1
    dw = torch.empty((N, K), dtype=torch.float32, device=x.device) if out is None else out
    nbytes = _native.lib().pdm_tg_wgrad_ws_bytes(R, K, N)
    ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=x.device)
    _native.call("pdm_tg_wgrad", _native.stream(x), R, K, N, dy.data_ptr(), dy.stride(0), x.data_ptr(), x.stride(0), dw.data_ptr(),
                 1 if accumulate else 0, ws.data_ptr(), nbytes, 0 if x_bn_coef is None else x_bn_coef.data_ptr())
    return dw


def colsum(y):
    """y (R, N) bf16 rows (N a multiple of 8, <= 512) -> (N,) fp32 column sums, fixed summation order (a bias gradient)."""
    R, N = y.shape
    assert y.dtype == torch.bfloat16 and y.stride(1) == 1 and N % 8 == 0 and N <= 512
    out = torch.empty((N,), dtype=torch.float32, device=y.device)
    ws = torch.empty((max(_native.lib().pdm_tg_colsum_ws_floats(R, N), 4),), dtype=torch.float32, device=y.device)
    _native.call("pdm_tg_colsum", _native.stream(y), R, N, y.data_ptr(), y.stride(0), out.data_ptr(), ws.data_ptr())
    return out

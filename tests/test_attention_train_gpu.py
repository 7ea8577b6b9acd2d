"""pdm_mha_forward_train and pdm_mha_backward on the GPU against float64 torch autograd of attention_ops.mha_torch on the CPU.

The bound has the form of test_attention_gpu.py's and takes its factor from it: for out, dq, dk and dv,
err_kernel <= 8 * err_torch, both maximum absolute errors against the float64 run, err_torch the error of fp32 torch autograd of
mha_torch on the device with the same inputs, dout and mask (the host mask uploaded).  The ratios are printed
(tools/attention_train_rate.py records them at the workload shapes).

Where the softmax is nearly one-hot (test_forced_rescale's inputs) D = dO . O cancels worse than torch's sum_j P dP: there dq and
dk are held against mha_backward_torch, the same algebra in torch operators, in fp32 on the device.
"""
import math

import numpy as np
import pytest
import torch

import test_attention_gpu as fwd
from arena import Arena
from pdm_ssd_amd import _native, attention_ops

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
FACTOR = 8.0
NAMES = ('out', 'dq', 'dk', 'dv')
SEED = 77


def host_keep(B, nh, P, N, p, step=0, seed=SEED):
    return None if p == 0.0 else torch.from_numpy(attention_ops.dropout_keep_host(seed, step, B, nh, P, N, p))


def autograd(q, k, v, dout, nh, keep, p):
    q, k, v = (t.detach().clone().requires_grad_(True) for t in (q, k, v))
    out = attention_ops.mha_torch(q, k, v, nh, keep, p)
    return (out.detach(),) + torch.autograd.grad(out, (q, k, v), dout)


def reference64(q, k, v, dout, nh, keep, p):
    return autograd(q.double().cpu(), k.double().cpu(), v.double().cpu(), dout.double().cpu(), nh, keep, p)


def kernel(q, k, v, dout, nh, p, kpc, seed=SEED):
    """out, dq, dk, dv through attention_ops.mha and autograd, the draws at step 0"""
    q, k, v = (t.detach().clone().requires_grad_(True) for t in (q, k, v))
    out = attention_ops.mha(q, k, v, nh, p, attention_ops.AttentionDraws(seed, DEV) if p > 0.0 else None, kpc)
    return (out.detach(),) + torch.autograd.grad(out, (q, k, v), dout)


def errors(got, want):
    return [float((g.double().cpu() - w).abs().max()) for g, w in zip(got, want)]


def check(name, got, base, want, which=NAMES):
    """got, base: (out, dq, dk, dv) of the kernel and of the comparator; want: the float64 reference"""
    eg, eb = errors(got, want), errors(base, want)
    for n, a, b in zip(NAMES, eg, eb):
        print(f'attention train {name} {n}: err_kernel {a:.3e} err_base {b:.3e} ratio {a / max(b, 1e-300):.3f}')
    for n, g, a, b in zip(NAMES, got, eg, eb):
        assert bool(torch.isfinite(g).all()), (name, n)
        if n in which:
            assert a <= FACTOR * b, (name, n, a, b)


def dout_like(B, P, C, seed):
    return torch.randn((B, P, C), generator=torch.Generator().manual_seed(seed)).to(DEV)


# ---- 1. float64 comparison -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('p', [0.0, 0.1])
@pytest.mark.parametrize('case', range(5))
def test_against_float64(case, p):
    B, P, N, C, nh, kpc = fwd.shapes()[case]
    q, k, v = fwd.inputs(B, P, N, C, 100 + case)
    dout = dout_like(B, P, C, 200 + case)
    keep = host_keep(B, nh, P, N, p)
    got = kernel(q, k, v, dout, nh, p, kpc)
    base = autograd(q, k, v, dout, nh, None if keep is None else keep.to(DEV), p)
    check(f'{(B, P, N, C, nh, kpc)} p = {p}', got, base, reference64(q, k, v, dout, nh, keep, p))


# ---- 2. forward bits and the saved maximum ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', range(5))
def test_forward_bits_and_the_raw_maximum(case):
    B, P, N, C, nh, kpc = fwd.shapes()[case]
    d = C // nh
    q, k, v = fwd.inputs(B, P, N, C, 100 + case)
    out, stats, used = attention_ops.mha_forward_train(q, k, v, nh, 0.0, None, kpc)
    assert used is None and torch.equal(out, attention_ops.mha_forward(q, k, v, nh, kpc))
    heads = lambda t: t.reshape(B, t.shape[1], nh, d).transpose(1, 2)
    want = (heads(q.double().cpu()) @ heads(k.double().cpu()).transpose(-1, -2)).max(-1).values
    torch32 = (heads(q) @ heads(k).transpose(-1, -2)).max(-1).values
    err_kernel = float((stats[..., 0].double().cpu() - want).abs().max())
    err_torch = float((torch32.double().cpu() - want).abs().max())
    print(f'attention train raw maximum {(B, P, N, C, nh, kpc)}: err_kernel {err_kernel:.3e} err_torch {err_torch:.3e}')
    assert err_kernel <= FACTOR * err_torch
    # the sum belongs to that maximum: exp(s - M) summed over the keys, at least the maximum's own 1
    assert bool((stats[..., 1] >= 1.0).all()) and bool((stats[..., 1] <= N).all())


# ---- 3. the mask on the device ---------------------------------------------------------------------------------------------------------
def test_device_mask_is_the_host_mask():
    step = torch.tensor([5], dtype=torch.int32, device=DEV)
    got = attention_ops.dropout_keep(SEED, step, 2, 2, 37, 247, 0.1)
    assert got.dtype == torch.bool and int(step) == 5
    assert np.array_equal(got.cpu().numpy(), attention_ops.dropout_keep_host(SEED, 5, 2, 2, 37, 247, 0.1))
    assert bool(attention_ops.dropout_keep(SEED, step, 1, 2, 3, 5, 0.0).all())


# ---- 4. forced rescale -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('p', [0.0, 0.1])
@pytest.mark.parametrize('where', list(fwd.SPIKES))
@pytest.mark.parametrize('C, nh', [(32, 2), (64, 2)])
def test_forced_rescale_backward(where, C, nh, p):
    """test_attention_gpu.test_forced_rescale's inputs: scores near 120, one key 30 above.  dv against torch autograd as in
    case 1; dq and dk against the D = dO . O formulation in torch operators, whose cancellation sets the scale here."""
    B, P, N, kpc = 1, 16, 300, 128
    d = C // nh
    g = torch.Generator().manual_seed(23)
    u = torch.randn(C, generator=g)
    u = (u.reshape(nh, d) / u.reshape(nh, d).norm(dim=1, keepdim=True)).reshape(C)
    q = torch.randn((B, P, C), generator=g) * 0.1 + 2.0 * u
    k = torch.randn((B, N, C), generator=g) * 0.5 + (60.0 * math.sqrt(d)) * u
    k[:, fwd.SPIKES[where]] += (15.0 * math.sqrt(d)) * u
    v = torch.randn((B, N, C), generator=g)
    q, k, v = q.to(DEV), k.to(DEV), v.to(DEV)
    dout = dout_like(B, P, C, 29)
    keep = host_keep(B, nh, P, N, p)
    keep_dev = None if keep is None else keep.to(DEV)
    want = reference64(q, k, v, dout, nh, keep, p)
    got = kernel(q, k, v, dout, nh, p, kpc)
    check(f'spike in the {where}, d = {d}, p = {p} (torch autograd)', got, autograd(q, k, v, dout, nh, keep_dev, p), want, ('out', 'dv'))
    out32 = attention_ops.mha_torch(q, k, v, nh, keep_dev, p)
    formulation = (out32,) + attention_ops.mha_backward_torch(q, k, v, out32, dout, nh, keep_dev, p)
    check(f'spike in the {where}, d = {d}, p = {p} (D = dO . O in torch)', got, formulation, want, ('dq', 'dk'))


# ---- 5. one key, one query -------------------------------------------------------------------------------------------------------------
def test_single_key_single_query():
    q, k, v = fwd.inputs(2, 1, 1, 32, 7)
    dout = dout_like(2, 1, 32, 8)
    out, dq, dk, dv = kernel(q, k, v, dout, 2, 0.0, 0)
    assert torch.equal(out, v) and torch.equal(dv, dout)
    assert bool(torch.isfinite(dq).all()) and bool(torch.isfinite(dk).all())


# ---- 6. fully dropped rows -------------------------------------------------------------------------------------------------------------
def test_a_fully_dropped_row():
    B, P, N, C, nh, p = 1, 64, 1, 32, 2, 0.5
    d = C // nh
    q, k, v = fwd.inputs(B, P, N, C, 9)
    dout = dout_like(B, P, C, 10)
    keep = host_keep(B, nh, P, N, p)                                   # (1, nh, P, 1)
    assert not keep.all() and keep.any()
    out, dq, dk, dv = kernel(q, k, v, dout, nh, p, 0)
    scaled = v * (np.float32(1.0) / (np.float32(1.0) - np.float32(0.5))).item()
    kept = keep[0, :, :, 0].t().to(DEV)[:, :, None].expand(P, nh, d).reshape(1, P, C)      # per (query, head) -> channels
    assert torch.equal(out, torch.where(kept, scaled.expand(1, P, C), torch.zeros_like(out)))
    assert all(bool(torch.isfinite(t).all()) for t in (dq, dk, dv))
    # dv of the one key = the kept rows' dout, scaled; a dropped row adds nothing
    # (a sum of at most P fp32 terms in some order: |error| <= P 2^-24 sum |term|)
    terms = dout.double() * kept.double() * 2.0
    bound = P * 2.0 ** -24 * terms.abs().sum(1, keepdim=True)
    assert bool(((dv.double() - terms.sum(1, keepdim=True)).abs() <= bound).all())


# ---- 7. packed buffers and strides -----------------------------------------------------------------------------------------------------
def grads_of(fn, tensors, dout):
    leaves = [t.detach().clone().requires_grad_(True) for t in tensors]
    out = fn(*leaves)
    return (out.detach(),) + torch.autograd.grad(out, leaves, dout)


def test_packed_kv_and_a_padded_query_stride():
    B, P, N, C, nh, p = 2, 12, 240, 32, 2, 0.1
    g = torch.Generator().manual_seed(11)
    kv = torch.randn((B, N, 2 * C), generator=g).to(DEV)
    qpad = torch.randn((B, P, C + 8), generator=g).to(DEV)
    dout = dout_like(B, P, C, 12)
    draws = lambda: attention_ops.AttentionDraws(SEED, DEV)
    out, dqpad, dkv = grads_of(lambda a, b: attention_ops.mha_kv(a[..., :C], b, nh, p, draws(), 64), (qpad, kv), dout)
    assert dkv.shape == kv.shape and dkv.is_contiguous() and not bool(torch.isnan(dkv).any())
    want = kernel(qpad[..., :C].contiguous(), kv[..., :C].contiguous(), kv[..., C:].contiguous(), dout, nh, p, 64)
    assert torch.equal(out, want[0]) and torch.equal(dqpad[..., :C], want[1]) and not dqpad[..., C:].any()
    assert torch.equal(dkv[..., :C], want[2]) and torch.equal(dkv[..., C:], want[3])
    # the packed buffer is written everywhere: a poisoned one of the caller's, through the row strides
    q, k, v = qpad[..., :C], kv[..., :C], kv[..., C:]
    o, stats, used = attention_ops.mha_forward_train(q, k, v, nh, p, draws(), 64)
    packed = torch.full((B, N, 2 * C), float('nan'), device=DEV)
    attention_ops.mha_backward(q, k, v, o, dout, stats, nh, p, SEED, used, 64, dk=packed[..., :C], dv=packed[..., C:])
    assert torch.equal(packed, dkv)
    with pytest.raises(ValueError, match='strides'):
        attention_ops.mha_kv(q.transpose(0, 1).contiguous().transpose(0, 1), kv, nh)


def test_packed_qkv():
    B, P, C, nh, p = 2, 37, 64, 2, 0.1
    qkv = torch.randn((B, P, 3 * C), generator=torch.Generator().manual_seed(13)).to(DEV)
    dout = dout_like(B, P, C, 14)
    out, dqkv = grads_of(lambda a: attention_ops.mha_qkv(a, nh, p, attention_ops.AttentionDraws(SEED, DEV)), (qkv,), dout)
    assert dqkv.shape == qkv.shape and dqkv.is_contiguous()
    want = kernel(*(qkv[..., i * C:(i + 1) * C].contiguous() for i in range(3)), dout, nh, p, 0)
    assert torch.equal(out, want[0])
    for i in range(3):
        assert torch.equal(dqkv[..., i * C:(i + 1) * C], want[1 + i]), i
    with pytest.raises(ValueError, match='strides'):
        attention_ops.mha_qkv(qkv.transpose(0, 1).contiguous().transpose(0, 1), nh)


# ---- 8. determinism --------------------------------------------------------------------------------------------------------------------
def test_two_runs_give_the_same_bits_and_the_counter_advances_by_one():
    B, P, N, C, nh, kpc, p = 1, 37, 247, 64, 2, 64, 0.1
    q, k, v = fwd.inputs(B, P, N, C, 31)
    dout = dout_like(B, P, C, 32)
    draws = attention_ops.AttentionDraws(SEED, DEV)

    def run():
        leaves = [t.detach().clone().requires_grad_(True) for t in (q, k, v)]
        out = attention_ops.mha(*leaves, nh, p, draws, kpc)
        return (out.detach(),) + torch.autograd.grad(out, leaves, dout)
    first = run()
    assert int(draws.step) == 1
    second = run()
    assert int(draws.step) == 2 and not torch.equal(first[0], second[0])
    draws.reset(0)
    again = run()
    assert int(draws.step) == 1
    for n, a, b in zip(NAMES, first, again):
        assert torch.equal(a, b), n
    for n, a, b in zip(NAMES, first, kernel(q, k, v, dout, nh, p, kpc)):          # a fresh counter at 0
        assert torch.equal(a, b), n


def test_a_graph_replay_gives_the_eager_bits():
    B, P, N, C, nh, kpc = 1, 37, 247, 64, 2, 64
    q, k, v = fwd.inputs(B, P, N, C, 33)
    dout = dout_like(B, P, C, 34)

    def run():
        out, stats, _ = attention_ops.mha_forward_train(q, k, v, nh, 0.0, None, kpc)
        return (out,) + attention_ops.mha_backward(q, k, v, out, dout, stats, nh, 0.0, 0, None, kpc)
    eager = run()                                                      # (the warm-up call as well)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = run()
    graph.replay()
    torch.cuda.synchronize()
    for n, a, b in zip(NAMES, eager, captured):
        assert torch.equal(a, b), n


# ---- 9. arena --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('off', [4, 8, 12])
def test_arena_offsets(off):
    B, P, N, C, nh, kpc, p = 1, 37, 247, 64, 2, 64, 0.1
    q0, k0, v0 = fwd.inputs(B, P, N, C, 41)
    dout0 = dout_like(B, P, C, 42)
    want = kernel(q0, k0, v0, dout0, nh, p, kpc)
    arena = Arena(DEV, nbytes=8 << 20)
    nan = float('nan')
    q, k, v = arena.put(q0, off, nan), arena.put(k0, (off + 4) % 16, nan), arena.put(v0, (off + 8) % 16, nan)
    dout = arena.put(dout0, (off + 12) % 16, nan)
    out = arena.carve((B, P, C), torch.float32, off)
    stats = arena.carve((B, nh, P, 2), torch.float32, 4)
    dq, dk, dv = (arena.carve((B, n, C), torch.float32, (off + 4 * i) % 16) for i, n in enumerate((P, N, N)))
    lib = _native.lib()
    ws_f = arena.carve(lib.pdm_mha_forward_train_workspace_bytes(B, P, N, C, nh, kpc), torch.uint8, 8)
    ws_b = arena.carve(lib.pdm_mha_backward_workspace_bytes(B, P, N, C, nh, kpc), torch.uint8, 8)
    draws = attention_ops.AttentionDraws(SEED, DEV)
    o, s, used = attention_ops.mha_forward_train(q, k, v, nh, p, draws, kpc, out=out, stats=stats, workspace=ws_f)
    got = attention_ops.mha_backward(q, k, v, o, dout, s, nh, p, SEED, used, kpc, dq=dq, dk=dk, dv=dv, workspace=ws_b)
    assert o.data_ptr() == out.data_ptr() and got[0].data_ptr() == dq.data_ptr()
    for n, a, b in zip(NAMES, (o,) + got, want):
        assert torch.equal(a, b), n
    arena.check()


# ---- 10. refusals ----------------------------------------------------------------------------------------------------------------------
def test_refusals():
    q, k, v = fwd.inputs(1, 4, 100, 32, 5)
    dout = dout_like(1, 4, 32, 6)
    out, stats, _ = attention_ops.mha_forward_train(q, k, v, 2, 0.0, None, 64)
    with pytest.raises(_native.NativeLibraryError, match='workspace'):
        attention_ops.mha_backward(q, k, v, out, dout, stats, 2, keys_per_chunk=64, workspace=torch.empty(64, dtype=torch.uint8, device=DEV))
    with pytest.raises(_native.NativeLibraryError, match='workspace'):
        attention_ops.mha_forward_train(q, k, v, 2, 0.0, None, 64, workspace=torch.empty(64, dtype=torch.uint8, device=DEV))
    with pytest.raises(ValueError):
        attention_ops.mha(q, k, v, 4)                                  # d = 8
    big = torch.zeros((1, 4, 512), device=DEV)
    with pytest.raises(ValueError):
        attention_ops.mha(big, big, big, 16)                           # C = 512
    with pytest.raises(ValueError):
        attention_ops.mha(q, k, v, 2, 1.0, attention_ops.AttentionDraws(0, DEV))
    with pytest.raises(ValueError):
        attention_ops.mha(q, k, v, 2, 0.1)                             # dropout without draws
    lib = _native.lib()
    assert lib.pdm_mha_backward_workspace_bytes(1, 4, 100, 32, 4, 0) == 0 and lib.pdm_mha_backward_workspace_bytes(1, 4, 100, 512, 16, 0) == 0
    # the C entry points refuse by themselves what the Python layer refuses first
    rc = lib.pdm_mha_backward(None, 1, 4, 100, 32, 4, *([None, 32] * 3), None, None, None, 0.0, 0, None, 0, *([None, 32] * 3), None, 0)
    assert rc != 0 and b'heads' in lib.pdm_last_error()
    rc = lib.pdm_mha_forward_train(None, 1, 4, 100, 32, 2, *([None, 32] * 3), 0, 1.0, 0, None, None, None, None, None, 0)
    assert rc != 0 and b'dropout_p' in lib.pdm_last_error()


# ---- 11. no P x N tensor ---------------------------------------------------------------------------------------------------------------
def test_no_p_by_n_tensor_is_allocated():
    B, P, N, C, nh, p = 1, 200, 8192, 128, 8, 0.1
    g = torch.Generator().manual_seed(51)
    q = torch.randn((B, P, C), generator=g).to(DEV).requires_grad_(True)
    kv = torch.randn((B, N, 2 * C), generator=g).to(DEV).requires_grad_(True)
    dout = dout_like(B, P, C, 52)
    draws = attention_ops.AttentionDraws(SEED, DEV)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out = attention_ops.mha_kv(q, kv, nh, p, draws)
    out.backward(dout)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    limit = B * nh * P * N * 4 // 2
    print(f'attention train peak allocation {peak / 1e6:.1f} MB, limit {limit / 1e6:.1f} MB')
    assert q.grad is not None and kv.grad.shape == kv.shape
    assert peak < limit

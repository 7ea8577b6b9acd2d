"""pdm_mha_forward on the GPU against a float64 softmax(Q K^T / sqrt(d)) V computed on the CPU over the full tensor.

The bound: err_kernel <= 8 * err_torch, both maximum absolute errors against that reference, err_torch the error of
torch.nn.functional.scaled_dot_product_attention in fp32 on the device with the same inputs.  The factor 8 covers the
chunked summation order and a hardware exp2 against torch's expf; it admits nothing coarser than fp32.  The observed
ratios are printed (tools/transfusion_rate.py records them in profiles/transfusion_rate.json).
"""
import math

import numpy as np
import pytest
import torch

from arena import Arena
from pdm_ssd_amd import attention_ops

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
FACTOR = 8.0


def reference64(q, k, v, nheads):
    return attention_ops.mha_reference(q.double().cpu(), k.double().cpu(), v.double().cpu(), nheads)


def sdpa(q, k, v, nheads):
    B, P, C = q.shape
    d = C // nheads
    qh, kh, vh = (t.reshape(B, t.shape[1], nheads, d).transpose(1, 2) for t in (q, k, v))
    return torch.nn.functional.scaled_dot_product_attention(qh, kh, vh).transpose(1, 2).reshape(B, P, C)


def check(name, q, k, v, nheads, out):
    """out: the kernel's result for (q, k, v); asserts finiteness and the bound, prints the figures first"""
    want = reference64(q, k, v, nheads)
    err_kernel = float((out.double().cpu() - want).abs().max())
    err_torch = float((sdpa(q.contiguous(), k.contiguous(), v.contiguous(), nheads).double().cpu() - want).abs().max())
    print(f'attention {name}: err_kernel {err_kernel:.3e} err_torch {err_torch:.3e} ratio {err_kernel / max(err_torch, 1e-300):.3f}')
    assert bool(torch.isfinite(out).all())
    assert err_kernel <= FACTOR * err_torch, (name, err_kernel, err_torch)
    return err_kernel, err_torch


def inputs(B, P, N, C, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn((B, n, C), generator=g).to(DEV) for n in (P, N, N)]


def shapes():
    kd = attention_ops.default_keys_per_chunk()
    return [(2, 12, 240, 32, 2, 0), (1, 37, 247, 64, 2, 64), (1, 16, 1000, 128, 8, 64), (1, 200, 200, 128, 8, 0), (1, 5, 3 * kd + 5, 32, 2, 0)]


@pytest.mark.parametrize('case', range(5))
def test_against_float64(case):
    B, P, N, C, nh, kpc = shapes()[case]
    q, k, v = inputs(B, P, N, C, 100 + case)
    out = attention_ops.mha_forward(q, k, v, nh, kpc)
    assert out.shape == (B, P, C) and out.dtype == torch.float32
    check(f'{(B, P, N, C, nh, kpc)}', q, k, v, nh, out)


def test_single_key_returns_the_value_row_bit_for_bit():
    q, k, v = inputs(2, 1, 1, 32, 7)
    out = attention_ops.mha_forward(q, k, v, 2)
    assert torch.equal(out, v)


def test_halves_of_one_projection_and_a_padded_query_stride():
    B, P, N, C, nh = 2, 12, 240, 32, 2
    g = torch.Generator().manual_seed(11)
    kv = torch.randn((B, N, 2 * C), generator=g).to(DEV)
    qpad = torch.randn((B, P, C + 8), generator=g).to(DEV)
    q, k, v = qpad[..., :C], kv[..., :C], kv[..., C:]
    assert not k.is_contiguous() and not q.is_contiguous()
    out = attention_ops.mha_forward(q, k, v, nh, 64)
    check('strided', q, k, v, nh, out)
    assert torch.equal(out, attention_ops.mha_forward(q.contiguous(), k.contiguous(), v.contiguous(), nh, 64))
    with pytest.raises(ValueError, match='strides'):
        attention_ops.mha_forward(q.transpose(0, 1).contiguous().transpose(0, 1), k, v, nh)


SPIKES = {'first chunk': 5, 'middle chunk, second step': 128 + 70, 'partial last chunk': 290}


@pytest.mark.parametrize('where', list(SPIKES))
@pytest.mark.parametrize('C, nh', [(32, 2), (64, 2)])
def test_forced_rescale(where, C, nh):
    """One key's score exceeds every other by about 30, so the running maximum jumps at a chosen step, and all scores carry a
    common offset of about 120: exp overflows unless the maximum is subtracted.  N = 300 in chunks of 128: 128, 128, 44."""
    B, P, N, kpc = 1, 16, 300, 128
    d = C // nh
    g = torch.Generator().manual_seed(23)
    u = torch.randn(C, generator=g)
    u = (u.reshape(nh, d) / u.reshape(nh, d).norm(dim=1, keepdim=True)).reshape(C)       # a unit direction per head
    q = torch.randn((B, P, C), generator=g) * 0.1 + 2.0 * u
    k = torch.randn((B, N, C), generator=g) * 0.5 + (60.0 * math.sqrt(d)) * u           # q . k / sqrt(d) ~ 120 for every key
    k[:, SPIKES[where]] += (15.0 * math.sqrt(d)) * u                                    # ... and ~ 150 for this one
    v = torch.randn((B, N, C), generator=g)
    q, k, v = q.to(DEV), k.to(DEV), v.to(DEV)
    scores = torch.einsum('bphd,bnhd->bhpn', q.double().reshape(B, P, nh, d).cpu(), k.double().reshape(B, N, nh, d).cpu()) / math.sqrt(d)
    assert float(scores.min()) > 89.0, 'exp(score) must overflow fp32'
    rest = scores.clone()
    rest[..., SPIKES[where]] = -1e30
    assert float((scores[..., SPIKES[where]] - rest.max(-1).values).min()) > 15.0
    out = attention_ops.mha_forward(q, k, v, nh, kpc)
    check(f'spike in the {where}, d = {d}', q, k, v, nh, out)


def test_two_runs_and_a_graph_replay_give_the_same_bits():
    B, P, N, C, nh, kpc = 1, 37, 247, 64, 2, 64
    q, k, v = inputs(B, P, N, C, 31)
    first = attention_ops.mha_forward(q, k, v, nh, kpc)             # (the warm-up call as well)
    assert torch.equal(first, attention_ops.mha_forward(q, k, v, nh, kpc))
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = attention_ops.mha_forward(q, k, v, nh, kpc)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(first, captured)


@pytest.mark.parametrize('off', [4, 8, 12])
def test_arena_offsets(off):
    """q, k, v at 4-, 8- and 12-byte offsets between NaN red zones, the output and the workspace at offsets of their own"""
    B, P, N, C, nh, kpc = 1, 37, 247, 64, 2, 64
    q0, k0, v0 = inputs(B, P, N, C, 41)
    want = attention_ops.mha_forward(q0, k0, v0, nh, kpc)
    arena = Arena(DEV, nbytes=8 << 20)
    nan = float('nan')
    q, k, v = arena.put(q0, off, nan), arena.put(k0, (off + 4) % 16, nan), arena.put(v0, (off + 8) % 16, nan)
    out = arena.carve((B, P, C), torch.float32, off)
    from pdm_ssd_amd import _native
    nbytes = _native.lib().pdm_mha_forward_workspace_bytes(B, P, N, C, nh, kpc)
    ws = arena.carve(nbytes, torch.uint8, 8)
    got = attention_ops.mha_forward(q, k, v, nh, kpc, out=out, workspace=ws)
    assert got.data_ptr() == out.data_ptr() and torch.equal(got, want)
    arena.check()


def test_workspace_too_small_is_refused():
    from pdm_ssd_amd import _native
    q, k, v = inputs(1, 4, 100, 32, 5)
    with pytest.raises(_native.NativeLibraryError, match='workspace'):
        attention_ops.mha_forward(q, k, v, 2, 64, workspace=torch.empty(64, dtype=torch.uint8, device=DEV))

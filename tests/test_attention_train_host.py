"""The host side of training through the fused attention: the dropout draws' numpy restatement, the torch formulations
(mha_torch, mha_backward_torch) and the head's build-defined keys.  No GPU."""
import math

import numpy as np
import pytest
import torch

import transfusion_train_case as ttc
from pdm_ssd_amd import attention_ops

SHAPES = [(2 * 2, 12, 240), (8, 200, 200)]          # (B * H, P, N)


def test_the_mask_is_a_function_of_its_arguments_and_of_the_step():
    a = attention_ops.dropout_keep_host(7, 3, 2, 2, 12, 240, 0.1)
    assert a.dtype == np.bool_ and a.shape == (2, 2, 12, 240)
    assert np.array_equal(a, attention_ops.dropout_keep_host(7, 3, 2, 2, 12, 240, 0.1))
    assert not np.array_equal(a, attention_ops.dropout_keep_host(7, 4, 2, 2, 12, 240, 0.1))
    assert not np.array_equal(a, attention_ops.dropout_keep_host(8, 3, 2, 2, 12, 240, 0.1))
    # (b, h) enter as b * H + h alone
    assert np.array_equal(a.reshape(4, 12, 240), attention_ops.dropout_keep_host(7, 3, 1, 4, 12, 240, 0.1)[0])


def test_one_draw_restated_with_python_integers():
    def fmix(h):
        h ^= h >> 16; h = h * 0x85EBCA6B & 0xFFFFFFFF; h ^= h >> 13; h = h * 0xC2B2AE35 & 0xFFFFFFFF
        return h ^ (h >> 16)
    seed, step, B, H, P, N, p = 12345, 9, 2, 3, 5, 7, 0.25
    got = attention_ops.dropout_keep_host(seed, step, B, H, P, N, p)
    for bh, i, j in [(0, 0, 0), (5, 4, 6), (3, 2, 1)]:
        key = fmix(fmix(seed ^ (step * 0x85EBCA6B & 0xFFFFFFFF)) ^ (bh * 0x9E3779B1 & 0xFFFFFFFF) ^ (i * 0x7F4A7C15 & 0xFFFFFFFF))
        keep = fmix(key ^ (j * 0x9E3779B1 & 0xFFFFFFFF)) >= math.floor(p * 2 ** 32)
        assert bool(got[bh // H, bh % H, i, j]) == keep


@pytest.mark.parametrize('BH, P, N', SHAPES)
@pytest.mark.parametrize('p', [0.1, 0.5])
def test_kept_fraction_within_five_sigma_and_no_row_fully_dropped(BH, P, N, p):
    for step in range(3):
        keep = attention_ops.dropout_keep_host(0, step, 1, BH, P, N, p)
        n = keep.size
        frac = keep.sum() / n
        print(f'kept fraction {(BH, P, N)} p = {p} step {step}: {frac:.4f}')
        assert abs(frac - (1.0 - p)) <= 5.0 * math.sqrt(p * (1.0 - p) / n)
        assert keep.any(axis=-1).all()


def test_p_zero_keeps_everything_and_p_one_is_refused():
    assert attention_ops.dropout_keep_host(1, 2, 2, 2, 3, 5, 0.0).all()
    with pytest.raises(ValueError):
        attention_ops.dropout_keep_host(1, 2, 2, 2, 3, 5, 1.0)


def inputs(B, P, N, C, seed, dtype=torch.float64):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn((B, n, C), generator=g, dtype=dtype) for n in (P, N, N, P)]


def test_mha_torch_without_a_mask_is_mha_reference():
    q, k, v, _ = inputs(2, 12, 50, 32, 1, torch.float32)
    assert torch.equal(attention_ops.mha_torch(q, k, v, 2), attention_ops.mha_reference(q, k, v, 2))


@pytest.mark.parametrize('p', [0.0, 0.1])
def test_the_explicit_backward_is_autograd_in_float64(p):
    B, P, N, C, nh = 2, 12, 50, 32, 2
    q, k, v, dout = inputs(B, P, N, C, 2)
    keep = None if p == 0.0 else torch.from_numpy(attention_ops.dropout_keep_host(3, 0, B, nh, P, N, p))
    for t in (q, k, v):
        t.requires_grad_(True)
    out = attention_ops.mha_torch(q, k, v, nh, keep, p)
    want = torch.autograd.grad(out, (q, k, v), dout)
    got = attention_ops.mha_backward_torch(q.detach(), k.detach(), v.detach(), out.detach(), dout, nh, keep, p)
    for name, a, b in zip(('dq', 'dk', 'dv'), got, want):
        assert float((a - b).abs().max()) <= 1e-12, name


def test_mha_on_the_cpu_is_the_torch_path_with_the_same_draws():
    B, P, N, C, nh, p = 1, 5, 9, 32, 2, 0.5
    q, k, v, _ = inputs(B, P, N, C, 4, torch.float32)
    draws = attention_ops.AttentionDraws(11, 'cpu')
    out = attention_ops.mha(q, k, v, nh, p, draws)
    keep = torch.from_numpy(attention_ops.dropout_keep_host(11, 0, B, nh, P, N, p))
    assert torch.equal(out, attention_ops.mha_torch(q, k, v, nh, keep, p)) and int(draws.step) == 1


def build_head(**keys):
    from pdm_ssd_amd.config import cfg_from_dict
    from pdm_ssd_amd.dense_heads import TransFusionHead
    import transfusion_case as tc
    cfg = ttc.train_cfg()
    cfg.update(keys)
    return TransFusionHead(model_cfg=cfg_from_dict(cfg), **tc.head_kwargs())


def test_the_keys_set_the_layer_and_leave_the_state_dict_alone():
    plain, fused = build_head(), build_head(FUSED_ATTENTION_TRAIN=True, ATTENTION_DROPOUT_SEED=5)
    assert plain.decoder.fused_train is False and plain.decoder.attention_seed == 0
    assert fused.decoder.fused_train is True and fused.decoder.attention_seed == 5
    assert list(plain.state_dict()) == list(fused.state_dict())
    assert len(fused.state_dict()) == 96
    assert not any('attn_step' in k for k in fused.state_dict())


def test_the_config_is_the_training_config_plus_the_key():
    import copy
    from pdm_ssd_amd import detector_config as dc
    want = copy.deepcopy(dc.TRANSFUSION_LIDAR_TRAIN_CFG)
    want['DENSE_HEAD']['FUSED_ATTENTION_TRAIN'] = True
    assert dc.TRANSFUSION_LIDAR_FUSED_TRAIN_CFG == want
    assert 'FUSED_ATTENTION_TRAIN' not in dc.TRANSFUSION_LIDAR_TRAIN_CFG['DENSE_HEAD']

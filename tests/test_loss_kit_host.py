"""The host tables the loss operators' entry points take (_native.map_tables, its per-channel sibling) and the one map check
(_native.check_map): no GPU."""
import types

import pytest
import torch

from pdm_ssd_amd import _native


def test_map_tables_of_none_a_permuted_bf16_view_and_padding():
    plain = torch.zeros((2, 3, 4, 5))
    view = torch.zeros((2, 4, 5, 3), dtype=torch.bfloat16).permute(0, 3, 1, 2)      # channels last
    ptrs, bf, st = _native.map_tables([plain, None, view])
    assert len(ptrs) == 3 and len(bf) == 3 and len(st) == 12
    assert ptrs[0] == plain.data_ptr() and bf[0] == 0 and list(st[0:4]) == [60, 20, 5, 1]
    assert ptrs[1] is None and bf[1] == 0 and list(st[4:8]) == [0, 0, 0, 0]
    assert ptrs[2] == view.data_ptr() and bf[2] == 1 and list(st[8:12]) == list(view.stride()) == [60, 1, 15, 3]
    ptrs, bf, st = _native.map_tables([view], slots=6)
    assert len(ptrs) == 6 and len(bf) == 6 and len(st) == 24
    assert ptrs[0] == view.data_ptr() and bf[0] == 1 and list(st[0:4]) == [60, 1, 15, 3]
    assert all(ptrs[k] is None and bf[k] == 0 for k in range(1, 6)) and not any(st[4:24])
    with pytest.raises(AssertionError, match='3 maps for 2 slots'):
        _native.map_tables([plain, None, view], slots=2)


def test_channel_tables_name_every_channel_as_a_plane():
    a = torch.zeros((2, 2, 4, 5))
    b = torch.zeros((2, 4, 5, 3), dtype=torch.bfloat16).permute(0, 3, 1, 2)
    ptrs, bf, st = _native.channel_tables([a, b])
    assert [ptrs[k] for k in range(5)] == [a.data_ptr(), a.data_ptr() + 4 * 20, b.data_ptr(), b.data_ptr() + 2, b.data_ptr() + 4]
    assert list(bf) == [0, 0, 1, 1, 1]
    assert list(st) == [40, 5, 1] * 2 + [60, 15, 3] * 3


def fake_map(shape, dtype=torch.float32, is_cuda=True):
    """what check_map reads of a tensor, so that its second assertion is reached without a GPU"""
    return types.SimpleNamespace(is_cuda=is_cuda, dtype=dtype, shape=torch.Size(shape), dim=lambda: len(shape))


def test_check_map_rejects_dtype_rank_and_channels_with_the_old_messages():
    _native.check_map('box_preds', fake_map((2, 14, 4, 5)), 2, 4, 5, 14)
    _native.check_map('hm', fake_map((2, 3, 4, 5), torch.bfloat16), 2, 4, 5)
    first = r'box_preds: fp32 or bf16 \(B, C, H, W\) on the GPU'
    with pytest.raises(AssertionError, match=first):
        _native.check_map('box_preds', fake_map((2, 14, 4, 5), torch.float16), 2, 4, 5, 14)
    with pytest.raises(AssertionError, match=first):
        _native.check_map('box_preds', fake_map((2, 14, 20)), 2, 4, 5, 14)
    with pytest.raises(AssertionError, match=first):
        _native.check_map('box_preds', torch.zeros((2, 14, 4, 5)), 2, 4, 5, 14)           # a CPU tensor
    with pytest.raises(AssertionError, match=r'box_preds: \(2, 12, 4, 5\), expected \(2, 14, 4, 5\)'):
        _native.check_map('box_preds', fake_map((2, 12, 4, 5)), 2, 4, 5, 14)
    with pytest.raises(AssertionError, match=r'map 1: \(2, 3, 4, 6\)$'):
        _native.check_map('map 1', fake_map((2, 3, 4, 6)), 2, 4, 5)

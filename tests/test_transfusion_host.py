"""TransFusionHead without a GPU: state-dict keys, the CPU path against the reference fixture, the torch formulations kept next
to the two operators, the builder, and the arguments that are refused."""
import numpy as np
import pytest
import torch

import transfusion_case as tc
from pdm_ssd_amd import attention_ops, transfusion_ops

TAGS = list(tc.TAGS)


@pytest.fixture(scope='module')
def heads():
    return {tag: tc.build_head(tag) for tag in TAGS}


@pytest.fixture(scope='module')
def predictions(heads):
    x = torch.from_numpy(tc.fixture()['spatial_features_2d'])
    with torch.no_grad():
        return {tag: heads[tag].predict(x) for tag in TAGS}


@pytest.mark.parametrize('tag', TAGS)
def test_state_dict_keys_and_shapes_are_the_references(heads, tag):
    want = tc.manifest()[f'state.{tag}']
    got = {k: list(v.shape) for k, v in heads[tag].state_dict().items()}
    assert len(want) == 96 and sorted(got) == sorted(want)             # (the manifest is written with sorted keys)
    assert got == want


def test_fixture_margins_hold():
    man, fx = tc.manifest(), tc.fixture()
    for tag, exempt in (('nus', (8, 9)), ('kitti', ())):
        tc.check_proposal_margins(tc.proposal_margins(fx[f'{tag}.dense_heatmap'], 3, exempt, tc.P), tc.P)
        assert man['margins'][tag]['decode_gap'] >= tc.MARGIN and min(man[f'kept.{tag}']) < tc.P
    assert not np.array_equal(fx['nus.index'], fx['kitti.index'])
    assert all(4 * g <= man['parity_abs'] for gaps in man['float32_to_float64_gap'].values() for g in gaps.values())


@pytest.mark.parametrize('tag', TAGS)
def test_cpu_head_reproduces_the_fixture(heads, predictions, tag):
    fx, tol = tc.fixture(), tc.manifest()['parity_abs']
    head, res = heads[tag], predictions[tag]
    assert np.array_equal(head.query_labels.numpy(), fx[f'{tag}.cls'])
    tc.check_predictions(res, tag, tol)
    dicts = head.get_bboxes(res)
    assert [len(d['pred_boxes']) for d in dicts] == tc.manifest()[f'kept.{tag}']
    tc.check_boxes(dicts, tag, tol)
    out = head({'batch_size': tc.B, 'spatial_features_2d': torch.from_numpy(fx['spatial_features_2d'])})
    tc.check_boxes(out['final_box_dicts'], tag, tol)


@pytest.mark.parametrize('tag, exempt', [('nus', [8, 9]), ('kitti', [])])
def test_torch_proposals_give_the_fixtures_queries(tag, exempt):
    fx = tc.fixture()
    index, cls, qhs, pos = transfusion_ops.proposals_torch(torch.from_numpy(fx[f'{tag}.dense_heatmap']), tc.P, 3, exempt, tc.H)
    assert index.dtype == torch.int64 and cls.dtype == torch.int64
    assert np.array_equal(index.numpy(), fx[f'{tag}.index']) and np.array_equal(cls.numpy(), fx[f'{tag}.cls'])
    assert np.array_equal(pos.numpy(), fx[f'{tag}.query_pos'])          # (n % 12 + 0.5, n // 12 + 0.5) on the 12 x 20 map
    tc.close(qhs.numpy(), fx[f'{tag}.query_heatmap_score'], 1e-6)


@pytest.mark.parametrize('tag', TAGS)
@pytest.mark.parametrize('vel', [True, False])
def test_torch_decode_gives_the_fixtures_boxes(tag, vel):
    tc.check_padded(tag, tc.fixture_decode(tag, transfusion_ops.decode_torch, vel=vel), vel)


def test_builder_builds_the_lidar_detector():
    from pdm_ssd_amd import detector_config
    from pdm_ssd_amd.dense_heads import TransFusionHead
    from pdm_ssd_amd.detectors import TransFusion
    net = detector_config.build_transfusion_lidar()
    assert isinstance(net, TransFusion) and isinstance(net.dense_head, TransFusionHead)
    head = net.dense_head
    assert len(head.state_dict()) == 96 and head.num_proposals == 200 and head.use_fused
    assert head.bev_pos.shape == (1, 180 * 180, 2) and head.decoder.nhead == 8
    assert not hasattr(head, 'bbox_assigner')


def test_training_mode_is_refused(heads):
    head = tc.build_head('nus').train()
    with pytest.raises(NotImplementedError, match='Hungarian'):
        head({'batch_size': tc.B, 'spatial_features_2d': torch.from_numpy(tc.fixture()['spatial_features_2d'])})


@pytest.mark.parametrize('fn', [transfusion_ops.decode, transfusion_ops.decode_torch], ids=['operator', 'torch'])
def test_negative_score_threshold_is_refused(fn):
    """(before anything touches a device: the operator's wrapper checks first)"""
    fx, man = tc.fixture(), tc.manifest()
    t = {k: torch.from_numpy(fx[f'nus.pred.{k}']) for k in tc.MAPS}
    with pytest.raises(ValueError, match='SCORE_THRESH'):
        fn(t['heatmap'], t['center'], t['height'], t['dim'], t['rot'], t['vel'], torch.from_numpy(fx['nus.cls']),
           torch.from_numpy(fx['nus.query_heatmap_score']), -0.1, man['post_center_range'], 0.0, 0.0, 0.05, 0.05, 8)


@pytest.mark.parametrize('C, heads_', [(32, 4), (64, 1), (30, 2), (512, 16)])
def test_unsupported_head_width_is_refused(C, heads_):
    q, kv = torch.zeros(1, 3, C), torch.zeros(1, 5, C)
    with pytest.raises(ValueError, match='C / heads'):
        attention_ops.mha_forward(q, kv, kv, heads_)


def test_library_rejects_what_the_wrapper_rejects():
    from pdm_ssd_amd import _native
    lib = _native.lib()
    assert lib.pdm_mha_forward_workspace_bytes(1, 3, 5, 32, 4, 0) == 0          # d = 8
    assert lib.pdm_mha_forward_workspace_bytes(1, 3, 5, 32, 2, 0) > 0
    assert lib.pdm_mha_forward(None, 1, 3, 5, 32, 4, None, 32, None, 32, None, 32, 0, None, None, 0) == -1   # PDM_E_BADARG
    assert b'C / heads' in lib.pdm_last_error()


def test_attention_reference_is_multihead_attention_between_its_projections():
    """mha_reference (the formulation the GPU tests and the module's fallback use) against nn.MultiheadAttention itself"""
    torch.manual_seed(0)
    C, nh, Pq, N, Bn = 32, 2, 5, 9, 2
    attn = torch.nn.MultiheadAttention(C, nh).eval().double()
    q, kv = torch.randn(Bn, Pq, C, dtype=torch.float64), torch.randn(Bn, N, C, dtype=torch.float64)
    with torch.no_grad():
        want = attn(q.transpose(0, 1), kv.transpose(0, 1), kv.transpose(0, 1))[0].transpose(0, 1)
        W, b = attn.in_proj_weight, attn.in_proj_bias
        lin = torch.nn.functional.linear
        mid = attention_ops.mha_reference(lin(q, W[:C], b[:C]), lin(kv, W[C:2 * C], b[C:2 * C]), lin(kv, W[2 * C:], b[2 * C:]), nh)
        got = lin(mid, attn.out_proj.weight, attn.out_proj.bias)
    assert float((got - want).abs().max()) <= 1e-12

"""TransFusion's decoder layer, head and detector trained through the fused attention (FUSED_ATTENTION_TRAIN): against the
nn.MultiheadAttention path of the same layer, the reference fixture of the head's loss, and themselves under dropout."""
import copy

import numpy as np
import pytest
import torch

import test_transfusion_train_gpu as base
import transfusion_case as tc
import transfusion_train_case as ttc

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
FACTOR = 8.0


def build_fused_head(dropout=0.0, **keys):
    """transfusion_train_case.build_train_head with the new key (and, for the dropout test, the shipped DROPOUT)"""
    from pdm_ssd_amd.config import cfg_from_dict
    from pdm_ssd_amd.dense_heads import TransFusionHead
    man = tc.manifest()
    cfg = ttc.train_cfg(FUSED_ATTENTION_TRAIN=True, **keys)
    cfg['DROPOUT'] = dropout
    head = TransFusionHead(model_cfg=cfg_from_dict(cfg), **tc.head_kwargs())
    total = tc.fill_transfusion(head, man['seed'], man['gain'], man['hm_gain'], man['hm_bias'])
    assert abs(total - man['weight_sum']) <= 1e-6 * man['weight_sum']
    return head.to(DEV).train()


def batch():
    fx = ttc.fixture()
    return {'batch_size': tc.B, 'spatial_features_2d': torch.from_numpy(fx['spatial_features_2d']).to(DEV),
            'gt_boxes': torch.from_numpy(fx['gt_boxes']).to(DEV)}


@pytest.mark.parametrize('fused_self, fused_cross', [(True, True), (False, True), (True, False)])
def test_decoder_layer_matches_the_torch_path_within_its_own_error(fused_self, fused_cross):
    """fused_self / fused_cross = False leaves that attention of the fused training path to torch operators"""
    from pdm_ssd_amd.utils.transfusion_utils import PositionEmbeddingLearned, TransformerDecoderLayer
    N = tc.H * tc.W
    layer = TransformerDecoderLayer(tc.HIDDEN, tc.NHEADS, tc.FFN, 0.0, 'relu', self_posembed=PositionEmbeddingLearned(2, tc.HIDDEN),
                                    cross_posembed=PositionEmbeddingLearned(2, tc.HIDDEN))
    tc.fill_transfusion(layer, 3)
    g = torch.Generator().manual_seed(4)
    query, key = torch.randn((tc.B, tc.HIDDEN, tc.P), generator=g), torch.randn((tc.B, tc.HIDDEN, N), generator=g)
    query_pos, key_pos = torch.rand((tc.B, tc.P, 2), generator=g) * 12, torch.rand((1, N, 2), generator=g) * 12
    dout = torch.randn((tc.B, tc.HIDDEN, tc.P), generator=g)

    def run(net, fused, cast):
        net = copy.deepcopy(net).to(cast[0], cast[1]).train()
        net.fused_train, net.fused_self, net.fused_cross = fused, fused_self, fused_cross
        out = net(*(t.to(cast[0], cast[1]) for t in (query, key, query_pos, key_pos)))
        out.backward(dout.to(cast[0], cast[1]))
        return {'out': out.detach().double().cpu(), **{n: p.grad.double().cpu() for n, p in net.named_parameters()}}
    want = run(layer, False, ('cpu', torch.float64))
    on, off = run(layer, True, (DEV, torch.float32)), run(layer, False, (DEV, torch.float32))
    assert set(on) == set(want) and len(on) > 30
    for name in want:
        e_on, e_off = float((on[name] - want[name]).abs().max()), float((off[name] - want[name]).abs().max())
        print(f'decoder layer (self {fused_self}, cross {fused_cross}) {name}: err_fused {e_on:.3e} err_torch {e_off:.3e}')
        assert e_on <= FACTOR * e_off, (name, e_on, e_off)


def test_head_reproduces_the_fixture_without_a_host_read():
    fx, man = ttc.fixture(), ttc.manifest()
    head = build_fused_head()
    assert head.decoder.fused_train and len(head.state_dict()) == 96
    head(batch())                                                       # (warm-up)
    b = batch()
    out, reads = base.host_reads(lambda: head(b))
    assert reads == 0
    assert np.array_equal(head.query_labels.cpu().numpy(), fx['cls'])
    assert np.array_equal(head.forward_ret_dict['targets']['assigned'].cpu().numpy(), fx['target.assigned'])
    tol = man['parity_abs'] + tc.manifest()['parity_abs'] * man['loss_sensitivity']
    tc.close(float(out['loss'].detach()), float(fx['loss_trans']), tol)


def test_dropout_in_the_head_replays_from_the_seed_and_the_counters():
    head = build_fused_head(dropout=0.1, ATTENTION_DROPOUT_SEED=3)
    assert head.decoder.attention_seed == 3

    def step():
        head.zero_grad()
        out = head(batch())
        out['loss'].backward()
        return out['loss'].detach().clone()
    torch.manual_seed(5)
    first, second = step(), step()
    assert int(head.decoder.attn_step_self) == 2 and int(head.decoder.attn_step_cross) == 2
    assert not torch.equal(first, second)
    for attn in (head.decoder.self_attn, head.decoder.multihead_attn):
        grad = attn.in_proj_weight.grad
        assert bool(torch.isfinite(grad).all()) and float(grad.abs().max()) > 0
    torch.manual_seed(5)
    head.decoder.reset_attention_steps()
    assert torch.equal(step(), first)


def test_detector_takes_a_training_step_through_the_fused_attention():
    """build_transfusion_lidar(TRANSFUSION_LIDAR_FUSED_TRAIN_CFG) at the shapes of test_detector_takes_a_training_step"""
    import pillarnet_reference as pnr
    import sparse_conv_reference as scr
    from pdm_ssd_amd import detector_config as dc
    cfg = copy.deepcopy(dc.TRANSFUSION_LIDAR_FUSED_TRAIN_CFG)
    cfg['DENSE_HEAD'].update(NUM_PROPOSALS=12)
    ds = dc.transfusion_dataset(point_cloud_range=[-9.6, -9.6, -5.0, 9.6, 9.6, 3.0], voxel_size=[0.1, 0.1, 0.2], grid_size=[192, 192, 40])
    torch.manual_seed(2)
    net = dc.build_transfusion_lidar(cfg, dataset=ds)
    assert net.dense_head.decoder.fused_train
    scr.fill_backbone(net.backbone_3d, 2, gain=0.6)
    pnr.fill_pillarnet(net.backbone_2d, 2)
    tc.fill_transfusion(net.dense_head, 2, 1.0, 54.1, -58.8)
    net = net.to(DEV).train()
    rng = np.random.default_rng(2)
    n = 8000
    rows = [np.concatenate([np.full((n, 1), b), rng.uniform(-9.5, 9.5, (n, 2)), rng.uniform(-4.8, 2.8, (n, 1)), rng.uniform(0, 1, (n, 2))], 1)
            for b in range(2)]
    pts = torch.from_numpy(np.concatenate(rows).astype(np.float32)).to(DEV)
    gt = np.zeros((2, 6, 10), dtype=np.float32)
    for b, m in ((0, 4), (1, 2)):
        gt[b, :m, :2] = rng.uniform(-8, 8, (m, 2))
        gt[b, :m, 2] = rng.uniform(-2, 0, m)
        gt[b, :m, 3:6] = rng.uniform(0.5, 4.0, (m, 3))
        gt[b, :m, 6] = rng.uniform(-3, 3, m)
        gt[b, :m, 9] = rng.integers(1, 11, m)
    ret, tb_dict, disp_dict = net({'batch_size': 2, 'points': pts, 'gt_boxes': torch.from_numpy(gt).to(DEV)})
    loss = ret['loss']
    assert bool(torch.isfinite(loss))
    assert int(net.dense_head.decoder.attn_step_cross) == 1            # the shipped DROPOUT = 0.1 drew once
    loss.backward()
    head = net.dense_head
    for name, p in head.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), name
    assert any(float(p.grad.abs().max()) > 0 for nm, p in head.named_parameters() if nm.startswith('decoder'))
    assert float(head.decoder.multihead_attn.in_proj_weight.grad.abs().max()) > 0

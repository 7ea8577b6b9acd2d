"""pdm_lsap, pdm_tf_assign, pdm_tf_loss and TransFusion's training step on the GPU: against the numpy solver, the reference
fixture (tests/golden/gen_transfusion_train_fixtures.py) and the torch formulations kept next to the operators."""
import warnings

import numpy as np
import pytest
import torch

import transfusion_case as tc
import transfusion_train_case as ttc
from arena import Arena
from pdm_ssd_amd import transfusion_ops

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


# ---- pdm_lsap ----------------------------------------------------------------------------------------------------------------------
def solve(cost, num_gt):
    got = transfusion_ops.lsap(torch.from_numpy(cost).to(DEV), torch.tensor(num_gt, dtype=torch.int32, device=DEV))
    return got[0].cpu().numpy(), got[1].cpu().numpy()


def check_against_host(cost, num_gt, got):
    B, P, G = cost.shape
    for b in range(B):
        want_rows, want_cols = transfusion_ops.lsap_host(cost[b, :, :num_gt[b]])
        assert np.array_equal(got[0][b], want_rows), b
        assert np.array_equal(got[1][b, :num_gt[b]], want_cols) and (got[1][b, num_gt[b]:] == -1).all(), b


@pytest.mark.parametrize('P, G', [(1, 1), (12, 5), (5, 12), (64, 64), (65, 3), (200, 40), (200, 0)])
def test_lsap_equals_the_host_solver(P, G):
    cost = np.random.default_rng(1000 * P + G).standard_normal((2, P, G)).astype(np.float32)
    got = solve(cost, [G, G])
    assert got[0].dtype == np.int32 and got[0].shape == (2, P) and got[1].shape == (2, G)
    check_against_host(cost, [G, G], got)


def test_lsap_reads_the_number_of_columns_per_sample_on_the_device():
    cost = np.random.default_rng(5).standard_normal((3, 20, 9)).astype(np.float32)
    got = solve(cost, [9, 0, 4])
    check_against_host(cost, [9, 0, 4], got)
    assert (got[0][1] == -1).all() and (got[1][1] == -1).all()
    assert (got[0][2] >= 0).sum() == 4


def test_lsap_reads_non_finite_costs_as_flt_max_and_two_runs_give_the_same_bits():
    """NaN, +Inf and -Inf are ordinary inputs of the operator: each is read as FLT_MAX (scipy raises instead); the loops are
    counted, so the kernel ends as on any other matrix"""
    cost = np.random.default_rng(6).standard_normal((2, 30, 8)).astype(np.float32)
    cost[0, 3, 2], cost[0, 7, :], cost[0, 11, 5] = np.nan, np.inf, -np.inf
    cost[1, :, 4] = np.nan                                             # a whole column: it must still be matched
    sub = np.where(np.isfinite(cost), cost, np.float32(transfusion_ops.FLT_MAX))
    got, again = solve(cost, [8, 8]), solve(cost, [8, 8])
    check_against_host(sub, [8, 8], got)
    for b in range(2):
        ttc.check_matching(sub[b], got[0][b], got[1][b])
    assert np.array_equal(got[0], again[0]) and np.array_equal(got[1], again[1])


def test_lsap_in_an_arena_with_a_row_stride():
    cost = np.random.default_rng(8).standard_normal((2, 13, 7)).astype(np.float32)
    arena = Arena(DEV, nbytes=4 << 20)
    wide = arena.carve((2, 13, 9), torch.float32, 4, float('nan'))
    wide.fill_(float('nan'))
    wide[:, :, :7] = torch.from_numpy(cost).to(DEV)
    num_gt = arena.put(np.array([7, 5], dtype=np.int32), 4, 0)
    got = transfusion_ops.lsap(wide[:, :, :7], num_gt)
    check_against_host(cost, [7, 5], (got[0].cpu().numpy(), got[1].cpu().numpy()))
    arena.check()


def test_lsap_refuses_more_than_1024_rows():
    with pytest.raises(ValueError, match='out of range'):
        transfusion_ops.lsap(torch.zeros((1, 1025, 3), device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV))


# ---- assign and loss -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def torch_targets():
    t = ttc.pred_tensors()
    return transfusion_ops.assign_torch(*ttc.map_args(t), torch.from_numpy(ttc.fixture()['gt_boxes']), *ttc.assign_args())


def arena_inputs(arena):
    fx = ttc.fixture()
    t = {k: arena.put(fx[f'pred.{k}'], 4 * (i % 4), float('nan')) for i, k in enumerate(ttc.GRAD_MAPS)}
    return t, arena.put(fx['gt_boxes'], 8, float('nan'))


def test_assign_reproduces_the_fixture_and_the_torch_formulation(torch_targets):
    arena = Arena(DEV, nbytes=8 << 20)
    t, gt = arena_inputs(arena)
    out = transfusion_ops.assign(*ttc.map_args(t), gt, *ttc.assign_args())
    ttc.check_targets(out, ttc.manifest()['parity_abs'])
    # the two formulations draw the same cells; a value is exp() of the same quotient in float32 here, in float64 there
    tc.close(out['heatmap'].cpu().numpy(), torch_targets['heatmap'].numpy(), 1e-6)
    assert np.array_equal(out['heatmap'].cpu().numpy() > 0, torch_targets['heatmap'].numpy() > 0)
    again = transfusion_ops.assign(*ttc.map_args(t), gt, *ttc.assign_args())
    assert all(torch.equal(out[k], again[k]) for k in out)
    arena.check()


def test_assign_without_velocities_and_without_a_valid_box(torch_targets):
    fx = ttc.fixture()
    t = ttc.pred_tensors(DEV)
    gt = torch.from_numpy(np.delete(fx['gt_boxes'], (7, 8), axis=2)).to(DEV)
    gt[1, :, 3:6] = 0                                                  # sample 1: nothing valid
    out = transfusion_ops.assign(*ttc.map_args(t, vel=False), gt, *ttc.assign_args())
    want = transfusion_ops.assign_torch(*ttc.map_args(ttc.pred_tensors(), vel=False), gt.cpu(), *ttc.assign_args())
    assert out['bbox_targets'].shape == (tc.B, tc.P, 8)
    for k in ('labels', 'assigned'):
        assert torch.equal(out[k].cpu(), want[k]), k
    for k in ('bbox_targets', 'bbox_weights', 'ious', 'heatmap', 'label_weights'):
        tc.close(out[k].cpu().numpy(), want[k].numpy(), ttc.manifest()['parity_abs'])
    assert int(out['num_pos']) == 5 and (out['labels'][1] == 10).all() and not out['heatmap'][1].any() and not out['ious'][1].any()
    tc.close(float(out['matched_ious']), float(want['matched_ious']), ttc.manifest()['parity_abs'])


def test_loss_reproduces_the_fixture():
    fx, tol = ttc.fixture(), ttc.manifest()['parity_abs']
    arena = Arena(DEV, nbytes=8 << 20)
    t, gt = arena_inputs(arena)
    for v in t.values():
        v.requires_grad_(True)
    targets = transfusion_ops.assign(*ttc.map_args(t), gt, *ttc.assign_args())
    losses = transfusion_ops.loss(*ttc.map_args(t), t['dense_heatmap'], targets, *ttc.loss_args())
    for name, value in zip(ttc.LOSSES, losses):
        print(name, float(value.detach()), float(fx[name]))
        tc.close(float(value.detach()), float(fx[name]), tol)
    total = sum(losses)
    tc.close(float(total.detach()), float(fx['loss_trans']), tol)
    total.backward()
    for k in ttc.GRAD_MAPS:
        tc.close(t[k].grad.cpu().numpy(), fx[f'grad.{k}'], tol)
    again = transfusion_ops.loss(*ttc.map_args(t), t['dense_heatmap'], targets, *ttc.loss_args())
    assert all(torch.equal(a.detach(), b.detach()) for a, b in zip(losses, again))
    arena.check()


def test_loss_backward_scales_with_the_incoming_gradient():
    t = ttc.pred_tensors(DEV, requires_grad=True)
    gt = torch.from_numpy(ttc.fixture()['gt_boxes']).to(DEV)
    targets = transfusion_ops.assign(*ttc.map_args(t), gt, *ttc.assign_args())
    l_cls, l_box, l_hm = transfusion_ops.loss(*ttc.map_args(t), t['dense_heatmap'], targets, *ttc.loss_args())
    (2.0 * l_cls + 3.0 * l_box + 0.5 * l_hm).backward()
    fx = ttc.fixture()
    for k, f in (('heatmap', 2.0), ('center', 3.0), ('vel', 3.0), ('dense_heatmap', 0.5)):
        tc.close(t[k].grad.cpu().numpy(), f * fx[f'grad.{k}'], 4 * ttc.manifest()['parity_abs'])


# ---- the training step ---------------------------------------------------------------------------------------------------------------
def host_reads(fn):
    """the synchronising device-to-host copies torch reports while fn() runs"""
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('warn')
    try:
        with warnings.catch_warnings(record=True) as seen:
            warnings.simplefilter('always')
            out = fn()
    finally:
        torch.cuda.set_sync_debug_mode('default')
    return out, sum('synchroniz' in str(w.message).lower() for w in seen)


def test_head_training_forward_reproduces_the_fixture_without_a_host_read():
    fx, man = ttc.fixture(), ttc.manifest()
    head = ttc.build_train_head(DEV)
    batch = lambda: {'batch_size': tc.B, 'spatial_features_2d': torch.from_numpy(fx['spatial_features_2d']).to(DEV),
                     'gt_boxes': torch.from_numpy(fx['gt_boxes']).to(DEV)}
    head(batch())                                                       # (warm-up: libraries load, workspaces are cached)
    b = batch()
    out, reads = host_reads(lambda: head(b))
    assert reads == 0
    assert np.array_equal(head.query_labels.cpu().numpy(), fx['cls'])
    assert np.array_equal(head.forward_ret_dict['targets']['assigned'].cpu().numpy(), fx['target.assigned'])
    tol = man['parity_abs'] + tc.manifest()['parity_abs'] * man['loss_sensitivity']       # (test_transfusion_train_host.py)
    tc.close(float(out['loss'].detach()), float(fx['loss_trans']), tol)
    assert all(v.is_cuda and not v.requires_grad for v in out['tb_dict'].values())


def test_detector_takes_a_training_step():
    """build_transfusion_lidar(TRANSFUSION_LIDAR_TRAIN_CFG) at the shapes of test_transfusion_gpu.py's detector test"""
    import copy
    import pillarnet_reference as pnr
    import sparse_conv_reference as scr
    from pdm_ssd_amd import detector_config as dc
    cfg = copy.deepcopy(dc.TRANSFUSION_LIDAR_TRAIN_CFG)
    cfg['DENSE_HEAD'].update(NUM_PROPOSALS=12)
    ds = dc.transfusion_dataset(point_cloud_range=[-9.6, -9.6, -5.0, 9.6, 9.6, 3.0], voxel_size=[0.1, 0.1, 0.2], grid_size=[192, 192, 40])
    torch.manual_seed(2)
    net = dc.build_transfusion_lidar(cfg, dataset=ds)
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
    assert bool(torch.isfinite(loss)) and set(tb_dict) == {'loss_heatmap', 'loss_cls', 'loss_bbox', 'matched_ious', 'loss_trans'}
    assert int(net.dense_head.forward_ret_dict['targets']['num_pos']) == 6
    loss.backward()
    head = net.dense_head
    for name, p in head.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), name
    for part in ('prediction_head', 'decoder', 'heatmap_head', 'shared_conv'):
        assert any(float(p.grad.abs().max()) > 0 for nm, p in head.named_parameters() if nm.startswith(part)), part

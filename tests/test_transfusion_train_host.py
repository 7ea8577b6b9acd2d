"""TransFusionHead's training half without a GPU: the numpy assignment solver against brute force and scipy, the torch
formulations of the assigner and the loss against the reference fixture (tests/golden/gen_transfusion_train_fixtures.py),
the head's training forward on the CPU, and the switch that keeps the eval-only head as it was."""
import numpy as np
import pytest
import torch

import transfusion_case as tc
import transfusion_train_case as ttc
from pdm_ssd_amd import transfusion_ops


# ---- lsap_host ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('P, G', [(1, 1), (3, 1), (5, 5), (8, 5), (7, 3), (2, 5), (4, 6), (6, 0)])
def test_lsap_host_equals_brute_force(P, G):
    rng = np.random.default_rng(100 * P + G)
    for _ in range(4):
        cost = rng.standard_normal((P, G)).astype(np.float32)
        gt_of_row, row_of_gt = transfusion_ops.lsap_host(cost)
        total = ttc.check_matching(cost, gt_of_row, row_of_gt)
        best, arg = ttc.brute_force(cost)
        assert abs(total - best) <= 1e-9
        assert frozenset((int(r), int(g)) for r, g in enumerate(gt_of_row) if g >= 0) in arg


@pytest.mark.parametrize('P, G', [(200, 40), (40, 200)])
def test_lsap_host_equals_scipy(P, G):
    scipy_optimize = pytest.importorskip('scipy.optimize')
    cost = np.random.default_rng(P + G).standard_normal((P, G)).astype(np.float32)
    rows, cols = scipy_optimize.linear_sum_assignment(cost)
    gt_of_row, row_of_gt = transfusion_ops.lsap_host(cost)
    want = np.full(P, -1, dtype=np.int32)
    want[rows] = cols
    assert np.array_equal(gt_of_row, want)
    ttc.check_matching(cost, gt_of_row, row_of_gt)


@pytest.mark.parametrize('P, G', [(7, 4), (4, 7), (6, 6)])
def test_lsap_host_on_tied_integer_costs(P, G):
    """costs in {0, 1, 2}: many optimal matchings; whichever is returned is a matching and has the optimal total"""
    rng = np.random.default_rng(P * 10 + G)
    for _ in range(4):
        cost = rng.integers(0, 3, (P, G)).astype(np.float32)
        total = ttc.check_matching(cost, *transfusion_ops.lsap_host(cost))
        assert total == ttc.brute_force(cost)[0]


def test_lsap_host_reads_non_finite_costs_as_flt_max():
    cost = np.random.default_rng(3).standard_normal((6, 4)).astype(np.float32)
    cost[0, 0], cost[2, 1], cost[3, :] = np.nan, np.inf, -np.inf
    sub = np.where(np.isfinite(cost), cost, np.float32(transfusion_ops.FLT_MAX))
    got, want = transfusion_ops.lsap_host(cost), transfusion_ops.lsap_host(sub)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    ttc.check_matching(sub, *got)
    assert got[0][3] == -1                                            # the row of FLT_MAX entries is the one left out


@pytest.mark.parametrize('shape', [(1025, 3), (3, 1025), (0, 3)])
def test_lsap_sizes_out_of_range_are_refused(shape):
    """(before anything touches a device: the operator's wrapper checks first)"""
    with pytest.raises(ValueError, match='out of range'):
        transfusion_ops.lsap(torch.zeros((1,) + shape), torch.zeros(1, dtype=torch.int32))
    with pytest.raises(ValueError, match='out of range'):
        transfusion_ops.lsap_host(np.zeros(shape, dtype=np.float32))


# ---- the fixture ---------------------------------------------------------------------------------------------------------------------
def test_fixture_margins_hold():
    man, fx = ttc.manifest(), ttc.fixture()
    assert all(4 * g <= man['parity_abs'] for g in man['float32_to_float64_gap'].values())
    assert min(man['second_best_gap']) >= tc.MARGIN
    tc.check_proposal_margins(tc.proposal_margins(fx['pred.dense_heatmap'], 3, (8, 9), tc.P), tc.P)
    gt = fx['gt_boxes']
    valid = (gt[..., 3] > 0) & (gt[..., 4] > 0)
    assert valid.sum(1).tolist() == [5, 3] and not valid[0, 2] and valid[0, 3]          # a zero-size row in the middle
    assert len(set(gt[0, valid[0], 9].tolist())) >= 3
    pos = fx['target.assigned'] >= 0
    assert (fx['target.ious'][pos] > 0).any() and (fx['target.ious'][pos] == 0).any()
    for b in range(tc.B):                                              # the recorded optimum is unique by brute force
        best, arg = ttc.brute_force(fx[f'cost.{b}'])
        assert len(arg) == 1 and next(iter(arg)) == frozenset((int(r), int(g)) for r, g in enumerate(fx['target.assigned'][b]) if g >= 0)


@pytest.fixture(scope='module')
def torch_targets():
    t = ttc.pred_tensors()
    detail = []
    out = transfusion_ops.assign_torch(*ttc.map_args(t), torch.from_numpy(ttc.fixture()['gt_boxes']), *ttc.assign_args(), detail=detail)
    return out, detail


def test_assign_torch_reproduces_the_fixture(torch_targets):
    out, detail = torch_targets
    fx, tol = ttc.fixture(), ttc.manifest()['parity_abs']
    for b, (cost, gt_of_row, _) in enumerate(detail):
        tc.close(cost, fx[f'cost.{b}'], tol)
        assert np.array_equal(gt_of_row, fx['target.assigned'][b])
    ttc.check_targets(out, tol)


def test_loss_torch_reproduces_the_fixture(torch_targets):
    fx, tol = ttc.fixture(), ttc.manifest()['parity_abs']
    t = ttc.pred_tensors(requires_grad=True)
    losses = transfusion_ops.loss_torch(*ttc.map_args(t), t['dense_heatmap'], torch_targets[0], *ttc.loss_args())
    for name, value in zip(ttc.LOSSES, losses):
        tc.close(float(value.detach()), float(fx[name]), tol)
    sum(losses).backward()
    tc.close(float(sum(losses).detach()), float(fx['loss_trans']), tol)
    for k in ttc.GRAD_MAPS:
        tc.close(t[k].grad.numpy(), fx[f'grad.{k}'], tol)


def test_assigner_for_one_sample_matches_the_fixture():
    from pdm_ssd_amd.dense_heads.target_assigner.hungarian_assigner import HungarianAssigner3D
    fx = ttc.fixture()
    cls_cost, reg_cost, iou_cost = ttc.assign_args()[:3]
    assigner = HungarianAssigner3D(cls_cost, reg_cost, iou_cost)
    t = ttc.pred_tensors()
    head = ttc.build_train_head()
    head.query_labels = torch.from_numpy(fx['cls'])
    boxes = transfusion_ops.decode_torch(*ttc.map_args(t), head.query_labels, torch.from_numpy(fx['pred.query_heatmap_score']), 0.0,
                                         [-1e4] * 3 + [1e4] * 3, tc.PC_RANGE[0], tc.PC_RANGE[1], tc.VOXEL[0], tc.VOXEL[1], tc.STRIDE)[0]
    for b in range(tc.B):
        gt = torch.from_numpy(fx['gt_boxes'][b])
        gt = gt[(gt[:, 3] > 0) & (gt[:, 4] > 0)]
        # (every score is positive and the range is wide open: the padded decode keeps all P boxes in query order)
        inds, ious = assigner.assign(boxes[b], gt[:, :9], gt[:, 9].long() - 1, t['heatmap'][b:b + 1], tc.PC_RANGE)
        assert np.array_equal(inds.numpy() - 1, fx['target.assigned'][b])
        tc.close(ious.clamp(0, 1).numpy(), fx['target.ious'][b], ttc.manifest()['parity_abs'])


# ---- the head ------------------------------------------------------------------------------------------------------------------------
def test_head_with_the_key_trains_on_the_cpu_and_gives_the_fixtures_loss():
    """The head's own training-mode predict lies within the eval fixture's parity_abs of the reference's maps, map by map; to
    first order loss_trans then moves by at most that distance times the summed |d loss_trans / d map| (loss_sensitivity of
    the manifest), on top of the training fixture's own bound.  Queries and assignment are discrete and must be the fixture's."""
    fx, man = ttc.fixture(), ttc.manifest()
    head = ttc.build_train_head()
    assert hasattr(head, 'bbox_assigner') and len(head.state_dict()) == 96
    batch = {'batch_size': tc.B, 'spatial_features_2d': torch.from_numpy(fx['spatial_features_2d']), 'gt_boxes': torch.from_numpy(fx['gt_boxes'])}
    out = head(batch)
    assert np.array_equal(head.query_labels.numpy(), fx['cls'])
    res = head.forward_ret_dict['pred_dicts']
    for k in ttc.GRAD_MAPS:
        tc.close(res[k].detach().numpy(), fx[f'pred.{k}'], tc.manifest()['parity_abs'])
    assert np.array_equal(head.forward_ret_dict['targets']['assigned'].numpy(), fx['target.assigned'])
    tol = man['parity_abs'] + tc.manifest()['parity_abs'] * man['loss_sensitivity']
    print('loss_trans', float(out['loss']), 'fixture', float(fx['loss_trans']), 'tolerance', tol)
    tc.close(float(out['loss']), float(fx['loss_trans']), tol)
    assert set(out['tb_dict']) == {'loss_heatmap', 'loss_cls', 'loss_bbox', 'matched_ious', 'loss_trans'}
    assert all(isinstance(v, torch.Tensor) and not v.requires_grad for v in out['tb_dict'].values())
    out['loss'].backward()
    for name, p in head.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), name
    for part in ('prediction_head', 'decoder', 'heatmap_head', 'shared_conv'):
        assert any(float(p.grad.abs().max()) > 0 for n, p in head.named_parameters() if n.startswith(part)), part


def test_reference_named_methods_give_the_fixtures_targets():
    fx, tol = ttc.fixture(), ttc.manifest()['parity_abs']
    head = ttc.build_train_head()
    gt = torch.from_numpy(fx['gt_boxes'])
    t = ttc.pred_tensors()
    labels, label_weights, bbox_targets, bbox_weights, num_pos, matched_ious, heatmap = head.get_targets(gt[..., :-1], gt[..., -1].long() - 1, t)
    assert np.array_equal(labels.numpy(), fx['target.labels']) and int(num_pos) == int(fx['target.num_pos'])
    tc.close(bbox_targets.numpy(), fx['target.bbox_targets'], tol)
    loss, tb = head.loss(gt[..., :-1], gt[..., -1].long() - 1, t)
    tc.close(float(loss), float(fx['loss_trans']), tol)
    valid = gt[0][(gt[0, :, 3] > 0) & (gt[0, :, 4] > 0)]
    one = head.get_targets_single(valid[:, :9], valid[:, 9].long() - 1, {k: v[:1] for k, v in t.items()})
    assert np.array_equal(one[0].numpy(), fx['target.labels'][:1])
    enc = head.encode_bbox(valid[:, :9])
    rows = fx['target.assigned'][0]
    tc.close(enc[rows[rows >= 0]].numpy(), fx['target.bbox_targets'][0][rows >= 0], tol)


def test_head_without_the_key_still_refuses_training():
    head = ttc.build_train_head(on_device=False)
    assert not hasattr(head, 'bbox_assigner')
    fx = ttc.fixture()
    with pytest.raises(NotImplementedError, match='Hungarian'):
        head({'batch_size': tc.B, 'spatial_features_2d': torch.from_numpy(fx['spatial_features_2d']), 'gt_boxes': torch.from_numpy(fx['gt_boxes'])})


def test_train_config_is_the_eval_config_plus_the_key():
    import copy
    from pdm_ssd_amd import detector_config as dc
    want = copy.deepcopy(dc.TRANSFUSION_LIDAR_CFG)
    want['DENSE_HEAD']['TARGET_ASSIGNER_CONFIG']['ASSIGN_ON_DEVICE'] = True
    assert dc.TRANSFUSION_LIDAR_TRAIN_CFG == want
    assert 'ASSIGN_ON_DEVICE' not in dc.TRANSFUSION_LIDAR_CFG['DENSE_HEAD']['TARGET_ASSIGNER_CONFIG']


def test_a_sample_without_a_valid_box_is_all_background():
    t = ttc.pred_tensors()
    gt = torch.from_numpy(ttc.fixture()['gt_boxes']).clone()
    gt[1, :, 3:6] = 0
    out = transfusion_ops.assign_torch(*ttc.map_args(t), gt, *ttc.assign_args())
    assert (out['labels'][1] == 10).all() and not out['bbox_weights'][1].any() and not out['ious'][1].any() and not out['heatmap'][1].any()
    assert int(out['num_pos']) == 5 and np.array_equal(out['labels'][0].numpy(), ttc.fixture()['target.labels'][0])

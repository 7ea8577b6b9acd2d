"""CenterHead's device operators (csrc/center_head.hip) against the reference fixture, against the torch formulations on
the device, and inside CenterPoint: targets, decode, regression loss, batched post-processing, a training step without
host synchronisation and a captured step."""
import copy

import numpy as np
import pytest
import torch

import center_head_case as case
from center_head_case import B, H, W, close, fixture
from pdm_ssd_amd import center_head_ops, heatmap_loss, synthetic
from pdm_ssd_amd.utils import centernet_utils, loss_utils

pytestmark = pytest.mark.gpu

GRID = dict(x0=case.PC_RANGE[0], y0=case.PC_RANGE[1], vx=case.VOXEL[0], vy=case.VOXEL[1], stride=case.STRIDE)


def random_boxes(Bn, M, extras, seed, x_hi=8.0, y_half=2.4):
    """(Bn, M, 8 + extras): three classes, padding rows and degenerate boxes scattered through the list"""
    rng = np.random.default_rng(seed)
    gt = np.zeros((Bn, M, 8 + extras), dtype=np.float32)
    sizes = np.array([[3.9, 1.6, 1.56], [0.8, 0.6, 1.73], [1.76, 0.6, 1.73]], dtype=np.float32)
    for b in range(Bn):
        for r in range(M):
            if rng.uniform() < 0.2:
                continue
            cls = int(rng.integers(1, 4))
            gt[b, r, :7] = [rng.uniform(-0.5, x_hi + 0.5), rng.uniform(-y_half - 0.3, y_half + 0.3), rng.uniform(-1.2, -0.6),
                            *(sizes[cls - 1] * rng.uniform(0.8, 1.2, 3)), rng.uniform(-3.1, 3.1)]
            gt[b, r, 7:7 + extras] = rng.standard_normal(extras)
            gt[b, r, -1] = cls
            if rng.uniform() < 0.1:
                gt[b, r, 3 + int(rng.integers(0, 2))] = 0.0
    return gt


# ---- targets -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["one", "two"])
def test_fused_targets_match_the_reference(dev, tag):
    head = case.build_head(case.HEADS[tag]).to(dev)
    gt = torch.from_numpy(fixture()['gt_boxes'].copy()).to(dev)
    td = head.assign_targets(gt, feature_map_size=(H, W))
    assert torch.equal(gt.cpu(), torch.from_numpy(fixture()['gt_boxes'])), 'gt_boxes must stay untouched'
    case.check_targets(td, f'{tag}.targets')
    if tag == "one":
        over = torch.from_numpy(fixture()['gt_boxes_over'].copy()).to(dev)
        case.check_targets(head.assign_targets(over, feature_map_size=(H, W)), 'one.targets_over')


def test_fused_targets_of_interleaved_heads(dev):
    head = case.build_head([['Car', 'Cyclist'], ['Pedestrian']]).to(dev)
    gt = torch.from_numpy(fixture()['gt_boxes'].copy()).to(dev)
    td = head.assign_targets(gt, feature_map_size=(H, W))
    assert torch.equal(gt.cpu(), torch.from_numpy(fixture()['gt_boxes']))
    for h, (src, inds, mask) in case.interleaved_expectation().items():
        assert np.array_equal(td['target_boxes_src'][h].cpu().numpy(), src), h
        assert np.array_equal(td['inds'][h].cpu().numpy(), inds) and np.array_equal(td['masks'][h].cpu().numpy(), mask), h


@pytest.mark.parametrize("extras, nmax, M", [(0, 6, 40), (2, 64, 40), (2, 300, 300)])
def test_fused_targets_match_the_torch_formulation(dev, extras, nmax, M):
    """odd map (13 x 21), more boxes than slots (nmax = 6), extra regression columns, more boxes than one scan chunk (300)"""
    head = case.build_head([['Car', 'Cyclist'], ['Pedestrian']], edit=lambda c: c['TARGET_ASSIGNER_CONFIG'].update(NUM_MAX_OBJS=nmax)).to(dev)
    gt = torch.from_numpy(random_boxes(3, M, extras, seed=extras + nmax)).to(dev)
    keep = gt.clone()
    fused = head.assign_targets(gt, feature_map_size=(13, 21))
    head.use_fused = False
    plain = head.assign_targets(gt, feature_map_size=(13, 21))
    assert torch.equal(gt, keep)
    for h in range(2):
        assert fused['target_boxes'][h].shape == (3, nmax, 8 + extras) and fused['target_boxes_src'][h].shape == (3, nmax, 8 + extras)
        for key in ('inds', 'masks'):
            assert fused[key][h].dtype == torch.int64 and torch.equal(fused[key][h], plain[key][h]), (key, h)
        assert torch.equal(fused['target_boxes_src'][h], plain['target_boxes_src'][h])
        close(fused['target_boxes'][h].cpu().numpy(), plain['target_boxes'][h].cpu().numpy())
        close(fused['heatmaps'][h].cpu().numpy(), plain['heatmaps'][h].cpu().numpy())
        assert int(fused['masks'][h].sum()) > 0


@pytest.mark.parametrize("source", ["fixture", "random"])
def test_heatmap_is_bit_equal_to_heatmap_targets(dev, source):
    """one head, every box within the slots, a radius cap (64) no box reaches: the shared device code draws the same bits"""
    gt_np = fixture()['gt_boxes'] if source == "fixture" else random_boxes(3, 50, 0, seed=9)
    hh, ww = (H, W) if source == "fixture" else (13, 21)
    head = case.build_head(case.HEADS['one'], edit=lambda c: c['TARGET_ASSIGNER_CONFIG'].update(NUM_MAX_OBJS=64)).to(dev)
    gt = torch.from_numpy(gt_np.copy()).to(dev)
    td = head.assign_targets(gt, feature_map_size=(hh, ww))
    want = heatmap_loss.heatmap_targets(gt, 3, hh, ww, GRID['x0'], GRID['y0'], GRID['vx'], GRID['vy'], GRID['stride'], 0.1, 2, 64)
    assert torch.equal(td['heatmaps'][0], want) and int((want == 1).sum()) > 0


# ---- decode ------------------------------------------------------------------------------------------------------------
def fused_decode(m, K, thresh, limit=case.LIMIT, global_of=(0, 1, 2)):
    return center_head_ops.center_decode(m['hm'], m['center'], m['center_z'], m['dim'], m['rot'], m.get('vel'), K, thresh, limit,
                                         GRID['x0'], GRID['y0'], GRID['vx'], GRID['vy'], GRID['stride'], list(global_of))


def plain_decode(m, K, thresh, limit=case.LIMIT):
    f = {k: v.float() for k, v in m.items()}
    return centernet_utils.decode_bbox_from_heatmap(
        heatmap=f['hm'].sigmoid(), rot_cos=f['rot'][:, 0:1], rot_sin=f['rot'][:, 1:2], center=f['center'], center_z=f['center_z'],
        dim=f['dim'].exp(), vel=f.get('vel'), point_cloud_range=case.PC_RANGE, voxel_size=case.VOXEL, feature_map_stride=case.STRIDE, K=K,
        score_thresh=thresh, post_center_limit_range=limit)


def check_padded(out, want, K, label_offset):
    """out = center_decode's padded tensors; want = per-sample dicts with 0-based labels"""
    boxes, scores, labels, count = (t.cpu() for t in out)
    assert count.dtype == torch.int32 and labels.dtype == torch.int64 and boxes.shape[1] == K
    for b, d in enumerate(want):
        n = len(d['pred_boxes'])
        assert int(count[b]) == n, (b, int(count[b]), n)
        assert np.array_equal(labels[b, :n].numpy(), np.asarray(d['pred_labels'].cpu() if torch.is_tensor(d['pred_labels']) else d['pred_labels'],
                                                                dtype=np.int64) + label_offset), b
        close(boxes[b, :n].numpy(), np.asarray(d['pred_boxes'].cpu() if torch.is_tensor(d['pred_boxes']) else d['pred_boxes']))
        close(scores[b, :n].numpy(), np.asarray(d['pred_scores'].cpu() if torch.is_tensor(d['pred_scores']) else d['pred_scores']))
        assert not boxes[b, n:].any() and not scores[b, n:].any() and not labels[b, n:].any(), 'padding rows are zero'


@pytest.mark.parametrize("tag", ["10", "all"])
def test_fused_decode_matches_the_reference(dev, tag):
    fx = fixture()
    K = 10 if tag == "10" else H * W
    thresh = float(fx[f'dec_thresh_{tag}'])
    m = case.decode_maps(dev)
    ranked = fused_decode(m, K, None, limit=[-1e9] * 3 + [1e9] * 3)
    assert ranked[3].tolist() == [K, K]
    case.check_decode_conditions(fx['dec_hm'], K, thresh, ranked[0].cpu().numpy())
    want = [{'pred_boxes': fx[f'dec{tag}.boxes.{b}'], 'pred_scores': fx[f'dec{tag}.scores.{b}'], 'pred_labels': fx[f'dec{tag}.labels.{b}']}
            for b in range(B)]
    check_padded(fused_decode(m, K, thresh), want, K, label_offset=1)
    if tag == "10":
        assert len(want[1]['pred_boxes']) == 0 and 0 < len(want[0]['pred_boxes']) < K


def distinct_logits(shape, dtype, seed):
    """per sample a permutation of logits no two of which share a sigmoid (equal scores have no order in torch.topk): an even
    grid over [-4, 4] in fp32; in bf16 consecutive bit patterns from 2^-7 upwards (three binades), both signs"""
    rng = np.random.default_rng(seed)
    n = int(np.prod(shape[1:]))
    if dtype == torch.float32:
        vals = torch.linspace(-4.0, 4.0, n)
    else:
        half = torch.from_numpy((0x3C00 + np.arange((n + 1) // 2)).astype(np.int16)).view(torch.bfloat16).float()
        vals = torch.cat([half, -half])[:n]
        assert float(half.max()) < 1.0 and len(torch.unique(vals.to(dtype).float().sigmoid())) == n
    return torch.stack([vals[torch.from_numpy(rng.permutation(n))] for _ in range(shape[0])]).reshape(shape).to(dtype)


@pytest.mark.parametrize("C, dtype, layout, vel, K", [
    (3, torch.float32, "contiguous", False, 37),
    (1, torch.float32, "contiguous", True, 13 * 21),          # one class, K = H * W, velocity
    (3, torch.bfloat16, "channels_last", False, 64),
    (2, torch.float32, "contiguous", True, 1500),             # more candidates than one workgroup pass (1024), 32 x 47 map
    (3, torch.float32, "channels_last", True, 100),
])
def test_fused_decode_matches_the_torch_formulation(dev, C, dtype, layout, vel, K):
    hh, ww = (32, 47) if K > 1024 else (13, 21)
    g = torch.Generator().manual_seed(K)
    m = {'hm': distinct_logits((3, C, hh, ww), dtype, seed=K)}
    for name, c, lo, hi in (('center', 2, -0.3, 1.3), ('center_z', 1, -2.6, 1.6), ('dim', 3, -0.5, 1.4), ('rot', 2, -1.0, 1.0)) + \
            ((('vel', 2, -3.0, 3.0),) if vel else ()):
        m[name] = (torch.rand((3, c, hh, ww), generator=g) * (hi - lo) + lo).to(dtype)
    m = {k: v.to(dev) for k, v in m.items()}
    if layout == "channels_last":
        m = {k: v.contiguous(memory_format=torch.channels_last) for k, v in m.items()}
        assert not m['dim'].is_contiguous()
    limit = [0.5, -2.0, -2.0, 0.4 * ww - 0.5, 0.4 * hh - 2.9, 1.0]
    want = plain_decode(m, K, 0.5, limit)
    out = fused_decode(m, K, 0.5, limit, global_of=[2, 0, 1][:C])
    assert out[0].shape == (3, K, 9 if vel else 7)
    remap = np.array([2, 0, 1])
    for d in want:
        d['pred_labels'] = torch.from_numpy(remap[d['pred_labels'].cpu().numpy().astype(np.int64)])
    check_padded(out, want, K, label_offset=1)
    assert 0 < int(out[3].min()) and int(out[3].max()) < K


def test_decode_ties_go_to_the_lower_flat_index(dev):
    hm = torch.full((1, 3, H, W), -5.0)
    tied = [(2, 3, 4), (0, 11, 19), (1, 0, 0), (0, 5, 5), (2, 3, 3), (1, 7, 9), (0, 5, 6)]        # (class, y, x), all logit 2
    for c, y, x in tied:
        hm[0, c, y, x] = 2.0
    zeros = {'center': torch.zeros(1, 2, H, W), 'center_z': torch.zeros(1, 1, H, W), 'dim': torch.zeros(1, 3, H, W)}
    m = {k: v.to(dev) for k, v in dict(zeros, hm=hm, rot=torch.ones(1, 2, H, W)).items()}
    order = sorted(tied)                                             # flat index c * H * W + y * W + x ascending
    wide = [-1e9] * 3 + [1e9] * 3
    for K in (5, 7, 9):
        boxes, scores, labels, count = (t.cpu() for t in fused_decode(m, K, None, wide))
        assert int(count[0]) == K
        # beyond the seven tied cells come the background's (all logit -5), again from the lowest flat index: (0, 0, 0), (0, 0, 1)
        expect = (order + [(0, 0, 0), (0, 0, 1)])[:K]
        assert labels[0].tolist() == [c + 1 for c, _, _ in expect]
        close(boxes[0, :, 0].numpy(), np.array([x * 0.4 for _, _, x in expect]), tol=1e-6)
        close(boxes[0, :, 1].numpy(), np.array([y * 0.4 - 2.4 for _, y, _ in expect]), tol=1e-6)
        assert torch.all(scores[0, :min(K, 7)] == scores[0, 0]) and torch.allclose(boxes[0, :, 6], torch.full((K,), np.pi / 4))
        assert torch.all(boxes[0, :, 3:6] == 1.0)


def test_decode_rejects_k_beyond_the_map(dev):
    m = case.decode_maps(dev)
    with pytest.raises(RuntimeError, match="out of range"):
        fused_decode(m, H * W + 1, 0.1)


# ---- regression loss ---------------------------------------------------------------------------------------------------
def split_maps(pred):
    return [pred[:, 0:2], pred[:, 2:3], pred[:, 3:6], pred[:, 6:8]]


def test_fused_reg_loss_matches_the_reference_and_repeats_bit_for_bit(dev):
    fx = fixture()
    inds, mask, target = (torch.from_numpy(fx[k]).to(dev) for k in ('reg_inds', 'reg_mask', 'reg_target'))
    w, lw = fx['reg_code_weights'].tolist(), float(fx['reg_loc_weight'])
    assert inds[0, 3] == inds[0, 1] and mask[0, 3] == 1 and mask[0, 1] == 1 and torch.isnan(target[0, 1, 4])     # shared cell, NaN element
    runs = []
    for _ in range(2):
        pred = torch.from_numpy(fx['reg_pred']).to(dev).requires_grad_(True)
        loc, per_code = center_head_ops.center_reg_loss(split_maps(pred), inds, mask, target, w, lw)
        assert not per_code.requires_grad
        (loc * 1.0).backward()
        runs.append((loc.detach().clone(), per_code.clone(), pred.grad.clone()))
    assert all(torch.equal(a, b) for a, b in zip(*runs)), 'two runs must give the same bits'
    loc, per_code, grad = (t.cpu() for t in runs[0])
    finite = [0, 1, 2, 3, 5, 6, 7]                      # code 4 holds the NaN target element: NaN in the reference, left out here
    close(per_code.numpy()[finite], fx['reg_per_code'][finite])
    cpu = loss_utils.RegLossCenterNet()(torch.from_numpy(fx['reg_pred']), mask.cpu(), inds.cpu(), target.cpu())
    close(per_code.numpy(), cpu.numpy())
    close(float(loc), float((cpu * torch.tensor(w)).sum() * lw))
    close(grad.numpy(), fx['reg_grad'])
    named = torch.zeros(B, H * W, dtype=torch.bool)
    for b in range(B):
        named[b, inds[b].cpu()[mask[b].cpu() > 0]] = True
    assert not grad.flatten(2)[~named[:, None].expand(-1, 8, -1)].any(), 'cells no slot names get exact zeros'
    assert torch.isfinite(grad).all()


def test_fused_reg_loss_with_an_all_zero_mask(dev):
    fx = fixture()
    inds, target = torch.from_numpy(fx['reg_inds']).to(dev), torch.from_numpy(fx['reg_target']).to(dev)
    pred = torch.from_numpy(fx['reg_pred']).to(dev).requires_grad_(True)
    loc, per_code = center_head_ops.center_reg_loss(split_maps(pred), inds, torch.zeros_like(inds), target, fx['reg_code_weights'].tolist(), 2.0)
    loc.backward()
    assert float(loc.detach()) == 0.0 and not per_code.any() and not pred.grad.any()
    close(per_code.cpu().numpy(), fx['reg_zero_per_code'])
    close(pred.grad.cpu().numpy(), fx['reg_zero_grad'])


@pytest.mark.parametrize("dtype, layout, extras, N", [(torch.float32, "contiguous", 0, 40), (torch.bfloat16, "channels_last", 2, 300),
                                                      (torch.float32, "channels_last", 2, 7)])
def test_fused_reg_loss_matches_the_torch_formulation(dev, dtype, layout, extras, N):
    """odd map, slots crowded into few cells (every cell shared), more slots than the workgroup has threads (300), bf16 and
    channels-last maps, velocity channels"""
    g = torch.Generator().manual_seed(N)
    hh, ww, D = 13, 21, 8 + extras
    sizes = [2, 1, 3, 2] + ([2] if extras else [])
    maps = [torch.randn((3, c, hh, ww), generator=g).to(dtype).to(dev) for c in sizes]
    if layout == "channels_last":
        maps = [t.contiguous(memory_format=torch.channels_last) for t in maps]
    maps = [t.requires_grad_(True) for t in maps]
    inds = torch.randint(0, 40, (3, N), generator=g).to(dev) * 5 % (hh * ww)
    mask = (torch.rand((3, N), generator=g) < 0.7).long().to(dev)
    target = torch.randn((3, N, D), generator=g).to(dev)
    target[1, 2, 3] = float('nan')
    w = [1.0, 1.0, 0.5, 1.0, 1.0, 1.0, 2.0, 1.0, 0.2, 0.2][:D]
    loc, per_code = center_head_ops.center_reg_loss(maps, inds, mask, target, w, 2.0)
    loc.backward()
    ref_maps = [t.detach().float().requires_grad_(True) for t in maps]
    want = loss_utils.RegLossCenterNet()(torch.cat(ref_maps, dim=1), mask, inds, target)
    want_loc = (want * want.new_tensor(w)).sum() * 2.0
    want_loc.backward()
    close(per_code.cpu().numpy(), want.detach().cpu().numpy())
    close(float(loc), float(want_loc))
    for t, r in zip(maps, ref_maps):
        assert t.grad.dtype == dtype and t.grad.shape == t.shape
        close(t.grad.float().cpu().numpy(), r.grad.cpu().numpy(), tol=1e-4 if dtype == torch.float32 else 2.0 ** -8)   # one bf16 rounding


def test_fused_reg_loss_sums_all_seventeen_accumulators_over_a_ragged_pass(dev):
    """D = 10 (velocity head) of the 17 accumulators the partial kernel always sums, 257 slots (the workgroup's second pass
    over the slots holds one), the heads' channels of one bf16 channels-last map (every channel's plane has a non-unit
    stride along W), two masked slots on one cell, one NaN target element; against RegLossCenterNet as above."""
    g = torch.Generator().manual_seed(257)
    hh, ww, D, N = 13, 21, 10, 257
    pred = torch.randn((2, D, hh, ww), generator=g).to(torch.bfloat16).to(dev).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    maps = list(torch.split(pred, [2, 1, 3, 2, 2], dim=1))                     # the five heads' channels of one channels-last map
    assert all(t.stride(3) == D for t in maps)
    inds = torch.randint(0, hh * ww, (2, N), generator=g)
    mask = (torch.rand((2, N), generator=g) < 0.7).long()
    inds[0, 256], mask[0, 256], mask[0, 3] = inds[0, 3], 1, 1                  # the last slot shares slot 3's cell
    target = torch.randn((2, N, D), generator=g)
    target[0, 256, 9] = float('nan')
    inds, mask, target = inds.to(dev), mask.to(dev), target.to(dev)
    w = [1.0, 1.0, 0.5, 1.0, 1.0, 1.0, 2.0, 1.0, 0.2, 0.2]
    runs = []
    for _ in range(2):
        pred.grad = None
        loc, per_code = center_head_ops.center_reg_loss(maps, inds, mask, target, w, 2.0)
        loc.backward()
        runs.append((loc.detach().clone(), per_code.clone(), pred.grad.clone()))
    assert all(torch.equal(a, b) for a, b in zip(*runs)), 'two runs must give the same bits'
    ref = pred.detach().float().requires_grad_(True)
    want = loss_utils.RegLossCenterNet()(ref, mask, inds, target)
    want_loc = (want * want.new_tensor(w)).sum() * 2.0
    want_loc.backward()
    close(per_code.cpu().numpy(), want.detach().cpu().numpy())
    close(float(loc.detach()), float(want_loc.detach()))
    assert pred.grad.dtype == torch.bfloat16 and pred.grad.shape == pred.shape
    close(pred.grad.float().cpu().numpy(), ref.grad.cpu().numpy(), tol=2.0 ** -8)          # one bf16 rounding


# ---- the head and the detector ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["one", "two"])
def test_head_on_the_gpu_matches_the_reference(dev, tag):
    fx = fixture()
    head = case.build_head(case.HEADS[tag], tag).to(dev).train()
    gt = torch.from_numpy(fx['gt_boxes'].copy()).to(dev)
    head({'batch_size': B, 'spatial_features_2d': torch.from_numpy(fx['spatial_features_2d']).to(dev), 'gt_boxes': gt})
    preds = head.forward_ret_dict['pred_dicts']
    case.check_targets(head.forward_ret_dict['target_dicts'], f'{tag}.targets')
    for h, pd in enumerate(preds):
        for name in ('hm',) + case.MAPS:
            close(pd[name].detach().cpu().numpy(), fx[f'{tag}.pred.{name}.{h}'])
            pd[name].retain_grad()
    loss, tb = head.get_loss()
    for k, v in tb.items():
        assert torch.is_tensor(v) and v.is_cuda and not v.requires_grad
        close(float(v), float(fx[f'{tag}.tb.{k}']))
    close(float(loss.detach()), float(fx[f"{tag}.loss"]))
    loss.backward()
    for h, pd in enumerate(preds):
        for name in ('hm',) + case.MAPS:
            close(pd[name].grad.cpu().numpy(), fx[f'{tag}.grad.{name}.{h}'])


def test_head_step_captured_in_a_graph_replays_to_the_same_loss(dev):
    """targets + both losses + their backward on fixed head outputs, captured after one warm-up call; the replay sees new
    values in the same buffers"""
    fx = fixture()
    head = case.build_head(case.HEADS['two']).to(dev).train()
    gt = torch.from_numpy(fx['gt_boxes'].copy()).to(dev)
    leaves = [{name: torch.from_numpy(fx[f'two.pred.{name}.{h}']).to(dev).requires_grad_(True) for name in ('hm',) + case.MAPS} for h in range(2)]

    def step():
        head.forward_ret_dict = {'pred_dicts': leaves, 'target_dicts': head.assign_targets(gt, feature_map_size=(H, W))}
        loss, _ = head.get_loss()
        grads = torch.autograd.grad(loss, [t for d in leaves for t in d.values()])
        return loss.detach(), grads

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        eager_loss, eager_grads = step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):                            # any host synchronisation in here would fail the capture
        loss, grads = step()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(loss, eager_loss) and all(torch.equal(a, b) for a, b in zip(grads, eager_grads))
    close(float(loss), float(fx['two.loss']))
    with torch.no_grad():
        gt[0, 0, 0] += 1.2                               # the Car moves three cells: other targets, another loss
    g.replay()
    torch.cuda.synchronize()
    moved = float(loss)
    with torch.cuda.stream(side):
        again, _ = step()
    torch.cuda.synchronize()
    assert moved != float(eager_loss) and moved == float(again)


SMALL_BACKBONE = {'NAME': 'PointNet2MSG',
                  'SA_CONFIG': {'NPOINTS': [512, 128, 32], 'RADIUS': [[0.5, 1.0], [1.0, 2.0], [2.0, 4.0]], 'NSAMPLE': [[16, 32], [16, 32], [16, 32]],
                                'MLPS': [[[16, 16, 32], [32, 32, 64]], [[64, 64, 128], [64, 96, 128]], [[128, 196, 256], [128, 196, 256]]]},
                  'FP_MLPS': [[128, 128], [256, 256], [512, 512]]}


def small_center_pdm(heads=None, **post):
    from pdm_ssd_amd.detector_config import CENTER_PDM_CFG, build_center_pdm
    cfg = copy.deepcopy(CENTER_PDM_CFG)
    cfg['BACKBONE_3D'] = copy.deepcopy(SMALL_BACKBONE)
    cfg['MAP_TO_BEV'] = dict(cfg['MAP_TO_BEV'], FEATURE_DIM=32, DILATION=[5, 5, 1])
    cfg['DENSE_HEAD']['SHARED_CONV_CHANNEL'] = 32
    if heads is not None:
        cfg['DENSE_HEAD']['CLASS_NAMES_EACH_HEAD'] = heads
    cfg['DENSE_HEAD']['POST_PROCESSING'].update(post)
    return build_center_pdm(cfg)


def scene(Bn, N, seed):
    rng = np.random.default_rng(seed)
    cl = synthetic.lidar_like_clouds(Bn, N, seed)
    gt = np.zeros((Bn, 6, 8), dtype=np.float32)
    sizes = np.array([[3.9, 1.6, 1.56], [0.8, 0.6, 1.73], [1.76, 0.6, 1.73]], dtype=np.float32)
    for b in range(Bn):
        k = 6 - b
        cls = rng.integers(1, 4, k)
        gt[b, :k, 0] = rng.uniform(5, 60, k); gt[b, :k, 1] = rng.uniform(-30, 30, k); gt[b, :k, 2] = rng.uniform(-1.5, -0.5, k)
        gt[b, :k, 3:6] = sizes[cls - 1] * rng.uniform(0.9, 1.1, (k, 3))
        gt[b, :k, 6] = rng.uniform(-np.pi, np.pi, k)
        gt[b, :k, 7] = cls
    return cl, gt


@pytest.mark.parametrize("heads", [None, [['Car', 'Cyclist'], ['Pedestrian']]])
def test_centerpoint_batched_eval_equals_the_per_sample_path(dev, heads):
    torch.manual_seed(4)
    model = small_center_pdm(heads, MAX_OBJ_PER_SAMPLE=200).to(dev).eval()
    with torch.no_grad():
        for head in model.dense_head.heads_list:
            head.hm[-1].bias.fill_(-1.5)                 # scores on both sides of SCORE_THRESH, NMS has work to do
    cl, gt = scene(2, 2048, 9)
    batch = {'batch_size': 2, 'points': torch.from_numpy(synthetic.to_batch_points(cl)).to(dev), 'gt_boxes': torch.from_numpy(gt).to(dev)}
    with torch.no_grad():
        loop, recall = model(dict(batch))
        model.dense_head.model_cfg.POST_PROCESSING['BATCHED'] = True
        batched, recall_b = model(dict(batch))
    assert recall == recall_b and recall['gt'] == 11
    assert len(loop) == len(batched) == 2
    for a, b in zip(loop, batched):
        assert 0 < len(a['pred_boxes']) and a['pred_boxes'].shape[1] == 7 and a['pred_labels'].dtype == torch.int64
        assert int(a['pred_labels'].min()) >= 1 and int(a['pred_labels'].max()) <= 3
        for key in ('pred_boxes', 'pred_scores', 'pred_labels'):
            assert torch.equal(a[key], b[key]), key


def test_center_pdm_training_step_issues_without_host_synchronisation(dev):
    """forward, targets and losses of a CenterPoint training step contain no blocking call (torch's sync debug mode raises at
    an .item(), a boolean-mask index, a pageable copy ...); loss and gradients are finite"""
    torch.manual_seed(1)
    model = small_center_pdm().to(dev).train()
    cl, gt = scene(2, 2048, 5)
    batch = {'batch_size': 2, 'points': torch.from_numpy(synthetic.to_batch_points(cl)).to(dev), 'gt_boxes': torch.from_numpy(gt).to(dev),
             'points_per_sample_checked': True}
    params = [p for p in model.parameters() if p.requires_grad]
    opt = torch.optim.AdamW(params, lr=1e-3, fused=True)
    for _ in range(2):     # first calls build caches (packed weights, grids)
        opt.zero_grad(set_to_none=True)
        ret, tb, disp = model(dict(batch))
        ret['loss'].backward()
        opt.step()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        opt.zero_grad(set_to_none=True)
        ret, tb, disp = model(dict(batch))
        ret['loss'].backward()
        total = torch.nn.utils.clip_grad_norm_(params, 10.0, foreach=True)
        opt.step()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert {'loss_rpn', 'hm_loss_head_0', 'loc_loss_head_0', 'rpn_loss'} <= set(tb) and all(torch.is_tensor(v) for v in tb.values())
    assert torch.isfinite(ret['loss']) and torch.isfinite(total) and float(tb['loc_loss_head_0']) > 0
    # the neck reads the second SA level (SOURCE_LAYER 2): the third SA module and the FP modules lie behind it, outside the
    # loss's graph, and every other parameter has a finite gradient
    behind = ('backbone_3d.SA_modules.2.', 'backbone_3d.FP_modules.')
    for name, p in model.named_parameters():
        if name.startswith(behind):
            assert p.grad is None or torch.isfinite(p.grad).all(), name
        else:
            assert p.grad is not None and torch.isfinite(p.grad).all(), name
    assert any(n.startswith('backbone_3d.SA_modules.0.') for n, _ in model.named_parameters())

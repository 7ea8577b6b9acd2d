"""The anchor head's device operators (csrc/anchor_head.hip) against the reference fixture, against the torch formulations on
the CPU (which tests/test_anchor_head.py pins to the reference), in odd layouts and dtypes, in a poisoned arena, twice for the
same bits, without host synchronisation, captured in a graph, and inside PointPillar."""
import copy
import ctypes

import numpy as np
import pytest
import torch

import anchor_head_case as case
from anchor_head_case import B, H, W, close, close_grad, fixture
from arena import Arena
from pdm_ssd_amd import _native, anchor_head_ops

pytestmark = pytest.mark.gpu

ODD_GRID = [42, 26, 1]            # stride 2: a 13 x 21 map, A = 1638, a multiple of neither 64 nor 256
WEIGHTS = dict(cls_weight=1.0, loc_weight=2.0, dir_weight=0.2, dir_offset=0.78539)


# ---- targets -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag, norm", [("norm0", False), ("norm1", True)])
def test_fused_targets_match_the_reference(dev, tag, norm):
    head = case.build_head(norm=norm).to(dev)
    assert head._flat_anchors.is_cuda and all(a.is_cuda for a in head.anchors)
    gt = torch.from_numpy(fixture()['gt_boxes'].copy()).to(dev)
    td = head.assign_targets(gt)
    assert torch.equal(gt.cpu(), torch.from_numpy(fixture()['gt_boxes'])), 'gt_boxes must stay untouched'
    case.check_targets(td, tag)
    again = head.assign_targets(gt)
    assert all(torch.equal(td[k], again[k]) for k in td), 'two runs must give the same bits'


def against_torch(dev, head, gt):
    """fused targets of gt (numpy) == the torch formulation's on the CPU; returns the fused dict"""
    fused = head.to(dev).assign_targets(torch.from_numpy(gt).to(dev))
    case.same_targets(fused, case.copy_head_cpu(head).assign_targets(torch.from_numpy(gt)))
    return fused


@pytest.mark.parametrize("norm", [False, True])
def test_fused_targets_on_an_odd_map(dev, norm):
    head = case.build_head(grid_size=ODD_GRID, norm=norm)
    assert head._flat_anchors.shape[0] == 1638
    gt = case.draw_boxes(head, 3, 40, seed=5)
    fused = against_torch(dev, head, gt)
    assert int(fused['num_pos'].min()) > 0 and int((fused['box_cls_labels'] == -1).sum()) > 0


@pytest.mark.parametrize("M, cls", [(65, 1), (257, 2)])
def test_fused_targets_with_many_boxes_of_one_class(dev, M, cls):
    """65 boxes of one class in one sample cross a wavefront; 257 cross the 256-box chunk the prepare kernel scans at once"""
    head = case.build_head(grid_size=ODD_GRID)
    gt = case.draw_boxes(head, 2, M, seed=M, classes=(cls,), fill=1.0)
    gt[1, 1:] = 0
    fused = against_torch(dev, head, gt)
    assert int(fused['num_pos'][0]) >= M // 2


def test_fused_targets_without_boxes_and_with_one(dev):
    head = case.build_head(grid_size=ODD_GRID)
    empty = against_torch(dev, head, np.zeros((2, 5, 8), dtype=np.float32))
    assert not empty['box_cls_labels'].any() and not empty['num_pos'].any() and not empty['box_reg_targets'].any()
    one = case.draw_boxes(head, 2, 1, seed=3, fill=1.0)
    assert int(against_torch(dev, head, one)['num_pos'].min()) >= 1
    none = against_torch(dev, head, np.zeros((2, 0, 8), dtype=np.float32))
    assert not none['box_cls_labels'].any()
    outside = np.zeros((1, 2, 8), dtype=np.float32)
    outside[0, 0] = [1.0, 0.0, -1.0, 3.9, 1.6, 1.5, 0.0, 7]         # a class outside 1 .. 3 takes no part
    outside[0, 1] = [3.0, 1.0, -1.0, 3.9, 1.6, 1.5, 0.0, -2]
    assert not against_torch(dev, head, outside)['box_cls_labels'].any()


def test_fused_targets_force_every_anchor_that_shares_a_best_iou(dev):
    """four anchors hold the box's best IoU (1/3, below unmatched) bit for bit: all four positive, as on the CPU"""
    head = case.tie_head()
    fused = against_torch(dev, head, case.tie_boxes())
    assert fused['num_pos'].tolist() == [4] and int((fused['box_cls_labels'] == 1).sum()) == 4


def test_more_boxes_than_max_gt_are_refused(dev):
    head = case.build_head().to(dev)
    with pytest.raises(ValueError, match="MAX_GT"):
        head.assign_targets(torch.zeros((1, anchor_head_ops.MAX_GT + 1, 8), device=dev))


# ---- loss and decode -----------------------------------------------------------------------------------------------------
def random_maps(hh, ww, seed, dtype=torch.float32, num_class=3, bins=2):
    g = torch.Generator().manual_seed(seed)
    return [(torch.randn((3, case.A_LOC * c, hh, ww), generator=g) * s).to(dtype).float() for c, s in ((num_class, 2.0), (7, 0.7), (bins, 1.5))]


def laid_out(t, layout, dtype, dev):
    t = t.to(dtype).to(dev)
    if layout == "channels_last":
        t = t.contiguous(memory_format=torch.channels_last)
        assert not t.is_contiguous()
    elif layout == "slice":
        wide = torch.full((t.shape[0], t.shape[1] + 5, t.shape[2], t.shape[3]), float('nan'), dtype=dtype, device=dev)
        wide[:, 3:3 + t.shape[1]] = t
        t = wide[:, 3:3 + t.shape[1]]
        assert not t.is_contiguous()
    return t


def fused_losses(head, maps, td):
    leaves = [None if t is None else t.detach().requires_grad_(True) for t in maps]
    w = dict(WEIGHTS)
    terms = anchor_head_ops.anchor_head_loss(leaves[0], leaves[1], leaves[2], td['box_cls_labels'], td['box_reg_targets'], td['num_pos'],
                                             head._anchor_rot, [1.0] * 7, head.num_class, num_dir_bins=2, **w)
    total = terms[0] + terms[1] + (terms[2] if leaves[2] is not None else 0.0)
    total.backward()
    return [t.detach() for t in terms], [None if t is None else t.grad for t in leaves]


@pytest.mark.parametrize("grid, layout, dtype, direction", [
    (case.GRID_SIZE, "contiguous", torch.float32, True),        # even W: two cells per access
    (ODD_GRID, "contiguous", torch.float32, True),              # odd W: one
    (case.GRID_SIZE, "channels_last", torch.float32, True),
    (case.GRID_SIZE, "slice", torch.float32, True),
    (case.GRID_SIZE, "contiguous", torch.bfloat16, True),       # bf16 pairs
    (ODD_GRID, "slice", torch.bfloat16, True),
    (case.GRID_SIZE, "channels_last", torch.bfloat16, False),
])
def test_fused_loss_and_decode_match_the_torch_formulation(dev, grid, layout, dtype, direction):
    """the torch formulation is fed the same (bf16-rounded) values in fp32"""
    head = case.build_head(grid_size=grid, direction=direction)
    hh, ww = grid[1] // 2, grid[0] // 2
    gt = case.draw_boxes(head, 3, 12, seed=hh)
    td_cpu = head.assign_targets(torch.from_numpy(gt))
    assert int(td_cpu['num_pos'].min()) > 0
    plain = random_maps(hh, ww, seed=ww, dtype=dtype)
    if not direction:
        plain[2] = None
    want_terms, want_grads = case.torch_losses(head, plain, td_cpu)
    head = head.to(dev)
    maps = [None if t is None else laid_out(t, layout, dtype, dev) for t in plain]
    td = {k: v.to(dev) for k, v in td_cpu.items()}
    terms, grads = fused_losses(head, maps, td)
    for got, want in zip(terms, want_terms):
        if want is not None:
            close(float(got), float(want))
    assert direction or float(terms[2]) == 0.0
    for got, want, m in zip(grads, want_grads, maps):
        if want is None:
            continue
        assert got.dtype == dtype and got.shape == m.shape
        if dtype == torch.float32:
            close_grad(got.cpu().numpy(), want.numpy())
        else:                                                        # the fp32 gradient rounded to bf16 once: half an ulp of 8 significant bits, 2^-8 relative
            err = (got.float().cpu() - want).abs()
            assert bool((err <= 2.0 ** -8 * want.abs() + case.TOL * float(want.abs().max())).all())
    # decode
    cpu = case.copy_head_cpu(head)
    _, want_boxes = cpu.generate_predicted_boxes(3, plain[0], plain[1], plain[2])
    cls, boxes = head.generate_predicted_boxes(3, maps[0], maps[1], maps[2])
    assert boxes.dtype == torch.float32 and boxes.shape == (3, hh * ww * 6, 7) and cls.dtype == torch.float32
    close(boxes.cpu().numpy(), want_boxes.numpy())
    assert torch.equal(cls.cpu(), plain[0].permute(0, 2, 3, 1).reshape(3, -1, 3))


def test_decode_takes_the_lower_bin_on_equal_logits(dev):
    head = case.build_head()
    box, dirs = torch.zeros((1, 42, H, W)), torch.zeros((1, 12, H, W))       # every pair of logits equal: bin 0
    _, want = head.generate_predicted_boxes(1, torch.zeros((1, 18, H, W)), box, dirs)
    head = head.to(dev)
    out = anchor_head_ops.anchor_decode(box.to(dev), dirs.to(dev), head._flat_anchors, 2, 0.78539, 0.0).cpu()
    close(out.numpy(), want.numpy())
    # bin 0's period is [0.78539, 0.78539 + pi): the rotation-0 anchors come out at pi, the rotation-1.57 anchors as they are
    close(out[0, 0::2, 6].numpy(), np.full(H * W * 3, np.pi))
    close(out[0, 1::2, 6].numpy(), np.full(H * W * 3, 1.57))
    dirs[:, 1::2] = 1.0                                              # bin 1 wins: one period further
    out1 = anchor_head_ops.anchor_decode(box.to(dev), dirs.to(dev), head._flat_anchors, 2, 0.78539, 0.0).cpu()
    close(out1[0, :, 6].numpy(), (out[0, :, 6] + np.pi).numpy())


# ---- the head against the fixture ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("state, kw, prefix", [('', {}, ''), ('nodir.', {'direction': False}, 'nodir.'), ('nc1.', {'num_class': 1}, 'nc1.')])
def test_head_on_the_gpu_matches_the_reference(dev, state, kw, prefix):
    fx = fixture()
    head = case.build_head(state=state, **kw).to(dev).train()
    feats = torch.from_numpy(fx['spatial_features_2d']).to(dev)
    head({'batch_size': B, 'spatial_features_2d': feats, 'gt_boxes': torch.from_numpy(fx['gt_boxes'].copy()).to(dev)})
    fr = head.forward_ret_dict
    case.check_targets(fr, 'norm0')
    keys = [k for k in case.MAPS if k in fr]
    for k in keys:
        assert fr[k].shape[2:] == (H, W)                             # as the convolutions leave them
        fr[k].retain_grad()
    loss, tb = head.get_loss()
    loss.backward()
    assert ('rpn_loss_dir' in tb) == (state != 'nodir.')
    for k, v in tb.items():
        assert torch.is_tensor(v) and v.is_cuda and v.dim() == 0 and not v.requires_grad
        close(float(v), float(fx[f'{prefix}tb.{k}']))
    if state == '':
        for k in keys:
            close(fr[k].detach().cpu().numpy(), fx[f'pred.{k}'])
            close_grad(fr[k].grad.cpu().numpy(), fx[f'grad.{k}'])
    if state == 'nc1.':
        close_grad(fr['cls_preds'].grad.cpu().numpy(), fx['nc1.grad.cls_preds'])
    if state != 'nc1.':
        head.eval()
        with torch.no_grad():
            bd = head({'batch_size': B, 'spatial_features_2d': feats})
        close(bd['batch_cls_preds'].cpu().numpy(), fx[f'{prefix}batch_cls_preds'])
        close(bd['batch_box_preds'].cpu().numpy(), fx[f'{prefix}batch_box_preds'])


# ---- arena -------------------------------------------------------------------------------------------------------------------
def host(ctype, values):
    return _native.host_array(ctype, values)


@pytest.mark.parametrize("grid", [ODD_GRID, case.GRID_SIZE])
def test_operators_in_a_poisoned_arena_at_a_4_byte_misalignment(dev, grid):
    """every tensor carved 4 bytes off a 16-byte boundary, float inputs surrounded by NaN: same results, red zones intact.  On
    the even map the fp32 pointers are not on a pair boundary, so the loss and the decode fall back from two cells a thread to
    one, while the expectation (torch's own aligned tensors) takes two: the same gradients and boxes bit for bit, and sums
    whose partials are cut differently"""
    head = case.build_head(grid_size=grid)
    hh, ww = grid[1] // 2, grid[0] // 2
    A = hh * ww * 6
    gt_np = case.draw_boxes(head, 3, 12, seed=8)
    plain = random_maps(hh, ww, seed=4)
    td_cpu = head.assign_targets(torch.from_numpy(gt_np))
    head = head.to(dev)
    want_td = head.assign_targets(torch.from_numpy(gt_np).to(dev))
    want_terms, want_grads = fused_losses(head, [t.to(dev) for t in plain], want_td)
    want_boxes = anchor_head_ops.anchor_decode(plain[1].to(dev), plain[2].to(dev), head._flat_anchors, 2, 0.78539, 0.0)
    nan = float('nan')
    ar = Arena(dev)
    stream = _native.stream(dev)
    anchors = ar.put(head._flat_anchors.cpu(), 4, nan)
    gt = ar.put(gt_np, 4, nan)
    labels, targets = ar.carve((3, A), torch.int32, 4), ar.carve((3, A, 7), torch.float32, 4)
    weights, num_pos = ar.carve((3, A), torch.float32, 4), ar.carve((3,), torch.int32, 4)
    nbytes = _native.lib().pdm_anchor_targets_workspace_bytes(3, 12, 3)
    ws = ar.carve((nbytes,), torch.uint8, 8)
    _native.call("pdm_anchor_targets", stream, 3, 12, 8, A, 6, 3, 3, anchors.data_ptr(), host(ctypes.c_int, [0, 0, 1, 1, 2, 2]),
                 host(ctypes.c_int, [-1, 0, 1, 2]), host(ctypes.c_float, [0.6, 0.5, 0.5]), host(ctypes.c_float, [0.45, 0.35, 0.35]),
                 gt.data_ptr(), 0, labels.data_ptr(), targets.data_ptr(), weights.data_ptr(), num_pos.data_ptr(), ws.data_ptr(), nbytes)
    torch.cuda.synchronize()
    ar.check()
    for got, key in ((labels, 'box_cls_labels'), (targets, 'box_reg_targets'), (weights, 'reg_weights'), (num_pos, 'num_pos')):
        assert torch.equal(got, want_td[key]), key
    case.same_targets({'box_cls_labels': labels, 'box_reg_targets': targets, 'reg_weights': weights, 'num_pos': num_pos}, td_cpu)

    ar.reset()
    maps = [ar.put(t, 4, nan) for t in plain]
    lab, tgt, npos = ar.put(want_td['box_cls_labels'].cpu(), 4, 0), ar.put(want_td['box_reg_targets'].cpu(), 4, nan), ar.put(want_td['num_pos'].cpu(), 4, 1)
    out = ar.carve((3,), torch.float32, 4)
    grads = [ar.carve(tuple(t.shape), torch.float32, 4) for t in plain]
    nbytes = _native.lib().pdm_anchor_head_loss_workspace_bytes(3, hh, ww)
    ws = ar.carve((nbytes,), torch.uint8, 8)
    _native.call("pdm_anchor_head_loss", stream, 3, hh, ww, 6, 3, 2, host(ctypes.c_void_p, [t.data_ptr() for t in maps]), host(ctypes.c_int, [0, 0, 0]),
                 host(ctypes.c_longlong, [s for t in maps for s in t.stride()]), lab.data_ptr(), tgt.data_ptr(), npos.data_ptr(),
                 host(ctypes.c_float, head._anchor_rot), host(ctypes.c_float, [1.0] * 7), 1.0, 2.0, 0.2, 0.78539, 1.0 / 9.0, 0.25, 2.0,
                 out.data_ptr(), grads[0].data_ptr(), grads[1].data_ptr(), grads[2].data_ptr(), ws.data_ptr(), nbytes)
    torch.cuda.synchronize()
    ar.check()
    if ww % 2:
        assert torch.equal(out, torch.stack(want_terms))
    else:
        close(out.cpu().numpy(), torch.stack(want_terms).cpu().numpy())
    for got, want in zip(grads, want_grads):
        assert torch.equal(got, want)

    ar.reset()
    maps = [ar.put(t, 4, nan) for t in plain[1:]]
    anchors = ar.put(head._flat_anchors.cpu(), 4, nan)
    boxes = ar.carve((3, A, 7), torch.float32, 4)
    _native.call("pdm_anchor_decode", stream, 3, hh, ww, 6, 2, host(ctypes.c_void_p, [t.data_ptr() for t in maps]), host(ctypes.c_int, [0, 0]),
                 host(ctypes.c_longlong, [s for t in maps for s in t.stride()]), anchors.data_ptr(), 0.78539, 0.0, boxes.data_ptr())
    torch.cuda.synchronize()
    ar.check()
    assert torch.equal(boxes, want_boxes) and torch.isfinite(boxes).all()


# ---- reproducibility, synchronisation, capture ---------------------------------------------------------------------------------
def test_two_calls_agree_bit_for_bit(dev):
    head = case.build_head()
    gt = torch.from_numpy(case.draw_boxes(head, 3, 40, seed=2)).to(dev)
    head = head.to(dev)
    maps = [t.to(dev) for t in random_maps(H, W, seed=6)]
    runs = []
    for _ in range(2):
        td = head.assign_targets(gt)
        terms, grads = fused_losses(head, maps, td)
        boxes = anchor_head_ops.anchor_decode(maps[1], maps[2], head._flat_anchors, 2, 0.78539, 0.0)
        runs.append(list(td.values()) + terms + grads + [boxes])
    assert all(torch.equal(a, b) for a, b in zip(*runs))


def test_loss_folds_more_block_partials_than_the_finish_kernel_has_threads(dev):
    """B = 1 on a 257 x 257 map: odd W takes the one-cell path, 66 049 cells make 259 workgroups, so the finish kernel's
    threads 0 .. 2 add a second partial (rows t, t + 256) and the rest one: a ragged second pass.  Two slots, one class,
    direction map on; against the torch formulation at the standing tolerance, and twice for the same bits."""
    def edit(cfg):
        cfg['ANCHOR_GENERATOR_CONFIG'] = cfg['ANCHOR_GENERATOR_CONFIG'][:1]
    hh = ww = 257
    head = case.build_head(num_class=1, grid_size=[2 * ww, 2 * hh, 1], pc_range=[0.0, -51.4, -3.0, 102.8, 51.4, 1.0], edit=edit)
    assert len(head._anchor_rot) == 2 and head._flat_anchors.shape[0] == hh * ww * 2
    assert 256 < -(-hh * ww // 256) < 512 and -(-hh * ww // 256) % 64 != 0
    rng = np.random.default_rng(11)
    gt = np.zeros((1, 24, 8), dtype=np.float32)
    gt[0, :, :7] = np.stack([rng.uniform(2, 100, 24), rng.uniform(-49, 49, 24), rng.uniform(-1.2, -0.6, 24), rng.uniform(3.5, 4.3, 24),
                             rng.uniform(1.5, 1.7, 24), rng.uniform(1.4, 1.7, 24), rng.uniform(-3.1, 3.1, 24)], 1)
    gt[0, :, 7] = 1
    head = head.to(dev)
    td = head.assign_targets(torch.from_numpy(gt).to(dev))
    assert int(td['num_pos'][0]) > 0
    g = torch.Generator().manual_seed(12)
    plain = [torch.randn((1, 2 * c, hh, ww), generator=g) * s for c, s in ((1, 2.0), (7, 0.7), (2, 1.5))]
    want_terms, want_grads = case.torch_losses(head, plain, td)
    maps = [t.to(dev) for t in plain]
    terms, grads = fused_losses(head, maps, td)
    again_terms, again_grads = fused_losses(head, maps, td)
    assert all(torch.equal(a, b) for a, b in zip(terms + grads, again_terms + again_grads)), 'two runs must give the same bits'
    for got, want in zip(terms, want_terms):
        close(float(got), float(want))
    for got, want in zip(grads, want_grads):
        close_grad(got.cpu().numpy(), want.numpy())


def small_step(head, feats, gt):
    """forward, get_loss, backward to the parameters -> loss and the gradients on the three conv outputs"""
    head({'batch_size': feats.shape[0], 'spatial_features_2d': feats, 'gt_boxes': gt})
    maps = [head.forward_ret_dict[k] for k in case.MAPS]
    loss, tb = head.get_loss()
    grads = torch.autograd.grad(loss, maps + [p for p in head.parameters()])
    assert all(g is not None for g in grads)
    return loss.detach(), grads[:3]


def test_training_step_without_host_synchronisation_and_captured_in_a_graph(dev):
    fx = fixture()
    head = case.build_head(state='').to(dev).train()
    feats = torch.from_numpy(fx['spatial_features_2d']).to(dev)
    gt = torch.from_numpy(fx['gt_boxes'].copy()).to(dev)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        small_step(head, feats, gt)                                  # warm-up
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            eager_loss, eager_grads = small_step(head, feats, gt)
        finally:
            torch.cuda.set_sync_debug_mode("default")
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    close(float(eager_loss), float(fx['tb.rpn_loss']))
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):                                        # any host synchronisation in here would fail the capture
        loss, grads = small_step(head, feats, gt)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(loss, eager_loss) and all(torch.equal(a, b) for a, b in zip(grads, eager_grads))
    with torch.no_grad():
        gt[1, 0, 0] += 1.7                                           # the lone Car of sample 1 moves a cell: other targets
    g.replay()
    torch.cuda.synchronize()
    moved = float(loss)
    with torch.cuda.stream(side):
        again = small_step(head, feats, gt)[0]
    torch.cuda.synchronize()
    assert moved != float(eager_loss) and moved == float(again)


# ---- the detector ------------------------------------------------------------------------------------------------------------
def small_point_pillar():
    from pdm_ssd_amd.detector_config import POINT_PILLAR_CFG, build_point_pillar, pillar_dataset
    cfg = copy.deepcopy(POINT_PILLAR_CFG)
    dataset = pillar_dataset(4, point_cloud_range=[0, -7.68, -3, 20.48, 7.68, 1], voxel_size=[0.16, 0.16, 4], grid_size=[128, 96, 1])
    return build_point_pillar(cfg, dataset=dataset)


def test_point_pillar_runs_eval_both_ways_and_a_training_step(dev):
    torch.manual_seed(3)
    model = small_point_pillar().to(dev)
    assert [type(m).__name__ for m in model.module_list] == ['DynamicPillarVFE', 'PointPillarScatter', 'BaseBEVBackbone', 'AnchorHeadSingle']
    assert model.dense_head._flat_anchors.shape == (48 * 64 * 6, 7)
    rng = np.random.default_rng(1)
    n = 3000
    pts = np.concatenate([np.stack([np.full(n, b), rng.uniform(0, 20.48, n), rng.uniform(-7.68, 7.68, n), rng.uniform(-2.5, 0.5, n),
                                    rng.uniform(0, 1, n)], axis=1) for b in range(2)]).astype(np.float32)
    gt = np.zeros((2, 3, 8), dtype=np.float32)
    gt[0, 0] = [6.0, 1.0, -1.0, 3.9, 1.6, 1.5, 0.3, 1]
    gt[0, 1] = [12.0, -3.0, -0.8, 0.8, 0.6, 1.7, -1.2, 2]
    gt[1, 0] = [15.7, -2.2, -0.9, 1.7, 0.6, 1.7, 2.1, 3]
    batch = {'batch_size': 2, 'points': torch.from_numpy(pts).to(dev), 'gt_boxes': torch.from_numpy(gt).to(dev)}
    model.eval()
    with torch.no_grad():
        model.dense_head.conv_cls.bias.fill_(-1.5)                   # scores on both sides of SCORE_THRESH, NMS has work to do
        model.dense_head.conv_cls.weight.normal_(0.0, 0.05)
        captured = {}
        orig = model.post_processing

        def grab(bd):                                                # both ways on the same head outputs
            captured['bd'] = bd
            return orig(bd)
        model.post_processing = grab
        loop, recall = model(dict(batch))
        del model.post_processing
        assert 'BATCHED' not in model.model_cfg.POST_PROCESSING and captured['bd']['batch_cls_preds'].shape == (2, 48 * 64 * 6, 3)
        model.model_cfg.POST_PROCESSING['BATCHED'] = True
        batched, recall_b = model.post_processing(captured['bd'])
        forward_b, recall_f = model(dict(batch))                     # and through forward with the key set
        del model.model_cfg.POST_PROCESSING['BATCHED']
    assert recall_f == recall and len(forward_b) == 2
    # a second forward does not repeat the first bit for bit (its scores were seen one ulp, 3e-8, away: the backbone's
    # convolutions are the library's), so its result is compared at TOL, and printed
    for a, b in zip(loop, forward_b):
        assert len(a['pred_boxes']) == len(b['pred_boxes']) and torch.equal(a['pred_labels'], b['pred_labels'])
        print('second forward: max |score difference| %.3g' % float((a['pred_scores'] - b['pred_scores']).abs().max()))
        close(b['pred_boxes'].cpu().numpy(), a['pred_boxes'].cpu().numpy())
        close(b['pred_scores'].cpu().numpy(), a['pred_scores'].cpu().numpy())
    assert recall == recall_b and recall['gt'] == 3 and len(loop) == len(batched) == 2
    for a, b in zip(loop, batched):
        assert 0 < len(a['pred_boxes']) and a['pred_boxes'].shape[1] == 7 and torch.isfinite(a['pred_boxes']).all()
        assert int(a['pred_labels'].min()) >= 1 and int(a['pred_labels'].max()) <= 3
        for key in ('pred_boxes', 'pred_scores', 'pred_labels'):
            assert torch.equal(a[key], b[key]), key
    model.train()
    ret, tb, _ = model(dict(batch))
    ret['loss'].backward()
    assert torch.isfinite(ret['loss']) and {'loss_rpn', 'rpn_loss_cls', 'rpn_loss_loc', 'rpn_loss_dir', 'rpn_loss'} <= set(tb)
    assert float(tb['rpn_loss_loc']) > 0 and float(tb['rpn_loss_dir']) > 0
    named = dict(model.named_parameters())
    for name in ('dense_head.conv_cls.weight', 'dense_head.conv_box.weight', 'dense_head.conv_dir_cls.weight', 'vfe.pfn_layers.0.linear.weight'):
        grad = named[name].grad
        assert grad is not None and torch.isfinite(grad).all() and bool(grad.any()), name

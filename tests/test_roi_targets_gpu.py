"""Second-stage training on the device: pdm_proposal_targets against the numpy restatement (tests/roi_target_reference.py)
and against the reference's own run (tests/golden/ref_roi_targets.npz), the draw's properties, graph capture, pdm_rcnn_loss
against the torch formulation and the reference's values, the limits, and the detector in training mode."""
import copy
import ctypes

import numpy as np
import pytest
import torch

import roi_head_case
import roi_target_reference as rt
import roi_target_case as host

SAMPLER = host.SAMPLER


@pytest.fixture(scope='module')
def fix():
    return dict(np.load(host.FIXTURE))


@pytest.fixture(scope='module')
def restated(fix, oracle):
    """the restatement's answer for the fixture case at steps 0 and 1, computed once"""
    return {(tag, step): rt.proposal_targets(fix['rois'], fix['roi_scores'], fix['roi_labels'], fix['gt_boxes'],
                                             dict(SAMPLER, CLS_SCORE_TYPE=tag), int(fix['draw'][0]), step)
            for tag, step in (('cls', 0), ('roi_iou', 0), ('cls', 1))}


def run_operator(dev, rois, scores, labels, gt, seed, state=None, cfg=SAMPLER, tag='cls'):
    from pdm_ssd_amd import roi_targets
    state = roi_targets.new_state(dev) if state is None else state
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)   # noqa: E731
    S = cfg['ROI_PER_IMAGE']
    out = roi_targets.proposal_targets(t(rois), t(scores), t(labels), t(gt), S, int(np.round(cfg['FG_RATIO'] * S)),
                                       cfg['SAMPLE_ROI_BY_EACH_CLASS'], cfg['HARD_BG_RATIO'], cfg['REG_FG_THRESH'], cfg['CLS_FG_THRESH'],
                                       cfg['CLS_BG_THRESH'], cfg['CLS_BG_THRESH_LO'], tag, seed, state)
    return {k: v.cpu().numpy() for k, v in out.items()}, state


def fixture_run(dev, fix, tag='cls', state=None):
    return run_operator(dev, fix['rois'], fix['roi_scores'], fix['roi_labels'], fix['gt_boxes'], int(fix['draw'][0]), state=state, tag=tag)


@pytest.mark.gpu
@pytest.mark.parametrize('tag', ['cls', 'roi_iou'])
def test_proposal_targets_match_restatement_and_reference(dev, fix, restated, tag):
    got, state = fixture_run(dev, fix, tag)
    want = restated[(tag, 0)]
    assert state.cpu().tolist() == [1, 0]                                  # the step advanced, no error
    for key in ('sampled_inds', 'gt_assignment', 'roi_labels', 'reg_valid_mask'):
        assert (got[key] == want[key]).all(), key
    assert (got['sampled_inds'] == fix[f'{tag}.sampled_inds']).all() and (got['gt_assignment'] == fix[f'{tag}.gt_assignment']).all()
    assert (got['roi_scores'] == want['roi_scores']).all()
    for ref, name in ((want, 'restatement'), ({k[len(tag) + 1:]: v for k, v in fix.items() if k.startswith(tag + '.')}, 'reference run')):
        for key in ('gt_iou_of_rois', 'rois', 'gt_of_rois_src', 'gt_of_rois'):
            err = float(np.abs(got[key] - ref[key]).max())
            print(tag, name, key, 'max abs difference', err)
            assert err <= 1e-5, (name, key, err)
        assert (got['roi_labels'] == ref['roi_labels']).all() and (got['reg_valid_mask'] == ref['reg_valid_mask']).all(), name
        if tag == 'cls':
            assert got['rcnn_cls_labels'].dtype == np.int64 and (got['rcnn_cls_labels'] == ref['rcnn_cls_labels']).all(), name
        else:   # the float ramp: one fp32 division of numbers below 1
            assert got['rcnn_cls_labels'].dtype == np.float32
            assert float(np.abs(got['rcnn_cls_labels'] - ref['rcnn_cls_labels']).max()) <= 1e-6, name


def sets_from_product_iou(dev, fix):
    """fg / hard / easy index sets per sample from iou3d_nms_utils.boxes_iou3d_gpu (not from the restatement)"""
    from pdm_ssd_amd.iou3d_nms import iou3d_nms_utils
    sets = []
    for b in range(fix['rois'].shape[0]):
        gt = rt.live_rows(fix['gt_boxes'][b])
        iou = iou3d_nms_utils.boxes_iou3d_gpu(torch.from_numpy(fix['rois'][b]).to(dev), torch.from_numpy(gt[:, 0:7].copy()).to(dev)).cpu().numpy()
        same = fix['roi_labels'][b][:, None] == gt[:, 7].astype(np.int64)[None, :]
        mo = np.where(same, iou, -1.0).max(1)
        mo = np.where(same.any(1), mo, 0.0)
        sets.append((set(np.flatnonzero(mo >= 0.55)), set(np.flatnonzero((mo < 0.55) & (mo >= 0.1))), set(np.flatnonzero(mo < 0.1))))
    return sets


@pytest.mark.gpu
def test_draw_properties(dev, fix, restated):
    got, state = fixture_run(dev, fix)
    idx = got['sampled_inds']
    (fg0, hard0, easy0), (fg1, hard1, easy1), (fg2, hard2, easy2) = sets_from_product_iou(dev, fix)
    # sample 0: fewer fg than fg_per_image = 8 -> all of them once, then min(int((16 - n_fg) * 0.8), n_hard) hard, the rest easy
    n_fg = len(fg0)
    assert 0 < n_fg < 8 and hard0 and easy0
    n_hard = min(int((16 - n_fg) * 0.8), len(hard0))
    assert set(idx[0, :n_fg]) == fg0                                                   # every fg, none twice
    assert set(idx[0, n_fg:n_fg + n_hard]) <= hard0 and set(idx[0, n_fg + n_hard:]) <= easy0
    # sample 1: no ground truth, bg only (every overlap 0: easy); sample 2: fg only, drawn with repetition
    assert not fg1 and not hard1 and set(idx[1]) <= easy1 and (got['gt_iou_of_rois'][1] == 0).all() and (got['gt_of_rois_src'][1] == 0).all()
    assert len(fg2) == fix['rois'].shape[1] and set(idx[2]) <= fg2 and (got['reg_valid_mask'][2] == 1).all()
    assert (got['gt_assignment'][2] != 1).all()                                        # never the interior zero row
    # the same seed and step give the same result; the next step another
    again, _ = fixture_run(dev, fix)
    assert all((again[k] == got[k]).all() for k in got)
    nxt, state = fixture_run(dev, fix, state=state)
    assert state.cpu().tolist() == [2, 0] and (nxt['sampled_inds'] == restated[('cls', 1)]['sampled_inds']).all()
    assert (nxt['sampled_inds'] != idx).any() and set(nxt['sampled_inds'][0, :n_fg]) == fg0
    other, _ = run_operator(dev, fix['rois'], fix['roi_scores'], fix['roi_labels'], fix['gt_boxes'], int(fix['draw'][0]) + 1)
    assert (other['sampled_inds'] != idx).any()


@pytest.mark.gpu
def test_background_draws_are_uniform(dev):
    """256 steps on one sample with 8 hard-bg candidates (IoU 0.34 .. 0.53) and 8 easy ones, no fg: 16 slots = 8 hard + 8 easy per
    step, so each hard candidate's count is Binomial(2048, 1 / 8): mean 256, sd 14.97; each must lie within 6 sd."""
    from pdm_ssd_amd import roi_targets
    gt = np.zeros((1, 2, 8), dtype=np.float32)
    gt[0, 0] = [10, 10, -1, 3.9, 1.6, 1.5, 0.0, 1]
    rois = np.zeros((1, 16, 7), dtype=np.float32)
    rois[0, :, 0:7] = gt[0, 0, 0:7]
    rois[0, :8, 0] += np.linspace(1.2, 1.9, 8)
    rois[0, 8:, 1] += 30 + np.arange(8)
    labels, scores = np.ones((1, 16), dtype=np.int64), np.zeros((1, 16), dtype=np.float32)
    state = roi_targets.new_state(dev)
    t = lambda a: torch.from_numpy(a).to(dev)   # noqa: E731
    r_, s_, l_, g_ = t(rois), t(scores), t(labels), t(gt)
    picks = []
    for _ in range(256):
        out = roi_targets.proposal_targets(r_, s_, l_, g_, 16, 8, True, 0.8, 0.55, 0.6, 0.45, 0.1, 'cls', 99, state)
        picks.append(out['sampled_inds'])
    picks = torch.stack(picks).cpu().numpy()[:, 0]
    assert state.cpu().tolist() == [256, 0]
    assert (picks[:, :8] < 8).all() and (picks[:, 8:] >= 8).all()
    count = np.bincount(picks[:, :8].ravel(), minlength=8)
    sd = np.sqrt(2048 * (1 / 8) * (7 / 8))
    print('hard-bg draw counts', count.tolist(), 'mean 256, 6 sd =', 6 * sd)
    assert (np.abs(count - 256) <= 6 * sd).all()
    count = np.bincount(picks[:, 8:].ravel() - 8, minlength=8)
    assert (np.abs(count - 256) <= 6 * sd).all()


@pytest.mark.gpu
def test_assign_targets_and_loss_capture_in_a_graph(dev, fix):
    head = host.template_head(fix, seed=int(fix['draw'][0])).to(dev)
    t = lambda a: torch.from_numpy(a).to(dev)   # noqa: E731
    bd = {'batch_size': 3, 'rois': t(fix['rois']), 'roi_scores': t(fix['roi_scores']), 'roi_labels': t(fix['roi_labels']),
          'gt_boxes': t(fix['gt_boxes'])}
    rcnn_cls, rcnn_reg = t(fix['rcnn_cls']), t(fix['rcnn_reg'])

    def step():
        targets = head.assign_targets(bd)
        head.forward_ret_dict = dict(targets, rcnn_cls=rcnn_cls, rcnn_reg=rcnn_reg)
        loss, tb = head.get_loss()
        return targets, loss, tb
    step()                                              # warm-up; allocates the layer's state
    state = head.proposal_target_layer.state(dev)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):                           # any host synchronisation in here would fail the capture
        targets, loss, tb = step()
    outs = list(targets.values()) + [loss] + list(tb.values())
    runs = []
    for _ in range(2):
        state.copy_(torch.tensor([5, 0], dtype=torch.int32))
        g.replay()
        torch.cuda.synchronize()
        assert state.cpu().tolist() == [6, 0]
        runs.append([o.clone() for o in outs])
    for a, b in zip(*runs):
        assert torch.equal(a, b)
    want, _ = fixture_run(dev, fix, state=torch.tensor([5, 0], dtype=torch.int32, device=dev))
    assert (targets['rois'].cpu().numpy() == want['rois']).all() and (targets['gt_of_rois'].cpu().numpy() == want['gt_of_rois']).all()
    assert np.isfinite(float(loss))


@pytest.mark.gpu
def test_fused_rcnn_loss_matches_the_reference_run(dev, fix):
    head = host.template_head(fix).to(dev)
    assert head.use_fused_loss and head._fused_loss_applies(host.loss_inputs(fix, 'cls', dev))
    host.check_losses_against_reference(head, fix, dev)


@pytest.mark.gpu
def test_fused_rcnn_loss_equals_torch_formulation(dev, fix):
    """the two bounds of test_point_head_fused_loss_equals_torch_formulation: losses to 1e-5 relative, gradients to 1e-4 of
    their scale; the fixture case, its float-label form, a case without fg, and unequal factors on the three losses"""
    fused, plain = host.template_head(fix).to(dev), host.template_head(fix).to(dev)
    plain.use_fused_loss = False
    for tag, rows, factors in (('cls', slice(None), (1.0, 1.0, 1.0)), ('roi_iou', slice(None), (1.0, 1.0, 1.0)),
                               ('cls', slice(1, 2), (1.0, 1.0, 1.0)), ('cls', slice(None), (0.5, 2.0, 3.0))):
        res = []
        for head in (fused, plain):
            ret = host.loss_inputs(fix, tag, dev, rows)
            assert head._fused_loss_applies(ret) == (head is fused)
            loss_cls, tb_cls = head.get_box_cls_layer_loss(ret)
            loss_reg, tb_reg = head.get_box_reg_layer_loss(ret)
            # unequal factors reach the two parts of loss_reg only through their own tensors
            if head is fused:
                _, part_reg, part_corner, fg = ret['fused_losses']
                assert not fg.requires_grad and len({x.untyped_storage().data_ptr() for x in ret['fused_losses']}) == 4
                assert all(x.dim() == 0 for x in ret['fused_losses'])
                assert float(fg) == float((ret['reg_valid_mask'] > 0).sum())
                total = factors[0] * loss_cls + factors[1] * part_reg + factors[2] * part_corner
            else:
                plain.model_cfg.LOSS_CONFIG.CORNER_LOSS_REGULARIZATION = False
                only_reg, _ = head.get_box_reg_layer_loss(ret)
                plain.model_cfg.LOSS_CONFIG.CORNER_LOSS_REGULARIZATION = True
                total = factors[0] * loss_cls + factors[1] * only_reg + factors[2] * (loss_reg - only_reg)
            grads = torch.autograd.grad(total, [ret['rcnn_cls'], ret['rcnn_reg']], allow_unused=True)
            grads = [torch.zeros_like(p) if g_ is None else g_ for g_, p in zip(grads, (ret['rcnn_cls'], ret['rcnn_reg']))]
            res.append((dict(tb_cls, **tb_reg), grads))
        (tb_f, g_f), (tb_p, g_p) = res
        for key in ('rcnn_loss_cls', 'rcnn_loss_reg', 'rcnn_loss_corner'):
            host.close(tb_f[key], tb_p[key], 1e-5, f'{tag} {rows} {key}')
        host.grad_close(g_f[0], g_p[0].cpu().numpy(), f'{tag} {rows} {factors} d / d rcnn_cls')
        host.grad_close(g_f[1], g_p[1].cpu().numpy(), f'{tag} {rows} {factors} d / d rcnn_reg')


@pytest.mark.gpu
def test_fused_rcnn_loss_folds_more_block_partials_than_the_finalize_kernel_has_threads(dev, fix):
    """n = 256 * 257 + 3 rows make 258 workgroups: the finalize kernel's threads 0 and 1 add a second partial, the rest one
    (a ragged second pass).  The fixture's rows repeated with seeded predictions; the bounds of
    test_fused_rcnn_loss_equals_torch_formulation, and twice for the same bits."""
    n = 256 * 257 + 3
    assert 256 < -(-n // 256) < 512 and -(-n // 256) % 64 != 0
    fused, plain = host.template_head(fix).to(dev), host.template_head(fix).to(dev)
    plain.use_fused_loss = False
    small = host.loss_inputs(fix, 'cls', dev)
    rows = torch.arange(n, device=dev) % small['reg_valid_mask'].numel()
    g = torch.Generator().manual_seed(n)
    res = []
    for head in (fused, fused, plain):
        ret = {k: small[k].flatten(0, 1)[rows][None].contiguous() for k in ('rois', 'gt_of_rois', 'gt_of_rois_src', 'reg_valid_mask', 'rcnn_cls_labels')}
        g.manual_seed(n)
        ret['rcnn_cls'] = torch.randn((n, 1), generator=g).to(dev).requires_grad_(True)
        ret['rcnn_reg'] = (torch.randn((n, 7), generator=g) * 0.3).to(dev).requires_grad_(True)
        assert head._fused_loss_applies(ret) == (head is fused)
        loss_cls, tb_cls = head.get_box_cls_layer_loss(ret)
        loss_reg, tb_reg = head.get_box_reg_layer_loss(ret)
        grads = torch.autograd.grad(loss_cls + loss_reg, [ret['rcnn_cls'], ret['rcnn_reg']])
        res.append((dict(tb_cls, **tb_reg), grads))
    (tb_f, g_f), (tb_again, g_again), (tb_p, g_p) = res
    for key in ('rcnn_loss_cls', 'rcnn_loss_reg', 'rcnn_loss_corner'):
        assert torch.equal(tb_f[key], tb_again[key]), 'two runs must give the same bits'
        host.close(tb_f[key], tb_p[key], 1e-5, key)
    assert torch.equal(g_f[0], g_again[0]) and torch.equal(g_f[1], g_again[1]), 'two runs must give the same bits'
    host.grad_close(g_f[0], g_p[0].cpu().numpy(), 'd / d rcnn_cls')
    host.grad_close(g_f[1], g_p[1].cpu().numpy(), 'd / d rcnn_reg')


@pytest.mark.gpu
def test_limits_and_refusals(dev, fix):
    from pdm_ssd_amd import _native, roi_targets
    from pdm_ssd_amd.roi_heads.target_assigner import ProposalTargetLayer

    def call(R, M, width=7):
        state = roi_targets.new_state(dev)
        out = roi_targets.proposal_targets(torch.zeros((1, R, width), device=dev), torch.zeros((1, R), device=dev),
                                           torch.ones((1, R), dtype=torch.long, device=dev), torch.zeros((1, M, 8), device=dev),
                                           16, 8, True, 0.8, 0.55, 0.6, 0.45, 0.1, 'cls', 0, state)
        return out, state
    for R, M in ((1025, 4), (4, 257)):
        with pytest.raises(_native.NativeLibraryError, match='code -2'):
            call(R, M)
    out, state = call(1024, 256)                          # the limits themselves are served; all-zero boxes: bg only
    assert state.cpu().tolist() == [1, 0] and (out['gt_iou_of_rois'] == 0).all()
    out, state = call(1, 0)                               # one RoI, no ground-truth row at all
    assert state.cpu().tolist() == [1, 0] and (out['sampled_inds'] == 0).all()
    with pytest.raises(ValueError, match='code size 7'):
        call(4, 4, width=8)
    # neither fg nor bg (NaN overlaps): a flag on the device, raised only when asked
    bd = {'batch_size': 2, 'rois': torch.from_numpy(fix['rois'][:2].copy()).to(dev), 'roi_scores': torch.from_numpy(fix['roi_scores'][:2]).to(dev),
          'roi_labels': torch.from_numpy(fix['roi_labels'][:2]).to(dev), 'gt_boxes': torch.from_numpy(fix['gt_boxes'][:2].copy()).to(dev)}
    bd['rois'][1, :, 5] = float('nan')                   # against all ground truth, every overlap of sample 1 is NaN
    everything = dict(SAMPLER, SAMPLE_ROI_BY_EACH_CLASS=False)
    quiet = ProposalTargetLayer(everything)
    got = quiet(bd)
    assert set(got) == {'rois', 'gt_of_rois', 'gt_iou_of_rois', 'roi_scores', 'roi_labels', 'reg_valid_mask', 'rcnn_cls_labels'}
    assert got['gt_of_rois'].shape == (2, 16, 8) and quiet.state(dev).cpu().tolist() == [1, 1]
    with pytest.raises(NotImplementedError):
        quiet.raise_if_failed()
    with pytest.raises(NotImplementedError):
        ProposalTargetLayer(everything, check=True)(bd)


@pytest.mark.gpu
def test_rcnn_loss_workspace_tail_is_untouched(dev):
    """pdm_proposal_targets takes no workspace; pdm_rcnn_loss does: one row, workspace_bytes + 256 with a pattern behind it"""
    from pdm_ssd_amd import _native
    n = 1
    nbytes = _native.lib().pdm_rcnn_loss_workspace_bytes(n)
    assert nbytes == 16 + 12
    ws = torch.full((nbytes + 256,), 0xA5, dtype=torch.uint8, device=dev)
    f = lambda *shape: torch.zeros(shape, device=dev)   # noqa: E731
    rois = torch.tensor([[1, 2, 0, 4, 2, 1.5, 0.3]], device=dev)
    gt = torch.tensor([[0.2, 0.1, 0.0, 4.1, 1.9, 1.5, 0.1, 1]], device=dev)
    src = torch.tensor([[1.2, 2.1, 0.0, 4.1, 1.9, 1.5, 0.4, 1]], device=dev)
    mask, labels = torch.ones(1, dtype=torch.long, device=dev), torch.ones(1, dtype=torch.long, device=dev)
    rcnn_cls, rcnn_reg = f(1), f(1, 7)
    dcls, dreg, dcorner, outs = f(1), f(1, 7), f(1, 7), [f(1) for _ in range(4)]
    cw = (ctypes.c_float * 7)(*([1.0] * 7))
    _native.call('pdm_rcnn_loss', torch.cuda.current_stream(dev).cuda_stream, n, rcnn_cls.data_ptr(), rcnn_reg.data_ptr(), rois.data_ptr(),
                 gt.data_ptr(), src.data_ptr(), mask.data_ptr(), labels.data_ptr(), 0, ctypes.cast(cw, ctypes.c_void_p), 1.0 / 9.0, 1.0, 1.0,
                 1.0, 1, dcls.data_ptr(), dreg.data_ptr(), dcorner.data_ptr(), *[o.data_ptr() for o in outs], ws.data_ptr(), nbytes)
    torch.cuda.synchronize()
    assert (ws[nbytes:] == 0xA5).all()
    assert float(outs[3]) == 1 and abs(float(outs[0]) - np.log(2)) < 1e-6 and float(outs[1]) > 0 and float(outs[2]) > 0


def train_cfg():
    cfg = copy.deepcopy(roi_head_case.REDUCED_POINT_RCNN_CFG)
    from pdm_ssd_amd.detector_config import POINT_RCNN_TRAIN_CFG
    cfg['ROI_HEAD']['TARGET_CONFIG'] = dict(copy.deepcopy(POINT_RCNN_TRAIN_CFG['ROI_HEAD']['TARGET_CONFIG']), ROI_PER_IMAGE=16)
    cfg['ROI_HEAD']['LOSS_CONFIG'] = copy.deepcopy(POINT_RCNN_TRAIN_CFG['ROI_HEAD']['LOSS_CONFIG'])
    cfg['ROI_HEAD']['NMS_CONFIG']['TRAIN'].update(NMS_PRE_MAXSIZE=512, NMS_POST_MAXSIZE=64)
    return cfg


def no_grad_anywhere(module):
    return all(p.grad is None for p in module.parameters())


@pytest.mark.gpu
def test_point_rcnn_trains_end_to_end(dev):
    from detector_case import scene_boxes
    from pdm_ssd_amd import synthetic
    from pdm_ssd_amd.detector_config import build_point_rcnn
    torch.manual_seed(3)
    model = build_point_rcnn(train_cfg()).to(dev).train()
    B, N = 2, 1024
    cl = synthetic.lidar_like_clouds(B, N, 5)
    gt = scene_boxes(B, 6, 3)
    cl[:, :200, :3] = gt[:, :1, :3] + np.random.default_rng(0).normal(0, 0.5, (B, 200, 3)).astype(np.float32)
    batch = {'batch_size': B, 'points': torch.from_numpy(synthetic.to_batch_points(cl)).to(dev), 'gt_boxes': torch.from_numpy(gt).to(dev)}
    # (1) the first stage's own proposals (NMS_CONFIG.TRAIN): the shape of the result, a finite loss, the keys
    ret_dict, tb_dict, disp_dict = model(dict(batch))
    assert set(ret_dict) == {'loss'} and isinstance(disp_dict, dict) and torch.isfinite(ret_dict['loss'])
    assert {'rcnn_loss_cls', 'rcnn_loss_reg', 'rcnn_loss_corner', 'rcnn_loss', 'point_loss_cls', 'point_loss_box'} <= set(tb_dict)
    assert all(isinstance(v, torch.Tensor) and v.dim() == 0 and not v.requires_grad for k, v in tb_dict.items() if k.startswith('rcnn_'))
    frd = model.roi_head.forward_ret_dict
    assert frd['rois'].shape == (B, 16, 7) and frd['rcnn_cls'].shape == (B * 16, 1) and frd['rcnn_reg'].shape == (B * 16, 7)
    assert 'fused_losses' in frd                                                     # the fused operator served the step
    # (2) proposals given (near the ground truth, so that there are fg rows whatever the untrained first stage proposes)
    rng = np.random.default_rng(1)
    rois = np.zeros((B, 64, 7), dtype=np.float32)
    labels = np.ones((B, 64), dtype=np.int64)
    for b in range(B):
        for k in range(64):
            g = gt[b, k % (6 - b)]
            rois[b, k], labels[b, k] = g[0:7], int(g[7])
            rois[b, k, 0:2] += rng.uniform(-1, 1, 2) * (0.05 if k < 24 else 0.5 if k < 48 else 10.0)
    given = dict(batch, rois=torch.from_numpy(rois).to(dev), roi_labels=torch.from_numpy(labels).to(dev),
                 roi_scores=torch.zeros((B, 64), device=dev))
    model.zero_grad(set_to_none=True)
    ret_dict, tb_dict, _ = model(given)
    assert torch.isfinite(ret_dict['loss']) and float(tb_dict['rcnn_loss_reg']) > 0 and float(tb_dict['rcnn_loss_corner']) > 0
    loss_rcnn, _ = model.roi_head.get_loss()
    assert float(loss_rcnn) == float(tb_dict['rcnn_loss'])
    loss_rcnn.backward(retain_graph=True)
    for name, p in model.roi_head.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), name
    for part in (model.roi_head.cls_layers, model.roi_head.reg_layers, model.roi_head.xyz_up_layer):
        assert any(float(p.grad.abs().max()) > 0 for p in part.parameters())
    assert no_grad_anywhere(model.backbone_3d) and no_grad_anywhere(model.point_head)   # pooling is under no_grad
    model.zero_grad(set_to_none=True)
    ret_dict['loss'].backward()
    for part in (model.backbone_3d, model.point_head, model.roi_head):
        grads = [p.grad for p in part.parameters() if p.grad is not None]
        assert grads and all(torch.isfinite(g_).all() for g_ in grads) and any(float(g_.abs().max()) > 0 for g_ in grads)

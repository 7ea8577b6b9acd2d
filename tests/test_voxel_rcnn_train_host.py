"""Voxel R-CNN's training form without a GPU: the float64 restatement of tests/voxel_rcnn_grad_reference.py against the
reference's own NeighborVoxelSAModuleMSG in training mode (tests/golden/ref_voxel_rcnn_train.npz,
gen_voxel_rcnn_train_fixtures.py), the moment form of the position BatchNorm against nn.BatchNorm2d on the materialised padded
tensor, the argument checks of the three new entry points (an error code before any launch), the predicates, the CPU refusal and
VOXEL_RCNN_TRAIN_CFG."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

import voxel_rcnn_case as case
import voxel_rcnn_grad_reference as vg

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SOURCES = case.HEAD_CFG['ROI_GRID_POOL']['FEATURES_SOURCE']
POOL_CFG = case.HEAD_CFG['ROI_GRID_POOL']['POOL_LAYERS']


@pytest.fixture(scope="module")
def ref():
    z = np.load(os.path.join(GOLDEN, "ref_voxel_rcnn_train.npz"))
    return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def rois():
    return np.load(os.path.join(GOLDEN, "ref_voxel_rcnn.npz"))['g2.rois']


def layer_groups(rois, src, G=2):
    cfg = POOL_CFG[src]
    S = cfg['NSAMPLE'][0]
    hits, offs = vg.level_groups(rois, G, case.levels()[src], cfg['QUERY_RANGES'][0], cfg['POOL_RADIUS'][0], S)
    return vg.kept(hits, offs, S)


@pytest.mark.parametrize("layer", [0, 1])
def test_float64_restatement_matches_the_reference_in_training_mode(ref, rois, layer):
    """Output, the three BatchNorms' running statistics and num_batches_tracked, every parameter gradient and the features'
    gradient of the reference's module (fp32) within 1e-4 of each tensor's largest entry (the eval head fixture's tolerance); the
    generator saw at most 2.7e-6 (ref_voxel_rcnn_train_manifest.json, restatement_error).  The winners' margins the generator
    searched for hold: 1e-4 of the largest slot value."""
    src = SOURCES[layer]
    with open(os.path.join(GOLDEN, "ref_voxel_rcnn_train_manifest.json")) as f:
        manifest = json.load(f)
    state = {k[len(f'layer{layer}.state.'):]: v for k, v in ref.items() if k.startswith(f'layer{layer}.state.')}
    rows, d, cnt = layer_groups(rois, src)
    assert (cnt == 0).any() and (cnt == rows.shape[1]).any()      # empty groups and overflowing ones
    assert layer == 1 or ((cnt > 0) & (cnt < rows.shape[1])).any()      # and, in the small window, padded ones
    mods = vg.scale_modules(state, '', 0)
    feats = torch.from_numpy(case.level_features(src, len(case.levels()[src]['indices']))).double().requires_grad_(True)
    out, _, x = vg.train_forward(mods, feats, rows, d)
    cot = torch.randn(out.shape, generator=torch.Generator().manual_seed(77 + layer), dtype=torch.float64)
    out.backward(cot)
    got = {'out': out.detach(), 'features.grad': feats.grad}
    got.update({k + '.grad': p.grad for k, p in vg.named_parameters(mods).items()})
    got.update(vg.running_stats(mods))
    names = [k[len(f'layer{layer}.'):] for k in ref if k.startswith(f'layer{layer}.') and '.state.' not in k]
    assert sorted(names) == sorted(got) and len(names) == 2 + 9 + 9
    for k in names:
        want = ref[f'layer{layer}.{k}']
        err = float(np.abs(got[k].numpy().reshape(want.shape) - want).max()) / max(float(np.abs(want).max()), 1e-30)
        assert err <= 1e-4, (k, err)
        assert err <= 2 * manifest['restatement_error'][src][k] + 1e-9, (k, err)
    assert int(ref[f'layer{layer}.mlps_pos.1.num_batches_tracked']) == 1
    gap, lowest = vg.winner_margins(x, float(x.detach().max()))
    assert gap >= 1e-4 and lowest >= 1e-4, (gap, lowest)


def position_case(which):
    """kept groups (rows, d) of: 'overflow' the x_conv2 level of the case (groups overflow S = 4, partly filled and empty ones
    beside them); 'empty_sample' the same with every group of sample 0 emptied as well (sample 1 is empty already)"""
    rois = np.load(os.path.join(GOLDEN, "ref_voxel_rcnn.npz"))['g2.rois']
    rows, d, cnt = layer_groups(rois, 'x_conv2')
    if which == 'empty_sample':
        per = rows.shape[0] // case.B
        assert (cnt[per:2 * per] == 0).all()
        rows, d = rows.copy(), d.copy()
        rows[:per], d[:per] = -1, 0
    return rows, d


@pytest.mark.parametrize("momentum", [0.1, None])
@pytest.mark.parametrize("which", ['overflow', 'empty_sample'])
def test_moment_form_of_the_position_batchnorm_equals_batchnorm2d(which, momentum):
    """Conv2d(3 -> C1) + BatchNorm2d in training mode on the materialised padded (1, 3, M, S) tensor against (a) the helper's
    moment form and (b) NeighborVoxelSAModuleMSG._position_norm, all float64, at 1e-12 of each tensor's largest entry: the
    output, the gradients of the weight, gamma and beta under a seeded cotangent, and both running statistics (momentum 0.1 and
    None, the cumulative average)."""
    from pdm_ssd_amd.pointnet2_stack.voxel_pool_modules import NeighborVoxelSAModuleMSG
    rows, d = position_case(which)
    _, dd = vg.padded(rows, d)
    M, S, C1 = rows.shape[0], rows.shape[1], 16
    mom = vg.moments(dd)
    g = torch.Generator().manual_seed(5)

    def fresh():
        conv, norm = nn.Conv2d(3, C1, 1, bias=False).double(), nn.BatchNorm2d(C1, momentum=momentum).double()
        gg = torch.Generator().manual_seed(9)
        with torch.no_grad():
            conv.weight.copy_(torch.randn(conv.weight.shape, generator=gg, dtype=torch.float64) * 0.3)
            norm.weight.copy_(torch.rand(C1, generator=gg, dtype=torch.float64) + 0.5)
            norm.bias.copy_(torch.randn(C1, generator=gg, dtype=torch.float64) * 0.2)
            norm.running_mean.copy_(torch.randn(C1, generator=gg, dtype=torch.float64) * 0.1)
            norm.running_var.copy_(torch.rand(C1, generator=gg, dtype=torch.float64) + 0.5)
        return conv, norm.train()
    cot = torch.randn((1, C1, M, S), generator=g, dtype=torch.float64)
    x = torch.from_numpy(dd).permute(2, 0, 1).unsqueeze(0)

    conv, norm = fresh()
    want = norm(conv(x))
    want.backward(cot)
    wanted = dict(out=want.detach(), dw=conv.weight.grad.reshape(C1, 3), dgamma=norm.weight.grad, dbeta=norm.bias.grad,
                  running_mean=norm.running_mean.clone(), running_var=norm.running_var.clone())

    def check(got, what):
        for k, w in wanted.items():
            err = float((got[k] - w).abs().max()) / float(w.abs().max())
            assert err <= 1e-12, (what, k, err)

    def position(conv, scale, shift):
        return (torch.einsum('msj,cj->cms', torch.from_numpy(dd), conv.weight.reshape(C1, 3)) * scale.view(-1, 1, 1) + shift.view(-1, 1, 1)).unsqueeze(0)

    conv, norm = fresh()        # (a) the helper's form; the running statistics by BatchNorm's rule
    scale, shift, mean, unbiased = vg.position_norm_from_moments(conv.weight.reshape(C1, 3), norm.weight, norm.bias, norm.eps, mom, M * S)
    out = position(conv, scale, shift)
    out.backward(cot)
    f = 1.0 if momentum is None else momentum
    check(dict(out=out.detach(), dw=conv.weight.grad.reshape(C1, 3), dgamma=norm.weight.grad, dbeta=norm.bias.grad,
               running_mean=(1 - f) * norm.running_mean + f * mean.detach(), running_var=(1 - f) * norm.running_var + f * unbiased.detach()), 'helper')

    conv, norm = fresh()        # (b) the module's
    scale, shift = NeighborVoxelSAModuleMSG._position_norm(conv, norm, torch.from_numpy(mom), M * S)
    out = position(conv, scale, shift)
    out.backward(cot)
    check(dict(out=out.detach(), dw=conv.weight.grad.reshape(C1, 3), dgamma=norm.weight.grad, dbeta=norm.bias.grad,
               running_mean=norm.running_mean, running_var=norm.running_var), 'module')
    assert int(norm.num_batches_tracked) == 1


def test_position_norm_from_a_padding_weighted_moment_by_hand():
    """Two grid points, S = 4: one hit at offset (1, 2, 3), which the padded tensor repeats four times, and an empty group of four
    zero offsets: N = 8, sums (4, 8, 12 | 4, 8, 12, 16, 24, 36).  With W = identity, gamma = 1, beta = 0, eps = 0 the module's
    _position_norm must give mean (0.5, 1, 1.5), variance (0.25, 1, 2.25): scale (2, 1, 2 / 3), shift (-1, -1, -1), and with
    momentum 0.1 running_mean 0.1 mean, running_var 0.9 + 0.1 (8 / 7) variance."""
    from pdm_ssd_amd.pointnet2_stack.voxel_pool_modules import NeighborVoxelSAModuleMSG
    rows = np.array([[5, -1, -1, -1], [-1, -1, -1, -1]], np.int32)
    d = np.zeros((2, 4, 3), np.float32)
    d[0, 0] = [1, 2, 3]
    idx, dd = vg.padded(rows, d)
    assert idx.tolist() == [[5, 5, 5, 5], [0, 0, 0, 0]]
    mom = vg.moments(dd)
    assert mom.tolist() == [4, 8, 12, 4, 8, 12, 16, 24, 36]
    conv, norm = nn.Conv2d(3, 3, 1, bias=False).double(), nn.BatchNorm2d(3, eps=0.0).double().train()
    with torch.no_grad():
        conv.weight.copy_(torch.eye(3, dtype=torch.float64).view(3, 3, 1, 1))
    scale, shift = NeighborVoxelSAModuleMSG._position_norm(conv, norm, torch.from_numpy(mom), 8)
    close = lambda a, b: float((a.detach() - torch.tensor(b, dtype=torch.float64)).abs().max()) <= 1e-15      # noqa: E731
    assert close(scale, [2, 1, 2 / 3]) and close(shift, [-1, -1, -1])
    assert close(norm.running_mean, [0.05, 0.1, 0.15]) and close(norm.running_var, [0.9 + 0.1 * 8 / 7 * v for v in (0.25, 1, 2.25)])
    assert int(norm.num_batches_tracked) == 1


def test_entry_points_validate_their_arguments_before_any_launch():
    """null pointers, small workspaces, M > 2^22, unsupported widths / windows / nsample / G, misalignment: an error code and a
    message, no launch"""
    from pdm_ssd_amd import _native
    lib = _native.lib()
    buf = (C.c_double * 4096)()
    ptr = C.cast(buf, C.c_void_p)
    off4 = C.c_void_p(ptr.value + 4)
    err = _native.NativeLibraryError
    grid = (3, 21, 8, 11)
    index_bytes = lib.pdm_sparse_index_workspace_bytes(100, *grid)
    M = 3 * 5 * 8
    qbytes = lib.pdm_roi_grid_query_workspace_bytes(M)
    assert qbytes >= 9 * 8 * 8 and lib.pdm_roi_grid_query_workspace_bytes((1 << 22) + 1) == 0 and lib.pdm_roi_grid_query_workspace_bytes(-1) == 0
    assert lib.pdm_roi_grid_query_workspace_bytes(1 << 22) > 0

    def query(**change):
        a = dict(B=3, n=5, roi_stride=7, rois=ptr, G=2, D=21, H=8, W=11, stride=2, vx=0.5, vy=0.5, vz=0.1, x0=0.0, y0=-4.0, z0=-3.0, P=100,
                 index=ptr, index_bytes=index_bytes, rz=1, ry=2, rx=3, radius=1.6, nsample=4, grp_row=ptr, grp_off=ptr, moments=ptr, ws=ptr,
                 ws_bytes=qbytes)
        a.update(change)
        _native.call("pdm_roi_grid_query", 0, *a.values())
    for change, text in ((dict(rois=None), 'null pointer'), (dict(index=None), 'null pointer'), (dict(grp_row=None), 'null pointer'),
                         (dict(grp_off=None), 'null pointer'), (dict(moments=None), 'null pointer'), (dict(ws=None), 'null pointer'),
                         (dict(ws_bytes=qbytes - 1), 'workspace too small'), (dict(index_bytes=index_bytes - 1), 'site index too small'),
                         (dict(B=32, D=41, H=160000, W=140800), '2\\^35 cells'), (dict(n=1 << 20), 'exceed 2\\^22'),
                         (dict(rz=5), 'at most 9 x 9 x 9'), (dict(rx=-1), 'at most 9 x 9 x 9'), (dict(nsample=33), 'nsample'),
                         (dict(nsample=0), 'nsample'), (dict(G=9), 'grid size'), (dict(G=0), 'grid size'), (dict(roi_stride=6), 'bad size'),
                         (dict(vz=0.0), 'voxel size'), (dict(stride=0), 'stride'), (dict(radius=-1.0), 'radius'),
                         (dict(moments=off4), '8-byte aligned'), (dict(ws=off4), '8-byte aligned'), (dict(index=off4), '8-byte aligned')):
        with pytest.raises(err, match=text):
            query(**change)

    def train(**change):
        a = dict(M=M, nsample=4, P=100, C1=16, grp_row=ptr, grp_off=ptr, feat=ptr, wp=ptr, scale_p=ptr, shift_p=ptr, pooled=ptr, arg=ptr)
        a.update(change)
        _native.call("pdm_roi_grid_pool_train", 0, *a.values())
    for change, text in ((dict(grp_row=None), 'null pointer'), (dict(grp_off=None), 'null pointer'), (dict(feat=None), 'null pointer'),
                         (dict(shift_p=None), 'null pointer'), (dict(pooled=None), 'null pointer'), (dict(arg=None), 'null pointer'),
                         (dict(C1=24), 'pooled channels'), (dict(C1=128), 'pooled channels'), (dict(nsample=33), 'nsample'),
                         (dict(nsample=0), 'nsample'), (dict(M=-1), 'bad size'), (dict(P=-1), 'bad size'), (dict(M=(1 << 22) + 1), 'exceed 2\\^22')):
        with pytest.raises(err, match=text):
            train(**change)
    train(M=0)      # nothing to do: no launch, no error

    gbytes = lib.pdm_roi_grid_pool_grad_workspace_bytes(M, 100, 16)
    assert gbytes >= 100 * 16 * 8 and lib.pdm_roi_grid_pool_grad_workspace_bytes((1 << 22) + 1, 100, 16) == 0
    assert lib.pdm_roi_grid_pool_grad_workspace_bytes(M, 100, 24) == 0 and lib.pdm_roi_grid_pool_grad_chunk_points(M, 24) == 0
    # the partition is a function of (M, C1) alone: 256 / C1 grid points while that gives at most 1024 partials, multiples beyond
    assert [lib.pdm_roi_grid_pool_grad_chunk_points(M, c) for c in (16, 32, 64)] == [16, 8, 4]
    assert lib.pdm_roi_grid_pool_grad_chunk_points(1 << 22, 32) == 4096 and lib.pdm_roi_grid_pool_grad_chunk_points(8 * 1024 + 1, 32) == 16

    def grad(**change):
        a = dict(M=M, nsample=4, P=100, C1=16, gpool=ptr, arg=ptr, grp_row=ptr, grp_off=ptr, wp=ptr, scale_p=ptr, dfeat=ptr, dwp=ptr, dscale=ptr,
                 dshift=ptr, ws=ptr, ws_bytes=gbytes)
        a.update(change)
        _native.call("pdm_roi_grid_pool_grad", 0, *a.values())
    for change, text in ((dict(gpool=None), 'null pointer'), (dict(arg=None), 'null pointer'), (dict(grp_row=None), 'null pointer'),
                         (dict(scale_p=None), 'null pointer'), (dict(dfeat=None), 'null pointer'), (dict(dwp=None), 'null pointer'),
                         (dict(dshift=None), 'null pointer'), (dict(ws=None), 'null pointer'), (dict(ws_bytes=gbytes - 1), 'workspace too small'),
                         (dict(ws=off4), '8-byte aligned'), (dict(C1=48), 'pooled channels'), (dict(nsample=40), 'nsample'),
                         (dict(M=(1 << 22) + 1), 'exceed 2\\^22'), (dict(P=-2), 'bad size')):
        with pytest.raises(err, match=text):
            grad(**change)


def test_predicates_accept_and_refuse_the_same_set():
    from pdm_ssd_amd.pointnet2_stack.voxel_pool_modules import NeighborVoxelSAModuleMSG as M
    ok = dict(query_ranges=[[4, 4, 4]], radii=[0.8], nsamples=[16], mlps=[[32, 32, 32]])
    assert M(**ok).fused_train_supported(6) and not M(**ok).fused_supported(6)              # training mode
    assert M(**ok).eval().fused_supported(6) and not M(**ok).eval().fused_train_supported(6)
    assert not M(**ok).fused_train_supported(9) and not M(**ok).fused_train_supported(0)
    for change in (dict(pool_method='avg_pool'), dict(mlps=[[32, 24, 32]]), dict(mlps=[[32, 32, 128]]), dict(mlps=[[12, 32, 32]]),
                   dict(query_ranges=[[5, 4, 4]]), dict(nsamples=[33])):
        assert not M(**dict(ok, **change)).fused_train_supported(6), change
        assert not M(**dict(ok, **change)).eval().fused_supported(6), change


def test_cpu_refusal_keeps_its_message_and_a_head_without_the_sampler_says_so():
    from pdm_ssd_amd.config import cfg_from_dict
    from pdm_ssd_amd.roi_heads import VoxelRCNNHead
    head = VoxelRCNNHead(backbone_channels=dict(case.BACKBONE_CHANNELS), model_cfg=cfg_from_dict(case.head_cfg(2)),
                         point_cloud_range=case.RANGE, voxel_size=case.VOXEL, num_class=1).train()
    assert not head.has_training_half
    with pytest.raises(NotImplementedError, match='off the device the RoI-grid pooling has no gradient yet'):
        head({'batch_size': 1, 'rois': torch.zeros((1, 2, 7))})
    with pytest.raises(NotImplementedError, match='ROI_PER_IMAGE'):
        head._require_training_half('VoxelRCNNHead')


def test_train_cfg_builds_a_head_with_the_training_half():
    from pdm_ssd_amd import detector_config as dc
    model = dc.build_voxel_rcnn(dc.VOXEL_RCNN_TRAIN_CFG)
    head = model.roi_head
    assert head.has_training_half and not dc.build_voxel_rcnn().roi_head.has_training_half
    t = dc.VOXEL_RCNN_TRAIN_CFG['ROI_HEAD']['TARGET_CONFIG']
    assert (t['ROI_PER_IMAGE'], t['FG_RATIO'], t['CLS_SCORE_TYPE'], t['CLS_FG_THRESH'], t['CLS_BG_THRESH'], t['CLS_BG_THRESH_LO'], t['HARD_BG_RATIO'],
            t['REG_FG_THRESH'], t['SAMPLE_ROI_BY_EACH_CLASS']) == (128, 0.5, 'roi_iou', 0.75, 0.25, 0.1, 0.8, 0.55, True)
    assert 'ROI_PER_IMAGE' not in dc.VOXEL_RCNN_CFG['ROI_HEAD']['TARGET_CONFIG'] and 'LOSS_CONFIG' not in dc.VOXEL_RCNN_CFG['ROI_HEAD']
    assert {k: list(v.shape) for k, v in model.state_dict().items()} == {k: list(v.shape) for k, v in dc.build_voxel_rcnn().state_dict().items()}
    assert all(l.fused_train_supported(6) for l in head.train().roi_grid_pool_layers)

"""The sparse pillar family on the device: DynamicPillarVFESimple2D, PillarBackBone8x, PillarRes18BackBone8x and
BaseBEVBackboneV1 against the reference's own modules run over a dense-convolution stub of spconv (tests/golden/ref_pillarnet.npz,
gen_pillarnet_fixtures.py), a training step of the backbones against the torch formulation over the same rulebooks, and the PillarNet
detector in eval mode and through one training step.

Exact: pillar_coords; every level's indices and shapes; two runs of everything; batched post-processing against the per-sample loop.
Bounded: features within 1e-4 absolute, the project's parity contract for fp32 features (the generator found float32 and float64
within 2.5e-5 of each other, a quarter of it); the training step within 4 e, e the float32 torch formulation's own deviation from
float64 (test_sparse_conv_grad_gpu.py's backbone-gradient convention).
"""
import contextlib
import copy
import json
import os

import numpy as np
import pytest
import torch

import pillarnet_reference as pnr
from pdm_ssd_amd import pillar_ops, sparse_conv_ops

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
LEVELS = ('x_conv1', 'x_conv2', 'x_conv3', 'x_conv4')


@pytest.fixture(scope="module")
def ref():
    z = np.load(os.path.join(GOLDEN, "ref_pillarnet.npz"))
    return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def manifest():
    with open(os.path.join(GOLDEN, "ref_pillarnet_manifest.json")) as f:
        return json.load(f)


@contextlib.contextmanager
def deterministic_convolutions():
    """torch's own convolutions (conv5, BaseBEVBackboneV1, the head) pick reproducible algorithms: without the flag two calls on
    identical input differ in the last bits on this device, whatever stands in front of them (test_pv_rcnn_pp_gpu.py's helper)"""
    before = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    try:
        yield
    finally:
        torch.backends.cudnn.deterministic = before


# ---- the encoder ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", list(pnr.VFE_CONFIGS))
def test_vfe_matches_the_reference(ref, manifest, dev, tag):
    """'a' and 'b' run the fused single-layer kernel with the permuted weight (zeros on the cluster columns), 'c' (two layers, no
    norm) the feature kernel, one index_select and segment_max; one host read each"""
    from pdm_ssd_amd import vfe
    g = pnr.PN
    net = vfe.__all__['DynamicPillarVFESimple2D'](model_cfg=pnr.VFE_CONFIGS[tag], num_point_features=4, voxel_size=g['voxel'],
                                                  grid_size=g['grid'], point_cloud_range=g['range'])
    assert {k: list(v.shape) for k, v in net.state_dict().items()} == manifest[f'DynamicPillarVFESimple2D.{tag}']
    fill = manifest[f'DynamicPillarVFESimple2D.{tag}.fill']
    assert abs(pnr.fill_vfe(net, fill['seed']) - fill['checksum']) <= 1e-9 * fill['checksum'], 'not the generator\'s parameters'
    net = net.to(dev).eval()
    pts = torch.from_numpy(ref['points']).to(dev)

    def forward():
        with torch.no_grad():
            return net({'points': pts, 'batch_size': g['B']})
    before = pillar_ops.HOST_READS
    bd = forward()
    assert pillar_ops.HOST_READS - before == 1
    assert bd['pillar_coords'].dtype == torch.int32 and np.array_equal(bd['pillar_coords'].cpu().numpy(), ref['pillar_coords'])
    err = float(np.abs(bd['pillar_features'].cpu().numpy() - ref[f'vfe.{tag}.features']).max())
    print(tag, 'pillars', len(ref['pillar_coords']), 'max err', err)
    assert err <= 1e-4 and net.get_output_feature_dim() == 32
    assert torch.equal(forward()['pillar_features'], bd['pillar_features'])


# ---- the backbones ----------------------------------------------------------------------------------------------------------------
def built(name, manifest, dev):
    from pdm_ssd_amd import backbones_2d, backbones_3d
    net = backbones_3d.__all__[name](model_cfg={}, input_channels=32, grid_size=pnr.PN['grid'])
    assert {k: list(v.shape) for k, v in net.state_dict().items()} == manifest[name]
    fill = manifest[f'{name}.fill']
    assert abs(pnr.fill_pillarnet(net, fill['seed'], fill['gain']) - fill['checksum']) <= 1e-9 * fill['checksum'], 'not the generator\'s parameters'
    fill = manifest['BaseBEVBackboneV1.fill']
    bev = backbones_2d.__all__['BaseBEVBackboneV1'](model_cfg=fill['cfg'])
    assert {k: list(v.shape) for k, v in bev.state_dict().items()} == manifest['BaseBEVBackboneV1']
    assert abs(pnr.fill_pillarnet(bev, fill['seed'], fill['gain']) - fill['checksum']) <= 1e-9 * fill['checksum']
    return net.to(dev), bev.to(dev)


@pytest.mark.parametrize("name", ['PillarBackBone8x', 'PillarRes18BackBone8x'])
def test_backbone_matches_the_reference_over_the_dense_convolution_stub(ref, manifest, dev, name):
    """Every sparse level's sites exactly and in the fixture's order (ascending key), its features, the dense x_conv5 and
    BaseBEVBackboneV1's spatial_features_2d within 1e-4; three host reads (the strided rulebooks); a second forward gives the same bits"""
    net, bev = built(name, manifest, dev)
    net, bev = net.eval(), bev.eval()

    def forward():
        bd = {'pillar_features': torch.from_numpy(ref['vfe.a.features']).to(dev), 'pillar_coords': torch.from_numpy(ref['pillar_coords']).to(dev),
              'batch_size': pnr.PN['B']}
        with torch.no_grad(), deterministic_convolutions():
            return bev(net(bd))
    before = sparse_conv_ops.HOST_READS
    bd = forward()
    assert sparse_conv_ops.HOST_READS - before == 3
    levels = dict(bd['multi_scale_2d_features'], x_conv4=bd['encoded_spconv_tensor'])
    for lv in LEVELS:
        t = levels[lv]
        assert list(t.spatial_shape) == ref[f'{name}.{lv}.shape'].tolist(), lv
        assert tuple(t.indices.shape)[1] == 3 and np.array_equal(t.indices.cpu().numpy(), ref[f'{name}.{lv}.indices']), lv
        err = float(np.abs(t.features.cpu().numpy() - ref[f'{name}.{lv}.features']).max())
        print(name, lv, 'sites', len(t.indices), 'max err', err)
        assert err <= 1e-4, lv
    dense4 = bd['multi_scale_2d_features']['x_conv4']
    assert torch.is_tensor(dense4) and torch.equal(dense4, bd['encoded_spconv_tensor'].dense()) and tuple(dense4.shape) == (3, 256, 6, 4)
    assert bd['multi_scale_2d_strides'] == {'x_conv1': 1, 'x_conv2': 2, 'x_conv3': 4, 'x_conv4': 8, 'x_conv5': 16}
    for key, got in (('x_conv5', bd['multi_scale_2d_features']['x_conv5']), ('spatial_features_2d', bd['spatial_features_2d'])):
        assert tuple(got.shape) == ref[f'{name}.{key}'].shape
        err = float(np.abs(got.cpu().numpy() - ref[f'{name}.{key}']).max())
        print(name, key, 'max err', err)
        assert err <= 1e-4, key
    again = forward()
    for lv in LEVELS[:3]:
        assert torch.equal(again['multi_scale_2d_features'][lv].features, bd['multi_scale_2d_features'][lv].features), lv
    assert torch.equal(again['encoded_spconv_tensor'].features, bd['encoded_spconv_tensor'].features)
    assert torch.equal(again['multi_scale_2d_features']['x_conv4'], dense4)
    assert torch.equal(again['multi_scale_2d_features']['x_conv5'], bd['multi_scale_2d_features']['x_conv5'])
    assert torch.equal(again['spatial_features_2d'], bd['spatial_features_2d'])


def test_backbone_of_no_pillar(manifest, dev):
    net, bev = built('PillarBackBone8x', manifest, dev)
    bd = {'pillar_features': torch.zeros((0, 32), device=dev), 'pillar_coords': torch.zeros((0, 3), dtype=torch.int32, device=dev), 'batch_size': 2}
    with torch.no_grad():
        bd = bev.eval()(net.eval()(bd))
    assert bd['encoded_spconv_tensor'].features.shape == (0, 256) and bd['encoded_spconv_tensor'].indices.shape == (0, 3)
    dense = bd['multi_scale_2d_features']['x_conv4']
    assert dense.shape == (2, 256, 6, 4) and float(dense.abs().max()) == 0.0
    assert bd['spatial_features_2d'].shape == (2, 256, 6, 4) and torch.isfinite(bd['spatial_features_2d']).all()


@pytest.mark.parametrize("name", ['PillarBackBone8x', 'PillarRes18BackBone8x'])
def test_backbone_training_step_equals_the_torch_formulation(ref, manifest, dev, name):
    """A training step on the fixture (271 / 180 / 87 / 34 rows per level), loss = mean(x_conv4 proj4) + mean(x_conv5 proj5): every
    parameter's gradient, every running statistic, x_conv4 and x_conv5 against the torch formulation over the same device rulebooks
    in float64 (per offset index_select -> mm -> index_add_, BatchNorm1d, ReLU; conv5 as it is).  The tolerance is measured, by
    test_sparse_conv_grad_gpu.py's convention: the same formulation runs on the CPU in float32 as well, e = max |f32 - f64| /
    max |f64| per tensor, and the bound is 4 e max |f64|: ours is another fp32 order of the same sums; the factor covers the different
    order and BatchNorm's amplification.  Three host reads in the forward, none in backward; every gradient finite.  (The residual
    blocks' convolution biases sit in front of a training BatchNorm: their gradient is rounding noise on both sides and e is large.)"""
    net, _ = built(name, manifest, dev)
    net = net.train()
    start = copy.deepcopy(net)
    feats, coords = ref['vfe.a.features'], ref['pillar_coords']
    before = sparse_conv_ops.HOST_READS
    bd = net({'pillar_features': torch.from_numpy(feats).to(dev), 'pillar_coords': torch.from_numpy(coords).to(dev), 'batch_size': pnr.PN['B']})
    assert sparse_conv_ops.HOST_READS - before == 3
    x4, x5 = bd['multi_scale_2d_features']['x_conv4'], bd['multi_scale_2d_features']['x_conv5']
    rows = [len(bd['multi_scale_2d_features'][k].indices) for k in LEVELS[:3]] + [len(bd['encoded_spconv_tensor'].indices)]
    assert rows == [271, 180, 87, 34]
    rng = np.random.default_rng(13)
    proj4, proj5 = (rng.uniform(-1, 1, tuple(t.shape)).astype(np.float32) for t in (x4, x5))
    before = sparse_conv_ops.HOST_READS
    ((x4 * torch.from_numpy(proj4).to(dev)).sum() / x4.numel() + (x5 * torch.from_numpy(proj5).to(dev)).sum() / x5.numel()).backward()
    assert sparse_conv_ops.HOST_READS == before
    ours = {'x_conv4': x4.detach().cpu().numpy(), 'x_conv5': x5.detach().cpu().numpy()}
    for n, p in net.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), n
        ours['grad.' + n] = p.grad.cpu().numpy()
    assert bool(net.conv1[0][0].weight.grad.any() if name == 'PillarBackBone8x' else net.conv1[0].conv1.weight.grad.any())
    for n, b in net.named_buffers():
        if n.endswith('running_mean') or n.endswith('running_var'):
            ours['stat.' + n] = b.cpu().numpy()
    enc = bd['encoded_spconv_tensor']
    books = {k: (rb.out_indices.cpu(), rb.nbr.cpu()) for k, rb in enc.indice_dict.items() if isinstance(rb, sparse_conv_ops.Rulebook)}
    books['out_shape'] = tuple(enc.spatial_shape)
    r64 = pnr.backbone2d_step(start, feats, coords, pnr.PN['B'], books, proj4, proj5, torch.float64)
    r32 = pnr.backbone2d_step(start, feats, coords, pnr.PN['B'], books, proj4, proj5, torch.float32)
    assert set(ours) | {'loss'} == set(r64)
    worst, failed = {}, []
    for key, got in ours.items():
        scale = np.abs(r64[key]).max()
        e = np.abs(r32[key] - r64[key]).max() / scale
        mine = np.abs(got - r64[key]).max() / scale
        kind = key.split('.')[0] + ('.' + key.split('.')[-1] if '.' in key else '')
        w = worst.setdefault(kind, [0.0, 0.0, 0.0])
        w[0], w[1], w[2] = max(w[0], e), max(w[1], mine), max(w[2], mine / e if e > 0 else np.inf if mine > 0 else 0.0)
        if not mine <= 4 * e:
            failed.append((key, e, mine))
    for kind, (e, mine, ratio) in sorted(worst.items()):
        print(f'{name} {kind}: largest e {e:.3g}, largest ours {mine:.3g}, largest ours / e {ratio:.3g}')
    assert not failed, failed


# ---- the detector -----------------------------------------------------------------------------------------------------------------
SMALL = dict(range=[0, -8, -3, 25.6, 8, 1], grid=[512, 320, 1])      # the training step's grid: 0.05 m pillars, a 64 x 40 map at stride 8


def scene(dev, lo=(0, -40, -3), hi=(70.4, 40, 1)):
    """a small synthetic batch: clusters around boxes of the three classes (all inside SMALL's range) and a uniform background"""
    rng = np.random.default_rng(21)
    gt = np.zeros((2, 3, 8), dtype=np.float32)
    gt[0, 0] = [12.0, 3.0, -1.0, 3.9, 1.6, 1.5, 0.3, 1]
    gt[0, 1] = [22.0, -6.0, -0.8, 0.8, 0.6, 1.7, -1.2, 2]
    gt[1, 0] = [20.0, 6.0, -0.9, 1.7, 0.6, 1.7, 2.1, 3]
    gt[1, 1] = [8.0, -2.0, -1.0, 4.1, 1.7, 1.5, 1.0, 1]
    rows = []
    for b in range(2):
        for box in gt[b]:
            if box[7] > 0:
                rows.append(np.concatenate([np.full((400, 1), b), box[:3] + rng.normal(0, 0.8, (400, 3)), rng.uniform(0, 1, (400, 1))], 1))
        rows.append(np.concatenate([np.full((600, 1), b), rng.uniform(lo, hi, (600, 3)), rng.uniform(0, 1, (600, 1))], 1))
    pts = np.concatenate(rows).astype(np.float32)
    return {'batch_size': 2, 'points': torch.from_numpy(pts[rng.permutation(len(pts))]).to(dev), 'gt_boxes': torch.from_numpy(gt).to(dev)}


def reads():
    return pillar_ops.HOST_READS + sparse_conv_ops.HOST_READS


def test_pillarnet_eval_forward(dev):
    """pred_dicts with the contract's keys, two runs bit for bit, batched post-processing equal to the per-sample loop; from the points
    to the head's input the step reads the host four times: the pillar path's one and one per strided sparse convolution"""
    from pdm_ssd_amd import detector_config as dc
    torch.manual_seed(5)
    model = dc.build_pillarnet().to(dev).eval()
    assert [type(m).__name__ for m in model.module_list] == ['DynamicPillarVFESimple2D', 'PillarBackBone8x', 'BaseBEVBackboneV1', 'CenterHead']
    batch = scene(dev)
    seen = {}
    model.backbone_2d.register_forward_hook(lambda m, a, out: seen.update(reads=reads(), sf=out['spatial_features_2d']))
    before = reads()
    with torch.no_grad(), deterministic_convolutions():
        pred, recall = model(dict(batch))
    assert seen['reads'] - before == 4 and tuple(seen['sf'].shape) == (2, 256, 200, 176)
    assert len(pred) == 2 and 'gt' in recall
    for p in pred:
        assert set(p) >= {'pred_boxes', 'pred_scores', 'pred_labels'} and p['pred_boxes'].shape[1] == 7
        assert torch.isfinite(p['pred_boxes']).all() and torch.isfinite(p['pred_scores']).all()
        assert len(p['pred_boxes']) == len(p['pred_scores']) == len(p['pred_labels'])
    with torch.no_grad(), deterministic_convolutions():
        again, _ = model(dict(batch))
    for a, b in zip(pred, again):
        for k in ('pred_boxes', 'pred_scores', 'pred_labels'):
            assert torch.equal(a[k], b[k]), k
    cfg = copy.deepcopy(dc.PILLARNET_CFG)
    cfg['DENSE_HEAD']['POST_PROCESSING']['BATCHED'] = False
    loop = dc.build_pillarnet(cfg).to(dev).eval()
    loop.load_state_dict(model.state_dict())
    with torch.no_grad(), deterministic_convolutions():
        want, _ = loop(dict(batch))
    for a, b in zip(pred, want):
        for k in ('pred_boxes', 'pred_scores', 'pred_labels'):
            assert torch.equal(a[k], b[k]), k


def test_pillarnet_takes_a_training_step(dev):
    """forward, loss.backward() on SMALL's grid (the step's cost is the dense convolutions' first calls): the loss is finite, every
    parameter has a finite gradient, the first sparse convolution's and the encoder's are nonzero, and the training forward reads the
    host no more often than the eval forward (four times), backward never"""
    from pdm_ssd_amd import detector_config as dc
    torch.manual_seed(5)
    ds = dc.pillarnet_dataset(4, SMALL['range'], dc.PILLARNET_VOXEL_SIZE, SMALL['grid'])
    model = dc.build_pillarnet(dc.PILLARNET_TRAIN_CFG, dataset=ds).to(dev).train()
    assert model.backbone_3d.sparse_shape == [320, 512]
    batch = scene(dev, SMALL['range'][:3], SMALL['range'][3:])
    seen = {}
    model.backbone_2d.register_forward_hook(lambda m, a, out: seen.update(reads=reads()))
    before = reads()
    ret, tb, _ = model(dict(batch))
    assert seen['reads'] - before == 4
    before = reads()
    ret['loss'].backward()
    assert reads() == before
    assert torch.isfinite(ret['loss'])
    for n, p in model.named_parameters():
        if p.requires_grad:
            assert p.grad is not None and torch.isfinite(p.grad).all(), n
    assert bool(model.backbone_3d.conv1[0][0].weight.grad.any()) and bool(model.backbone_3d.conv4[1][0].weight.grad.any())
    assert bool(model.vfe.pfn_layers[0].linear.weight.grad.any())

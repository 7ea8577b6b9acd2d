"""Part-A2 on the device: PartA2FCHead's fused path (pdm_roiaware_pool_sparse -> conv_part / conv_rpn -> pdm_sparse_fc) against its
composed path (the reference's formulation on this tree's operators), UNetV2 and the point head's shapes and row order, and
build_part_a2() end to end on a small grid.

The head case: B = 2 samples of 6 rois over 1500 + 1100 points in boxes' neighbourhoods, 16 point features, POOL_SIZE 4, reduced
FC widths.  One point in ten has score exactly 0 (its part features are all zero: cells holding only such points are occupied
but inactive), and no score lies within 1e-4 of SEG_MASK_SCORE_THRESH, so the mask is the same on both paths.  Tolerance 1e-4 on
rcnn_cls / rcnn_reg / batch_box_preds, what tests/test_pv_rcnn_gpu.py holds the same quantities of PVRCNNHead to: the paths share
the pooled rows and the four convolutions bit for bit and differ in the summation order of the first FC only.
"""
import copy

import numpy as np
import pytest
import torch

import sparse_conv_reference as scr
from pdm_ssd_amd import detector_config as dc
from pdm_ssd_amd import sparse_conv_ops
from pdm_ssd_amd.config import cfg_from_dict
from pdm_ssd_amd.roi_heads import PartA2FCHead

pytestmark = pytest.mark.gpu
THRESH = 0.3


def head_cfg(**over):
    cfg = copy.deepcopy(dc.PART_A2_CFG['ROI_HEAD'])
    cfg.update(SHARED_FC=[64, 64], CLS_FC=[32], REG_FC=[32])
    cfg['ROI_AWARE_POOL'].update(POOL_SIZE=4, NUM_FEATURES=32, MAX_POINTS_PER_VOXEL=4)
    cfg.update(over)
    return cfg_from_dict(cfg)


def head_case(dev, far=False):
    rng = np.random.default_rng(3)
    centres = np.array([[8, 0, -1], [14, 3, -1], [20, -4, -0.8], [9, 1, -1], [30, 6, -1], [40, -10, -1]], dtype=np.float32)
    rois = np.zeros((2, 6, 7), dtype=np.float32)
    for b in range(2):
        rois[b, :, :3] = centres + rng.uniform(-0.3, 0.3, (6, 3))
        rois[b, :, 3:6] = [3.9, 1.6, 1.56]
        rois[b, :, 6] = rng.uniform(-1.5, 1.5, 6)
    pts = []
    for b, n in enumerate((1500, 1100)):
        c = centres[rng.integers(0, 5, n)]                       # (roi 5 of each sample stays empty)
        xyz = c + rng.normal(0, [1.5, 0.9, 0.5], (n, 3))
        pts.append(np.concatenate([np.full((n, 1), b), xyz], 1))
    coords = np.concatenate(pts).astype(np.float32)
    if far:
        coords[:, 1] += 500
    P = len(coords)
    scores = rng.uniform(0, 1, P).astype(np.float32)
    scores[np.abs(scores - THRESH) < 1e-3] = 0.5
    scores[rng.random(P) < 0.1] = 0
    assert (np.abs(scores - THRESH) > 1e-4).all()
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)      # noqa: E731
    return {'batch_size': 2, 'rois': t(rois), 'roi_labels': torch.ones((2, 6), dtype=torch.long, device=dev), 'point_coords': t(coords),
            'point_features': t(rng.standard_normal((P, 16))), 'point_part_offset': t(rng.uniform(0, 1, (P, 3))),
            'point_cls_scores': t(scores)}


def built_head(dev, **over):
    torch.manual_seed(0)
    head = PartA2FCHead(input_channels=16, model_cfg=head_cfg(**over), num_class=1)
    g = torch.Generator().manual_seed(1)
    for m in head.modules():                                     # statistics a trained norm would hold, not the identity
        if isinstance(m, torch.nn.BatchNorm1d):
            m.running_mean.copy_(torch.randn(m.num_features, generator=g) * 0.1)
            m.running_var.copy_(torch.rand(m.num_features, generator=g) + 0.5)
            m.weight.data.copy_(torch.rand(m.num_features, generator=g) + 0.5)
            m.bias.data.copy_(torch.randn(m.num_features, generator=g) * 0.1)
    return head.to(dev).eval()


@pytest.mark.parametrize("disable_part", [False, True])
def test_head_fused_path_against_its_composed_path(dev, disable_part):
    head = built_head(dev, DISABLE_PART=disable_part)
    bd = head_case(dev)
    before = sparse_conv_ops.HOST_READS
    with torch.no_grad():
        fused = head(dict(bd))
    assert head.last_path == 'fused' and fused['cls_preds_normalized'] is False
    assert sparse_conv_ops.HOST_READS == before + 1, 'the fused path reads the row count and nothing else'
    with torch.no_grad():
        again = head(dict(bd))
    assert all(torch.equal(fused[k], again[k]) for k in ('rcnn_cls', 'rcnn_reg', 'batch_box_preds')), 'two runs differ'
    head.pool_cfg['FUSED'] = False
    with torch.no_grad():
        composed = head(dict(bd))
    assert head.last_path == 'composed'
    worst = {k: float((fused[k] - composed[k]).abs().max()) for k in ('rcnn_cls', 'rcnn_reg', 'batch_box_preds', 'batch_cls_preds')}
    print('PartA2FCHead fused against composed, DISABLE_PART', disable_part, worst, 'scale', float(composed['rcnn_cls'].abs().max()))
    assert max(worst.values()) <= 1e-4
    assert fused['rcnn_cls'].shape == (12, 1) and fused['rcnn_reg'].shape == (12, 7) and fused['batch_box_preds'].shape == (2, 6, 7)
    assert float(fused['rcnn_cls'].std()) > 0, 'the rois see different features'


def test_head_takes_the_composed_path_below_three_active_cells_and_refuses_training(dev):
    head = built_head(dev)
    with torch.no_grad():
        out = head(dict(head_case(dev, far=True)))
    assert head.last_path == 'composed' and bool(torch.isfinite(out['rcnn_cls']).all()) and bool(torch.isfinite(out['batch_box_preds']).all())
    with pytest.raises(NotImplementedError):
        head.train()(dict(head_case(dev)))


def test_state_dict_keys_are_the_reference_modules(dev):
    head = built_head(dev)
    keys = list(head.state_dict())
    for prefix in ('conv_part.0.0.weight', 'conv_part.1.1.running_var', 'conv_rpn.0.0.weight', 'conv_rpn.1.0.weight', 'shared_fc_layer.0.weight',
                   'shared_fc_layer.1.running_mean', 'shared_fc_layer.4.weight', 'cls_layers.0.weight', 'cls_layers.4.bias', 'reg_layers.4.weight'):
        assert prefix in keys, prefix
    assert head.conv_part[0][0].indice_key == 'rcnn_subm1' and head.conv_part[1][0].indice_key == 'rcnn_subm1_1'
    assert head.conv_rpn[0][0].indice_key == 'rcnn_subm2' and head.conv_rpn[1][0].indice_key == 'rcnn_subm1_2'
    assert tuple(head.shared_fc_layer[0].weight.shape) == (64, 32 * 64, 1)


def small_cfg():
    cfg = copy.deepcopy(dc.PART_A2_CFG)
    cfg['ROI_HEAD']['NMS_CONFIG']['TEST'].update(NMS_POST_MAXSIZE=8, NMS_PRE_MAXSIZE=256)
    cfg['ROI_HEAD']['ROI_AWARE_POOL'].update(POOL_SIZE=4)
    cfg['POST_PROCESSING']['SCORE_THRESH'] = 0.0
    return cfg


def test_build_part_a2_runs_end_to_end(dev):
    """the D1 grid, 3000 synthetic points, 2 samples, 8 test rois, a 4 x 4 x 4 RoI grid: module order, the UNet's point rows (one
    per input voxel, in the voxels' order, at the voxel centres), finite results, labels in range, at least one box at
    SCORE_THRESH 0; training mode raises"""
    d = scr.D1
    torch.manual_seed(0)
    model = dc.build_part_a2(small_cfg(), dataset=dc.voxel_dataset(4, d['range'], d['voxel'], d['grid'])).to(dev).eval()
    assert [type(m).__name__ for m in model.module_list] == ['DynamicMeanVFE', 'UNetV2', 'HeightCompression', 'BaseBEVBackbone',
                                                             'AnchorHeadSingle', 'PointIntraPartOffsetHead', 'PartA2FCHead']
    rng = np.random.default_rng(1)
    lo, hi = np.array(d['range'][:3]) + 0.05, np.array(d['range'][3:]) - 0.05
    pts = np.concatenate([np.repeat(np.arange(2), 1500)[:, None], rng.uniform(lo, hi, (3000, 3)), rng.uniform(0, 1, (3000, 1))], 1).astype(np.float32)
    bd = {'batch_size': 2, 'points': torch.from_numpy(pts).to(dev)}
    seen = {}
    model.roi_head.register_forward_hook(lambda m, i, out: seen.update(out))
    with torch.no_grad():
        preds, _ = model(bd)
    P = seen['voxel_coords'].shape[0]
    assert seen['point_features'].shape == (P, 16) and seen['point_coords'].shape == (P, 4) and seen['point_part_offset'].shape == (P, 3)
    assert seen['point_cls_scores'].shape == (P,) and seen['encoded_spconv_tensor_stride'] == 8
    vc = seen['voxel_coords'].float()
    centre = (vc[:, [3, 2, 1]] + 0.5) * torch.tensor(d['voxel'], device=dev) + torch.tensor(d['range'][:3], device=dev)
    assert torch.equal(seen['point_coords'][:, 0], vc[:, 0]) and float((seen['point_coords'][:, 1:] - centre).abs().max()) < 1e-5
    assert seen['rois'].shape[:2] == (2, 8) and model.roi_head.last_path == 'fused'
    assert len(preds) == 2 and sum(len(p['pred_boxes']) for p in preds) >= 1
    for p in preds:
        assert bool(torch.isfinite(p['pred_boxes']).all()) and bool(torch.isfinite(p['pred_scores']).all())
        assert bool(((p['pred_labels'] >= 1) & (p['pred_labels'] <= 3)).all())
    with pytest.raises(NotImplementedError):
        model.train()(bd)


# ---- against the reference's own modules on the CPU (tests/golden/ref_part_a2.npz, gen_part_a2_fixtures.py) --------------------
import json  # noqa: E402
import os  # noqa: E402

import part_a2_reference as par  # noqa: E402
from pdm_ssd_amd.backbones_3d import UNetV2  # noqa: E402
from pdm_ssd_amd.dense_heads import PointIntraPartOffsetHead  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def ref():
    z = np.load(os.path.join(GOLDEN, "ref_part_a2.npz"))
    return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def manifest():
    with open(os.path.join(GOLDEN, "ref_part_a2_manifest.json")) as f:
        return json.load(f)


def load_state(module, ref, prefix):
    module.load_state_dict({k[len(prefix):]: torch.from_numpy(v) for k, v in ref.items() if k.startswith(prefix)})
    return module


def ref_modules(ref, dev):
    net = UNetV2(cfg_from_dict({'RETURN_ENCODED_TENSOR': True}), 4, list(scr.B1_GRID), par.GEO['voxel'], par.GEO['range'])
    checksum = scr.fill_backbone(net, par.UNET_SEED, par.UNET_GAIN)
    assert abs(checksum - float(ref['unet.checksum'])) <= 1e-6 * checksum, 'the seeded UNet parameters are the generator\'s'
    ph = load_state(PointIntraPartOffsetHead(1, 16, cfg_from_dict(copy.deepcopy(par.POINT_CFG))), ref, 'point_head.state.')
    head = load_state(PartA2FCHead(input_channels=16, model_cfg=cfg_from_dict(copy.deepcopy(par.ROI_CFG)), num_class=1), ref, 'roi_head.state.')
    return net.to(dev).eval(), ph.to(dev).eval(), head.to(dev).eval()


def test_state_dict_keys_equal_the_reference_manifest(ref, manifest, dev):
    net, ph, head = ref_modules(ref, 'cpu')
    for module, tag in ((net, 'UNetV2'), (ph, 'PointIntraPartOffsetHead'), (head, 'PartA2FCHead')):
        want = next(v for k, v in manifest.items() if k.startswith(tag + '('))
        assert {k: list(v.shape) for k, v in module.state_dict().items()} == want, tag
        assert list(module.state_dict()) == list(want), tag


def test_modules_match_the_reference(ref, dev):
    """UNetV2's point features and encoded tensor, the point head's scores and part offsets, and the RoI head's outputs on both
    of its paths within 1e-4 of the reference's own modules on the CPU (the tolerance tests/test_pv_rcnn_gpu.py and
    tests/test_sparse_conv_gpu.py hold the same kinds of quantity to); the pooled rows are the reference's active cells row for row."""
    net, ph, head = ref_modules(ref, dev)
    coords, feats = scr.b1_voxels(4)
    with torch.no_grad():
        bd = ph(net({'voxel_features': torch.from_numpy(feats).to(dev), 'voxel_coords': torch.from_numpy(coords).to(dev), 'batch_size': scr.B1_B}))
    enc = bd['encoded_spconv_tensor']
    assert np.array_equal(enc.indices.cpu().numpy(), ref['unet.encoded.indices']) and list(enc.spatial_shape) == ref['unet.encoded.shape'].tolist()
    worst = {'encoded': float(np.abs(enc.features.cpu().numpy() - ref['unet.encoded.features']).max()),
             'point_features': float(np.abs(bd['point_features'].cpu().numpy() - ref['unet.point_features']).max()),
             'point_coords': float(np.abs(bd['point_coords'].cpu().numpy() - ref['unet.point_coords']).max()),
             'point_cls_scores': float(np.abs(bd['point_cls_scores'].cpu().numpy() - ref['point_head.point_cls_scores']).max()),
             'point_part_offset': float(np.abs(bd['point_part_offset'].cpu().numpy() - ref['point_head.point_part_offset']).max())}
    print('UNetV2 + point head against the reference:', worst)
    assert max(worst.values()) <= 1e-4
    # the RoI head on the reference's own point outputs (so that its inputs are the fixture's bit for bit)
    t = lambda k: torch.from_numpy(ref[k]).to(dev)      # noqa: E731
    hb = {'batch_size': scr.B1_B, 'rois': t('roi_head.rois'), 'roi_labels': torch.ones((3, 5), dtype=torch.long, device=dev),
          'point_coords': t('unet.point_coords'), 'point_features': t('unet.point_features'),
          'point_cls_scores': t('point_head.point_cls_scores'), 'point_part_offset': t('point_head.point_part_offset')}
    assert float(np.abs(ref['point_head.point_cls_scores'] - par.ROI_CFG['SEG_MASK_SCORE_THRESH']).min()) > 1e-4
    from pdm_ssd_amd.pv_rcnn_ops import sample_counts
    from pdm_ssd_amd.roiaware_pool3d.roiaware_pool3d_utils import roiaware_pool_sparse
    batch_idx, xyz, part, rpn = head._point_inputs(hb)
    rows = roiaware_pool_sparse(hb['rois'], xyz, sample_counts(batch_idx, 3), part, rpn, 3, 4)[0]
    assert np.array_equal(rows.cpu().numpy(), ref['roi_head.coords'])
    for fused in (True, False):
        head.pool_cfg['FUSED'] = fused
        with torch.no_grad():
            out = head(dict(hb))
        assert head.last_path == ('fused' if fused else 'composed')
        worst = {k: float(np.abs(out[k].cpu().numpy() - ref[f'roi_head.{k}']).max()) for k in ('batch_cls_preds', 'batch_box_preds')}
        print('PartA2FCHead', head.last_path, 'against the reference:', worst)
        assert max(worst.values()) <= 1e-4

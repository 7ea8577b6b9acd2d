"""SECOND-IoU off the device: the float64 restatement of the crop and its bound against the reference's own SECONDHead on the CPU
(tests/golden/ref_second_iou.npz, gen_second_iou_fixtures.py), SECONDHead's keys, CPU path and losses against the same fixture,
SECONDNetIoU's score rules on hand-made inputs, the argument checks of the two entry points (made before any launch, so they run
without a GPU), the packed weight's layout, the configuration and the registries.
"""
import copy
import json
import math
import os

import numpy as np
import pytest
import torch

import bev_crop_reference as bcr
from pdm_ssd_amd import _native, bev_roi_ops, detector_config as dc, detectors, roi_heads
from pdm_ssd_amd.config import cfg_from_dict
from pdm_ssd_amd.detectors.second_net_iou import SECONDNetIoU
from pdm_ssd_amd.roi_heads import SECONDHead
from pdm_ssd_amd.utils import loss_utils

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
H, W = bcr.CASES['small']
HEAD_CFG = {'CLASS_AGNOSTIC': True, 'SHARED_FC': [32, 32], 'IOU_FC': [32, 32], 'DP_RATIO': 0.3,
            'ROI_GRID_POOL': {'GRID_SIZE': 7, 'IN_CHANNEL': 16, 'DOWNSAMPLE_RATIO': bcr.RATIO},
            'TARGET_CONFIG': {'BOX_CODER': 'ResidualCoder'},
            'NMS_CONFIG': {'TEST': {'NMS_TYPE': 'nms_gpu', 'MULTI_CLASSES_NMS': False, 'NMS_PRE_MAXSIZE': 64, 'NMS_POST_MAXSIZE': 6,
                                    'NMS_THRESH': 0.7}},
            'LOSS_CONFIG': {'IOU_LOSS': 'BinaryCrossEntropy', 'LOSS_WEIGHTS': {'rcnn_iou_weight': 1.5, 'code_weights': [1.0] * 7}}}


@pytest.fixture(scope="module")
def ref():
    z = np.load(os.path.join(GOLDEN, "ref_second_iou.npz"))
    return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def manifest():
    with open(os.path.join(GOLDEN, "ref_second_iou_manifest.json")) as f:
        return json.load(f)


def built_head(**over):
    cfg = copy.deepcopy(HEAD_CFG)
    cfg.update(over)
    return SECONDHead(input_channels=16, model_cfg=cfg_from_dict(cfg), num_class=1, point_cloud_range=bcr.pc_range(H, W), voxel_size=bcr.VOXEL)


def fixture_head(ref):
    head = built_head()
    head.load_state_dict({k[len('state.'):]: torch.from_numpy(v) for k, v in ref.items() if k.startswith('state.')})
    return head.eval()


def test_delta_is_four_times_what_the_reference_deviates_from_float64(ref):
    units = {k: float(v) for k, v in ref.items() if k.startswith('delta.units.') and k != 'delta.units.max'}
    assert len(units) == 16 and max(units.values()) == float(ref['delta.units.max'])
    assert float(ref['delta.units.max']) <= bcr.MEASURED_UNITS < float(ref['delta.units.max']) + 0.1
    assert bcr.DELTA_UNITS == 4 * bcr.MEASURED_UNITS


def test_float64_restatement_and_bound_against_the_reference_head(ref):
    """the reference's own roi_grid_pool output lies within the bound built from float64 (the bound is never tighter than the
    reference is to itself) and no element is exempt; wholly outside rois are exactly 0; the transposed and the swapped sampling
    leave the bound"""
    rois, feat, r = ref['rois'], ref['spatial_features_2d'], bcr.pc_range(H, W)
    want, T = bcr.crop64(rois, feat, r[0], r[1], bcr.CELL, bcr.CELL, 7)
    bound = bcr.crop_bound(feat, rois.shape[1], T)
    err = np.abs(ref['pooled'].astype(np.float64) - want)
    print('reference fp32 against float64: max err / bound', float((err / np.maximum(bound, 1e-300)).max()), 'max err', float(err.max()))
    assert ref['pooled'].shape == (12, 16, 7, 7) and (err <= bound).all()
    _, outside = bcr.make_rois(H, W, 2, 6, 7, seed=5)
    assert np.array_equal(bcr.make_rois(H, W, 2, 6, 7, seed=5)[0], rois) and outside.any()
    assert (ref['pooled'][outside.reshape(-1)] == 0).all() and (want[outside.reshape(-1)] == 0).all()
    for wrong in ({'transpose_ij': True}, {'swap_xy': True}):
        assert (np.abs(bcr.crop64(rois, feat, r[0], r[1], bcr.CELL, bcr.CELL, 7, **wrong)[0] - want) > bound).any(), wrong


def test_torch_formulation_is_within_the_bound(ref):
    rois, feat, r = ref['rois'], ref['spatial_features_2d'], bcr.pc_range(H, W)
    want, T = bcr.crop64(rois, feat, r[0], r[1], bcr.CELL, bcr.CELL, 7)
    got = bev_roi_ops.bev_roi_crop(torch.from_numpy(rois), torch.from_numpy(feat), r, bcr.VOXEL, bcr.RATIO, 7)
    assert got.shape == (12, 16, 7, 7) and (np.abs(got.numpy().astype(np.float64) - want) <= bcr.crop_bound(feat, 6, T)).all()
    out = torch.full((12, 16 * 49 + 3), 7.0)
    assert bev_roi_ops.bev_roi_crop(torch.from_numpy(rois), torch.from_numpy(feat), r, bcr.VOXEL, bcr.RATIO, 7, out=out) is out
    assert torch.equal(out[:, :784], got.view(12, -1)) and bool((out[:, 784:] == 7).all())


@pytest.mark.parametrize("drop", [0.3, 0])
def test_state_dict_keys_equal_the_reference_manifest(manifest, drop):
    want = manifest[f'SECONDHead(IN_CHANNEL=16,GRID_SIZE=7,SHARED_FC=[32,32],IOU_FC=[32,32],DP_RATIO={drop})']
    head = built_head(DP_RATIO=drop)
    assert {k: list(v.shape) for k, v in head.state_dict().items()} == want and list(head.state_dict()) == list(want)
    assert ('shared_fc_layer.5.weight' in want) == (drop > 0) and ('shared_fc_layer.3.weight' in want) == (drop == 0)


def test_cpu_path_matches_the_reference_head(ref):
    head = fixture_head(ref)
    bd = {'batch_size': 2, 'rois': torch.from_numpy(ref['rois']), 'roi_labels': torch.ones((2, 6), dtype=torch.long),
          'spatial_features_2d': torch.from_numpy(ref['spatial_features_2d']), 'dataset_cfg': 'ignored'}
    with torch.no_grad():
        out = head(bd)
    assert head.last_path == 'torch' and out['cls_preds_normalized'] is False and out['batch_box_preds'] is out['rois']
    got, want = out['batch_cls_preds'].numpy().reshape(12, 1), ref['rcnn_iou']
    assert out['batch_cls_preds'].shape == (2, 6, 1)
    print('rcnn_iou on the CPU path against the reference: max |err|', float(np.abs(got - want).max()), 'scale', float(np.abs(want).max()))
    assert np.abs(got - want).max() <= 1e-5 * np.abs(want).max()


@pytest.mark.parametrize("kind", ['BinaryCrossEntropy', 'L2', 'smoothL1', 'focalbce'])
def test_iou_losses_match_the_reference(ref, kind):
    head = built_head(LOSS_CONFIG={'IOU_LOSS': kind, 'LOSS_WEIGHTS': {'rcnn_iou_weight': float(ref['loss.weight']), 'code_weights': [1.0] * 7}},
                      TARGET_CONFIG={'BOX_CODER': 'ResidualCoder', 'ROI_PER_IMAGE': 6, 'FG_RATIO': 0.5, 'CLS_SCORE_TYPE': 'roi_iou',
                                     'CLS_FG_THRESH': 0.75, 'CLS_BG_THRESH': 0.25, 'CLS_BG_THRESH_LO': 0.1, 'HARD_BG_RATIO': 0.8,
                                     'REG_FG_THRESH': 0.55})
    logits = torch.from_numpy(ref['loss.logits']).view(12, 1).requires_grad_()
    head.forward_ret_dict = {'rcnn_iou': logits, 'rcnn_cls_labels': torch.from_numpy(ref['loss.labels'])}
    loss, tb = head.get_loss()
    assert abs(float(loss.detach()) - float(ref[f'loss.{kind}'])) <= 1e-5 * abs(float(ref[f'loss.{kind}']))
    assert set(tb) == {'rcnn_loss_iou', 'rcnn_loss'} and all(torch.is_tensor(v) and v.dim() == 0 and not v.requires_grad for v in tb.values())
    loss.backward()
    assert float(logits.grad[7].abs()) == 0 and float(logits.grad.abs().sum()) > 0, 'the row labelled -1 is ignored'
    with pytest.raises(NotImplementedError):
        built_head(LOSS_CONFIG={'IOU_LOSS': 'huber', 'LOSS_WEIGHTS': {'rcnn_iou_weight': 1.0}}).get_box_iou_layer_loss(head.forward_ret_dict)


def test_sigmoid_focal_cls_loss_is_the_unweighted_focal_loss():
    x, t = torch.linspace(-3, 3, 7), torch.tensor([0, 1, 0.5, 1, 0, 0.25, 1])
    want = loss_utils.SigmoidFocalClassificationLoss()(x, t, torch.ones(7))
    assert torch.equal(loss_utils.sigmoid_focal_cls_loss(x, t), want)


def test_a_head_without_the_samplers_settings_refuses_training(ref):
    head = fixture_head(ref).train()
    with pytest.raises(NotImplementedError):
        head({'batch_size': 2, 'rois': torch.from_numpy(ref['rois']), 'spatial_features_2d': torch.from_numpy(ref['spatial_features_2d'])})
    with pytest.raises(ValueError):
        SECONDHead(input_channels=16, model_cfg=cfg_from_dict(copy.deepcopy(HEAD_CFG)), num_class=1)


# ---- SECONDNetIoU's score rules ----------------------------------------------------------------------------------------------

NAMES = ['Car', 'Pedestrian', 'Cyclist']


def test_score_rules_on_hand_made_inputs():
    iou = torch.tensor([0.9, 0.2, 0.6, 0.4])
    cls = torch.tensor([0.1, 0.8, 0.5, 0.7])
    labels = torch.tensor([1, 3, 3, 1])                     # class 2 is absent: the reference would serve classes 1 and 2 only
    f = SECONDNetIoU.nms_scores
    assert f(iou, cls, labels, {}, NAMES) is iou and f(iou, cls, labels, {'SCORE_TYPE': 'iou'}, NAMES) is iou
    assert f(iou, cls, labels, {'SCORE_TYPE': 'cls'}, NAMES) is cls
    got = f(iou, cls, labels, {'SCORE_TYPE': 'weighted_iou_cls', 'SCORE_WEIGHTS': {'iou': 0.75, 'cls': 0.25}}, NAMES)
    assert torch.allclose(got, torch.tensor([0.7, 0.35, 0.575, 0.475]), atol=1e-7)
    by_class = {'SCORE_TYPE': 'score_by_class', 'SCORE_BY_CLASS': {'Car': 'iou', 'Pedestrian': 'iou', 'Cyclist': 'cls'}}
    assert torch.equal(f(iou, cls, labels, by_class, NAMES), torch.tensor([0.9, 0.8, 0.5, 0.4]))
    full = torch.tensor([1, 2, 3, 1])
    assert torch.equal(f(iou, cls, full, by_class, NAMES), torch.tensor([0.9, 0.2, 0.5, 0.4]))
    assert torch.equal(f(iou, cls, labels, cfg_from_dict(by_class), NAMES), torch.tensor([0.9, 0.8, 0.5, 0.4]))
    with pytest.raises(NotImplementedError, match='num_pts_iou_cls'):
        f(iou, cls, labels, {'SCORE_TYPE': 'num_pts_iou_cls'}, NAMES)
    with pytest.raises(NotImplementedError):
        f(iou, cls, labels, {'SCORE_TYPE': 'score_by_class', 'SCORE_BY_CLASS': {'Car': 'iou', 'Pedestrian': 'both', 'Cyclist': 'cls'}}, NAMES)
    with pytest.raises(NotImplementedError):
        f(iou, cls, labels, {'SCORE_TYPE': 'other'}, NAMES)


@pytest.mark.parametrize("key, where", [('MULTI_CLASSES_NMS', 'nms'), ('OUTPUT_RAW_SCORE', 'post')])
def test_post_processing_refuses_what_the_reference_refuses(key, where):
    cfg = copy.deepcopy(dc.SECOND_IOU_CFG['POST_PROCESSING'])
    (cfg['NMS_CONFIG'] if where == 'nms' else cfg)[key] = True
    stub = SECONDNetIoU.__new__(SECONDNetIoU)
    torch.nn.Module.__init__(stub)
    stub.model_cfg, stub.num_class, stub.class_names = cfg_from_dict({'POST_PROCESSING': cfg}), 3, NAMES
    with pytest.raises(NotImplementedError, match=key):
        stub.post_processing({'batch_size': 0})


# ---- configuration and registries -----------------------------------------------------------------------------------------------

def test_configuration_and_registries():
    assert roi_heads.__all__['SECONDHead'] is SECONDHead and detectors.__all__['SECONDNetIoU'] is SECONDNetIoU
    cfg, train = dc.SECOND_IOU_CFG, dc.SECOND_IOU_TRAIN_CFG
    assert cfg['NAME'] == 'SECONDNetIoU' and all(cfg[k] == dc.SECOND_CFG[k] for k in ('VFE', 'BACKBONE_3D', 'MAP_TO_BEV', 'BACKBONE_2D', 'DENSE_HEAD'))
    assert 'SCORE_TYPE' not in dc.SECOND_CFG['POST_PROCESSING']['NMS_CONFIG'], 'SECOND_CFG is left as it was'
    head = cfg['ROI_HEAD']
    assert head['NAME'] == 'SECONDHead' and head['CLASS_AGNOSTIC'] and head['ROI_GRID_POOL'] == {'GRID_SIZE': 7, 'IN_CHANNEL': 512, 'DOWNSAMPLE_RATIO': 8}
    assert head['SHARED_FC'] == [256, 256] and head['IOU_FC'] == [256, 256] and head['DP_RATIO'] == 0.3
    assert (head['NMS_CONFIG']['TRAIN']['NMS_POST_MAXSIZE'], head['NMS_CONFIG']['TRAIN']['NMS_THRESH']) == (512, 0.8)
    assert (head['NMS_CONFIG']['TEST']['NMS_POST_MAXSIZE'], head['NMS_CONFIG']['TEST']['NMS_THRESH']) == (100, 0.7)
    assert 'ROI_PER_IMAGE' not in head['TARGET_CONFIG'] and 'LOSS_CONFIG' not in head
    target, loss = train['ROI_HEAD']['TARGET_CONFIG'], train['ROI_HEAD']['LOSS_CONFIG']
    assert target['ROI_PER_IMAGE'] == 128 and target['CLS_SCORE_TYPE'] == 'roi_iou' and (target['CLS_BG_THRESH'], target['CLS_FG_THRESH']) == (0.25, 0.75)
    assert loss['IOU_LOSS'] == 'BinaryCrossEntropy' and loss['LOSS_WEIGHTS']['rcnn_iou_weight'] == 1.0 and len(loss['LOSS_WEIGHTS']['code_weights']) == 7
    assert sum(cfg['BACKBONE_2D']['NUM_UPSAMPLE_FILTERS']) == head['ROI_GRID_POOL']['IN_CHANNEL']


# ---- the entry points' argument checks and the packed weight ---------------------------------------------------------------------

def crop_call(**over):
    a = dict(B=1, n=2, stride=7, rois=8, C=16, H=13, W=9, feat=8, x0=0.0, y0=0.0, cx=0.4, cy=0.4, G=7, out=8, ld=16 * 49)
    a.update(over)
    _native.call("pdm_bev_roi_crop", 0, a['B'], a['n'], a['stride'], a['rois'], a['C'], a['H'], a['W'], a['feat'], a['x0'], a['y0'], a['cx'],
                 a['cy'], a['G'], a['out'], a['ld'])


@pytest.mark.parametrize("over", [{'G': 1}, {'G': 9}, {'stride': 6}, {'H': 1}, {'W': 1}, {'C': 0}, {'cx': 0.0}, {'cy': -0.4}, {'ld': 16 * 49 - 1},
                                  {'rois': None}, {'feat': None}, {'out': None}, {'H': 40000}, {'n': -1}, {'cx': math.inf}])
def test_crop_checks_its_arguments_before_any_launch(over):
    with pytest.raises(_native.NativeLibraryError, match='bev_roi_crop'):
        crop_call(**over)


def test_crop_of_no_roi_launches_nothing():
    crop_call(n=0, rois=None, feat=None, out=None)
    crop_call(B=0, rois=None, feat=None, out=None)


def fc_call(**over):
    a = dict(B=1, n=2, stride=7, rois=16, C=16, H=13, W=9, feat=16, G=7, Cout=32, w=16, scale=None, shift=None, out=16, ws=16, bytes=1 << 20)
    a.update(over)
    _native.call("pdm_bev_roi_crop_fc", 0, a['B'], a['n'], a['stride'], a['rois'], a['C'], a['H'], a['W'], a['feat'], 0.0, 0.0, 0.4, 0.4, a['G'],
                 a['Cout'], a['w'], a['scale'], a['shift'], 1, a['out'], a['ws'], a['bytes'])


@pytest.mark.parametrize("over", [{'G': 1}, {'C': 24}, {'C': 528}, {'Cout': 24}, {'Cout': 1040}, {'w': 20}, {'w': None}, {'scale': 16}, {'shift': 16},
                                  {'ws': None}, {'ws': 24}, {'bytes': 16}, {'out': None}, {'stride': 5}])
def test_crop_fc_checks_its_arguments_before_any_launch(over):
    with pytest.raises(_native.NativeLibraryError, match='bev_roi_crop_fc'):
        fc_call(**over)


def test_crop_fc_plan_is_a_function_of_the_sizes():
    lib = _native.lib()
    assert lib.pdm_bev_roi_crop_fc_packed_floats(512, 7, 256) == 512 * 49 * 256 and lib.pdm_bev_roi_crop_fc_packed_floats(24, 7, 256) == 0
    assert lib.pdm_bev_roi_crop_fc_chunks(1, 16, 2, 16) == 1                # 64 indices: one stage of 128
    assert lib.pdm_bev_roi_crop_fc_chunks(1, 512, 7, 256) == 196            # 196 stages, one tile: a chunk per stage
    chunks = lib.pdm_bev_roi_crop_fc_chunks(3200, 512, 7, 256)              # 100 tiles: about 1024 workgroups
    assert 1 < chunks <= 11 and lib.pdm_bev_roi_crop_fc_workspace_bytes(3200, 512, 7, 256) >= chunks * 3200 * 256 * 4
    assert lib.pdm_bev_roi_crop_fc_workspace_bytes(0, 512, 7, 256) == 0 and lib.pdm_bev_roi_crop_fc_chunks(5, 512, 1, 256) == 0


def test_packed_weight_layout():
    C, G, cout = 16, 2, 32
    w = torch.arange(cout * C * G * G, dtype=torch.float32).view(cout, C * G * G, 1)
    packed = bev_roi_ops.pack_crop_fc_weight(w, C, G).view(C * G * G // 16, cout // 16, 64, 4)
    for kb, nb, lane, j in [(0, 0, 0, 0), (3, 1, 63, 3), (2, 0, 17, 1), (1, 1, 40, 2)]:
        assert float(packed[kb, nb, lane, j]) == float(w[16 * nb + (lane & 15), 16 * kb + 4 * (lane >> 4) + j, 0])
    with pytest.raises(ValueError):
        bev_roi_ops.pack_crop_fc_weight(w, 8, G)
    with pytest.raises(ValueError):
        bev_roi_ops.bev_roi_crop(torch.zeros(1, 1, 7), torch.zeros(1, 1, 4, 4), [0, 0, 0, 1, 1, 1], [0.1, 0.1, 0.1], 1, 1)

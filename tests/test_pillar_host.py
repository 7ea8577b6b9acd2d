"""The pillar path's modules and registries on the CPU: construction, state_dict manifests against the reference's
(tests/golden/ref_pillar_manifest.json, written by gen_pillar_fixtures.py), BaseBEVBackbone's forward against the
reference's output, the CenterPoint-Pillar assembly, and the operators' argument checks (no GPU is touched: the checks
come before any launch)."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from pdm_ssd_amd.config import cfg_from_dict

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def manifest():
    with open(os.path.join(GOLDEN, "ref_pillar_manifest.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def ref():
    return np.load(os.path.join(GOLDEN, "ref_pillar.npz"))


def shapes_of(module):
    return {k: list(v.shape) for k, v in module.state_dict().items()}


@pytest.mark.parametrize("name", ["small", "kitti", "downsample", "extra_deblock", "no_upsample"])
def test_bev_backbone_state_dict_equals_the_reference_manifest(manifest, name):
    from pdm_ssd_amd.backbones_2d import BaseBEVBackbone
    entry = manifest['bev_cfgs'][name]
    net = BaseBEVBackbone(cfg_from_dict(entry['cfg']), entry['input_channels'])
    assert shapes_of(net) == manifest[f'BaseBEVBackbone({name})']
    assert net.num_bev_features == manifest[f'BaseBEVBackbone({name}).num_bev_features']
    if name == 'downsample':     # UPSAMPLE_STRIDES [0.5, 1, 2] with USE_CONV_FOR_NO_STRIDE: a stride-2 conv, a 1 x 1 conv, a deconv
        kinds = [type(d[0]).__name__ for d in net.deblocks]
        assert kinds == ['Conv2d', 'Conv2d', 'ConvTranspose2d']
        assert net.deblocks[0][0].stride == (2, 2) and net.deblocks[1][0].kernel_size == (1, 1)
    if name == 'extra_deblock':
        assert len(net.deblocks) == len(net.blocks) + 1


@pytest.mark.parametrize("name", ["small", "downsample"])
def test_bev_backbone_forward_equals_the_reference(manifest, ref, name):
    """the same torch convolutions on the same weights: 1e-5"""
    from pdm_ssd_amd.backbones_2d import BaseBEVBackbone
    entry = manifest['bev_cfgs'][name]
    net = BaseBEVBackbone(cfg_from_dict(entry['cfg']), entry['input_channels']).eval()
    net.load_state_dict({k[len(f'bev.{name}.state.'):]: torch.from_numpy(ref[k]) for k in ref.files if k.startswith(f'bev.{name}.state.')})
    x = torch.from_numpy(ref['g1.c4.canvas'][[0, 2]])
    with torch.no_grad():
        d = net({'spatial_features': x})
    want = ref[f'bev.{name}.out']
    assert tuple(d['spatial_features_2d'].shape) == want.shape
    assert float((d['spatial_features_2d'] - torch.from_numpy(want)).abs().max()) <= 1e-5
    assert 'spatial_features_1x' in d and 'spatial_features_2x' in d and d['spatial_features_2x'].shape[2] == x.shape[2] // 2


def test_vfe_and_scatter_construct_with_the_reference_keys(manifest):
    from pdm_ssd_amd.backbones_2d.map_to_bev import PointPillarScatter
    from pdm_ssd_amd.vfe import DynamicPillarVFE
    geo = dict(voxel_size=[0.5, 0.5, 4.0], grid_size=[40, 24, 1], point_cloud_range=[0.0, -6.0, -3.0, 20.0, 6.0, 1.0])
    for name, C_, kw in (('g1.c4', 4, {}), ('g1.c4.abs0.dist1', 4, dict(USE_ABSLOTE_XYZ=False, WITH_DISTANCE=True)), ('g1.c5', 5, {}),
                         ('g1.c4.f32_64', 4, dict(NUM_FILTERS=[32, 64])), ('g1.c4.nonorm', 4, dict(USE_NORM=False))):
        cfg = dict({'USE_NORM': True, 'WITH_DISTANCE': False, 'USE_ABSLOTE_XYZ': True, 'NUM_FILTERS': [64]}, **kw)
        vfe = DynamicPillarVFE(model_cfg=cfg_from_dict(cfg), num_point_features=C_, **geo)
        assert shapes_of(vfe) == manifest[f'DynamicPillarVFE({name})'], name
        assert vfe.get_output_feature_dim() == 64
    assert 'pfn_layers.0.linear.weight' in manifest['DynamicPillarVFE(g1.c4)'] and 'pfn_layers.0.norm.running_var' in manifest['DynamicPillarVFE(g1.c4)']
    sc = PointPillarScatter(model_cfg=cfg_from_dict({'NUM_BEV_FEATURES': 64}), grid_size=[40, 24, 1])
    assert sc.num_bev_features == 64 and (sc.nx, sc.ny, sc.nz) == (40, 24, 1) and not sc.state_dict()
    with pytest.raises(AssertionError):
        PointPillarScatter(model_cfg=cfg_from_dict({'NUM_BEV_FEATURES': 64}), grid_size=[40, 24, 2])
    with pytest.raises(AssertionError):
        DynamicPillarVFE(model_cfg=cfg_from_dict(cfg), num_point_features=4, voxel_size=[0.5, 0.5, 2.0], grid_size=[40, 24, 2],
                         point_cloud_range=geo['point_cloud_range'])


def test_registries_hold_the_pillar_modules():
    from pdm_ssd_amd import detectors
    assert 'DynamicPillarVFE' in detectors.VFE and 'BaseBEVBackbone' in detectors.BACKBONES_2D
    assert {'PDMNeck', 'PointPillarScatter'} <= set(detectors.MAP_TO_BEV)


def test_center_pillar_config_builds_a_centerpoint():
    from pdm_ssd_amd.detector_config import CENTER_PDM_CFG, CENTER_PILLAR_CFG, build_center_pillar
    model = build_center_pillar()
    assert [type(m).__name__ for m in model.module_list] == ['DynamicPillarVFE', 'PointPillarScatter', 'BaseBEVBackbone', 'CenterHead']
    assert model.backbone_2d.num_bev_features == 384 and model.dense_head.shared_conv[0].in_channels == 384
    assert model.vfe.get_output_feature_dim() == 64 and model.map_to_bev_module.num_bev_features == 64
    assert model.backbone_3d is None and model.pfe is None and model.point_head is None
    assert model.dataset.grid_size == [432, 496, 1] and model.dataset.voxel_size == [0.16, 0.16, 4]
    assert model.dataset.point_cloud_range == [0, -39.68, -3, 69.12, 39.68, 1]
    assert model.dense_head.feature_map_stride == 2 and CENTER_PDM_CFG['DENSE_HEAD']['TARGET_ASSIGNER_CONFIG']['FEATURE_MAP_STRIDE'] == 8
    assert CENTER_PILLAR_CFG['BACKBONE_2D']['LAYER_NUMS'] == [3, 5, 5] and CENTER_PILLAR_CFG['BACKBONE_2D']['NUM_UPSAMPLE_FILTERS'] == [128, 128, 128]
    keys = set(model.state_dict())
    assert {'vfe.pfn_layers.0.linear.weight', 'vfe.pfn_layers.0.norm.running_mean', 'backbone_2d.blocks.0.1.weight',
            'backbone_2d.blocks.2.16.weight', 'backbone_2d.deblocks.2.0.weight', 'backbone_2d.deblocks.0.1.running_var',
            'dense_head.shared_conv.0.weight', 'global_step'} <= keys
    assert not any(k.startswith('map_to_bev_module.') for k in keys)


def test_a_vfe_outside_the_registry_still_names_spconv():
    from pdm_ssd_amd.detector_config import CENTER_PILLAR_CFG, build_center_pillar
    for slot, name in (('VFE', 'MeanVFE'), ('VFE', 'PillarVFE'), ('BACKBONE_2D', 'BaseBEVBackboneV1')):
        bad = dict(CENTER_PILLAR_CFG, **{slot: dict(CENTER_PILLAR_CFG[slot], NAME=name)})
        with pytest.raises(AssertionError, match="spconv"):
            build_center_pillar(bad)


def test_pillar_entry_points_validate_their_arguments_before_any_launch():
    from pdm_ssd_amd import _native
    lib = _native.lib()
    buf = (C.c_int * 64)()
    p = C.cast(buf, C.c_void_p)
    assert lib.pdm_pillar_assign_workspace_bytes(1000, 2, 40, 24) % 256 == 0 and lib.pdm_pillar_assign_workspace_bytes(1000, 2, 40, 24) > 0
    assert lib.pdm_pillar_assign_workspace_bytes(1000, 65536, 1024, 1024) == 0

    def assign(N=10, C1=5, B=2, nx=40, ny=24, nz=1, points=p, record=p, ws=p, ws_bytes=1 << 30, vx=0.5):
        _native.call("pdm_pillar_assign", 0, N, C1, points, B, nx, ny, nz, 0.0, 0.0, vx, 0.5, p, p, p, p, p, p, p, p, record, ws, ws_bytes)
    with pytest.raises(_native.NativeLibraryError, match="nz = 1"):
        assign(nz=2)
    with pytest.raises(_native.NativeLibraryError, match="cells exceed int32"):
        assign(B=65536, nx=1024, ny=1024)
    with pytest.raises(_native.NativeLibraryError, match="point elements exceed int32"):
        assign(N=2 ** 30, C1=5)
    with pytest.raises(_native.NativeLibraryError, match="null pointer"):
        assign(points=None)
    with pytest.raises(_native.NativeLibraryError, match="null pointer"):
        assign(record=None)
    with pytest.raises(_native.NativeLibraryError, match="8-byte aligned"):
        assign(ws=C.c_void_p(C.addressof(buf) + 4))
    with pytest.raises(_native.NativeLibraryError, match="workspace too small"):
        assign(ws_bytes=16)
    with pytest.raises(_native.NativeLibraryError, match="voxel size"):
        assign(vx=0.0)
    with pytest.raises(_native.NativeLibraryError, match="nz = 1"):
        _native.call("pdm_pillar_scatter", 0, 4, 8, p, p, 2, 40, 24, 3, p)
    with pytest.raises(_native.NativeLibraryError, match="null pointer"):
        _native.call("pdm_pillar_scatter", 0, 4, 8, p, None, 2, 40, 24, 1, p)
    with pytest.raises(_native.NativeLibraryError, match="null pointer"):
        _native.call("pdm_pillar_scatter_grad", 0, 4, 8, None, p, 2, 40, 24, 1, p)
    with pytest.raises(_native.NativeLibraryError, match="null pointer"):
        _native.call("pdm_pillar_segment_max", 0, 4, 8, p, None, p, p, p)
    with pytest.raises(_native.NativeLibraryError, match="null pointer"):
        _native.call("pdm_pillar_features", 0, 4, 5, p, p, p, p, None, 1, 0, 0.5, 0.5, 0.25, 0.25, -1.0, p)
    with pytest.raises(_native.NativeLibraryError, match="at most 16"):
        _native.call("pdm_pillar_fused_pfn", 0, 4, 8, 13, p, p, p, p, p, p, 1, 0, 0.5, 0.5, 0.25, 0.25, -1.0, p, p, p, p)
    # empty calls return before any launch
    _native.call("pdm_pillar_segment_max", 0, 0, 8, None, None, None, None, None)
    _native.call("pdm_pillar_features", 0, 0, 5, None, None, None, None, None, 1, 0, 0.5, 0.5, 0.25, 0.25, -1.0, None)
    _native.call("pdm_pillar_scatter_grad", 0, 0, 8, None, None, 2, 40, 24, 1, None)

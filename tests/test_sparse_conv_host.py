"""The voxel path without a GPU: the numpy restatement of tests/sparse_conv_reference.py against the fixture (the reference's own
DynamicMeanVFE and backbones over a dense-convolution stub of spconv, gen_sparse_conv_fixtures.py), the backbones' state_dict
keys and shapes against the manifest, the registries, the detectors' module lists and channel threading, the argument checks of
every new entry point (they come before any launch), and the eval-only contract."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import sparse_conv_reference as scr

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def ref():
    z = np.load(os.path.join(GOLDEN, "ref_sparse_conv.npz"))
    return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def manifest():
    with open(os.path.join(GOLDEN, "ref_sparse_conv_manifest.json")) as f:
        return json.load(f)


@pytest.mark.parametrize("tag", ['v1', 'v2'])
def test_numpy_voxel_assign_matches_the_reference(ref, tag):
    geo = scr.V1 if tag == 'v1' else scr.V2
    pts = ref[f'{tag}.points']
    assert np.array_equal(pts, scr.v1_points() if tag == 'v1' else scr.v2_points(), equal_nan=True)
    got = scr.voxel_assign(pts, geo['B'], geo['range'], geo['voxel'], geo['grid'])
    for k in ('kept_idx', 'unq_inv', 'voxel_coords', 'voxel_count'):
        assert np.array_equal(got[k], ref[f'{tag}.{k}']), k
    assert np.array_equal(got['mean64'], ref[f'{tag}.mean64'])
    assert (np.diff(got['keys']) > 0).all()
    if tag == 'v1':     # what the shape is there for
        assert got['voxel_count'].max() == 1100 and (got['voxel_count'] == 1).sum() > 100
        assert 1 not in got['voxel_coords'][:, 0] and {0, 2} <= set(got['voxel_coords'][:, 0].tolist())
        dropped = np.setdiff1d(np.arange(len(pts)), got['kept_idx'])
        assert np.isfinite(pts[got['kept_idx'], 1:4]).all() and len(dropped) > 8


@pytest.mark.parametrize("name", ['VoxelBackBone8x', 'VoxelResBackBone8x'])
def test_numpy_rulebook_reproduces_every_level_of_the_reference_backbones(ref, name):
    """the four strided geometries chained: the restatement's output sites, in its order, are the fixture's at every level"""
    idx = ref['b1.coords']
    assert np.array_equal(idx, scr.b1_voxels(4)[0])
    shape = (scr.B1_GRID[2] + 1, scr.B1_GRID[1], scr.B1_GRID[0])
    for lv, geo in (('x_conv2', 'k3s2p1'), ('x_conv3', 'k3s2p1'), ('x_conv4', 'k3s2p011'), ('out', 'k311s211p0')):
        idx, nbr, shape = scr.rulebook(idx, scr.B1_B, shape, *scr.GEOMETRIES[geo])
        assert list(shape) == ref[f'{name}.{lv}.shape'].tolist(), lv
        assert np.array_equal(idx, ref[f'{name}.{lv}.indices']), lv
        assert (nbr >= 0).any(1).all()
    assert len(idx) >= 8
    assert np.array_equal(ref[f'{name}.x_conv1.indices'], ref['b1.coords'])


def test_numpy_rulebook_never_wraps_and_never_crosses_a_sample():
    idx = scr.r1_indices()
    assert len(idx) >= 400 and 1 not in idx[:, 0] and len({tuple(c) for c in idx.tolist()}) == len(idx)
    _, nbr, _ = scr.rulebook(idx, scr.R1_B, scr.R1_SHAPE, *scr.GEOMETRIES['subm3'])
    assert np.array_equal(nbr[:, 13], np.arange(len(idx)))
    for i, j in zip(*np.nonzero(nbr >= 0)):
        d = idx[nbr[i, j]] - idx[i]
        assert d[0] == 0 and np.abs(d[1:]).max() <= 1
        assert (d[1] + 1) * 9 + (d[2] + 1) * 3 + d[3] + 1 == j
    assert (nbr >= 0).sum(1).max() == 27            # the full block's centre


@pytest.mark.parametrize("name", ['VoxelBackBone8x', 'VoxelResBackBone8x'])
def test_backbone_state_dict_keys_and_shapes_match_the_reference(manifest, name):
    from pdm_ssd_amd import backbones_3d
    net = backbones_3d.__all__[name](model_cfg={}, input_channels=4, grid_size=scr.B1_GRID)
    assert {k: list(v.shape) for k, v in net.state_dict().items()} == manifest[name]
    assert net.sparse_shape == [41, 16, 21] and net.num_point_features == 128
    assert net.backbone_channels == {'x_conv1': 16, 'x_conv2': 32, 'x_conv3': 64, 'x_conv4': 64 if name == 'VoxelBackBone8x' else 128}
    fill = manifest[f'{name}.fill']
    assert abs(scr.fill_backbone(net, fill['seed'], fill['gain']) - fill['checksum']) <= 1e-9 * fill['checksum']


def test_backbone_config_keys():
    from pdm_ssd_amd.backbones_3d import VoxelBackBone8x, VoxelResBackBone8x
    assert VoxelBackBone8x({'last_pad': (1, 0, 0)}, 4, scr.B1_GRID).conv_out[0].padding == (1, 0, 0)
    assert VoxelBackBone8x({}, 4, scr.B1_GRID).conv_out[0].padding == (0, 0, 0)
    assert VoxelResBackBone8x({}, 4, scr.B1_GRID).conv1[0].conv1.bias is not None
    assert VoxelResBackBone8x({'USE_BIAS': False}, 4, scr.B1_GRID).conv1[0].conv1.bias is None
    assert VoxelResBackBone8x({}, 5, scr.B1_GRID).conv_input[0].weight.shape == (16, 3, 3, 3, 5)


def test_registries():
    from pdm_ssd_amd import backbones_3d, detectors, vfe
    from pdm_ssd_amd.backbones_2d import map_to_bev
    from pdm_ssd_amd.detectors import detector3d_template as t
    assert vfe.__all__['DynamicMeanVFE'] is t.VFE['DynamicMeanVFE'] and 'MeanVFE' not in t.VFE and 'PillarVFE' not in t.VFE
    assert map_to_bev.__all__['HeightCompression'] is t.MAP_TO_BEV['HeightCompression']
    assert t.BACKBONES_3D['VoxelBackBone8x'] is backbones_3d.VoxelBackBone8x and t.BACKBONES_3D['VoxelResBackBone8x'] is backbones_3d.VoxelResBackBone8x
    assert 'PointNet2MSG' in t.BACKBONES_3D and detectors.__all__['SECONDNet'].__name__ == 'SECONDNet'


def test_detector_module_lists_and_channel_threading():
    from pdm_ssd_amd import detector_config as dc
    second = dc.build_second()
    assert [type(m).__name__ for m in second.module_list] == ['DynamicMeanVFE', 'VoxelBackBone8x', 'HeightCompression', 'BaseBEVBackbone',
                                                              'AnchorHeadSingle']
    assert second.backbone_3d.sparse_shape == [41, 1600, 1408] and second.backbone_3d.conv_input[0].in_channels == 4
    assert second.map_to_bev_module.num_bev_features == 256 and second.backbone_2d.num_bev_features == 512
    assert second.backbone_2d.blocks[0][1].in_channels == 256 and second.dense_head.conv_cls.in_channels == 512
    assert all(a['feature_map_stride'] == 8 for a in dc.SECOND_CFG['DENSE_HEAD']['ANCHOR_GENERATOR_CONFIG'])
    assert all(a['feature_map_stride'] == 2 for a in dc.POINT_PILLAR_CFG['DENSE_HEAD']['ANCHOR_GENERATOR_CONFIG'])
    center = dc.build_center_voxel(num_point_features=5)
    assert [type(m).__name__ for m in center.module_list] == ['DynamicMeanVFE', 'VoxelResBackBone8x', 'HeightCompression', 'BaseBEVBackbone',
                                                              'CenterHead']
    assert center.backbone_3d.conv_input[0].in_channels == 5 and center.vfe.get_output_feature_dim() == 5
    assert dc.CENTER_VOXEL_CFG['DENSE_HEAD']['TARGET_ASSIGNER_CONFIG']['FEATURE_MAP_STRIDE'] == 8
    assert dc.voxel_dataset().point_cloud_range == [0, -40, -3, 70.4, 40, 1] and dc.voxel_dataset().grid_size == [1408, 1600, 40]


def test_training_mode_and_inputs_that_require_grad_raise():
    from pdm_ssd_amd import spconv
    from pdm_ssd_amd.backbones_3d import VoxelBackBone8x
    bd = {'voxel_features': torch.zeros((1, 4)), 'voxel_coords': torch.zeros((1, 4), dtype=torch.int32), 'batch_size': 1}
    with pytest.raises(NotImplementedError, match='next step'):
        VoxelBackBone8x({}, 4, scr.B1_GRID).train()(dict(bd))
    conv = spconv.SubMConv3d(4, 16, 3, indice_key='k').eval()
    x = spconv.SparseConvTensor(torch.zeros((1, 4), requires_grad=True), bd['voxel_coords'], [41, 16, 21], 1)
    with pytest.raises(NotImplementedError, match='gradients'):
        conv(x)
    with pytest.raises(NotImplementedError):
        spconv.SparseSequential(conv, torch.nn.BatchNorm1d(16).train(), torch.nn.ReLU())(x.replace_feature(torch.zeros((1, 4))))


def test_pack_weight_layout_and_refusals():
    from pdm_ssd_amd import sparse_conv_ops
    w = torch.arange(32 * 27 * 5, dtype=torch.float32).reshape(32, 3, 3, 3, 5)
    p = sparse_conv_ops.pack_weight(w).reshape(27, 1, 2, 64, 4)
    for k, nb, lane, j in ((0, 0, 0, 0), (26, 1, 17, 0), (13, 1, 15, 3), (5, 0, 16, 0), (5, 0, 33, 1)):
        cin, cout = 4 * (lane >> 4) + j, 16 * nb + (lane & 15)
        assert float(p[k, 0, nb, lane, j]) == (float(w.reshape(32, 27, 5)[cout, k, cin]) if cin < 5 else 0.0)
    for shape in ((16, 3, 3, 3, 2), (16, 3, 3, 3, 9), (24, 3, 3, 3, 16), (256, 3, 3, 3, 16)):
        with pytest.raises(ValueError, match='channels'):
            sparse_conv_ops.pack_weight(torch.zeros(shape))


def test_entry_points_validate_their_arguments_before_any_launch():
    """null pointers, over-int32 and over-2^35 sizes, unsupported channel counts, a too-small workspace, a zero voxel size: an
    error code and a message, no launch (no GPU is touched: the checks come first)"""
    from pdm_ssd_amd import _native
    lib = _native.lib()
    buf = (C.c_float * 4096)()
    ptr = C.cast(buf, C.c_void_p)
    err = _native.NativeLibraryError
    grid, geo = (3, 21, 16, 40), (0.0, -4.0, -3.0, 0.5, 0.5, 0.1)
    need = lib.pdm_voxel_assign_workspace_bytes(100, 5, *grid)
    assert need > 0 and lib.pdm_voxel_assign_workspace_bytes(100, 5, 32, 140800, 160000, 40) == 0
    assert lib.pdm_voxel_assign_workspace_bytes(100, 5, 32, 1408, 1600, 40) > 32 * 1408 * 1600 * 40 // 8      # 2.9e9 cells: over int32, served
    outs = (ptr,) * 6
    with pytest.raises(err, match='voxel size must be positive'):
        _native.call("pdm_voxel_assign", 0, 100, 5, ptr, *grid, 0.0, -4.0, -3.0, 0.5, 0.0, 0.1, *outs, ptr, 1 << 30)
    with pytest.raises(err, match='null pointer'):
        _native.call("pdm_voxel_assign", 0, 100, 5, None, *grid, *geo, *outs, ptr, 1 << 30)
    with pytest.raises(err, match='workspace too small'):
        _native.call("pdm_voxel_assign", 0, 100, 5, ptr, *grid, *geo, *outs, ptr, need - 1)
    with pytest.raises(err, match='2\\^35 cells'):
        _native.call("pdm_voxel_assign", 0, 100, 5, ptr, 32, 140800, 160000, 40, *geo, *outs, ptr, 1 << 30)
    with pytest.raises(err, match='bad size'):
        _native.call("pdm_voxel_assign", 0, 100, 3, ptr, *grid, *geo, *outs, ptr, 1 << 30)

    conv = (3, 41, 16, 21, 3, 3, 3, 2, 2, 2, 1, 1, 1, 0)
    need = lib.pdm_sparse_rulebook_workspace_bytes(100, *conv)
    assert need > 0 and lib.pdm_sparse_rulebook_workspace_bytes(100, 3, 41, 16, 21, 5, 3, 3, 1, 1, 1, 0, 0, 0, 0) == 0
    for name, tail in (("pdm_sparse_sites", (ptr,)), ("pdm_sparse_rulebook", (ptr, ptr))):
        head = (100, ptr) if name == "pdm_sparse_sites" else (100, ptr, 50)
        with pytest.raises(err, match='workspace too small'):
            _native.call(name, 0, *head, *conv, *tail, ptr, need - 1)
        with pytest.raises(err, match='null pointer'):
            _native.call(name, 0, head[0], None, *head[2:], *conv, *tail, ptr, need)
        with pytest.raises(err, match='at most 27 offsets'):
            _native.call(name, 0, *head, 3, 41, 16, 21, 5, 3, 3, 1, 1, 1, 0, 0, 0, 0, *tail, ptr, need)
        with pytest.raises(err, match='stride 1'):
            _native.call(name, 0, *head, 3, 41, 16, 21, 3, 3, 3, 2, 2, 2, 1, 1, 1, 1, *tail, ptr, need)
        with pytest.raises(err, match='exceed int32'):
            _native.call(name, 0, 1 << 27, *head[1:], *conv, *tail, ptr, 1 << 40)
        with pytest.raises(err, match='2\\^35 cells'):
            _native.call(name, 0, *head, 32, 41, 160000, 140800, *conv[4:], *tail, ptr, 1 << 40)
    with pytest.raises(err, match='null pointer'):
        _native.call("pdm_sparse_rulebook", 0, 100, ptr, 50, *conv, ptr, None, ptr, need)

    ok = (100, 100, 27, 16, 32, ptr, ptr, ptr, None, None, None, 0, ptr)
    for cin, cout, text in ((2, 16, 'input channels'), (12, 16, 'input channels'), (256, 16, 'input channels'), (16, 8, 'output channels'),
                            (16, 48, 'output channels'), (16, 256, 'output channels')):
        with pytest.raises(err, match=text):
            _native.call("pdm_sparse_conv", 0, 100, 100, 27, cin, cout, *ok[5:])
    with pytest.raises(err, match='offsets'):
        _native.call("pdm_sparse_conv", 0, 100, 100, 28, *ok[3:])
    with pytest.raises(err, match='null pointer'):
        _native.call("pdm_sparse_conv", 0, *ok[:6], None, *ok[7:])
    with pytest.raises(err, match='come together'):
        _native.call("pdm_sparse_conv", 0, *ok[:8], ptr, None, None, 0, ptr)
    with pytest.raises(err, match='16-byte aligned'):
        _native.call("pdm_sparse_conv", 0, *ok[:7], C.c_void_p(ptr.value + 4), *ok[8:])
    with pytest.raises(err, match='exceed int32'):
        _native.call("pdm_sparse_conv", 0, 1 << 27, *ok[1:])
    assert lib.pdm_sparse_conv_packed_floats(27, 5, 32) == 27 * 1 * 2 * 256 and lib.pdm_sparse_conv_packed_floats(27, 5, 24) == 0

    need = lib.pdm_sparse_to_dense_workspace_bytes(3, 2, 200, 176)
    assert need >= 4 * 3 * 2 * 200 * 176 and lib.pdm_sparse_to_dense_workspace_bytes(64, 41, 1600, 1408) == 0
    with pytest.raises(err, match='workspace too small'):
        _native.call("pdm_sparse_to_dense", 0, 10, 16, ptr, ptr, 3, 2, 200, 176, ptr, ptr, need - 1)
    with pytest.raises(err, match='null pointer'):
        _native.call("pdm_sparse_to_dense", 0, 10, 16, ptr, None, 3, 2, 200, 176, ptr, ptr, need)
    with pytest.raises(err, match='exceed int32'):
        _native.call("pdm_sparse_to_dense", 0, 10, 16, ptr, ptr, 64, 41, 1600, 1408, ptr, ptr, 1 << 40)
    with pytest.raises(err, match='bad size'):
        _native.call("pdm_sparse_to_dense", 0, 10, 0, ptr, ptr, 3, 2, 200, 176, ptr, ptr, need)

"""Voxel R-CNN without a GPU: the numpy restatement of the RoI-grid pooling (tests/voxel_rcnn_reference.py) against the
reference's own NeighborVoxelSAModuleMSG (tests/golden/ref_voxel_rcnn.npz, gen_voxel_rcnn_fixtures.py), state_dict keys and
shapes against the reference's, the registries and build_voxel_rcnn()'s module list, the argument checks of the new entry
points (an error code before any launch), and the training-mode refusal."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import voxel_rcnn_case as case
import voxel_rcnn_reference as vr

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def ref():
    z = np.load(os.path.join(GOLDEN, "ref_voxel_rcnn.npz"))
    return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def manifest():
    with open(os.path.join(GOLDEN, "ref_voxel_rcnn_manifest.json")) as f:
        return json.load(f)


def test_levels_are_the_fixtures(ref):
    for name, lv in case.levels().items():
        assert np.array_equal(lv['indices'], ref[f'{name}.indices']) and list(lv['shape']) == ref[f'{name}.shape'].tolist()
    for name in case.HEAD_CFG['ROI_GRID_POOL']['FEATURES_SOURCE']:
        assert np.array_equal(case.level_features(name, len(ref[f'{name}.indices'])), ref[f'{name}.features'])


@pytest.mark.parametrize("G", case.GRID_SIZES)
def test_numpy_restatement_matches_the_reference_module(ref, G):
    """Pooled features of both source levels within 2e-5 of the reference's own module (fp32 there, float64 behind fp32 geometry
    here; the features are of order 1), with empty groups, partly filled ones and overflowing ones all present."""
    state = {k[len(f'g{G}.state.'):]: v for k, v in ref.items() if k.startswith(f'g{G}.state.')}
    pool_cfg = case.HEAD_CFG['ROI_GRID_POOL']['POOL_LAYERS']
    for i, src in enumerate(case.HEAD_CFG['ROI_GRID_POOL']['FEATURES_SOURCE']):
        cfg, stride = pool_cfg[src], dict((n, s) for n, s, _ in case.LEVEL_GEOMETRY)[src]
        got, hits = vr.module_forward(state, f'roi_grid_pool_layers.{i}.', 0, ref[f'g{G}.rois'], G, ref[f'{src}.indices'], ref[f'{src}.features'],
                                      tuple(ref[f'{src}.shape']), stride, case.VOXEL, case.RANGE, cfg['QUERY_RANGES'][0], cfg['POOL_RADIUS'][0],
                                      cfg['NSAMPLE'][0])
        sizes = [len(h) for h in hits]
        assert 0 in sizes and cfg['NSAMPLE'][0] in sizes
        assert got.shape == ref[f'g{G}.pooled{i}'].shape
        assert float(np.abs(got - ref[f'g{G}.pooled{i}']).max()) <= 2e-5


def test_grid_points_order_and_negative_cells():
    """x index slowest, z fastest; a grid point below the range minimum has a negative cell, floored (not truncated) at a stride"""
    rois = np.array([[[1.0, 2.0, 3.0, 4.0, 2.0, 6.0, 0.0]]], dtype=np.float32)
    p = vr.grid_points(rois, 2)
    assert p.tolist() == [[0, 1.5, 1.5], [0, 1.5, 4.5], [0, 2.5, 1.5], [0, 2.5, 4.5], [2, 1.5, 1.5], [2, 1.5, 4.5], [2, 2.5, 1.5], [2, 2.5, 4.5]]
    quarter = np.array([[[0.0, 0.0, 0.0, 4.0, 2.0, 2.0, np.pi / 2]]], dtype=np.float32)
    assert np.allclose(vr.grid_points(quarter, 2)[0], [0.5, -1.0, -0.5], atol=1e-6)
    c = vr.cells(np.array([[-0.3, -4.6, -3.05]], np.float32), case.RANGE, case.VOXEL, 2)
    assert c.tolist() == [[-1, -1, -1]]         # base cells (-1, -2, -1): floor(-1 / 2) = floor(-2 / 2) = -1, truncation gives 0
    assert vr.centres(np.array([[3, 2, 1]]), 4, case.VOXEL, case.RANGE).tolist() == [[3.0, 1.0, np.float32(3.5) * np.float32(0.4) + np.float32(-3.0)]]


def test_state_dict_keys_and_shapes_match_the_reference(manifest):
    from pdm_ssd_amd import detector_config as dc
    from pdm_ssd_amd.config import cfg_from_dict
    from pdm_ssd_amd.roi_heads import VoxelRCNNHead
    for G in case.GRID_SIZES:
        head = VoxelRCNNHead(backbone_channels=dict(case.BACKBONE_CHANNELS), model_cfg=cfg_from_dict(case.head_cfg(G)),
                             point_cloud_range=case.RANGE, voxel_size=case.VOXEL, num_class=1)
        want = manifest[f'VoxelRCNNHead(reduced: tests/voxel_rcnn_case.py HEAD_CFG, GRID_SIZE={G}, num_class=1)']
        assert {k: list(v.shape) for k, v in head.state_dict().items()} == want
    model = dc.build_voxel_rcnn()
    want = manifest['VoxelRCNNHead(VOXEL_RCNN_CFG, VoxelBackBone8x channels, num_class=1)']
    assert {k: list(v.shape) for k, v in model.roi_head.state_dict().items()} == want
    assert 'shared_fc_layer.4.weight' in want and 'shared_fc_layer.3.weight' not in want      # the Dropout at child 3 shifts the indices
    second = {k: list(v.shape) for k, v in dc.build_second().state_dict().items()}
    mine = {k: list(v.shape) for k, v in model.state_dict().items()}
    assert {k: v for k, v in mine.items() if not k.startswith('roi_head.')} == second
    assert {k[len('roi_head.'):]: v for k, v in mine.items() if k.startswith('roi_head.')} == want


def test_registries_and_module_list():
    from pdm_ssd_amd import detector_config as dc
    from pdm_ssd_amd import detectors, roi_heads
    from pdm_ssd_amd.pointnet2_stack import voxel_pool_modules
    from pdm_ssd_amd.utils import common_utils
    assert roi_heads.__all__['VoxelRCNNHead'].__name__ == 'VoxelRCNNHead' and detectors.__all__['VoxelRCNN'].__name__ == 'VoxelRCNN'
    assert hasattr(common_utils, 'get_voxel_centers') and hasattr(common_utils, 'generate_voxel2pinds')
    model = dc.build_voxel_rcnn()
    assert [type(m).__name__ for m in model.module_list] == ['DynamicMeanVFE', 'VoxelBackBone8x', 'HeightCompression', 'BaseBEVBackbone',
                                                             'AnchorHeadSingle', 'VoxelRCNNHead']
    head = model.roi_head
    assert head.num_class == 1 and head.num_pooled_channels == 96 and head.shared_fc_layer[0].in_features == 216 * 96
    assert [type(m) for m in head.roi_grid_pool_layers] == [voxel_pool_modules.NeighborVoxelSAModuleMSG] * 3
    assert [l.mlps_in[0][0].in_channels for l in head.roi_grid_pool_layers] == [32, 64, 64]
    assert all(l.fused_supported(6) for l in head.eval().roi_grid_pool_layers)
    cfg = dc.VOXEL_RCNN_CFG['ROI_HEAD']
    assert cfg['NMS_CONFIG']['TEST'] == {'NMS_TYPE': 'nms_gpu', 'MULTI_CLASSES_NMS': False, 'NMS_PRE_MAXSIZE': 2048, 'NMS_POST_MAXSIZE': 100,
                                         'NMS_THRESH': 0.7}
    assert dc.VOXEL_RCNN_CFG['ROI_HEAD']['ROI_GRID_POOL']['POOL_LAYERS']['x_conv2']['MLPS'] == [[32, 32]]      # building edits no config
    assert {k: v for k, v in dc.VOXEL_RCNN_CFG.items() if k not in ('NAME', 'ROI_HEAD')} == {k: v for k, v in dc.SECOND_CFG.items() if k != 'NAME'}


def test_what_the_fused_operator_refuses_goes_to_the_composed_path():
    from pdm_ssd_amd.pointnet2_stack.voxel_pool_modules import NeighborVoxelSAModuleMSG as M
    ok = dict(query_ranges=[[4, 4, 4]], radii=[0.8], nsamples=[16], mlps=[[32, 32, 32]])
    assert M(**ok).eval().fused_supported(6)
    assert not M(**ok).fused_supported(6)                                   # training mode
    assert not M(**ok).eval().fused_supported(9)
    for change in (dict(pool_method='avg_pool'), dict(mlps=[[32, 24, 32]]), dict(mlps=[[32, 32, 128]]), dict(mlps=[[12, 32, 32]]),
                   dict(query_ranges=[[5, 4, 4]]), dict(nsamples=[33])):
        assert not M(**dict(ok, **change)).eval().fused_supported(6), change
    m = M(query_ranges=[[1, 1, 1], [2, 2, 2]], radii=[0.4, 0.8], nsamples=[4, 8], mlps=[[16, 16, 16], [16, 32, 32]])
    assert sorted(k.split('.')[0] for k in m.state_dict()) == sorted(['mlps_in'] * 12 + ['mlps_pos'] * 12 + ['mlps_out'] * 12)
    assert len(m.groupers) == 2 and m.out_channels() == [16, 32]


def test_training_mode_forward_raises():
    from pdm_ssd_amd.config import cfg_from_dict
    from pdm_ssd_amd.roi_heads import VoxelRCNNHead
    head = VoxelRCNNHead(backbone_channels=dict(case.BACKBONE_CHANNELS), model_cfg=cfg_from_dict(case.head_cfg(2)),
                         point_cloud_range=case.RANGE, voxel_size=case.VOXEL, num_class=1).train()
    with pytest.raises(NotImplementedError, match='no gradient yet'):
        head({'batch_size': 1, 'rois': torch.zeros((1, 2, 7))})


def test_entry_points_validate_their_arguments_before_any_launch():
    """null pointers, a workspace that is too small, more than 2^35 cells, unsupported widths, windows, nsample and grid sizes,
    columns that do not fit the row, misaligned packed weights: an error code and a message, no launch"""
    from pdm_ssd_amd import _native
    lib = _native.lib()
    buf = (C.c_float * 4096)()
    ptr = C.cast(buf, C.c_void_p)
    err = _native.NativeLibraryError
    grid = (3, 21, 8, 11)
    need = lib.pdm_sparse_index_workspace_bytes(100, *grid)
    assert need > 0 and lib.pdm_sparse_index_workspace_bytes(100, 32, 41, 160000, 140800) == 0 and lib.pdm_sparse_index_workspace_bytes(-1, *grid) == 0
    kitti = lib.pdm_sparse_index_workspace_bytes(100000, 32, 21, 800, 704)
    cells = 32 * 21 * 800 * 704     # a bit a cell, 4 bytes per group of 256 cells, 4 bytes a row: 1/28 of the dense table's 4 bytes a cell
    assert cells // 8 + cells // 64 + 4 * 100000 <= kitti < cells // 8 + cells // 64 + 4 * 100000 + 8192
    with pytest.raises(err, match='null pointer'):
        _native.call("pdm_sparse_index", 0, 100, None, *grid, ptr, need)
    with pytest.raises(err, match='null pointer'):
        _native.call("pdm_sparse_index", 0, 100, ptr, *grid, None, need)
    with pytest.raises(err, match='workspace too small'):
        _native.call("pdm_sparse_index", 0, 100, ptr, *grid, ptr, need - 1)
    with pytest.raises(err, match='2\\^35 cells'):
        _native.call("pdm_sparse_index", 0, 100, ptr, 32, 41, 160000, 140800, ptr, 1 << 40)
    with pytest.raises(err, match='bad size'):
        _native.call("pdm_sparse_index", 0, -1, ptr, *grid, ptr, need)
    with pytest.raises(err, match='8-byte aligned'):
        _native.call("pdm_sparse_index", 0, 100, ptr, *grid, C.c_void_p(ptr.value + 4), need)

    def pool(**change):
        a = dict(B=3, n=5, roi_stride=7, rois=ptr, G=2, D=21, H=8, W=11, stride=2, vx=0.5, vy=0.5, vz=0.1, x0=0.0, y0=-4.0, z0=-3.0, P=100,
                 index=ptr, index_bytes=need, C1=16, feat=ptr, wp=ptr, scale_p=ptr, shift_p=ptr, rz=1, ry=2, rx=3, radius=1.6, nsample=4,
                 C2=32, wout=ptr, scale_o=ptr, shift_o=ptr, out=ptr, out_stride=48, out_offset=16)
        a.update(change)
        _native.call("pdm_roi_grid_pool", 0, *a.values())
    for change, text in ((dict(rois=None), 'null pointer'), (dict(index=None), 'null pointer'), (dict(feat=None), 'null pointer'),
                         (dict(wout=None), 'null pointer'), (dict(shift_o=None), 'null pointer'), (dict(out=None), 'null pointer'),
                         (dict(index_bytes=need - 1), 'site index too small'), (dict(B=32, D=41, H=160000, W=140800), '2\\^35 cells'),
                         (dict(C1=24), 'pooled channels'), (dict(C1=128), 'pooled channels'), (dict(C2=8), 'output channels'),
                         (dict(C2=128), 'output channels'), (dict(rz=5), 'at most 9 x 9 x 9'), (dict(rx=-1), 'at most 9 x 9 x 9'),
                         (dict(nsample=33), 'nsample'), (dict(nsample=0), 'nsample'), (dict(G=9), 'grid size'), (dict(G=0), 'grid size'),
                         (dict(out_offset=17), 'do not fit'), (dict(out_stride=31, out_offset=0), 'do not fit'), (dict(roi_stride=6), 'bad size'),
                         (dict(vz=0.0), 'voxel size'), (dict(stride=0), 'stride'), (dict(radius=-1.0), 'radius'),
                         (dict(wout=C.c_void_p(ptr.value + 4)), '16-byte aligned'), (dict(index=C.c_void_p(ptr.value + 4)), '8-byte aligned'),
                         (dict(n=1 << 28), 'exceed int32')):
        with pytest.raises(err, match=text):
            pool(**change)
    pool(n=0)       # nothing to do: no launch, no error

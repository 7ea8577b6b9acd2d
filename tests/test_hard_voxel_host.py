"""Hard voxels, the host side (no GPU): the numpy restatement of the generator against a hand-derived case and against its
closed form, the registry names, the two hard-voxel detector configs against the reference's state_dict manifest, and the
entry points' argument checks, which come before any launch."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import hard_voxel_reference as hvr

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

HAND_ROWS = np.array([
    [0.5, 0.5, 0.5],        # 0  cell (0, 0, 0): voxel 0, slot 0
    [3.5, 1.5, 0.5],        # 1  cell (3, 1, 0): voxel 1, slot 0
    [0.2, 0.9, 0.1],        # 2  voxel 0, slot 1
    [1.5, 0.5, 0.5],        # 3  cell (1, 0, 0): a third cell, refused at max_voxels = 2
    [3.1, 1.1, 0.9],        # 4  voxel 1, slot 1: taken AFTER a refused row (continue, not break)
    [0.7, 0.3, 0.2],        # 5  voxel 0 is full at T = 2
    [4.0, 0.5, 0.5],        # 6  x = range end: outside
    [1.0, 1.0, 1.0],        # 7  z = range end: outside
    [-0.1, 0.5, 0.5],       # 8  outside
    [1.5, 0.6, 0.5],        # 9  the refused cell again
    [np.nan, 0.5, 0.5],     # 10 NaN: outside
    [3.9, 1.9, 0.0],        # 11 voxel 1 is full at T = 2
], dtype=np.float32)
HAND_GEO = dict(point_cloud_range=[0, 0, 0, 4, 2, 1], voxel_size=[1, 1, 1], grid_size=[4, 2, 1])


@pytest.mark.parametrize("fn", [hvr.voxelize_loop, hvr.voxelize_closed_form], ids=['loop', 'closed_form'])
def test_the_restatement_gives_the_hand_derived_answer(fn):
    slot_rows, coords, num = fn(HAND_ROWS, T=2, max_voxels=2, **HAND_GEO)
    assert slot_rows.tolist() == [[0, 2], [1, 4]] and coords.tolist() == [[0, 0, 0], [0, 1, 3]] and num.tolist() == [2, 2]
    slot_rows, coords, num = fn(HAND_ROWS, T=2, max_voxels=3, **HAND_GEO)
    assert slot_rows.tolist() == [[0, 2], [1, 4], [3, 9]] and coords.tolist() == [[0, 0, 0], [0, 1, 3], [0, 0, 1]] and num.tolist() == [2, 2, 2]
    slot_rows, coords, num = fn(HAND_ROWS, T=4, max_voxels=1, **HAND_GEO)
    assert slot_rows.tolist() == [[0, 2, 5, -1]] and coords.tolist() == [[0, 0, 0]] and num.tolist() == [3]


def test_the_batch_collate_of_the_hand_derived_case():
    pts = np.concatenate([np.concatenate([np.full((12, 1), b, dtype=np.float32), HAND_ROWS], 1) for b in (0, 2)])
    pts = np.concatenate([np.array([[-1, 0.5, 0.5, 0.5]], dtype=np.float32), pts, np.array([[3, 0.5, 0.5, 0.5]], dtype=np.float32)])
    v = hvr.voxelize_batch(pts, 3, T=2, max_voxels=2, **HAND_GEO)
    assert v['slot_rows'].tolist() == [[1, 3], [2, 5], [13, 15], [14, 17]]
    assert v['voxel_coords'].tolist() == [[0, 0, 0, 0], [0, 0, 1, 3], [2, 0, 0, 0], [2, 0, 1, 3]] and v['voxel_num_points'].tolist() == [2] * 4
    assert np.array_equal(v['voxels'][1], pts[[2, 5], 1:]) and v['voxels'].shape == (4, 2, 3)
    with pytest.raises(AssertionError, match='grouped by sample'):
        hvr.voxelize_batch(pts[::-1], 3, T=2, max_voxels=2, **HAND_GEO)


@pytest.mark.parametrize("seed", range(6))
def test_the_closed_form_equals_the_loop_on_random_inputs(seed):
    rng = np.random.default_rng(seed)
    n, T, cap = int(rng.integers(1, 400)), int(rng.integers(1, 6)), int(rng.integers(1, 40))
    rows = rng.uniform(-0.5, 4.5, (n, 3)).astype(np.float32) * np.array([1, 0.5, 0.5], dtype=np.float32)
    geo = dict(point_cloud_range=[0, 0, 0, 4, 2, 2], voxel_size=[0.5, 0.5, 1.0], grid_size=[8, 4, 2])
    a, b = hvr.voxelize_loop(rows, T=T, max_voxels=cap, **geo), hvr.voxelize_closed_form(rows, T=T, max_voxels=cap, **geo)
    assert len(a[0]) > 0 and all(np.array_equal(x, y) for x, y in zip(a, b))


def test_registry_has_the_hard_names_and_still_refuses_the_plain_ones():
    from pdm_ssd_amd import detectors, vfe
    from pdm_ssd_amd.detector_config import POINT_PILLAR_HARD_CFG, SECOND_HARD_CFG, build_point_pillar, build_second
    assert vfe.__all__['HardMeanVFE'] is vfe.MeanVFE and vfe.__all__['HardPillarVFE'] is vfe.PillarVFE
    assert detectors.VFE['HardMeanVFE'] is vfe.MeanVFE and detectors.VFE['HardPillarVFE'] is vfe.PillarVFE
    assert 'MeanVFE' not in detectors.VFE and 'PillarVFE' not in detectors.VFE
    for build, cfg, name in ((build_point_pillar, POINT_PILLAR_HARD_CFG, 'PillarVFE'), (build_second, SECOND_HARD_CFG, 'MeanVFE')):
        with pytest.raises(AssertionError, match="spconv"):
            build(dict(cfg, VFE=dict(cfg['VFE'], NAME=name)))


def test_the_two_hard_configs_build_with_the_manifest_s_keys():
    from pdm_ssd_amd.detector_config import (POINT_PILLAR_CFG, POINT_PILLAR_HARD_CFG, SECOND_CFG, SECOND_HARD_CFG, build_point_pillar,
                                             build_second)
    with open(os.path.join(GOLDEN, "ref_hard_voxel_manifest.json")) as f:
        manifest = json.load(f)
    pp = build_point_pillar(POINT_PILLAR_HARD_CFG)
    assert [type(m).__name__ for m in pp.module_list] == ['PillarVFE', 'PointPillarScatter', 'BaseBEVBackbone', 'AnchorHeadSingle']
    assert {k: list(v.shape) for k, v in pp.vfe.state_dict().items()} == manifest['PillarVFE(h1.m2000.c4)']
    assert pp.vfe.get_output_feature_dim() == 64 and pp.vfe.grid_size == [432, 496, 1]
    second = build_second(SECOND_HARD_CFG)
    assert [type(m).__name__ for m in second.module_list] == ['MeanVFE', 'VoxelBackBone8x', 'HeightCompression', 'BaseBEVBackbone', 'AnchorHeadSingle']
    assert {k: list(v.shape) for k, v in second.vfe.state_dict().items()} == manifest['MeanVFE'] == {}
    assert second.vfe.get_output_feature_dim() == 4
    caps = {'train': 16000, 'test': 40000}
    assert POINT_PILLAR_HARD_CFG['VFE']['MAX_POINTS_PER_VOXEL'] == 32 and POINT_PILLAR_HARD_CFG['VFE']['MAX_NUMBER_OF_VOXELS'] == caps
    assert SECOND_HARD_CFG['VFE']['MAX_POINTS_PER_VOXEL'] == 5 and SECOND_HARD_CFG['VFE']['MAX_NUMBER_OF_VOXELS'] == caps
    for hard, soft in ((POINT_PILLAR_HARD_CFG, POINT_PILLAR_CFG), (SECOND_HARD_CFG, SECOND_CFG)):
        assert {k: v for k, v in hard.items() if k != 'VFE'} == {k: v for k, v in soft.items() if k != 'VFE'}
    # the same state_dict keys as the dynamic encoder: a PointPillars checkpoint loads into either
    assert set(pp.vfe.state_dict()) == set(build_point_pillar().vfe.state_dict())


def test_voxelizer_caps_come_from_the_module_s_config():
    from pdm_ssd_amd.config import cfg_from_dict
    from pdm_ssd_amd.vfe.mean_vfe import voxelizer_caps
    cfg = cfg_from_dict({'MAX_POINTS_PER_VOXEL': 5, 'MAX_NUMBER_OF_VOXELS': {'train': 16000, 'test': 40000}})
    assert voxelizer_caps(cfg, True, 'x') == (5, 16000) and voxelizer_caps(cfg, False, 'x') == (5, 40000)
    assert voxelizer_caps({'MAX_POINTS_PER_VOXEL': 32, 'MAX_NUMBER_OF_VOXELS': 100}, True, 'x') == (32, 100)
    with pytest.raises(ValueError, match='MAX_POINTS_PER_VOXEL'):
        voxelizer_caps({'MAX_NUMBER_OF_VOXELS': 100}, False, 'x')
    with pytest.raises(ValueError, match='MAX_NUMBER_OF_VOXELS'):
        voxelizer_caps({'MAX_POINTS_PER_VOXEL': 5}, False, 'x')


@pytest.mark.parametrize("name", ['HardMeanVFE', 'HardPillarVFE'])
def test_a_missing_max_points_per_voxel_raises_and_names_the_key(name):
    """no `voxels` in the batch and no MAX_POINTS_PER_VOXEL in the config: refused before anything touches the device"""
    from pdm_ssd_amd import vfe
    cfg = {'USE_NORM': True, 'WITH_DISTANCE': False, 'USE_ABSLOTE_XYZ': True, 'NUM_FILTERS': [64], 'MAX_NUMBER_OF_VOXELS': 100}
    module = vfe.__all__[name](model_cfg=cfg, num_point_features=4, voxel_size=[0.5, 0.5, 4], grid_size=[40, 24, 1],
                               point_cloud_range=[0, -6, -3, 20, 6, 1]).eval()
    with pytest.raises(ValueError, match='MAX_POINTS_PER_VOXEL'):
        module({'points': None, 'batch_size': 1})


def test_entry_points_validate_their_arguments_before_any_launch():
    from pdm_ssd_amd import _native
    lib = _native.lib()
    buf = (C.c_int * 64)()
    p = C.cast(buf, C.c_void_p)
    limit = lib.pdm_hard_voxel_max_points()
    assert limit >= 64
    need = lib.pdm_hard_voxelize_workspace_bytes(1000, 2, 40, 24, 1)
    assert need > 0 and need % 256 == 0
    assert lib.pdm_hard_voxelize_workspace_bytes(1000, 32, 1408, 1600, 40) > 0           # 2.9e9 cells: 64-bit keys
    assert lib.pdm_hard_voxelize_workspace_bytes(1000, 2, 40, 24, 1 << 30) == 0 and lib.pdm_hard_voxelize_workspace_bytes(-1, 2, 40, 24, 1) == 0

    def voxelize(N=10, C1=5, B=2, nx=40, ny=24, nz=1, T=8, max_voxels=50, points=p, slot_rows=p, record=p, ws=p, ws_bytes=1 << 30, vz=4.0):
        _native.call("pdm_hard_voxelize", 0, N, C1, points, B, nx, ny, nz, 0.0, 0.0, 0.0, 0.5, 0.5, vz, T, max_voxels, slot_rows, p, p, None,
                     record, ws, ws_bytes)
    for kw, msg in ((dict(T=0), "points per voxel"), (dict(T=limit + 1), "points per voxel"), (dict(max_voxels=0), "max_voxels"),
                    (dict(nz=1 << 30), "2\\^35 cells"), (dict(ws_bytes=need - 1, N=1000), "workspace too small"), (dict(points=None), "null pointer"),
                    (dict(slot_rows=None), "null pointer"), (dict(record=None), "null pointer"), (dict(ws=None), "null pointer"),
                    (dict(N=-1), "bad size"), (dict(C1=3), "bad size"), (dict(vz=0.0), "voxel size"),
                    (dict(ws=C.c_void_p(C.addressof(buf) + 4)), "8-byte aligned")):
        with pytest.raises(_native.NativeLibraryError, match=msg):
            voxelize(**kw)

    def slots(name, *tail, M=4, T=8, C1=5):
        _native.call(name, 0, M, *tail[:1], T, C1, *tail[1:]) if name == "pdm_hard_pillar_pfn" else _native.call(name, 0, M, T, C1, *tail)
    for name, tail in (("pdm_hard_voxel_materialize", (p, p, p)), ("pdm_hard_voxel_mean", (p, p, p, p)),
                       ("pdm_hard_pillar_pfn", (64, p, p, p, p, 1, 0, 0.5, 0.5, 4.0, 0.25, 0.25, -1.0, p, p, p, p))):
        for kw, msg in ((dict(T=0), "points per voxel"), (dict(T=limit + 1), "points per voxel"), (dict(M=-1), "bad size")):
            with pytest.raises(_native.NativeLibraryError, match=msg):
                slots(name, *tail, **kw)
        nulls = tuple(None if x is p else x for x in tail)
        with pytest.raises(_native.NativeLibraryError, match="null pointer"):
            slots(name, *nulls)
        slots(name, *nulls, M=0)            # nothing to do: no pointer is needed and nothing is launched
    with pytest.raises(_native.NativeLibraryError, match="feature columns"):
        slots("pdm_hard_pillar_pfn", 64, p, p, p, p, 1, 1, 0.5, 0.5, 4.0, 0.25, 0.25, -1.0, p, p, p, p, C1=12)

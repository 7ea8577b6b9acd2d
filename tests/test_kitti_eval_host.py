"""KITTI evaluation, host side (no GPU): the plain restatement (tests/kitti_eval_reference.py) reproduces the fixture made
by the reference's own evaluator (tests/golden/ref_kitti_eval.npz); the tables, get_thresholds and the mAP sums of
pdm_ssd_amd.kitti_eval; the C ABI of the new entry points."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

import kitti_eval_reference as kr
from pdm_ssd_amd import _native
from pdm_ssd_amd import kitti_eval as ke

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden')
CLASSES = ['Car', 'Pedestrian', 'Cyclist']
NEW_SYMBOLS = ['pdm_kitti_boxes_to_camera', 'pdm_kitti_eval_overlaps', 'pdm_kitti_eval_dt_flags', 'pdm_kitti_eval_workspace_bytes',
               'pdm_kitti_eval_pass1', 'pdm_kitti_eval_pass2']


@pytest.fixture(scope='module')
def fixture():
    z, gts, dts = kr.load_fixture(os.path.join(GOLDEN, 'ref_kitti_eval.npz'))
    with open(os.path.join(GOLDEN, 'ref_kitti_eval.json')) as fh:
        j = json.load(fh)
    return z, gts, dts, j


@pytest.fixture(scope='module')
def restated(fixture):
    z, gts, dts, _ = fixture
    detail = {}
    text, ret, maps, rets = kr.official_result(gts, dts, CLASSES, overlaps=kr.fixture_overlaps(z), detail=detail)
    return text, ret, maps, rets, detail


def test_restatement_reproduces_flags_thresholds_and_counts(fixture, restated):
    z, detail = fixture[0], restated[4]
    for t in range(54):
        mi, c, d, k = t // 18, (t // 6) % 3, (t // 2) % 3, t % 2
        n = z['num_thresholds'][t]
        thr, pr = detail[mi][('thresholds', c, d, k)], detail[mi][('pr', c, d, k)]
        assert len(thr) == n and np.array_equal(thr, z['thresholds'][t, :n]), t
        assert np.array_equal(pr[:, :3], z['pr'][t, :n, :3]), t            # tp, fp, fn exactly
        if mi == 0:
            assert np.allclose(pr[:, 3], z['pr'][t, :n, 3], rtol=1e-9, atol=0), t
        ign_gt, ign_dt, valid = detail[mi][('flags', c, d)]
        assert np.array_equal(ign_gt, z['ign_gt'][c * 3 + d]) and np.array_equal(ign_dt, z['ign_dt'][c * 3 + d])
        assert valid == z['valid_gt'][t]


def test_restatement_reproduces_curves_maps_and_text(fixture, restated):
    z, _, _, j = fixture
    text, ret, maps, rets, _ = restated
    for mi in range(3):
        assert np.array_equal(rets[mi]['precision'], z['precision'][mi]) and np.array_equal(rets[mi]['recall'], z['recall'][mi])
    assert np.allclose(rets[0]['orientation'], z['orientation'], rtol=1e-9, atol=0)
    for got, key in zip(maps, ('mAP_bbox', 'mAP_bev', 'mAP_3d', 'mAP_aos', 'mAP_bbox_R40', 'mAP_bev_R40', 'mAP_3d_R40', 'mAP_aos_R40')):
        if 'aos' in key:
            assert np.allclose(got, z[key], rtol=1e-9, atol=0), key
        else:
            assert np.array_equal(got, z[key]), key
    assert text == j['result']
    assert set(ret) == set(j['ret_dict'])
    for k, v in j['ret_dict'].items():
        assert np.isclose(ret[k], v, rtol=1e-9, atol=0), k


def test_restatement_with_its_own_float64_overlaps_decides_the_same(fixture, restated):
    """the fixture's margin (1e-3) covers the difference between the reference's fp32 rotated overlap and a float64 clip"""
    z, gts, dts, _ = fixture
    worst = 0.0
    for m, key in enumerate(('overlaps_bbox', 'overlaps_bev', 'overlaps_3d')):
        mine = np.concatenate([kr.frame_overlaps(g, d, m).ravel() for g, d in zip(gts, dts)])
        diff = np.abs(mine - z[key]).max()
        worst = max(worst, diff)
        assert diff < (1e-12 if m == 0 else float(z['margin'])), (key, diff)
    detail = {}
    kr.official_result(gts, dts, CLASSES, detail=detail)
    for t in range(54):
        mi, c, d, k = t // 18, (t // 6) % 3, (t // 2) % 3, t % 2
        n = z['num_thresholds'][t]
        assert np.array_equal(detail[mi][('pr', c, d, k)][:, :3], z['pr'][t, :n, :3]), t


def test_restated_conversion_is_close_to_the_reference(fixture):
    z = fixture[0]
    k = 0
    for f in range(len(z['pred_count'])):
        n = int(z['pred_count'][f])
        cam, img, alpha = kr.boxes_to_camera(z['pred_boxes'][f, :n], z['V2C'][f], z['R0'][f], z['P2'][f], z['image_shape'][f])
        want = np.concatenate([z['dt_location'][k:k + n], z['dt_dimensions'][k:k + n], z['dt_rotation_y'][k:k + n, None]], 1)
        assert np.abs(cam - want).max(initial=0) < 1e-4 and np.abs(img - z['dt_bbox'][k:k + n]).max(initial=0) < 1e-2
        assert np.abs(alpha - z['dt_alpha'][k:k + n]).max(initial=0) < 1e-5
        k += n


def test_fixture_covers_the_required_cases(fixture):
    z, gts, dts, _ = fixture
    assert len(gts) == 60 and any(len(g['name']) == 0 and len(d['name']) for g, d in zip(gts, dts))
    assert any(len(g['name']) and not len(d['name']) for g, d in zip(gts, dts))
    assert any(len(g['name']) == 0 and len(d['name']) == 0 for g, d in zip(gts, dts))
    assert z['num_thresholds'].min() >= 10 and (z['pr'][np.arange(54), z['num_thresholds'] - 1, :3] > 0).all()
    for key in ('mAP_bbox_R40', 'mAP_bev_R40', 'mAP_3d_R40'):
        assert (z[key] > 5).all() and (z[key] < 95).all()
    for name in ('Van', 'Person_sitting', 'DontCare'):
        assert (z['gt_name'] == name).sum() > 3
    for key in ('overlaps_bbox', 'overlaps_bev', 'overlaps_3d'):
        assert min(np.abs(z[key] - th).min() for th in (0.25, 0.5, 0.7)) >= float(z['margin'])


def test_tables_and_flags(fixture):
    z = fixture[0]
    assert ke.CLASS_NAMES == kr.CLASS_NAMES and ke.MIN_HEIGHT == (40, 25, 25) and ke.MAX_OCCLUSION == (0, 1, 2)
    assert ke.MAX_TRUNCATION == (0.15, 0.3, 0.5)
    assert np.array_equal(ke.official_min_overlaps(), kr.MIN_OVERLAPS)
    ids = ke.name_ids(['Car', 'car', 'Pedestrian', 'Cyclist', 'Van', 'Person_sitting', 'Truck', 'DontCare', 'dontcare', 'Tram', 'Misc'])
    assert ids.tolist() == [0, 0, 1, 2, 3, 4, 5, 6, 7, 7, 7]
    flags = ke.gt_ignore_flags(ke.name_ids(z['gt_name']), z['gt_bbox'], z['gt_occluded'], z['gt_truncated'], [0, 1, 2], [0, 1, 2])
    assert flags.dtype == np.int8 and np.array_equal(flags, z['ign_gt'])
    # the boundary cases of clean_data: > on occlusion / truncation, <= on the height
    names = ke.name_ids(['Car'] * 4)
    bbox = np.array([[0, 0, 10, 40.0], [0, 0, 10, 40.5], [0, 0, 10, 25.0], [0, 0, 10, 90.0]])
    f = ke.gt_ignore_flags(names, bbox, np.array([0., 0, 0, 1]), np.array([0.15, 0.16, 0.0, 0.3]), [0], [0, 1, 2])
    assert f.tolist() == [[1, 1, 1, 1], [0, 0, 1, 0], [0, 0, 1, 0]]


def test_get_thresholds_on_hand_made_lists():
    for fn in (ke.get_thresholds, kr.get_thresholds):
        assert list(fn(np.array([]), 5)) == []
        assert list(fn(np.array([0.7]), 1)) == [0.7]
        assert list(fn(np.array([0.7]), 4)) == [0.7]
        # ties: every recall level a tied score reaches repeats it
        assert list(fn(np.array([0.5, 0.9, 0.5, 0.5]), 4)) == [0.9, 0.5, 0.5, 0.5]
        # more true positives than sample points: at most 41 thresholds, descending, the first and the last score among them
        s = np.linspace(0.01, 0.99, 200)
        t = list(fn(s.copy(), 200))
        assert len(t) == 41 and t == sorted(t, reverse=True) and t[0] == s[-1] and t[-1] == s[0]
        # 10 of 20 found: recall stops at 0.5 -> 21 levels
        assert len(fn(np.linspace(0.1, 1, 10), 20)) == 10
    rng = np.random.default_rng(0)
    for n, g in ((3, 3), (57, 80), (300, 310)):
        s = np.round(rng.uniform(0, 1, n), 2)
        assert list(ke.get_thresholds(s.copy(), g)) == list(kr.get_thresholds(s.copy(), g))


def test_map_sums_on_known_curves():
    ones = np.ones((2, 41))
    assert np.allclose(ke.get_mAP(ones), 100) and np.allclose(ke.get_mAP_R40(ones), 100)
    step = np.zeros(41)
    step[:21] = 1.0          # precision 1 up to recall 0.5
    assert np.isclose(ke.get_mAP(step), 6 / 11 * 100) and np.isclose(ke.get_mAP_R40(step), 20 / 40 * 100)
    ramp = np.linspace(1, 0, 41)
    assert ke.get_mAP(ramp) == kr.get_mAP(ramp) and ke.get_mAP_R40(ramp) == kr.get_mAP_R40(ramp)


def test_result_text_and_keys_from_known_maps(fixture):
    z, _, _, j = fixture
    maps = [z[k] for k in ('mAP_bbox', 'mAP_bev', 'mAP_3d', 'mAP_aos', 'mAP_bbox_R40', 'mAP_bev_R40', 'mAP_3d_R40', 'mAP_aos_R40')]
    text, ret = ke.format_result([0, 1, 2], ke.official_min_overlaps()[:, :, [0, 1, 2]], maps, True)
    assert text == j['result'] and {k: float(v) for k, v in ret.items()} == j['ret_dict']
    text, ret = ke.format_result([0], ke.official_min_overlaps()[:, :, [0]], maps, False)
    assert 'aos' not in text and sorted(ret) == sorted('Car_%s/%s_R40' % (a, b) for a in ('3d', 'bev', 'image') for b in ('easy', 'moderate', 'hard'))


def test_new_symbols_are_declared_bound_and_exported():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, 'include', 'pdmssd_hip.h')).read(), flags=re.S)
    raw = C.CDLL(_native.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in _native.EXPORTS and hasattr(raw, name), name
    assert 'kitti_eval.hip' in open(os.path.join(ROOT, 'pdm_ssd_amd', 'csrc', 'Makefile')).read()


def test_entry_points_refuse_bad_arguments_with_an_error_code():
    lib = _native.lib()
    buf = (C.c_double * 64)()
    p = C.cast(buf, C.c_void_p)
    m3, m_bad = C.cast((C.c_int * 3)(0, 1, 2), C.c_void_p), C.cast((C.c_int * 3)(0, 5, 2), C.c_void_p)
    assert lib.pdm_kitti_eval_workspace_bytes(-1, 54) == 0 and lib.pdm_kitti_eval_workspace_bytes(10, 5000) == 0
    assert lib.pdm_kitti_eval_workspace_bytes(3769, 54) == 128 * 54 * 64 * 32
    assert lib.pdm_kitti_eval_workspace_bytes(5, 54) == 5 * 54 * 64 * 32
    with pytest.raises(_native.NativeLibraryError, match="kitti_boxes_to_camera.*code -1"):
        _native.call("pdm_kitti_boxes_to_camera", 0, -1, 4, p, p, p, p, p, None, p, p, p)
    with pytest.raises(_native.NativeLibraryError, match="null pointer"):
        _native.call("pdm_kitti_boxes_to_camera", 0, 2, 4, p, None, p, p, p, None, p, p, p)
    with pytest.raises(_native.NativeLibraryError, match="metric 5"):
        _native.call("pdm_kitti_eval_overlaps", 0, 1, p, p, p, 4, 3, m_bad, p, p, p, p, p)
    with pytest.raises(_native.NativeLibraryError, match="code -2"):
        _native.call("pdm_kitti_eval_overlaps", 0, 1, p, p, p, 1 << 31, 3, m3, p, p, p, p, p)
    with pytest.raises(_native.NativeLibraryError, match="difficulty 3"):
        _native.call("pdm_kitti_eval_dt_flags", 0, 4, p, p, 3, m3, 1, C.cast((C.c_int * 1)(3), C.c_void_p), p)
    with pytest.raises(_native.NativeLibraryError, match="classes=9"):
        _native.call("pdm_kitti_eval_dt_flags", 0, 4, p, p, 9, m3, 3, m3, p)
    pass1 = lambda max_dt, K: _native.call("pdm_kitti_eval_pass1", 0, 1, p, p, p, max_dt, 3, m3, 3, 3, K, p, 4, p, 2, p, 2, p, p, p, 2, p)
    with pytest.raises(_native.NativeLibraryError, match="code -2"):
        pass1(5000, 2)
    with pytest.raises(_native.NativeLibraryError, match="combinations"):
        pass1(10, 100)
    pass2 = lambda ws_bytes, max_dt=10: _native.call("pdm_kitti_eval_pass2", 0, 1, p, p, p, max_dt, 3, m3, 3, 3, 2, p, 4, p, 2, p, 2, p, p, p, p,
                                                     p, p, p, p, p, 1, p, ws_bytes, p)
    with pytest.raises(_native.NativeLibraryError, match="workspace 16 < "):
        pass2(16)
    with pytest.raises(_native.NativeLibraryError, match="code -2"):
        pass2(1 << 20, max_dt=4097)
    # no frames, no work: nothing is launched and nothing is an error
    _native.call("pdm_kitti_eval_overlaps", 0, 0, None, None, None, 0, 3, m3, None, None, None, None, None)
    _native.call("pdm_kitti_eval_dt_flags", 0, 0, None, None, 3, m3, 3, m3, None)
    _native.call("pdm_kitti_boxes_to_camera", 0, 0, 8, None, None, None, None, None, None, None, None, None)

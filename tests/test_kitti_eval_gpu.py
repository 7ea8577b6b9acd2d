"""KITTI evaluation on the device (pdm_ssd_amd/kitti_eval.py, csrc/kitti_eval.hip) against the fixture produced by the
reference's own evaluator and conversion code (tests/golden/ref_kitti_eval.npz, gen_kitti_eval_fixtures.py) and against the
plain restatement (tests/kitti_eval_reference.py) beyond it.

Measured on an MI355X (max over the fixture's 9379 within-frame pairs / 734 detections):
  BEV overlap |device - fixture| = 0 and 3D overlap = 0: the kernel restates rotate_iou.py's fp32 operations one rounding
  at a time, and the fixture's overlaps were computed in exactly that arithmetic (numpy float32 scalars);
  camera box 1.907e-06 m, image box 1.221e-04 px, alpha 2.384e-07 rad (fp32 products summed in another order than BLAS).
The bounds asserted are the fixture's margin / 10 (no decision of the fixture can flip) and 4 x the measured value."""
import json
import os

import numpy as np
import pytest
import torch

import kitti_eval_reference as kr
from pdm_ssd_amd import kitti_eval as ke

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
CLASSES = ['Car', 'Pedestrian', 'Cyclist']
MEASURED_BEV = 0.0
MEASURED_3D = 0.0
MEASURED_CAM = 1.907e-06
MEASURED_IMG = 1.221e-04
MEASURED_ALPHA = 2.384e-07


def guard(measured):
    """regression bound: 4 x the value measured on the device (a measured 0 leaves room for one fp32 / fp64 ulp of 1)"""
    return max(4 * measured, 1e-15)


@pytest.fixture(scope='module')
def fixture():
    z, gts, dts = kr.load_fixture(os.path.join(GOLDEN, 'ref_kitti_eval.npz'))
    with open(os.path.join(GOLDEN, 'ref_kitti_eval.json')) as fh:
        j = json.load(fh)
    return z, gts, dts, j


@pytest.fixture(scope='module')
def device_run(fixture, dev):
    z, gts, dts, j = fixture
    keep, stats = {}, {}
    text, ret = ke.get_official_eval_result(gts, dts, CLASSES, device=dev, keep=keep, stats=stats)
    return text, ret, keep, stats


def padded_of(z, dev, frames=None):
    sel = slice(None) if frames is None else frames
    padded = {'boxes': torch.from_numpy(z['pred_boxes'][sel]).to(dev), 'scores': torch.from_numpy(z['pred_scores'][sel]).to(dev),
              'labels': torch.from_numpy(z['pred_labels'][sel]).to(dev), 'count': torch.from_numpy(z['pred_count'][sel]).to(dev)}
    calib = {'V2C': torch.from_numpy(z['V2C'][sel]).to(dev), 'R0': torch.from_numpy(z['R0'][sel]).to(dev),
             'P2': torch.from_numpy(z['P2'][sel]).to(dev)}
    return padded, calib, torch.from_numpy(z['image_shape'][sel]).to(dev)


def counts_equal(keep, z):
    sums = keep['sums'].reshape(54, 41, 4)
    assert np.array_equal(keep['num_thresholds'].reshape(54), z['num_thresholds'])
    assert np.array_equal(keep['thresholds'].reshape(54, 41), z['thresholds'])
    for t in range(54):
        n = z['num_thresholds'][t]
        assert np.array_equal(sums[t, :n, :3], z['pr'][t, :n, :3].astype(np.int64)), t


def test_overlaps_match_the_fixture(fixture, device_run):
    z = fixture[0]
    ov = device_run[2]['overlaps'].cpu().numpy()
    m = float(z['margin'])
    d_bbox = np.abs(ov[0] - z['overlaps_bbox']).max()
    d_bev = np.abs(ov[1] - z['overlaps_bev']).max()
    d_3d = np.abs(ov[2] - z['overlaps_3d']).max()
    print('overlap differences: bbox %.3e bev %.3e 3d %.3e over %d pairs' % (d_bbox, d_bev, d_3d, ov.shape[1]))
    assert d_bbox <= 1e-12
    assert d_bev < m / 10 and d_3d < m / 10
    assert d_bev <= guard(MEASURED_BEV) and d_3d <= guard(MEASURED_3D)


def test_flags_and_valid_counts_match_the_fixture(fixture, device_run):
    z, keep = fixture[0], device_run[2]
    assert np.array_equal(keep['ign_gt'], z['ign_gt'])
    assert np.array_equal(keep['ign_dt'].cpu().numpy(), z['ign_dt'])
    assert np.array_equal(np.repeat(np.tile(keep['total_valid'], 3), 2), z['valid_gt'])


def test_counts_thresholds_and_similarity_match_the_fixture(fixture, device_run):
    z, keep = fixture[0], device_run[2]
    counts_equal(keep, z)
    pr = keep['pr'].reshape(54, 41, 4)
    for t in range(18):        # the similarity is summed for the bbox metric only
        n = z['num_thresholds'][t]
        assert np.allclose(pr[t, :n, 3], z['pr'][t, :n, 3], rtol=1e-9, atol=0), t
    k = 0
    for t in range(54):        # pass 1: the same true-positive scores
        mi, cd, kk = t // 18, (t // 2) % 9, t % 2
        s = keep['tp_scores'][mi, kk, keep['cd_base'][cd]:keep['cd_base'][cd + 1]]
        assert np.array_equal(np.sort(s[~np.isnan(s)]), z['tp_scores'][k:k + z['tp_len'][t]]), t
        k += z['tp_len'][t]


def test_end_result_matches_the_fixture(fixture, device_run):
    z, _, _, j = fixture
    text, ret, keep, stats = device_run
    r = keep['ret']
    assert np.array_equal(r['precision'], z['precision']) and np.array_equal(r['recall'], z['recall'])
    assert np.allclose(r['orientation'][0], z['orientation'], rtol=1e-9, atol=0)
    maps = keep['maps']
    for got, key in zip(maps, ('mAP_bbox', 'mAP_bev', 'mAP_3d', 'mAP_aos', 'mAP_bbox_R40', 'mAP_bev_R40', 'mAP_3d_R40', 'mAP_aos_R40')):
        if 'aos' in key:
            assert np.allclose(got, z[key], rtol=1e-9, atol=0), key
        else:
            assert np.array_equal(got, z[key]), key
    want = j['result'].split('\n')
    have = text.split('\n')
    assert len(want) == len(have)
    for a, b in zip(have, want):
        if a.startswith('aos'):
            assert [abs(float(x) - float(y)) <= 0.011 for x, y in zip(a[8:].split(', '), b[8:].split(', '))] == [True] * 3
        else:
            assert a == b
    assert set(ret) == set(j['ret_dict'])
    for k_, v in j['ret_dict'].items():
        assert (np.isclose(ret[k_], v, rtol=1e-9, atol=0) if '_aos/' in k_ else ret[k_] == v), k_
    assert stats['reads'] == 2 and stats['launches'] == 3 + 1 + 1 + 2


def test_conversion_matches_the_reference_and_the_chain_gives_the_counts(fixture, dev):
    z, gts = fixture[0], fixture[1]
    padded, calib, shape = padded_of(z, dev)
    ev = ke.KittiEvaluator(CLASSES)
    cam, img, alpha = ev.add_batch(padded, calib, shape, frame_ids=list(range(len(gts))))
    live = (np.arange(z['pred_boxes'].shape[1])[None] < z['pred_count'][:, None])
    cam, img, alpha = cam.cpu().numpy(), img.cpu().numpy(), alpha.cpu().numpy()
    assert not cam[~live].any() and not img[~live].any() and not alpha[~live].any()
    want_cam = np.concatenate([z['dt_location'], z['dt_dimensions'], z['dt_rotation_y'][:, None]], 1)
    d_cam = np.abs(cam[live] - want_cam).max()
    d_img = np.abs(img[live] - z['dt_bbox']).max()
    d_alpha = np.abs(alpha[live] - z['dt_alpha']).max()
    print('conversion differences: camera box %.3e m, image box %.3e px, alpha %.3e rad' % (d_cam, d_img, d_alpha))
    assert d_cam <= guard(MEASURED_CAM) and d_img <= guard(MEASURED_IMG) and d_alpha <= guard(MEASURED_ALPHA)
    for lim in (25, 40):
        assert np.array_equal((img[live][:, 3] - img[live][:, 1]) < lim, (z['dt_bbox'][:, 3] - z['dt_bbox'][:, 1]) < lim)
    keep = {}
    text, ret = ev.evaluate(gts, keep=keep)
    counts_equal(keep, z)
    # the reference-format dicts
    annos = ev.annos()
    assert len(annos) == len(gts) and annos[3]['frame_id'] == 3
    empty = [a for a, n in zip(annos, z['pred_count']) if n == 0][0]
    assert empty['name'].shape == (0,) and empty['bbox'].shape == (0, 4) and empty['boxes_lidar'].shape == (0, 7)
    full = annos[0]
    n0 = int(z['pred_count'][0])
    assert list(full['name']) == list(z['dt_name'][:n0]) and full['bbox'].dtype == np.float32 and full['score'].dtype == np.float32
    assert full['location'].shape == (n0, 3) and full['dimensions'].shape == (n0, 3) and np.array_equal(full['boxes_lidar'], z['pred_boxes'][0, :n0])
    assert set(full) == {'name', 'truncated', 'occluded', 'alpha', 'bbox', 'dimensions', 'location', 'rotation_y', 'score',
                         'boxes_lidar', 'frame_id'}


def restated_counts(gts, dts):
    detail = {}
    kr.official_result(gts, dts, CLASSES, detail=detail)
    return detail


def assert_counts_equal_restatement(keep, detail, similarity=True):
    sums, nthr, thr = keep['sums'].reshape(54, 41, 4), keep['num_thresholds'].reshape(54), keep['thresholds'].reshape(54, 41)
    pr = keep['pr'].reshape(54, 41, 4)
    for t in range(54):
        mi, c, d, k = t // 18, (t // 6) % 3, (t // 2) % 3, t % 2
        want_thr, want = detail[mi][('thresholds', c, d, k)], detail[mi][('pr', c, d, k)]
        assert nthr[t] == len(want_thr) and np.array_equal(thr[t, :nthr[t]], want_thr), t
        assert np.array_equal(sums[t, :nthr[t], :3], want[:, :3].astype(np.int64)), t
        if similarity and mi == 0:
            assert np.allclose(pr[t, :nthr[t], 3], want[:, 3], rtol=1e-9, atol=0), t


def test_counts_equal_the_restatement_on_300_seeded_frames(dev):
    gts, dts = kr.synthetic_frames(7, 300, margin=1e-3)        # the no-fragile-decision rule, checked in float64
    keep = {}
    ke.get_official_eval_result(gts, dts, CLASSES, device=dev, keep=keep)
    assert_counts_equal_restatement(keep, restated_counts(gts, dts))


def test_two_runs_are_bit_equal(fixture, dev):
    z, gts, dts, _ = fixture
    a, b = {}, {}
    ta, _ = ke.get_official_eval_result(gts, dts, CLASSES, device=dev, keep=a)
    tb, _ = ke.get_official_eval_result(gts, dts, CLASSES, device=dev, keep=b)
    assert ta == tb and np.array_equal(a['sums'], b['sums'])           # similarity bits included
    assert torch.equal(a['overlaps'], b['overlaps']) and np.array_equal(a['tp_scores'], b['tp_scores'], equal_nan=True)


def test_empty_inputs(fixture, dev):
    text, ret = ke.get_official_eval_result([], [], CLASSES, device=dev)
    assert all(v == 0 for v in ret.values()) and 'aos' not in text and len(ret) == 27
    z, gts, dts, _ = fixture
    none = [ke.empty_prediction(0) for _ in gts]
    keep = {}
    text, ret = ke.get_official_eval_result(gts, none, CLASSES, device=dev, keep=keep)
    assert all(v == 0 for v in ret.values()) and 'aos' not in text and not keep['num_thresholds'].any()
    ev = ke.KittiEvaluator(CLASSES)
    padded, calib, shape = padded_of(z, dev)
    padded['count'] = torch.zeros_like(padded['count'])
    ev.add_batch(padded, calib, shape)
    text2, ret2 = ev.evaluate(gts)
    assert text2 == text and all(len(a['name']) == 0 for a in ev.annos())


def test_a_frame_with_more_detections_than_a_wave(dev):
    rng = np.random.default_rng(11)
    gt, dt = kr.synthetic_frames(11, 1, gt_range=(40, 41))
    gt, dt = gt[0], dt[0]
    # up to 500 detections: the frame's own ones and copies of them moved about, scores on a 0.01 grid; a copy with a
    # fragile overlap or image height is left out (the no-fragile-decision rule, in float64)
    n = len(dt['name'])
    pick = rng.integers(0, n, 700)
    pool = {k: v[pick].copy() for k, v in dt.items()}
    pool['location'] = pool['location'] + rng.normal(0, 0.4, (700, 3))
    pool['bbox'] = pool['bbox'] + rng.normal(0, 8, (700, 4))
    pool['score'] = np.round(rng.uniform(0.05, 1, 700), 2)
    ok = np.ones(700, bool)
    h = np.abs(pool['bbox'][:, 3] - pool['bbox'][:, 1])
    ok &= (np.abs(h - 25) >= 1e-3) & (np.abs(h - 40) >= 1e-3)
    for metric in range(3):
        ov = kr.frame_overlaps(gt, pool, metric)
        for th in (0.25, 0.5, 0.7):
            ok &= (np.abs(ov - th) >= 1e-3).all(1)
    rows = np.nonzero(ok)[0][:500 - n]
    assert len(rows) == 500 - n
    dt = {k: np.concatenate([dt[k], pool[k][rows]]) for k in dt}
    assert kr.frame_is_robust(gt, dt, 1e-3)
    more_g, more_d = kr.synthetic_frames(12, 6)
    gts, dts = [gt] + more_g, [dt] + more_d
    keep = {}
    ke.get_official_eval_result(gts, dts, CLASSES, device=dev, keep=keep)
    assert max(len(d['name']) for d in dts) == 500
    assert_counts_equal_restatement(keep, restated_counts(gts, dts))


def test_uneven_batches_equal_one_batch(fixture, dev):
    z, gts = fixture[0], fixture[1]
    F = len(gts)
    one = ke.KittiEvaluator(CLASSES)
    one.add_batch(*padded_of(z, dev))
    a = {}
    ta, ra = one.evaluate(gts, keep=a)
    many = ke.KittiEvaluator(CLASSES)
    for lo, hi in ((0, 1), (1, 8), (8, 37), (37, F)):
        padded, calib, shape = padded_of(z, dev, slice(lo, hi))
        if lo == 8:        # a batch with fewer slots per sample
            cut = int(z['pred_count'][lo:hi].max())
            padded = {k: (v[:, :cut].contiguous() if v.dim() > 1 else v) for k, v in padded.items()}
        many.add_batch(padded, calib, shape)
    b = {}
    tb, rb = many.evaluate(gts, keep=b)
    assert ta == tb and np.array_equal(a['sums'], b['sums']) and ra.keys() == rb.keys()
    assert one.stats['reads'] == 3 and many.stats['reads'] == 3


def test_add_batch_is_graph_capturable(fixture, dev):
    z, gts = fixture[0], fixture[1]
    padded, calib, shape = padded_of(z, dev)
    eager = ke.KittiEvaluator(CLASSES)
    eager.add_batch(padded, calib, shape)
    want = {}
    eager.evaluate(gts, keep=want)
    static = {k: torch.zeros_like(v) if k != 'labels' else torch.ones_like(v) for k, v in padded.items()}
    ev = ke.KittiEvaluator(CLASSES)
    ev.add_batch(static, calib, shape)        # warm-up
    ev.reset()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ev.add_batch(static, calib, shape)
    for k in static:
        static[k].copy_(padded[k])
    graph.replay()
    got = {}
    ev.evaluate(gts, keep=got)
    assert np.array_equal(got['sums'], want['sums'])


def test_the_call_stays_inside_its_workspace(fixture, dev):
    z, gts, dts, _ = fixture
    nbytes = ke.workspace_bytes(len(gts), 54)
    assert nbytes > 0
    ws = torch.full((nbytes + 256,), 0xA5, dtype=torch.uint8, device=dev)
    keep = {}
    ke.evaluate_device(ke._pack_annos(gts, False), ke._dt_to_device(ke._pack_annos(dts, True), dev), [0, 1, 2], [0, 1, 2], [0, 1, 2],
                       ke.official_min_overlaps()[:, :, [0, 1, 2]], compute_aos=1, workspace=ws[:nbytes + 0], keep=keep)
    torch.cuda.synchronize()
    assert bool((ws[nbytes:] == 0xA5).all())
    assert bool((ws[:nbytes] != 0xA5).any())
    counts_equal(keep, z)
    with pytest.raises(AssertionError):
        ke.evaluate_device(ke._pack_annos(gts, False), ke._dt_to_device(ke._pack_annos(dts, True), dev), [0, 1, 2], [0, 1, 2], [0, 1, 2],
                           ke.official_min_overlaps()[:, :, [0, 1, 2]], workspace=ws[:nbytes - 8])


def test_eval_class_has_the_reference_shapes(fixture, dev):
    z, gts, dts, _ = fixture
    ret = ke.eval_class(gts, dts, [0, 1, 2], [0, 1, 2], 2, ke.official_min_overlaps()[:, :, [0, 1, 2]], device=dev)
    assert ret['precision'].shape == (3, 3, 2, 41)
    assert np.array_equal(ret['precision'], z['precision'][2]) and np.array_equal(ret['recall'], z['recall'][2])
    ret = ke.eval_class(gts, dts, [1], [2, 0], 0, ke.official_min_overlaps()[:1, :, [1]], compute_aos=True, device=dev)
    assert ret['orientation'].shape == (1, 2, 1, 41)
    assert np.array_equal(ret['precision'][0, :, 0], z['precision'][0][1, [2, 0], 0])
    assert np.allclose(ret['orientation'][0, :, 0], z['orientation'][1, [2, 0], 0], rtol=1e-9, atol=0)

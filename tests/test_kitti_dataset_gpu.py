"""The device side of the KITTI dataset front end (pdm_ssd_amd/kitti_dataset.py, csrc/kitti_data.hip) against the
reference's own run on the synthetic tree (tests/golden/ref_kitti_data.*), float64 / float32 numpy restatements, and
the chain into the augmentor, the detector and the evaluator.

Compared exactly: every FOV decision the fixture does not mark fragile (and every decision at all against the float64
restatement in the device's operation order), num_points_in_gt of every object without a fragile point (the others may
differ by at most their fragile count), and the database: counts, offsets and points bit for bit on every object."""
import os
import pickle

import numpy as np
import pytest
import torch

import augment_reference as ar
import kitti_tree
from kitti_data_case import CLASS_NAMES, Case

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def case():
    return Case()


@pytest.fixture(scope='module')
def tree(case, tmp_path_factory):
    root = tmp_path_factory.mktemp('kitti')
    case.write_tree(root)
    return root


def dataset(tree, dev, split='train', infos=None):
    from pdm_ssd_amd import kitti_dataset as kd
    ds = kd.KittiDataset(tree, CLASS_NAMES, split=split, device=dev)
    if infos is not None:
        ds.infos = infos
    return ds


def upload_split(case, tree, dev, split):
    """the split's frames on the device, with the fixture's own boxes -> (ds, frames, clouds, (raw, counts, calib, shape))"""
    ds = dataset(tree, dev, split)
    frames = case.frames(split)
    clouds = [ds.get_lidar(f['idx']) for f in frames]
    calibs = [ds.get_calib(f['idx']) for f in frames]
    return ds, frames, clouds, calibs, ds._frames_to_device(clouds, calibs, [f['image_shape'] for f in frames])


def random_frames(seed, B, n_lo, n_hi, dev):
    """B seeded frames of n_lo..n_hi lidar-like points around the whole vehicle, a perturbed calibration each"""
    from pdm_ssd_amd import kitti_dataset as kd
    from pdm_ssd_amd.input_path import upload_raw
    from pdm_ssd_amd.kitti_eval import stack_calib
    rng = np.random.default_rng(seed)
    clouds, calibs, shapes = [], [], []
    for b in range(B):
        n = int(rng.integers(n_lo, n_hi + 1))
        r = rng.uniform(2.0, 80.0, n)
        a = rng.uniform(-np.pi, np.pi, n)
        clouds.append(np.stack([r * np.cos(a), r * np.sin(a), rng.uniform(-2.5, 1.5, n), rng.uniform(0, 1, n)], 1).astype(np.float32))
        p2, r0, v2c = kitti_tree.frame_calib(rng)
        calibs.append(kd.Calibration({'P2': p2.astype(np.float32), 'R0': r0.astype(np.float32), 'Tr_velo2cam': v2c.astype(np.float32)}))
        shapes.append(kitti_tree.IMAGE_SIZES[b % 3])
    raw, counts, _ = upload_raw(clouds, dev)
    shape = torch.tensor(shapes, dtype=torch.int32, device=dev)
    return clouds, calibs, shapes, (raw, counts, stack_calib(calibs, dev), shape)


def restated_flags(clouds, calibs, shapes):
    from pdm_ssd_amd import kitti_dataset as kd
    return [kd.fov_flag_numpy(c[:, :3], k, s) for c, k, s in zip(clouds, calibs, shapes)]


def check_crop(out, clouds, flags):
    """rows = the kept rows of every frame in input order; counts; flags"""
    want = np.concatenate([c[f] for c, f in zip(clouds, flags)])
    assert out['counts'].cpu().tolist() == [int(f.sum()) for f in flags]
    assert np.array_equal(out['rows'].cpu().numpy()[:len(want)], want)
    if 'flags' in out:
        assert np.array_equal(out['flags'].cpu().numpy().astype(bool), np.concatenate(flags))


@pytest.mark.parametrize('split', ['train', 'val'])
def test_fov_crop_equals_the_reference_off_the_fragile_points(case, tree, dev, split):
    from pdm_ssd_amd import kitti_dataset as kd
    ds, frames, clouds, calibs, (raw, counts, calib, shape) = upload_split(case, tree, dev, split)
    out = kd.fov_crop(raw, counts, calib, shape, flags=True)
    got = np.split(out['flags'].cpu().numpy().astype(bool), np.cumsum([len(c) for c in clouds])[:-1])
    for f, g in zip(frames, got):
        ok = ~f['fov_fragile']
        assert np.array_equal(g[ok], f['fov'][ok]), f['idx']
    check_crop(out, clouds, restated_flags(clouds, calibs, [f['image_shape'] for f in frames]))
    assert out['host_counts'] == out['counts'].cpu().tolist() and len(out['rows']) == sum(out['host_counts'])


def test_fov_crop_equals_float64_numpy_on_every_point_of_fifty_large_frames(dev):
    from pdm_ssd_amd import kitti_dataset as kd
    for part in range(5):
        clouds, calibs, shapes, (raw, counts, calib, shape) = random_frames(100 + part, 10, 100000, 130000, dev)
        flags = restated_flags(clouds, calibs, shapes)
        a = kd.fov_crop(raw, counts, calib, shape, flags=True)
        check_crop(a, clouds, flags)
        assert 0 < a['flags'].sum().item() < raw.shape[0]
        p = kd.fov_crop_padded(raw, counts, calib, shape, flags=True)
        n = sum(a['host_counts'])
        assert int(p['overflow'][0]) == 0 and torch.equal(p['counts'], a['counts']) and torch.equal(p['flags'], a['flags'])
        assert p['rows'].shape[0] == raw.shape[0] and torch.equal(p['rows'][:n], a['rows'])
        again = kd.fov_crop(raw, counts, calib, shape, flags=True)
        assert torch.equal(again['rows'], a['rows']) and torch.equal(again['flags'], a['flags'])


def test_fov_crop_one_frame_empty_result_zero_points_and_overflow(dev):
    from pdm_ssd_amd import kitti_dataset as kd
    clouds, calibs, shapes, (raw, counts, calib, shape) = random_frames(7, 1, 5000, 5000, dev)
    check_crop(kd.fov_crop(raw, counts, calib, shape, flags=True), clouds, restated_flags(clouds, calibs, shapes))
    behind = raw.clone()
    behind[:, 0] = -behind[:, 0].abs() - 1.0                       # everything behind the camera
    out = kd.fov_crop(behind, counts, calib, shape)
    assert out['host_counts'] == [0] and out['rows'].shape == (0, 4)
    # a frame of zero points between two others, five features per point
    clouds, calibs, shapes, _ = random_frames(8, 3, 3000, 4000, dev)
    clouds[1] = clouds[1][:0]
    clouds = [np.concatenate([c, c[:, 3:4] * 2], 1) for c in clouds]
    from pdm_ssd_amd.input_path import upload_raw
    from pdm_ssd_amd.kitti_eval import stack_calib
    raw, counts, _ = upload_raw(clouds, dev)
    shape = torch.tensor(shapes, dtype=torch.int32, device=dev)
    flags = restated_flags(clouds, calibs, shapes)
    out = kd.fov_crop(raw, counts, stack_calib(calibs, dev), shape, flags=True)
    check_crop(out, clouds, flags)
    assert out['host_counts'][1] == 0 and out['rows'].shape[1] == 5
    # a capacity one row short: the flag is set and nothing is written at or past it
    total = sum(out['host_counts'])
    buf = torch.full((total + 64, 5), 7.25, dtype=torch.float32, device=dev)
    p = kd.fov_crop_padded(raw, counts, stack_calib(calibs, dev), shape, capacity_rows=total - 1, out_rows=buf)
    assert int(p['overflow'][0]) == 1 and p['counts'].sum().item() == total
    assert (buf[total - 1:] == 7.25).all() and torch.equal(buf[:total - 1], out['rows'][:total - 1])


def membership(case, tree, dev, split):
    from pdm_ssd_amd import kitti_dataset as kd
    ds, frames, clouds, calibs, dev_frames = upload_split(case, tree, dev, split)
    boxes, box_count, centres = kd.pad_boxes([f['annos']['gt_boxes_lidar'] for f in frames], dev)
    return frames, clouds, kd.BoxMembership(*dev_frames, boxes, box_count), centres


@pytest.mark.parametrize('split', ['train', 'val'])
def test_num_points_in_gt_equals_the_reference(case, tree, dev, split):
    frames, clouds, m, _ = membership(case, tree, dev, split)
    got = m.num_points_in_gt.cpu().numpy()
    db = m.db_count.cpu().numpy()
    exact = loose = 0
    for k, (f, pts) in enumerate(zip(frames, clouds)):
        n = len(f['annos']['gt_boxes_lidar'])
        want = f['annos']['num_points_in_gt'][:n]
        assert (f['annos']['num_points_in_gt'][n:] == -1).all()
        for i in range(n):
            if f['object_fragile'][i] == 0:
                assert got[k, i] == want[i], (f['idx'], i)
                exact += 1
            else:
                assert abs(int(got[k, i]) - int(want[i])) <= f['object_fragile'][i], (f['idx'], i)
                loose += 1
            box = f['annos']['gt_boxes_lidar'][i].astype(np.float32)
            assert db[k, i] == int(ar.points_in_box_cpu(pts, box).sum()), (f['idx'], i)     # the margin rule, every point
        assert not got[k, n:].any() and not db[k, n:].any()
    assert exact > 10 * max(loose, 1)
    zero = [f for f in frames if f['idx'] == kitti_tree.CASES['zero_points']]
    if zero:
        k = [f['idx'] for f in frames].index(zero[0]['idx'])
        assert 0 in got[k, :len(zero[0]['annos']['gt_boxes_lidar'])].tolist()


def test_database_is_bit_equal_to_the_reference(case, tree, dev):
    frames, clouds, m, centres = membership(case, tree, dev, 'train')
    points, offsets, boxes = m.gather(centres)
    want_off = case.z['db_offsets']
    assert np.array_equal(offsets.cpu().numpy(), want_off) and offsets.dtype == torch.int64
    assert np.array_equal(points.cpu().numpy(), case.z['db_points'])
    assert m.totals.cpu().tolist() == [int(want_off[-1]), len(want_off) - 1]
    want_boxes = np.concatenate([f['annos']['gt_boxes_lidar'] for f in frames]).astype(np.float32)
    assert np.array_equal(boxes.cpu().numpy(), want_boxes)
    counts = np.concatenate([m.db_count.cpu().numpy()[k, :len(f['annos']['gt_boxes_lidar'])] for k, f in enumerate(frames)])
    assert np.array_equal(counts, np.diff(want_off))
    # a point inside two boxes went to both: the overlapping pair shares points
    k = [f['idx'] for f in frames].index(kitti_tree.CASES['overlapping'])
    bx = frames[k]['annos']['gt_boxes_lidar'].astype(np.float32)
    both = ar.points_in_box_cpu(clouds[k], bx[-1]) & ar.points_in_box_cpu(clouds[k], bx[-2])
    assert both.any()
    again = m.gather(centres)
    assert all(torch.equal(a, b) for a, b in zip(again, (points, offsets, boxes)))


def test_written_database_reads_back_as_the_built_one(case, tree, dev):
    from pdm_ssd_amd import augment
    infos = [case.info_of(f) for f in case.frames('train')]
    ds = dataset(tree, dev, 'train', infos)
    path = os.path.join(tree, 'kitti_infos_train.pkl')
    with open(path, 'wb') as f:
        pickle.dump(infos, f)
    written = ds.create_groundtruth_database(path, split='train', batch_frames=3)
    assert list(written.keys()) == case.meta['db']['classes']
    assert sorted(os.listdir(os.path.join(tree, 'gt_database'))) == case.meta['db']['files']
    for name, entries in case.meta['db']['infos'].items():
        assert [e['num_points_in_gt'] for e in written[name]] == [e['num_points_in_gt'] for e in entries]
    disk = augment.GTDatabase.from_reference_infos(tree, ['kitti_dbinfos_train.pkl'], CLASS_NAMES, None, 4, dev)
    built = ds.build_gt_database(infos, batch_frames=5)
    assert len(built) == len(disk) > 0
    for k in ('points', 'offsets', 'boxes'):
        assert torch.equal(getattr(built, k), getattr(disk, k)), k
    assert np.array_equal(built.class_ids, disk.class_ids)


def test_get_infos_counts_on_the_device(case, tree, dev):
    """the public path: files -> thread pool -> batches on the device -> info dicts"""
    ds = dataset(tree, dev, 'val')
    infos = ds.get_infos(num_workers=4, batch_frames=3)
    for info, f in zip(infos, case.frames('val')):
        a = info['annos']
        assert list(a.keys()) == case.meta['val']['anno_keys']
        got, want = a['num_points_in_gt'], f['annos']['num_points_in_gt']
        assert got.dtype == np.int32 and got.shape == want.shape
        n = len(a['gt_boxes_lidar'])
        assert (got[n:] == -1).all()
        if np.array_equal(a['gt_boxes_lidar'], f['annos']['gt_boxes_lidar']):     # the same BLAS bits as the fixture's machine
            assert (np.abs(got[:n] - want[:n]) <= f['object_fragile']).all(), f['idx']


def test_workspaces_are_sized_honestly(case, tree, dev):
    """each entry point with exactly *_workspace_bytes + 256 bytes: the patterned tail comes back untouched"""
    from pdm_ssd_amd import _native
    from pdm_ssd_amd import kitti_dataset as kd
    ds, frames, clouds, calibs, (raw, counts, calib, shape) = upload_split(case, tree, dev, 'train')
    B = len(frames)
    boxes, box_count, centres = kd.pad_boxes([f['annos']['gt_boxes_lidar'] for f in frames], dev)
    lib = _native.lib()
    n_fov = int(lib.pdm_kitti_data_fov_workspace_bytes(B))
    n_box = int(lib.pdm_kitti_data_boxes_workspace_bytes(B, boxes.shape[1]))
    assert n_fov > 0 and n_box > 0 and lib.pdm_kitti_data_fov_workspace_bytes(2000) == 0
    assert lib.pdm_kitti_data_boxes_workspace_bytes(B, 257) == 0

    def guarded(n):
        ws = torch.empty((n + 256,), dtype=torch.uint8, device=dev)
        ws[:n] = 0
        ws[n:] = 0xA5
        return ws
    ws = guarded(n_fov)
    ref = kd.fov_crop(raw, counts, calib, shape)
    out = kd.fov_crop(raw, counts, calib, shape, workspace=ws)             # fov_count + fov_fill
    torch.cuda.synchronize()
    assert (ws[n_fov:] == 0xA5).all() and torch.equal(out['rows'], ref['rows'])
    ws = guarded(n_box)
    m = kd.BoxMembership(raw, counts, calib, shape, boxes, box_count, workspace=ws)   # boxes_count
    got = m.gather(centres)                                                            # boxes_fill
    torch.cuda.synchronize()
    assert (ws[n_box:] == 0xA5).all()
    assert np.array_equal(got[0].cpu().numpy(), case.z['db_points'])
    with pytest.raises(_native.NativeLibraryError, match='workspace'):
        kd.fov_crop(raw, counts, calib, shape, workspace=ws[:n_fov - 1])


def test_crop_augment_sample_replays_from_a_graph(case, tree, dev):
    from pdm_ssd_amd import augment
    from pdm_ssd_amd import kitti_dataset as kd
    from pdm_ssd_amd.input_path import sample_points_batch
    ds, frames, clouds, calibs, (raw, counts, calib, shape) = upload_split(case, tree, dev, 'train')
    infos = [case.info_of(f) for f in frames]
    db = ds.build_gt_database(infos)
    groups = [f'{c}:3' for k, c in enumerate(CLASS_NAMES) if db.counts[k] > 0]
    cfg = [{'NAME': 'gt_sampling', 'SAMPLE_GROUPS': groups, 'REMOVE_EXTRA_WIDTH': [0.0, 0.0, 0.0]},
           {'NAME': 'random_world_flip', 'ALONG_AXIS_LIST': ['x']},
           {'NAME': 'random_world_rotation', 'WORLD_ROT_ANGLE': [-0.785, 0.785]}]
    batches = kd.KittiBatches(ds, len(frames), training=False)
    gt_host = [batches.frame_boxes(i)[1] for i in infos]
    M = max(len(b) for b in gt_host)
    gt = np.zeros((len(frames), M, 8), np.float32)
    for k, b in enumerate(gt_host):
        gt[k, :len(b)] = b
    gt = torch.from_numpy(gt).to(dev)
    aug = augment.BatchAugmentor(cfg, ds.cfg['POINT_CLOUD_RANGE'], CLASS_NAMES, database=db, seed=5)
    ref = augment.BatchAugmentor(cfg, ds.cfg['POINT_CLOUD_RANGE'], CLASS_NAMES, database=db, seed=5)
    cap = int(raw.shape[0]) + len(frames) * aug.K * 400
    ws = kd.fov_workspace(len(frames), dev)

    def chain(a):
        crop = kd.fov_crop_padded(raw, counts, calib, shape, workspace=ws)
        out = a.augment_padded(crop['rows'], crop['counts'], gt, cap)
        return crop, out, sample_points_batch(out['rows'], out['counts'], 1024, seed=9)
    chain(aug)                                   # warm-up (allocates the augmentor's workspace)
    chain(ref)
    ref.state.copy_(aug.state)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        crop, out, pts = chain(aug)
    for _ in range(2):
        g.replay()
        wcrop, want, wpts = chain(ref)
        torch.cuda.synchronize()
        assert torch.equal(aug.state, ref.state) and int(out['overflow'][0]) == 0 and int(crop['overflow'][0]) == 0
        assert torch.equal(crop['counts'], wcrop['counts']) and torch.equal(out['counts'], want['counts'])
        n = int(want['counts'].sum())
        assert torch.equal(out['rows'][:n], want['rows'][:n]) and torch.equal(out['boxes'], want['boxes'])
        assert torch.equal(pts, wpts)


def test_end_to_end_from_a_kitti_directory(case, tree, dev):
    """create_kitti_infos -> KittiBatches(training) + BatchAugmentor on the built database -> one training step;
    KittiBatches(evaluation) -> detector -> post_process_padded -> KittiEvaluator.  Random weights: only that the chain
    connects is checked."""
    from pdm_ssd_amd import augment, detectors, kitti_eval, post_process
    from pdm_ssd_amd import kitti_dataset as kd
    from pdm_ssd_amd.detector_config import build_pdm_ssd
    from test_detector_gpu import SMALL
    names = kd.create_kitti_infos(tree, class_names=CLASS_NAMES, device=dev, batch_frames=4)
    for s, p in names.items():
        with open(p, 'rb') as f:
            infos = pickle.load(f)
        want = {'train': 8, 'val': 8, 'trainval': 16, 'test': 3}[s]
        assert len(infos) == want and ('annos' in infos[0]) == (s != 'test')
    assert os.path.exists(os.path.join(tree, 'kitti_dbinfos_train.pkl'))
    train = kd.KittiDataset(tree, CLASS_NAMES, split='train', device=dev)
    assert len(train) == 8
    db = train.build_gt_database()
    groups = [f'{c}:2' for k, c in enumerate(CLASS_NAMES) if db.counts[k] > 0]
    cfg = [{'NAME': 'gt_sampling', 'SAMPLE_GROUPS': groups, 'REMOVE_EXTRA_WIDTH': [0.0, 0.0, 0.0]},
           {'NAME': 'random_world_flip', 'ALONG_AXIS_LIST': ['x']},
           {'NAME': 'random_world_scaling', 'WORLD_SCALE_RANGE': [0.95, 1.05]}]
    aug = augment.BatchAugmentor(cfg, train.cfg['POINT_CLOUD_RANGE'], CLASS_NAMES, database=db, seed=1)
    torch.manual_seed(1)
    model = build_pdm_ssd(SMALL).to(dev).train()
    seen = 0
    for batch in kd.KittiBatches(train, 2, training=True, augmentor=aug, num_points=2048, shuffle_seed=3):
        assert batch['points'].shape == (2 * 2048, 5) and batch['gt_boxes'].shape[2] == 8 and len(batch['frame_id']) == 2
        seen += 1
        if seen == 1:
            ret = detectors.model_fn_decorator()(model, {k: batch[k] for k in ('batch_size', 'points', 'gt_boxes')})
            assert torch.isfinite(ret.loss)
            ret.loss.backward()
            grads = [p.grad for p in model.parameters() if p.grad is not None]
            assert grads and all(torch.isfinite(g).all() for g in grads)
    assert seen == 4
    val = kd.KittiDataset(tree, CLASS_NAMES, split='val', device=dev)
    model = model.eval()
    with torch.no_grad():
        model.point_head.cls_layers[-1].bias.fill_(0.5)
    ev = kitti_eval.KittiEvaluator(CLASS_NAMES)
    post = dict(SMALL['POST_PROCESSING'])
    for batch in kd.KittiBatches(val, 4, training=False, num_points=2048):
        bd = {'batch_size': batch['batch_size'], 'points': batch['points']}
        with torch.no_grad():
            for module in model.module_list:
                bd = module(bd)
        padded = post_process.post_process_padded(bd, post, len(CLASS_NAMES))
        ev.add_batch(padded, batch['calib'], batch['image_shape'], frame_ids=batch['frame_id'])
    text, ret = ev.evaluate(val.gt_annos())
    assert isinstance(text, str) and 'Car' in text
    for c in CLASS_NAMES:
        for key in ('3d/easy_R40', '3d/moderate_R40', 'bev/hard_R40', 'image/easy_R40'):
            assert f'{c}_{key}' in ret, (c, key)

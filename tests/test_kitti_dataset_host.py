"""The host side of the KITTI dataset front end (pdm_ssd_amd/kitti_dataset.py) against the fixture the reference's own
dataset code produced on the synthetic tree (tests/golden/ref_kitti_data.npz / .json, gen_kitti_data_fixtures.py).  No GPU.

Bit-equal: every parsed field (calibration, labels, difficulty, image shapes, dimensions and heading of
gt_boxes_lidar), which both sides form with the same numpy conversions from the same text.  NOT bit-equal, and why: the
x, y, z of gt_boxes_lidar (and of boxes3d_kitti_camera_to_lidar) go through a float32 matrix product and a matrix
inverse in BLAS / LAPACK, whose summation order and fused multiply-adds depend on the CPU the library dispatches for.
They are held to 2e-4 m: a 4-term float32 dot product of coordinates up to 80 m carries at most
4 * 2^-24 * 4 * 80 = 8e-5 m, and the float32 inverse's relative error of about 1e-6 adds 8e-5 m at that range.
"""
import concurrent.futures as futures
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

from kitti_data_case import CLASS_NAMES, Case

XYZ_TOL = 2e-4


@pytest.fixture(scope='module')
def case():
    return Case()


@pytest.fixture(scope='module')
def tree(case, tmp_path_factory):
    root = tmp_path_factory.mktemp('kitti')
    case.write_tree(root)
    return root


def dataset(tree, split='train'):
    from pdm_ssd_amd import kitti_dataset as kd
    return kd.KittiDataset(tree, CLASS_NAMES, split=split, device='cpu')


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b)


@pytest.mark.parametrize('split', ['train', 'val', 'test'])
def test_info_fields_equal_the_reference(case, tree, split):
    ds = dataset(tree, split)
    assert ds.sample_id_list == case.meta[split]['frames']
    for want in case.frames(split):
        info, calib, points = ds._host_info(want['idx'], split != 'test', False)
        assert points is None
        keys = [k for k in case.meta[split]['keys']]
        assert list(info.keys()) == keys
        assert info['point_cloud'] == {'num_features': 4, 'lidar_idx': want['idx']}
        assert info['image']['image_idx'] == want['idx'] and same(info['image']['image_shape'], want['image_shape'])
        for k in ('P2', 'R0_rect', 'Tr_velo_to_cam'):
            assert same(info['calib'][k], want['calib'][k]), k
            assert str(info['calib'][k].dtype) == case.meta[split][f'calib_{k}_dtype']
        if split == 'test':
            assert 'annos' not in info
            continue
        a, w = info['annos'], want['annos']
        assert list(a.keys()) == [k for k in case.meta[split]['anno_keys'] if k != 'num_points_in_gt']
        assert list(a['name']) == list(w['name']) and a['name'].dtype.kind == 'U'
        for k in ('truncated', 'occluded', 'alpha', 'bbox', 'dimensions', 'location', 'rotation_y', 'score', 'difficulty', 'index'):
            assert same(a[k], w[k]), (want['idx'], k)
        g, wg = a['gt_boxes_lidar'], w['gt_boxes_lidar']
        assert g.dtype == wg.dtype == np.float64 and g.shape == wg.shape
        assert np.array_equal(g[:, 3:], wg[:, 3:])
        assert np.abs(g[:, :3] - wg[:, :3]).max(initial=0) <= XYZ_TOL
        assert np.array_equal(g[:, :3], g[:, :3].astype(np.float32))          # float32 values in a float64 row


def test_calibration_from_dict_and_round_trip(tree):
    from pdm_ssd_amd import kitti_dataset as kd
    c = kd.Calibration(os.path.join(tree, 'training', 'calib', '000004.txt'))
    assert c.P2.dtype == c.R0.dtype == c.V2C.dtype == np.float32 and c.P2.shape == (3, 4) and c.R0.shape == (3, 3)
    d = kd.Calibration({'P2': c.P2, 'R0': c.R0, 'Tr_velo2cam': c.V2C})
    rng = np.random.default_rng(0)
    p = np.stack([rng.uniform(2, 70, 200), rng.uniform(-30, 30, 200), rng.uniform(-2, 1, 200)], 1).astype(np.float32)
    rect = c.lidar_to_rect(p)
    assert rect.dtype == np.float32 and np.array_equal(rect, d.lidar_to_rect(p))
    assert np.abs(c.rect_to_lidar(rect) - p).max() <= 1e-3
    img, depth = c.rect_to_img(rect)
    assert img.shape == (200, 2) and np.abs(depth - rect[:, 2]).max() <= 1e-5
    corners = np.repeat(rect[:25, None], 8, 1).astype(np.float64)
    boxes, pts = c.corners3d_to_img_boxes(corners)
    assert boxes.shape == (25, 4) and pts.shape == (25, 8, 2)
    hom = np.concatenate([rect[:25].astype(np.float64), np.ones((25, 1))], 1) @ c.P2.T.astype(np.float64)
    want = hom[:, :2] / hom[:, 2:3]                       # this one divides by the homogeneous depth, not by rect z
    assert np.abs(boxes[:, :2] - want).max() <= 1e-9 and np.abs(boxes[:, 2:] - want).max() <= 1e-9


@pytest.mark.parametrize('split', ['train', 'val'])
def test_float64_fov_restatement_equals_the_reference_off_the_fragile_points(case, tree, split):
    """fov_flag_numpy is the operation order the device follows; the reference's float32 flags equal it on every
    point the fixture does not mark fragile"""
    from pdm_ssd_amd import kitti_dataset as kd
    ds = dataset(tree, split)
    kept = 0
    for want in case.frames(split):
        pts = ds.get_lidar(want['idx'])
        assert len(pts) == want['num_points']
        got = kd.fov_flag_numpy(pts[:, :3], ds.get_calib(want['idx']), want['image_shape'])
        ok = ~want['fov_fragile']
        assert np.array_equal(got[ok], want['fov'][ok]), want['idx']
        kept += int(got.sum())
    assert kept > 0


def test_label_levels_and_png_shapes(tree, tmp_path):
    from pdm_ssd_amd import kitti_dataset as kd
    assert kd.kitti_obj_level([0, 0, 10, 50], 0.0, 0) == 0 and kd.kitti_obj_level([0, 0, 10, 50], 0.2, 0) == 1
    assert kd.kitti_obj_level([0, 0, 10, 30], 0.4, 2) == 2 and kd.kitti_obj_level([0, 0, 10, 20], 0.0, 0) == -1
    assert kd.kitti_obj_level([0, 0, 10, 50], 0.0, 3) == -1
    import kitti_tree
    for h, w in kitti_tree.IMAGE_SIZES + [(1, 1), (3000, 17)]:
        p = tmp_path / f'{h}_{w}.png'
        kitti_tree.write_png(str(p), h, w)
        s = kd.image_shape(p)
        assert s.dtype == np.int32 and s.tolist() == [h, w]
    bad = tmp_path / 'bad.png'
    bad.write_bytes(b'not a png at all, but long enough to hold a header')
    with pytest.raises(ValueError):
        kd.image_shape(bad)
    assert kd.read_split(tree, 'nope') is None and kd.read_split(tree, 'trainval') == sorted(kd.read_split(tree, 'train') + kd.read_split(tree, 'val'))


def test_camera_to_lidar_boxes_and_the_class_column(case, tree):
    from pdm_ssd_amd import kitti_dataset as kd
    ds = dataset(tree, 'train')
    ds.infos = [case.info_of(f) for f in case.frames('train')]
    batches = kd.KittiBatches(ds, 4, training=False)
    seen = set()
    for info, want in zip(ds.infos, case.frames('train')):
        calib, boxes = batches.frame_boxes(info)
        names = [n for n in want['annos']['name'] if n != 'DontCare']
        assert boxes.dtype == np.float32 and boxes.shape == (len(names), 8)
        ref = want['annos']['gt_boxes_lidar']
        assert np.abs(boxes[:, :3] - ref[:, :3]).max(initial=0) <= XYZ_TOL
        assert np.abs(boxes[:, 3:7] - ref[:, 3:7]).max(initial=0) <= 1e-6      # float32 here (as __getitem__), float64 there
        for n, c in zip(names, boxes[:, 7]):
            assert c == (CLASS_NAMES.index(n) + 1 if n in CLASS_NAMES else -1)
            seen.add(n)
    assert {'Car', 'Pedestrian', 'Van'} <= seen
    assert kd.class_column(['Cyclist', 'Tram', 'Car'], CLASS_NAMES).tolist() == [3.0, -1.0, 1.0]


def test_written_pickles_load_without_this_package(case, tree, tmp_path):
    ds = dataset(tree, 'val')
    infos = [ds._host_info(i, True, False)[0] for i in ds.sample_id_list]
    path = tmp_path / 'kitti_infos_val.pkl'
    with open(path, 'wb') as f:
        pickle.dump(infos, f)
    code = ("import pickle, sys\n"
            "infos = pickle.load(open(sys.argv[1], 'rb'))\n"
            "assert not any(m.split('.')[0] in ('pdm_ssd_amd', 'torch') for m in sys.modules), 'needs more than numpy'\n"
            "print(len(infos), sorted(infos[0]['annos'])[0])\n")
    out = subprocess.run([sys.executable, '-c', code, str(path)], capture_output=True, text=True, cwd=str(tmp_path), check=True)
    assert out.stdout.split() == [str(len(infos)), 'alpha']


def test_db_infos_keys_order_and_files(case, tree, monkeypatch):
    """create_groundtruth_database's host half (names, keys, order, file contents) with the device result replaced by the
    reference's own database points; the device result itself is compared in the GPU tests"""
    from pdm_ssd_amd import augment
    from pdm_ssd_amd import kitti_dataset as kd
    ds = dataset(tree, 'train')
    infos = [case.info_of(f) for f in case.frames('train')]
    info_path = os.path.join(tree, 'kitti_infos_train.pkl')
    with open(info_path, 'wb') as f:
        pickle.dump(infos, f)
    monkeypatch.setattr(ds, '_database_batches', lambda infos, *a: iter([(infos, case.z['db_points'], case.z['db_offsets'])]))
    got = ds.create_groundtruth_database(info_path, split='train')
    with open(os.path.join(tree, 'kitti_dbinfos_train.pkl'), 'rb') as f:
        assert list(pickle.load(f).keys()) == list(got.keys())
    db = case.meta['db']
    assert sorted(os.listdir(os.path.join(tree, 'gt_database'))) == db['files']
    assert list(got.keys()) == db['classes']
    for name in db['classes']:
        assert len(got[name]) == len(db['infos'][name])
        for k, (e, w) in enumerate(zip(got[name], db['infos'][name])):
            assert list(e.keys()) == db['keys']
            assert {key: type(v).__name__ + (':' + str(v.dtype) if hasattr(v, 'dtype') else '') for key, v in e.items()} == \
                db[f'{name}_types']
            assert e['name'] == name and e['path'] == w['path'] and e['image_idx'] == w['image_idx'] and e['gt_idx'] == w['gt_idx']
            assert e['num_points_in_gt'] == w['num_points_in_gt'] and int(e['difficulty']) == w['difficulty']
            assert float(e['score']) == w['score']
            assert same(e['box3d_lidar'], case.z[f'db_{name}_box3d_lidar'][k]) and same(e['bbox'], case.z[f'db_{name}_bbox'][k])
    # and the files read back through the existing loader
    back = augment.GTDatabase.from_reference_infos(tree, ['kitti_dbinfos_train.pkl'], CLASS_NAMES, None, 4, 'cpu')
    assert len(back) == sum(len(db['infos'].get(c, [])) for c in CLASS_NAMES)
    first = got[CLASS_NAMES[0]][0]
    n = first['num_points_in_gt']
    assert np.array_equal(back.points[:n].numpy(), np.fromfile(os.path.join(tree, first['path']), np.float32).reshape(-1, 4))


def test_thread_pool_never_exceeds_sixteen(tree, monkeypatch):
    from pdm_ssd_amd import kitti_dataset as kd
    assert kd.MAX_WORKERS == 16 and kd.pool_size(64) == 16 and kd.pool_size(0) == 1 and kd.pool_size(4) == 4
    sizes = []
    real = futures.ThreadPoolExecutor

    def recording(max_workers=None, *a, **k):
        sizes.append(max_workers)
        return real(max_workers, *a, **k)
    monkeypatch.setattr(kd.futures, 'ThreadPoolExecutor', recording)
    ds = dataset(tree, 'test')
    infos = ds.get_infos(num_workers=10 ** 6, has_label=False, count_inside_pts=False)
    assert len(infos) == len(ds.sample_id_list) and sizes == [16]
    src = open(kd.__file__).read()
    assert 'cpu_count' not in src.replace('never sized by os.cpu_count()', '')


def test_entry_points_validate_their_arguments_before_any_launch():
    """no GPU is touched: the checks come first (and B = 0 is a no-op), so the binding table's arity is exercised here"""
    import ctypes as C

    from pdm_ssd_amd import _native
    lib = _native.lib()
    assert lib.pdm_kitti_data_fov_workspace_bytes(4) > 0 and lib.pdm_kitti_data_fov_workspace_bytes(1025) == 0
    assert lib.pdm_kitti_data_boxes_workspace_bytes(4, 256) > lib.pdm_kitti_data_boxes_workspace_bytes(4, 8) > 0
    assert lib.pdm_kitti_data_boxes_workspace_bytes(4, 257) == 0
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p)
    frames0 = (0, 4, 0, p, p, p, p, p, p)
    _native.call("pdm_kitti_data_fov_count", 0, *frames0, 0, p, p, None, p, 1 << 20)
    _native.call("pdm_kitti_data_fov_fill", 0, *frames0, 0, p, p, p, p, 1 << 20)
    _native.call("pdm_kitti_data_boxes_count", 0, *frames0, 8, p, p, p, p, p, p, 1 << 20)
    _native.call("pdm_kitti_data_boxes_fill", 0, *frames0, 8, p, p, p, p, p, p, 0, 0, p, p, p, p, 1 << 20)
    frames = (2, 4, 16, p, p, p, p, p, p)
    with pytest.raises(_native.NativeLibraryError, match="workspace"):
        _native.call("pdm_kitti_data_fov_count", 0, *frames, 0, p, p, None, p, 8)
    with pytest.raises(_native.NativeLibraryError, match="at most 256 boxes"):
        _native.call("pdm_kitti_data_boxes_count", 0, *frames, 300, p, p, p, p, p, p, 1 << 20)
    with pytest.raises(_native.NativeLibraryError, match="C=2"):
        _native.call("pdm_kitti_data_fov_fill", 0, 2, 2, 16, p, p, p, p, p, p, 0, p, p, p, p, 1 << 20)
    with pytest.raises(_native.NativeLibraryError, match="workspace"):
        _native.call("pdm_kitti_data_boxes_fill", 0, *frames, 8, p, p, p, p, p, p, 0, 0, p, p, p, p, 8)

"""Host-side checks of the batched augmentor (pdm_ssd_amd/augment.py, csrc/augment.hip): the numpy restatement
(tests/augment_reference.py) against the reference's own augmentation run (tests/golden/ref_augment.npz, written by
tests/golden/gen_augment_fixtures.py), the draw definitions, config parsing and the reference database reader.
No GPU is used."""
import os
import pickle

import numpy as np
import pytest

import augment_reference as ar

HERE = os.path.dirname(os.path.abspath(__file__))
FIX = os.path.join(HERE, 'golden', 'ref_augment.npz')
CLASS_NAMES = ['Car', 'Pedestrian', 'Cyclist']


def fixture():
    return dict(np.load(FIX))


def split(rows, counts):
    return np.split(rows, np.cumsum(counts)[:-1])


@pytest.mark.parametrize('key', ['A', 'B'])
def test_restatement_reproduces_the_reference_run(key):
    f = fixture()
    db = {'points': f[f'{key}_db_points'], 'offsets': f[f'{key}_db_offsets'], 'boxes': f[f'{key}_db_boxes']}
    groups = [tuple(g) for g in f[f'{key}_groups']]
    scenes = split(f['in_points'], f['in_counts'])
    want_pts = split(f[f'{key}_out_points'], f[f'{key}_out_counts'])
    want_box = split(f[f'{key}_out_boxes'], f[f'{key}_box_counts'])
    rejected = 0
    for b, pts in enumerate(scenes):
        rows, boxes, acc = ar.apply_scene(pts, f['in_boxes'][b], db, groups, f[f'{key}_sampled'][b], int(f[f'{key}_flip'][b]),
                                          f[f'{key}_angle'][b], f[f'{key}_scale'][b], list(f[f'{key}_ops']), f['pc_range'],
                                          f[f'{key}_extra'])
        rejected += int((f[f'{key}_sampled'][b] >= 0).sum()) - len(acc)
        assert rows.shape == want_pts[b].shape, (b, rows.shape, want_pts[b].shape)
        assert np.abs(rows - want_pts[b]).max(initial=0) <= 1e-5
        assert boxes.shape == want_box[b].shape
        assert np.array_equal(boxes[:, 7], want_box[b][:, 7])
        assert np.abs(boxes[:, :7] - want_box[b][:, :7]).max(initial=0) <= 1e-5
    assert rejected > 0                                   # the collision cases are exercised


def test_fixture_covers_the_required_cases():
    f = fixture()
    assert set(f['A_flip'].tolist()) == {0, 1} and f['B_scale_skipped'].all() and not f['A_scale_skipped'].any()
    assert (f['in_boxes'][..., 7] < 0).any()                               # a non-target box
    assert f['B_limit'] and not f['A_limit']
    # a short slice at an epoch end: Car (5 entries, 3 per scene) takes 3, then 2
    assert (f['A_sampled'][1, :3] >= 0).sum() == 2
    # points and boxes out of range are dropped
    assert f['A_out_counts'].sum() < f['in_counts'].sum() + 200


def test_permutation_is_a_bijection_per_epoch():
    for n in [1, 2, 3, 5, 17, 64, 100, 1000]:
        for e in range(3):
            kp = ar.perm_key(7, 1, e)
            p = [ar.perm(i, n, kp) for i in range(n)]
            assert sorted(p) == list(range(n))
    kp0, kp1 = ar.perm_key(7, 0, 0), ar.perm_key(7, 0, 1)
    assert [ar.perm(i, 100, kp0) for i in range(100)] != [ar.perm(i, 100, kp1) for i in range(100)]


def test_pointer_rule_short_slices_and_limit_whole_scene():
    B = 4
    gt = np.zeros((B, 3, 8), np.float32)
    gt[1, 0, 7] = 1           # scene 1 has one Car
    gt[2, :3, 7] = 1          # scene 2 has three: with LIMIT it draws nothing
    groups = [(0, 3, 5, 0), (1, 2, 4, 5)]
    st = ar.initial_state([5, 4])
    sampled, st2, walk = ar.schedule(st, groups, gt, limit=False, seed=1)
    assert [w[4] for w in walk if w[1] == 0] == [3, 2, 3, 2]      # short slice at every epoch end
    assert [w[2] for w in walk if w[1] == 0] == [0, 0, 1, 1]
    assert st2.tolist() == [1, 1, 6, 1, 4]                          # the pointer advances by sample_num regardless
    assert ((sampled[:, :3] >= 0) & (sampled[:, :3] < 5)).all(1).tolist() == [True, False, True, False]
    assert set(sampled[0, :3]) | set(sampled[1, :2]) == set(range(5))   # one epoch = every entry once
    sampled, st3, walk = ar.schedule(st, groups, gt, limit=True, seed=1)
    cars = [(w[0], w[4]) for w in walk if w[1] == 0]
    assert cars == [(0, 3), (1, 2), (3, 3)]                       # scene 1 asks for 2, scene 2 for 0 (skipped)
    assert (sampled[2, :3] == -1).all()
    assert st3[2] == 3 and st3[1] == 1


def test_scene_params_follow_the_documented_keys():
    flip, angle, scale = ar.scene_params(5, 0, 64, 3, (-0.5, 0.5), (0.9, 1.1))
    assert set(flip.tolist()) == {0, 1, 2, 3}
    assert (angle >= -0.5).all() and (angle <= 0.5).all() and (scale >= 0.9).all() and (scale <= 1.1).all()
    f2, a2, s2 = ar.scene_params(5, 1, 64, 3, (-0.5, 0.5), (0.9, 1.1))
    assert not np.array_equal(a2, angle)


def test_config_parsing_and_rejection():
    from pdm_ssd_amd import augment
    base = {'NAME': 'gt_sampling', 'SAMPLE_GROUPS': ['Car:20', 'Pedestrian:15', 'Cyclist:15', 'Truck:3'],
            'REMOVE_EXTRA_WIDTH': [0.0, 0.0, 0.0], 'LIMIT_WHOLE_SCENE': True}
    cfg = {'DISABLE_AUG_LIST': ['placeholder'],
           'AUG_CONFIG_LIST': [base, {'NAME': 'random_world_flip', 'ALONG_AXIS_LIST': ['x']},
                               {'NAME': 'random_world_rotation', 'WORLD_ROT_ANGLE': [-0.785, 0.785]},
                               {'NAME': 'random_world_scaling', 'WORLD_SCALE_RANGE': [0.95, 1.05]}]}
    plan = augment.parse_config(cfg, CLASS_NAMES)
    assert plan['sampling']['groups'] == [('Car', 20), ('Pedestrian', 15), ('Cyclist', 15)]
    assert plan['ops'] == [1, 3, 4] and plan['ops_code'] == 0x431 and plan['flip_axes'] == 1
    skipped = augment.parse_config([{'NAME': 'random_world_scaling', 'WORLD_SCALE_RANGE': [1.0, 1.0005]}], CLASS_NAMES)
    assert skipped['ops'] == [] and skipped['scale'] is None
    disabled = augment.parse_config(dict(cfg, DISABLE_AUG_LIST=['gt_sampling']), CLASS_NAMES)
    assert disabled['sampling'] is None
    for bad, word in [({'NAME': 'random_local_rotation'}, 'random_local_rotation'),
                      ({'NAME': 'random_world_frustum_dropout'}, 'random_world_frustum_dropout'),
                      ({'NAME': 'random_world_translation'}, 'random_world_translation'),
                      (dict(base, USE_ROAD_PLANE=True), 'USE_ROAD_PLANE'),
                      (dict(base, IMG_AUG_TYPE='by_depth'), 'IMG_AUG_TYPE'),
                      (dict(base, FILTER_OBJ_POINTS_BY_TIMESTAMP=True), 'FILTER_OBJ_POINTS_BY_TIMESTAMP'),
                      ({'NAME': 'random_world_flip', 'ALONG_AXIS_LIST': ['z']}, 'ALONG_AXIS_LIST')]:
        with pytest.raises(ValueError, match=word):
            augment.parse_config([bad], CLASS_NAMES)
    with pytest.raises(ValueError, match='gt_sampling'):
        augment.parse_config([{'NAME': 'random_world_flip', 'ALONG_AXIS_LIST': ['x']}, base], CLASS_NAMES)
    with pytest.raises(ValueError, match='GTDatabase'):
        augment.BatchAugmentor([base], [0, -40, -3, 70.4, 40, 1], CLASS_NAMES, database=None, device='cpu')


def test_gt_database_from_reference_infos(tmp_path):
    from pdm_ssd_amd import augment
    rng = np.random.default_rng(0)
    (tmp_path / 'gt_database').mkdir()
    infos = {'Car': [], 'Pedestrian': [], 'Van': []}
    want = {}
    for k, (name, n, diff, dt) in enumerate([('Car', 6, 0, np.float32), ('Car', 3, 0, np.float32), ('Pedestrian', 5, 2, np.float32),
                                             ('Pedestrian', 7, 0, np.float64), ('Car', 8, 1, np.float32), ('Van', 9, 0, np.float32)]):
        pts = rng.normal(size=(n, 4)).astype(dt)
        path = f'gt_database/{k}.bin'
        pts.tofile(str(tmp_path / path))
        box = rng.normal(size=7).astype(np.float32)
        infos[name].append({'name': name, 'path': path, 'box3d_lidar': box, 'num_points_in_gt': n, 'difficulty': diff})
        want[k] = (pts.astype(np.float32), box)
    with open(tmp_path / 'db.pkl', 'wb') as f:
        pickle.dump(infos, f)
    db = augment.GTDatabase.from_reference_infos(tmp_path, ['db.pkl'], ['Car', 'Pedestrian'],
                                                 {'filter_by_difficulty': [2], 'filter_by_min_points': ['Car:5']}, 4, 'cpu')
    # Car 1 (3 points) and Pedestrian 2 (difficulty 2) are filtered; Van is not a class; the float64 file is read as such
    assert db.counts.tolist() == [2, 1] and db.first.tolist() == [0, 2]
    expect = [0, 4, 3]
    assert db.offsets.tolist() == np.cumsum([0] + [want[k][0].shape[0] for k in expect]).tolist()
    assert np.array_equal(db.points.numpy(), np.concatenate([want[k][0] for k in expect]))
    assert np.array_equal(db.boxes.numpy(), np.stack([want[k][1] for k in expect]))
    assert db.class_ids.tolist() == [0, 0, 1]

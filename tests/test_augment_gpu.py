"""The batched device augmentor (pdm_ssd_amd/augment.py, csrc/augment.hip) against the reference's own augmentation run
(tests/golden/ref_augment.npz) and the numpy restatement (tests/augment_reference.py): exact counts, order, draws and
state; bit-equal rows and boxes with its own draws; overflow, graph replay and the training chain."""
import os

import numpy as np
import pytest
import torch

import augment_reference as ar

HERE = os.path.dirname(os.path.abspath(__file__))
FIX = os.path.join(HERE, 'golden', 'ref_augment.npz')
CLASS_NAMES = ['Car', 'Pedestrian', 'Cyclist']
RANGE = [0.0, -40.0, -3.0, 70.4, 40.0, 1.0]
SIZES = np.array([[3.9, 1.6, 1.56], [0.8, 0.6, 1.73], [1.76, 0.6, 1.73]], np.float32)


def split(rows, counts):
    return np.split(np.asarray(rows), np.cumsum(counts)[:-1])


def fixture_augmentor(f, key, dev):
    from pdm_ssd_amd import augment
    groups = [tuple(g) for g in f[f'{key}_groups']]
    names = {1: 'x', 2: 'y'}
    cfg = [{'NAME': 'gt_sampling', 'SAMPLE_GROUPS': [f'{CLASS_NAMES[c]}:{n}' for c, n in groups],
            'LIMIT_WHOLE_SCENE': bool(f[f'{key}_limit']), 'REMOVE_EXTRA_WIDTH': f[f'{key}_extra'].tolist()},
           {'NAME': 'random_world_flip', 'ALONG_AXIS_LIST': [names[o] for o in f[f'{key}_ops'] if o in names]},
           {'NAME': 'random_world_rotation', 'WORLD_ROT_ANGLE': [-0.5, 0.5]},
           {'NAME': 'random_world_scaling', 'WORLD_SCALE_RANGE': [0.95, 1.05] if 4 in f[f'{key}_ops'] else [1.0, 1.0]}]
    db = augment.GTDatabase.from_arrays(f[f'{key}_db_points'], f[f'{key}_db_offsets'], f[f'{key}_db_boxes'],
                                        f[f'{key}_db_class'], CLASS_NAMES, dev)
    return augment.BatchAugmentor(cfg, f['pc_range'].tolist(), CLASS_NAMES, database=db, seed=3)


def upload(f, dev):
    return (torch.from_numpy(f['in_points']).to(dev), torch.from_numpy(f['in_counts']).to(dev),
            torch.from_numpy(f['in_boxes']).to(dev))


@pytest.mark.gpu
@pytest.mark.parametrize('key', ['A', 'B'])
def test_device_output_equals_the_reference_run_with_its_draws(dev, key):
    f = dict(np.load(FIX))
    aug = fixture_augmentor(f, key, dev)
    raw, counts, gt = upload(f, dev)
    params = {'sampled': f[f'{key}_sampled'], 'flip': f[f'{key}_flip'], 'angle': f[f'{key}_angle'], 'scale': f[f'{key}_scale']}
    out = aug(raw, counts, gt, params=params)
    assert out['host_counts'] == f[f'{key}_out_counts'].tolist()
    assert out['box_counts'].cpu().tolist() == f[f'{key}_box_counts'].tolist()
    got = out['rows'].cpu().numpy()
    want = f[f'{key}_out_points']
    assert np.array_equal(got[:, 3:], want[:, 3:])                       # row order: the features ride along
    assert np.abs(got[:, :3] - want[:, :3]).max() <= 1e-5
    boxes = out['boxes'].cpu().numpy()
    for b, wb in enumerate(split(f[f'{key}_out_boxes'], f[f'{key}_box_counts'])):
        assert np.array_equal(boxes[b, :len(wb), 7], wb[:, 7])
        assert np.abs(boxes[b, :len(wb), :7] - wb[:, :7]).max(initial=0) <= 1e-5
        assert not boxes[b, len(wb):].any()


def synthetic_case(dev, B=4, seed=0, n_db=(40, 30, 25), npts=3000, limit=False, ops=('x', 'rot', 'scale')):
    from pdm_ssd_amd import augment
    rng = np.random.default_rng(seed)
    pts, offs, boxes, cids = [], [0], [], []
    for c, n in enumerate(n_db):
        for _ in range(n):
            dims = SIZES[c] * rng.uniform(0.9, 1.1, 3)
            box = np.array([rng.uniform(2, 68), rng.uniform(-38, 38), rng.uniform(-1.5, -0.5), *dims, rng.uniform(-3.1, 3.1)])
            k = int(rng.integers(3, 30))
            pts.append(np.concatenate([rng.uniform(-0.5, 0.5, (k, 3)) * dims, rng.uniform(0, 1, (k, 1))], 1))
            offs.append(offs[-1] + k)
            boxes.append(box)
            cids.append(c)
    db = augment.GTDatabase.from_arrays(np.concatenate(pts).astype(np.float32), np.asarray(offs),
                                        np.asarray(boxes, np.float32), cids, CLASS_NAMES, dev)
    counts = rng.integers(npts // 2, npts, B).astype(np.int32)
    raw = np.concatenate([np.stack([rng.uniform(-5, 75, n), rng.uniform(-45, 45, n), rng.uniform(-2.5, 0.5, n),
                                    rng.uniform(0, 1, n)], 1) for n in counts]).astype(np.float32)
    M = 8
    gt = np.zeros((B, M, 8), np.float32)
    for b in range(B):
        m = int(rng.integers(1, M + 1))
        cls = rng.integers(1, 4, m)
        gt[b, :m, 0], gt[b, :m, 1], gt[b, :m, 2] = rng.uniform(2, 68, m), rng.uniform(-38, 38, m), -1.0
        gt[b, :m, 3:6] = SIZES[cls - 1]
        gt[b, :m, 6] = rng.uniform(-3, 3, m)
        gt[b, :m, 7] = np.where(rng.uniform(size=m) < 0.2, -1, cls)
    cfg = [{'NAME': 'gt_sampling', 'SAMPLE_GROUPS': ['Car:6', 'Pedestrian:4', 'Cyclist:4'], 'LIMIT_WHOLE_SCENE': limit,
            'REMOVE_EXTRA_WIDTH': [0.1, 0.1, 0.0]}]
    if 'x' in ops:
        cfg.append({'NAME': 'random_world_flip', 'ALONG_AXIS_LIST': ['x']})
    if 'rot' in ops:
        cfg.append({'NAME': 'random_world_rotation', 'WORLD_ROT_ANGLE': [-0.785, 0.785]})
    if 'scale' in ops:
        cfg.append({'NAME': 'random_world_scaling', 'WORLD_SCALE_RANGE': [0.95, 1.05]})
    aug = augment.BatchAugmentor(cfg, RANGE, CLASS_NAMES, database=db, seed=seed + 11)
    host = {'raw': raw, 'counts': counts, 'gt': gt,
            'db': {'points': db.points.cpu().numpy(), 'offsets': db.host_offsets, 'boxes': db.boxes.cpu().numpy()}}
    return aug, (torch.from_numpy(raw).to(dev), torch.from_numpy(counts).to(dev), torch.from_numpy(gt).to(dev)), host


def restate(aug, host, state):
    groups = [(c, n, ln, fi) for c, n, ln, fi in zip(aug.g_cls, aug.g_num, aug.g_len, aug.g_first)]
    sampled, new_state, _ = ar.schedule(state, groups, host['gt'], aug.limit, aug.seed)
    B = len(host['counts'])
    flip, angle, scale = ar.scene_params(aug.seed, int(state[0]), B, aug.plan['flip_axes'], aug.plan['rot'], aug.plan['scale'])
    res = [ar.apply_scene(p, host['gt'][b], host['db'], groups, sampled[b], int(flip[b]), angle[b], scale[b], aug.plan['ops'],
                          aug.range, aug.extra)
           for b, p in enumerate(split(host['raw'], host['counts']))]
    return sampled, new_state, (flip, angle, scale), res


@pytest.mark.gpu
@pytest.mark.parametrize('limit', [False, True])
def test_own_draws_equal_the_restatement_bit_for_bit(dev, limit):
    aug, (raw, counts, gt), host = synthetic_case(dev, B=5, seed=1 + limit, limit=limit)
    state = aug.state.cpu().numpy().astype(np.int64)
    for call in range(3):                     # three calls: the pointer crosses epoch ends
        sampled, state, (flip, angle, scale), res = restate(aug, host, state)
        out = aug(raw, counts, gt)
        assert np.array_equal(out['params']['sampled'].cpu().numpy(), sampled)
        assert np.array_equal(out['params']['flip'].cpu().numpy(), flip)
        assert np.array_equal(out['params']['angle'].cpu().numpy(), angle)
        assert np.array_equal(out['params']['scale'].cpu().numpy(), scale)
        assert np.array_equal(aug.state.cpu().numpy(), state), call
        acc = out['accepted'].cpu().numpy()
        boxes = out['boxes'].cpu().numpy()
        rows = split(out['rows'].cpu().numpy(), out['host_counts'])
        for b, (r, bx, a) in enumerate(res):
            assert acc[b, :len(a)].tolist() == a and (acc[b, len(a):] == -1).all()
            assert np.array_equal(rows[b], r), (call, b)
            assert np.array_equal(boxes[b, :len(bx)], bx), (call, b)


@pytest.mark.gpu
def test_properties_on_random_scenes(dev):
    aug, (raw, counts, gt), host = synthetic_case(dev, B=6, seed=5, ops=())
    aug.range = [-1e4, -1e4, -1e4, 1e4, 1e4, 1e4]                      # no transform, nothing out of range
    out = aug(raw, counts, gt)
    acc = out['accepted'].cpu().numpy()
    nacc = out['num_accepted'].cpu().numpy()
    rows = split(out['rows'].cpu().numpy(), out['host_counts'])
    db = host['db']
    assert nacc.sum() > 0
    for b, scene in enumerate(split(host['raw'], host['counts'])):
        ids = acc[b, :nacc[b]]
        abox = db['boxes'][ids]
        present = host['gt'][b][host['gt'][b, :, 7] != 0, :7]
        others = np.concatenate([present, abox])
        from oracle import cpu_oracle as o
        ov = o.boxes_overlap_bev(abox, others)
        for i in range(len(abox)):
            ov[i, len(present) + i] = 0
        assert (ov == 0).all()                                           # no accepted box overlaps another box in BEV
        obj = np.concatenate([db['points'][db['offsets'][i]:db['offsets'][i + 1]] for i in ids]) if len(ids) else np.zeros((0, 4))
        shift = np.concatenate([np.repeat(db['boxes'][i][None, :3], db['offsets'][i + 1] - db['offsets'][i], 0) for i in ids]) \
            if len(ids) else np.zeros((0, 3))
        n_obj = len(obj)
        assert np.array_equal(rows[b][:n_obj, 3:], obj[:, 3:])             # the object points are present ...
        assert np.array_equal(rows[b][:n_obj, :3], (obj[:, :3] + shift).astype(np.float32))     # ... and shifted
        inside = np.zeros(len(scene), bool)
        for bx in abox:
            large = bx.copy()
            large[3:6] += np.float32(0.1), np.float32(0.1), np.float32(0.0)
            inside |= ar.points_in_box_cpu(scene, large)
        assert np.array_equal(rows[b][n_obj:], scene[~inside])             # removed <=> inside an enlarged accepted box


@pytest.mark.gpu
def test_same_seed_and_state_match_and_state_advances(dev):
    aug1, (raw, counts, gt), host = synthetic_case(dev, B=3, seed=7)
    aug2, _, _ = synthetic_case(dev, B=3, seed=7)
    s0 = aug1.state.clone()
    o1 = aug1(raw, counts, gt)
    o2 = aug2(raw, counts, gt)
    for k in ('rows', 'boxes', 'accepted'):
        assert torch.equal(o1[k], o2[k]), k
    _, want_state, _, _ = restate(aug1, host, s0.cpu().numpy().astype(np.int64))
    assert np.array_equal(aug1.state.cpu().numpy(), want_state) and int(want_state[0]) == 1
    o3 = aug1(raw, counts, gt)
    assert not torch.equal(o3['params']['angle'], o1['params']['angle'])


@pytest.mark.gpu
def test_overflow_sets_the_flag_and_writes_nothing_past_capacity(dev):
    aug, (raw, counts, gt), _ = synthetic_case(dev, B=3, seed=9)
    st = aug.state.clone()
    full = aug(raw, counts, gt)
    total = len(full['rows'])
    aug.state.copy_(st)
    guard = 4096
    buf = torch.full((total - 1 + guard, 4), 7.25, dtype=torch.float32, device=dev)
    out = aug.augment_padded(raw, counts, gt, total - 1, out_rows=buf)
    torch.cuda.synchronize()
    assert int(out['overflow'][0]) == 1
    assert out['counts'].sum().item() == total
    assert (buf[total - 1:] == 7.25).all()
    assert torch.equal(buf[:total - 1], full['rows'][:total - 1])
    aug.state.copy_(st)
    ok = aug.augment_padded(raw, counts, gt, total)
    assert int(ok['overflow'][0]) == 0 and torch.equal(ok['rows'], full['rows'])


@pytest.mark.gpu
def test_graph_replay_equals_eager_calls(dev):
    aug, (raw, counts, gt), _ = synthetic_case(dev, B=4, seed=13)
    ref, _, _ = synthetic_case(dev, B=4, seed=13)
    cap = int(raw.shape[0]) + 4 * 2000
    aug.augment_padded(raw, counts, gt, cap)           # warm-up (allocates the workspace)
    ref.augment_padded(raw, counts, gt, cap)
    ref.state.copy_(aug.state)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = aug.augment_padded(raw, counts, gt, cap)
    for _ in range(2):
        g.replay()
        want = ref.augment_padded(raw, counts, gt, cap)
        torch.cuda.synchronize()
        assert torch.equal(aug.state, ref.state)
        assert torch.equal(out['counts'], want['counts']) and int(out['overflow'][0]) == 0
        n = int(want['counts'].sum())
        assert torch.equal(out['rows'][:n], want['rows'][:n])
        for k in ('boxes', 'box_counts', 'accepted', 'num_accepted'):
            assert torch.equal(out[k], want[k]), k
        for k in ('sampled', 'flip', 'angle', 'scale'):
            assert torch.equal(out['params'][k], want['params'][k]), k


@pytest.mark.gpu
def test_augment_and_sample_feeds_a_training_step(dev):
    from pdm_ssd_amd import detectors
    from pdm_ssd_amd.detector_config import build_pdm_ssd
    from test_detector_gpu import SMALL
    aug, (raw, counts, gt), _ = synthetic_case(dev, B=2, seed=17, npts=6000)
    points, boxes = aug.augment_and_sample(raw, counts, gt, 2048, sample_seed=3)
    assert points.shape == (2 * 2048, 5) and boxes.shape[2] == 8 and boxes.shape[1] > 0
    torch.manual_seed(1)
    model = build_pdm_ssd(SMALL).to(dev).train()
    ret = detectors.model_fn_decorator()(model, {'batch_size': 2, 'points': points, 'gt_boxes': boxes})
    assert torch.isfinite(ret.loss)
    ret.loss.backward()
    assert all(p.grad is None or torch.isfinite(p.grad).all() for p in model.parameters())

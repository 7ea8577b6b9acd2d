"""Training augmentation at bs=32 on KITTI-like scenes: the batched device path (augment.BatchAugmentor: draw, collision
select, scene count / scan / fill) against the CPU restatement per scene (tests/augment_reference.py: the reference's
gt_sampling, world transforms and range mask in numpy, one scene at a time, as a dataloader worker runs them).
Scenes: ~120 k points each (synthetic.uniform_clouds), 8 scene boxes, SAMPLE_GROUPS Car:20, Pedestrian:15,
Cyclist:15 from a synthetic database of a few thousand objects, flip x, rotation +-pi/4, scaling 0.95-1.05.
Device calls are timed with events around the whole call: augment_padded (no synchronisation) and __call__ (one host
read).  Prints one JSON line.

  python tools/augment_rate.py [--bs 32] [--points 120000] [--calls 50] [--warmup 5] [--cpu-scenes 4]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

from pdm_ssd_amd import augment, synthetic  # noqa: E402

CLASS_NAMES = ['Car', 'Pedestrian', 'Cyclist']
SIZES = np.array([[3.9, 1.6, 1.56], [0.8, 0.6, 1.73], [1.76, 0.6, 1.73]], np.float32)
CFG = {'AUG_CONFIG_LIST': [
    {'NAME': 'gt_sampling', 'SAMPLE_GROUPS': ['Car:20', 'Pedestrian:15', 'Cyclist:15'], 'LIMIT_WHOLE_SCENE': False,
     'REMOVE_EXTRA_WIDTH': [0.0, 0.0, 0.0]},
    {'NAME': 'random_world_flip', 'ALONG_AXIS_LIST': ['x']},
    {'NAME': 'random_world_rotation', 'WORLD_ROT_ANGLE': [-0.78539816, 0.78539816]},
    {'NAME': 'random_world_scaling', 'WORLD_SCALE_RANGE': [0.95, 1.05]}], 'DISABLE_AUG_LIST': ['placeholder']}


def database(n_per_class, dev, seed=0):
    rng = np.random.default_rng(seed)
    pts, offs, boxes, cids = [], [0], [], []
    for c, n in enumerate(n_per_class):
        for _ in range(n):
            dims = SIZES[c] * rng.uniform(0.9, 1.1, 3)
            boxes.append([rng.uniform(2, 68), rng.uniform(-38, 38), rng.uniform(-1.8, -0.6), *dims, rng.uniform(-3.1, 3.1)])
            k = int(min(rng.exponential(120), 2000)) + 5
            pts.append(np.concatenate([rng.uniform(-0.5, 0.5, (k, 3)) * dims, rng.uniform(0, 1, (k, 1))], 1))
            offs.append(offs[-1] + k)
            cids.append(c)
    return augment.GTDatabase.from_arrays(np.concatenate(pts).astype(np.float32), np.asarray(offs), np.asarray(boxes, np.float32),
                                          cids, CLASS_NAMES, dev)


def scene_boxes(B, M, seed=1):
    rng = np.random.default_rng(seed)
    gt = np.zeros((B, M, 8), np.float32)
    cls = rng.integers(1, 4, (B, M))
    gt[..., 0], gt[..., 1], gt[..., 2] = rng.uniform(5, 65, (B, M)), rng.uniform(-35, 35, (B, M)), -1.0
    gt[..., 3:6] = SIZES[cls - 1]
    gt[..., 6] = rng.uniform(-3, 3, (B, M))
    gt[..., 7] = cls
    return gt


def timed(fn, *args, **kw):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    out = fn(*args, **kw)
    e.record()
    e.synchronize()
    return s.elapsed_time(e), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--bs', type=int, default=32)
    ap.add_argument('--points', type=int, default=120000)
    ap.add_argument('--calls', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--cpu-scenes', type=int, default=4)
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    B, N = a.bs, a.points
    db = database((2000, 800, 600), dev)
    aug = augment.BatchAugmentor(CFG, list(synthetic.KITTI_RANGE), CLASS_NAMES, database=db, seed=1)
    clouds = synthetic.uniform_clouds(B, N, 4321)
    clouds[..., 0] -= 5.0                       # a margin outside the range on every side
    clouds[..., 1] *= 1.1
    gt_host = scene_boxes(B, 8)
    raw = torch.from_numpy(clouds.reshape(B * N, 4)).to(dev)
    counts = torch.full((B,), N, dtype=torch.int32, device=dev)
    gt = torch.from_numpy(gt_host).to(dev)
    cap = B * N + B * aug.K * 2000
    for _ in range(a.warmup):
        aug.augment_padded(raw, counts, gt, cap)
        aug(raw, counts, gt)
    padded, exact = [], []
    for _ in range(a.calls):
        padded.append(timed(aug.augment_padded, raw, counts, gt, cap)[0])
        exact.append(timed(aug, raw, counts, gt)[0])
    out = aug(raw, counts, gt)
    rows_out = len(out['rows'])
    acc = out['num_accepted'].float().mean().item()

    import augment_reference as ar
    host_db = {'points': db.points.cpu().numpy(), 'offsets': db.host_offsets, 'boxes': db.boxes.cpu().numpy()}
    p = {k: v.cpu().numpy() for k, v in out['params'].items()}
    groups = [(c, n) for c, n in zip(aug.g_cls, aug.g_num)]
    cpu = []
    same = True
    rows = np.split(out['rows'].cpu().numpy(), np.cumsum(out['host_counts'])[:-1])
    for b in range(min(a.cpu_scenes, B)):
        t0 = time.perf_counter()
        r, bx, accepted = ar.apply_scene(clouds[b], gt_host[b], host_db, groups, p['sampled'][b], int(p['flip'][b]), p['angle'][b],
                                         p['scale'][b], aug.plan['ops'], aug.range, aug.extra)
        cpu.append((time.perf_counter() - t0) * 1e3)
        same &= bool(np.array_equal(r, rows[b]))
    res = {'metric': 'augment_ms_per_batch', 'bs': B, 'points_per_scene': N, 'samples_per_scene': aug.K,
           'database_objects': len(db), 'database_points': int(db.points.shape[0]),
           'device_padded_ms_median': statistics.median(padded), 'device_padded_ms_min': min(padded),
           'device_exact_ms_median': statistics.median(exact), 'device_exact_ms_min': min(exact),
           'cpu_restatement_ms_per_scene_median': statistics.median(cpu),
           'cpu_restatement_ms_per_batch_one_core': statistics.median(cpu) * B,
           'cpu_scenes_timed': len(cpu), 'cpu_rows_equal_device': same,
           'accepted_per_scene_mean': acc, 'rows_out': rows_out, 'device': torch.cuda.get_device_name(0)}
    print(json.dumps(res))


if __name__ == '__main__':
    main()

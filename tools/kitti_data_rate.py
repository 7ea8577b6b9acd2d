"""Infos + ground-truth database per frame on a synthetic KITTI tree: the batched device path
(kitti_dataset.KittiDataset.get_infos + create_groundtruth_database) against a single-thread numpy / scipy restatement
of the reference's per-frame loop (calibration, labels, FOV flag in float32, one Delaunay hull per object for
num_points_in_gt, points_in_boxes_cpu's rule per object for the database, one file per object).

Three numbers per side, all per frame, medians over --repeats runs after --warmup runs on the same tree:
  device_kernels_ms   HIP events around the device part of a batch only (crop-free: boxes_count, the read of the totals,
                      boxes_fill), frames already in HBM
  device_wall_ms      wall clock of get_infos + create_groundtruth_database: file reads (thread pool), upload, kernels, the
                      reads of the results, pickles and one .bin per object; ends after the last file is written
  cpu_wall_ms         wall clock of the restatement over --cpu-frames frames on one thread, files included
Writes profiles/kitti_data_rate.json (or --out) and prints the same JSON line.

  python tools/kitti_data_rate.py [--frames 64] [--points 120000] [--batch-frames 16] [--repeats 5] [--warmup 1]
"""
import argparse
import json
import os
import pickle
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import augment_reference as ar  # noqa: E402
import kitti_tree  # noqa: E402
from pdm_ssd_amd import kitti_dataset as kd  # noqa: E402

CLASS_NAMES = ['Car', 'Pedestrian', 'Cyclist']


def corners_of(boxes):
    """boxes_to_corners_3d in float32"""
    t = np.array([[1, 1, -1], [1, -1, -1], [-1, -1, -1], [-1, 1, -1], [1, 1, 1], [1, -1, 1], [-1, -1, 1], [-1, 1, 1]], np.float32) / 2
    b = boxes.astype(np.float32)
    c = b[:, None, 3:6] * t[None]
    ca, sa = np.cos(b[:, 6]), np.sin(b[:, 6])
    x = c[..., 0] * ca[:, None] - c[..., 1] * sa[:, None]
    y = c[..., 0] * sa[:, None] + c[..., 1] * ca[:, None]
    return np.stack([x, y, c[..., 2]], -1) + b[:, None, :3]


def cpu_frame(ds, idx, out_dir):
    """one frame as the reference's process_single_scene + its database loop do it, single thread"""
    from scipy.spatial import Delaunay
    info, calib, points = ds._host_info(idx, True, True)
    a = info['annos']
    shape = info['image']['image_shape']
    rect = calib.lidar_to_rect(points[:, 0:3])
    img, depth = calib.rect_to_img(rect)
    fov = (img[:, 0] >= 0) & (img[:, 0] < shape[1]) & (img[:, 1] >= 0) & (img[:, 1] < shape[0]) & (depth >= 0)
    pts_fov = points[fov]
    boxes = a['gt_boxes_lidar']
    n = -np.ones(len(a['name']), dtype=np.int32)
    for k, c in enumerate(corners_of(boxes)):
        n[k] = int((Delaunay(c).find_simplex(pts_fov[:, 0:3]) >= 0).sum())
    a['num_points_in_gt'] = n
    entries = 0
    for i in range(len(boxes)):
        obj = points[ar.points_in_box_cpu(points, boxes[i].astype(np.float32))]
        obj[:, :3] -= boxes[i, :3]
        obj.tofile(os.path.join(out_dir, '%s_%s_%d.bin' % (idx, a['name'][i], i)))
        entries += 1
    return info, entries


def device_run(ds, ids, batch_frames, workers):
    t0 = time.perf_counter()
    infos = ds.get_infos(num_workers=workers, sample_id_list=ids, batch_frames=batch_frames)
    path = os.path.join(ds.root, 'kitti_infos_train.pkl')
    with open(path, 'wb') as f:
        pickle.dump(infos, f)
    db = ds.create_groundtruth_database(path, split='train', batch_frames=batch_frames, num_workers=workers)
    return (time.perf_counter() - t0) * 1e3, infos, db


def kernel_ms(ds, infos, batch_frames, repeats):
    """device part of one batch, frames resident: count -> read totals -> fill, HIP events"""
    part = infos[:batch_frames]
    clouds = [ds.get_lidar(i['point_cloud']['lidar_idx']) for i in part]
    raw, counts, calib, shape = ds._frames_to_device(clouds, [kd._calib_of_info(i) for i in part],
                                                     [i['image']['image_shape'] for i in part])
    boxes, box_count, centres = kd.pad_boxes([i['annos']['gt_boxes_lidar'] for i in part], ds.device)
    ws = kd.boxes_workspace(len(part), boxes.shape[1], ds.device)
    times = []
    for k in range(repeats + 2):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        m = kd.BoxMembership(raw, counts, calib, shape, boxes, box_count, workspace=ws)
        m.gather(centres)
        e.record()
        e.synchronize()
        if k >= 2:
            times.append(s.elapsed_time(e))
    return statistics.median(times), len(part), int(raw.shape[0])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=64)
    ap.add_argument('--points', type=int, default=120000)
    ap.add_argument('--batch-frames', type=int, default=16)
    ap.add_argument('--workers', type=int, default=8)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--cpu-frames', type=int, default=8)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'kitti_data_rate.json'))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("kitti_data_rate needs a GPU: a rate measured elsewhere says nothing about this path")
    dev = torch.device('cuda:0')
    with tempfile.TemporaryDirectory() as tmp:
        kitti_tree.write_tree(tmp, seed=1, n_train=a.frames, n_val=0, n_test=0, n_points=a.points)
        ds = kd.KittiDataset(tmp, CLASS_NAMES, split='train', device=dev, load_infos=False)
        ids = ['%06d' % k for k in range(a.frames)]
        walls = []
        for k in range(a.warmup + a.repeats):
            ms, infos, db = device_run(ds, ids, a.batch_frames, a.workers)
            if k >= a.warmup:
                walls.append(ms)
        kern, kb, krows = kernel_ms(ds, infos, a.batch_frames, a.repeats)
        objects = sum(len(i['annos']['gt_boxes_lidar']) for i in infos)
        out_dir = os.path.join(tmp, 'cpu_db')
        os.makedirs(out_dir)
        cpu, same = [], True
        for idx, info in list(zip(ids, infos))[:a.cpu_frames]:
            t0 = time.perf_counter()
            ref, _ = cpu_frame(ds, idx, out_dir)
            cpu.append((time.perf_counter() - t0) * 1e3)
            # the float32 BLAS flag and qhull may differ from the device on a fragile point: report, do not assert
            same &= bool(np.array_equal(ref['annos']['num_points_in_gt'], info['annos']['num_points_in_gt']))
    res = {'metric': 'kitti_infos_and_database_ms_per_frame', 'frames': a.frames, 'points_per_frame': a.points,
           'objects': objects, 'batch_frames': a.batch_frames, 'reader_threads': kd.pool_size(a.workers),
           'device_wall_ms_per_frame_median': statistics.median(walls) / a.frames,
           'device_wall_ms_per_frame_min': min(walls) / a.frames, 'device_wall_runs': len(walls),
           'device_kernels_ms_per_frame_median': kern / kb, 'device_kernels_batch_frames': kb, 'device_kernels_batch_rows': krows,
           'cpu_wall_ms_per_frame_median': statistics.median(cpu), 'cpu_wall_ms_per_frame_min': min(cpu),
           'cpu_frames_timed': len(cpu), 'cpu_counts_equal_device': same,
           'what_the_clocks_include': {'device_wall': 'file reads, upload, kernels, result reads, pickles, one .bin per object',
                                       'device_kernels': 'boxes_count, read of the totals, boxes_fill; frames resident',
                                       'cpu_wall': 'file reads, float32 FOV flag, Delaunay hull per object, margin rule per '
                                                   'object, one .bin per object; one thread'},
           'device': torch.cuda.get_device_name(0)}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')
    print(json.dumps(res))


if __name__ == '__main__':
    main()

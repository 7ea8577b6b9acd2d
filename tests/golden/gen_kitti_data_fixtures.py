#!/usr/bin/env python3
"""Generates tests/golden/ref_kitti_data.npz / .json by running the REFERENCE's own dataset code on the CPU over the
synthetic KITTI tree of tests/kitti_tree.py: pcdet/datasets/kitti/kitti_dataset.py (get_infos,
create_groundtruth_database, get_fov_flag), utils/calibration_kitti.py, object3d_kitti.py and box_utils.py (in_hull over
boxes_to_corners_3d) are imported from where they lie, nothing copied.  Only what this image lacks is replaced:
  - pcdet.datasets.dataset by a DatasetTemplate that keeps the constructor's arguments (the real one imports skimage,
    torchvision, PIL and the voxel generators, none of which get_infos touches),
  - SharedArray by an empty module (imported by common_utils, never called here),
  - skimage.io.imread by a function returning zeros of the PNG's shape (read from its IHDR chunk),
  - roiaware_pool3d_utils.points_in_boxes_cpu by the stub gen_augment_fixtures.py uses, over
    tests/augment_reference.py::points_in_box_cpu (points_in_boxes_cpu's rule in float32, one rounding at a time),
  - the name `Path`, which kitti_dataset.py imports only when run as a script.
Numbers only are recorded: the info fields, the reference's FOV flags as packed bits, the per-object counts, the
database points and db-infos.

Fragile decisions, marked from a float64 restatement and never compared by the tests:
  - FOV: a projected pixel within 1e-2 px of an image border, or a depth term within 1e-4 m of zero;
  - hull: a point within 1e-5 m of a face of a box (in the fp32 box's own frame).
The generator FAILS if either share exceeds 1e-3 or if the reference disagrees with float64 on a non-fragile decision.
Run in the authoring container only (needs the reference tree); the outputs are committed and reproduce byte for byte.
"""
import contextlib
import hashlib
import io
import json
import os
import pickle
import struct
import sys
import tempfile
import types
import zipfile
from pathlib import Path

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))

import augment_reference as ar  # noqa: E402
import kitti_tree  # noqa: E402

REF = '/root/reference'
CLASS_NAMES = ['Car', 'Pedestrian', 'Cyclist']
SEED = 0
FOV_PX, FOV_DEPTH, HULL_M, MAX_SHARE = 1e-2, 1e-4, 1e-5, 1e-3


class EasyDict(dict):
    def __init__(self, d=None):
        super().__init__()
        for k, v in (d or {}).items():
            self[k] = EasyDict(v) if isinstance(v, dict) else v

    __getattr__ = dict.__getitem__


def png_shape(path):
    with open(str(path), 'rb') as f:
        head = f.read(24)
    w, h = struct.unpack('>II', head[16:24])
    return h, w


def install_reference():
    def pkg(name, path=None):
        m = types.ModuleType(name)
        m.__path__ = [path] if path else []
        sys.modules[name] = m
        return m
    pkg('pcdet', f'{REF}/pcdet')
    pkg('pcdet.ops', f'{REF}/pcdet/ops')
    pkg('pcdet.utils', f'{REF}/pcdet/utils')
    pkg('pcdet.datasets')
    pkg('pcdet.datasets.kitti', f'{REF}/pcdet/datasets/kitti')
    sys.modules['SharedArray'] = types.ModuleType('SharedArray')
    sk = pkg('skimage')
    sk.io = types.ModuleType('skimage.io')
    sk.io.imread = lambda path: np.zeros(png_shape(path) + (3,), dtype=np.uint8)
    sys.modules['skimage.io'] = sk.io
    ds = types.ModuleType('pcdet.datasets.dataset')

    class DatasetTemplate:
        def __init__(self, dataset_cfg=None, class_names=None, training=True, root_path=None, logger=None):
            self.dataset_cfg, self.class_names, self.training = dataset_cfg, class_names, training
            self.root_path, self.logger = root_path, logger

        @property
        def mode(self):
            return 'train' if self.training else 'test'
    ds.DatasetTemplate = DatasetTemplate
    sys.modules[ds.__name__] = ds
    roi = pkg('pcdet.ops.roiaware_pool3d')
    ru = types.ModuleType('pcdet.ops.roiaware_pool3d.roiaware_pool3d_utils')

    def points_in_boxes_cpu(points, boxes):
        p = points.numpy() if torch.is_tensor(points) else np.asarray(points)
        bx = boxes.numpy() if torch.is_tensor(boxes) else np.asarray(boxes)
        out = np.stack([ar.points_in_box_cpu(p.astype(np.float32), b) for b in bx.astype(np.float32)]).astype(np.int32) \
            if len(bx) else np.zeros((0, len(p)), np.int32)
        return torch.from_numpy(out) if torch.is_tensor(points) else out
    ru.points_in_boxes_cpu = points_in_boxes_cpu
    roi.roiaware_pool3d_utils = ru
    sys.modules[ru.__name__] = ru
    from pcdet.datasets.kitti import kitti_dataset
    from pcdet.utils import box_utils
    kitti_dataset.Path = Path
    return kitti_dataset, box_utils


def projection64(points, calib):
    """(u, v, depth term) in float64 from the float32 inputs"""
    p = points[:, :3].astype(np.float64)
    V, R, P = (np.asarray(m, np.float32).astype(np.float64) for m in (calib.V2C, calib.R0, calib.P2))
    cam = p @ V[:, :3].T + V[:, 3]
    rect = cam @ R.T
    hom = rect @ P[:, :3].T + P[:, 3]
    with np.errstate(divide='ignore', invalid='ignore'):
        return hom[:, 0] / rect[:, 2], hom[:, 1] / rect[:, 2], hom[:, 2] - P[2, 3]


def fov64(points, calib, shape):
    u, v, d = projection64(points, calib)
    h, w = float(shape[0]), float(shape[1])
    flag = (u >= 0) & (u < w) & (v >= 0) & (v < h) & (d >= 0)
    with np.errstate(invalid='ignore'):
        near = (np.abs(u) < FOV_PX) | (np.abs(u - w) < FOV_PX) | (np.abs(v) < FOV_PX) | (np.abs(v - h) < FOV_PX) | \
            (np.abs(d) < FOV_DEPTH) | ~np.isfinite(u) | ~np.isfinite(v)
    return flag, near


def hull64(points, box32):
    """(inside, fragile) of the exact oriented box (the fp32 box, arithmetic in float64)"""
    b = box32.astype(np.float64)
    X, Y, Z = (points[:, k].astype(np.float64) - b[k] for k in range(3))
    c, s = np.cos(b[6]), np.sin(b[6])
    loc = np.stack([X * c + Y * s, Y * c - X * s, Z], 1)
    gap = np.abs(loc) - b[3:6] / 2.0                   # > 0 outside along that axis
    inside = (gap <= 0).all(1)
    fragile = (np.abs(gap) < HULL_M).any(1) & (gap < HULL_M).all(1)
    return inside, fragile


def tree_digest(root):
    h = hashlib.sha256()
    for part in ('training', 'testing'):
        for sub in ('velodyne', 'calib', 'label_2'):
            d = os.path.join(root, part, sub)
            for name in sorted(os.listdir(d)) if os.path.isdir(d) else []:
                h.update(name.encode())
                with open(os.path.join(d, name), 'rb') as f:
                    h.update(f.read())
    return h.hexdigest()


def write_npz(path, arrays):
    """an .npz whose bytes depend on the arrays alone (np.savez stamps the current time into the archive)"""
    with zipfile.ZipFile(path, 'w', zipfile.ZIP_DEFLATED) as z:
        for name in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(arrays[name]), allow_pickle=False)
            info = zipfile.ZipInfo(name + '.npy', date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


ANNO_KEYS = ('truncated', 'occluded', 'alpha', 'bbox', 'dimensions', 'location', 'rotation_y', 'score', 'difficulty', 'index',
             'gt_boxes_lidar', 'num_points_in_gt')


def main():
    kd_ref, box_utils = install_reference()
    out, meta = {}, {}
    with tempfile.TemporaryDirectory() as tmp:
        split = kitti_tree.write_tree(tmp, seed=SEED)
        meta['tree'] = {'seed': SEED, 'sha256': tree_digest(tmp), 'split': split}
        cfg = EasyDict({'DATA_SPLIT': {'train': 'train', 'test': 'val'}, 'INFO_PATH': {'train': [], 'test': []},
                        'FOV_POINTS_ONLY': True})
        with contextlib.redirect_stdout(io.StringIO()):
            ds = kd_ref.KittiDataset(dataset_cfg=cfg, class_names=CLASS_NAMES, training=False, root_path=Path(tmp))
            infos = {}
            for s in ('train', 'val'):
                ds.set_split(s)
                infos[s] = ds.get_infos(num_workers=1, has_label=True, count_inside_pts=True)
            ds.set_split('test')
            infos['test'] = ds.get_infos(num_workers=1, has_label=False, count_inside_pts=False)
            train_pkl = os.path.join(tmp, 'kitti_infos_train.pkl')
            with open(train_pkl, 'wb') as f:
                pickle.dump(infos['train'], f)
            ds.set_split('train')
            ds.create_groundtruth_database(train_pkl, split='train')
        with open(os.path.join(tmp, 'kitti_dbinfos_train.pkl'), 'rb') as f:
            dbinfos = pickle.load(f)

        totals = {'points': 0, 'fov_fragile': 0, 'hull_tests': 0, 'hull_fragile': 0}
        for s in ('train', 'val', 'test'):
            meta[s] = {'frames': [i['point_cloud']['lidar_idx'] for i in infos[s]], 'names': [], 'keys': list(infos[s][0].keys())}
            out[f'{s}_image_shape'] = np.stack([i['image']['image_shape'] for i in infos[s]])
            for key in ('P2', 'R0_rect', 'Tr_velo_to_cam'):
                out[f'{s}_calib_{key}'] = np.stack([i['calib'][key] for i in infos[s]])
                meta[s][f'calib_{key}_dtype'] = str(infos[s][0]['calib'][key].dtype)
            if s == 'test':
                continue
            meta[s]['anno_keys'] = list(infos[s][0]['annos'].keys())
            meta[s]['names'] = [list(map(str, i['annos']['name'])) for i in infos[s]]
            out[f'{s}_num_gt'] = np.array([len(i['annos']['name']) for i in infos[s]], np.int32)
            out[f'{s}_num_objects'] = np.array([len(i['annos']['gt_boxes_lidar']) for i in infos[s]], np.int32)
            for key in ANNO_KEYS:
                out[f'{s}_{key}'] = np.concatenate([i['annos'][key] for i in infos[s]], 0)
                meta[s][f'{key}_dtype'] = str(infos[s][0]['annos'][key].dtype)
            # the reference's FOV flags, the fragile marks and the per-object fragile counts
            ds.set_split(s)
            flags, fragile, counts, obj_fragile = [], [], [], []
            for info in infos[s]:
                idx = info['point_cloud']['lidar_idx']
                points = ds.get_lidar(idx)
                calib = ds.get_calib(idx)
                shape = info['image']['image_shape']
                ref_flag = ds.get_fov_flag(calib.lidar_to_rect(points[:, 0:3]), shape, calib)
                f64, near = fov64(points, calib, shape)
                bad = (ref_flag != f64) & ~near
                assert not bad.any(), f"{s} {idx}: the reference's FOV flag differs from float64 on {int(bad.sum())} non-fragile points"
                flags.append(ref_flag)
                fragile.append(near)
                counts.append(len(points))
                totals['points'] += len(points)
                totals['fov_fragile'] += int(near.sum())
                boxes = info['annos']['gt_boxes_lidar']
                corners = box_utils.boxes_to_corners_3d(boxes)
                for k in range(len(boxes)):
                    inside, frag = hull64(points, boxes[k].astype(np.float32))
                    ref_in = box_utils.in_hull(points[:, 0:3], corners[k])
                    bad = (ref_in != inside) & ~frag
                    assert not bad.any(), f"{s} {idx} box {k}: in_hull differs from float64 on {int(bad.sum())} non-fragile points"
                    totals['hull_tests'] += len(points)
                    totals['hull_fragile'] += int(frag.sum())
                    # a count can move by a point whose FOV flag is fragile and which is in (or fragile to) the hull, or
                    # whose hull decision is fragile and which is in (or fragile to) the FOV
                    obj_fragile.append(int(((near & (inside | frag)) | (frag & (f64 | near))).sum()))
            out[f'{s}_point_counts'] = np.array(counts, np.int32)
            out[f'{s}_fov_bits'] = np.packbits(np.concatenate(flags))
            out[f'{s}_fov_fragile_bits'] = np.packbits(np.concatenate(fragile))
            out[f'{s}_object_fragile'] = np.array(obj_fragile, np.int32)

        # the database: every object's file in frame / object order, and the db-infos as written
        pts, offs = [], [0]
        for info in infos['train']:
            idx = info['point_cloud']['lidar_idx']
            for i in range(len(info['annos']['gt_boxes_lidar'])):
                p = np.fromfile(os.path.join(tmp, 'gt_database', '%s_%s_%d.bin' % (idx, info['annos']['name'][i], i)),
                                dtype=np.float32).reshape(-1, 4)
                pts.append(p)
                offs.append(offs[-1] + len(p))
        out['db_points'] = np.concatenate(pts, 0)
        out['db_offsets'] = np.array(offs, np.int64)
        meta['db'] = {'files': sorted(os.listdir(os.path.join(tmp, 'gt_database'))), 'classes': list(dbinfos.keys()),
                      'keys': list(next(iter(dbinfos.values()))[0].keys()), 'infos': {}}
        for name, entries in dbinfos.items():
            meta['db']['infos'][name] = [{'path': e['path'], 'image_idx': e['image_idx'], 'gt_idx': int(e['gt_idx']),
                                          'num_points_in_gt': int(e['num_points_in_gt']), 'difficulty': int(e['difficulty']),
                                          'score': float(e['score'])} for e in entries]
            out[f'db_{name}_box3d_lidar'] = np.stack([e['box3d_lidar'] for e in entries])
            out[f'db_{name}_bbox'] = np.stack([e['bbox'] for e in entries])
            meta['db'][f'{name}_types'] = {k: type(v).__name__ + (':' + str(v.dtype) if hasattr(v, 'dtype') else '')
                                           for k, v in entries[0].items()}
    meta['fragile'] = {'fov_margin_px': FOV_PX, 'fov_margin_depth_m': FOV_DEPTH, 'hull_margin_m': HULL_M,
                       'fov_share': totals['fov_fragile'] / totals['points'],
                       'hull_share': totals['hull_fragile'] / totals['hull_tests'], **totals}
    assert meta['fragile']['fov_share'] <= MAX_SHARE, meta['fragile']
    assert meta['fragile']['hull_share'] <= MAX_SHARE, meta['fragile']
    write_npz(os.path.join(HERE, 'ref_kitti_data.npz'), out)
    with open(os.path.join(HERE, 'ref_kitti_data.json'), 'w') as fh:
        json.dump(meta, fh, indent=1, sort_keys=True)
        fh.write('\n')
    print('wrote ref_kitti_data.npz (%d arrays, %d bytes); fragile shares: FOV %.2e, hull %.2e' % (
        len(out), os.path.getsize(os.path.join(HERE, 'ref_kitti_data.npz')), meta['fragile']['fov_share'],
        meta['fragile']['hull_share']))


if __name__ == '__main__':
    main()

#!/usr/bin/env python3
"""Generates tests/golden/ref_augment.npz by running the REFERENCE's own augmentation code on the CPU:
pcdet/datasets/augmentor/database_sampler.py (DataBaseSampler: PREPARE filters, sample_with_fixed_number, the
collision test, add_sampled_boxes_to_scene), augmentor_utils.py (random_flip_along_x / _y, global_rotation,
global_scaling), common_utils.limit_period / mask_points_by_range and box_utils.mask_boxes_outside_range_numpy —
imported from where they lie, nothing copied — over a tiny synthetic database written to a temporary directory
(dbinfos .pkl + gt_database/*.bin).  Only what this image lacks is replaced:
  - SharedArray, skimage and kitti_common by empty modules (imported, never called here),
  - iou3d_nms_utils.boxes_bev_iou_cpu by a stub over the CPU oracle's rotated-box IoU (iou3d_cpu.cpp's arithmetic),
  - roiaware_pool3d_utils.points_in_boxes_cpu by a stub over a restatement with points_in_boxes_cpu's 1e-2 margin.
np.random.permutation / choice / uniform are wrapped to RECORD the draws (choice, the flip coin, is scripted so that
both outcomes occur).  The class column and the dropping of non-target boxes follow dataset.py:158-215.
Two configurations: A (flip x, rotation, scaling; colliding pairs, a collision with a scene box and with an earlier
class's acceptance, a non-target box, a short slice at an epoch end, boxes and points out of range) and B
(LIMIT_WHOLE_SCENE, flips along x and y, a skipped scaling).  Scene points within 1e-4 of a database box face are
dropped before the run, so that no in / out decision is fp-fragile.
Run in the authoring container only (needs the reference tree); the .npz output is committed.
"""
import os
import pickle
import sys
import tempfile
import types
from pathlib import Path

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))
from oracle import cpu_oracle as o  # noqa: E402

import augment_reference as ar  # noqa: E402

REF = '/root/reference'
CLASS_NAMES = ['Car', 'Pedestrian', 'Cyclist']
PC_RANGE = np.array([0, -40, -3, 70.4, 40, 1], dtype=np.float32)
C = 4


class EasyDict(dict):
    def __init__(self, d=None):
        super().__init__()
        for k, v in (d or {}).items():
            self[k] = EasyDict(v) if isinstance(v, dict) else v

    __getattr__ = dict.__getitem__


def install_reference():
    def pkg(name, path=None):
        m = types.ModuleType(name)
        m.__path__ = [path] if path else []
        sys.modules[name] = m
        return m
    pkg('pcdet', f'{REF}/pcdet')
    pkg('pcdet.ops', f'{REF}/pcdet/ops')
    pkg('pcdet.utils', f'{REF}/pcdet/utils')
    pkg('pcdet.datasets', f'{REF}/pcdet/datasets')
    pkg('pcdet.datasets.augmentor', f'{REF}/pcdet/datasets/augmentor')
    pkg('pcdet.datasets.kitti')
    pkg('pcdet.datasets.kitti.kitti_object_eval_python')
    kc = types.ModuleType('pcdet.datasets.kitti.kitti_object_eval_python.kitti_common')
    sys.modules[kc.__name__] = kc
    sys.modules['SharedArray'] = types.ModuleType('SharedArray')
    sk = pkg('skimage')
    sk.io = types.ModuleType('skimage.io')
    sys.modules['skimage.io'] = sk.io
    iou = pkg('pcdet.ops.iou3d_nms')
    iu = types.ModuleType('pcdet.ops.iou3d_nms.iou3d_nms_utils')

    def boxes_bev_iou_cpu(a, b):
        return o.boxes_iou_bev(np.asarray(a, np.float32), np.asarray(b, np.float32))
    iu.boxes_bev_iou_cpu = boxes_bev_iou_cpu
    iou.iou3d_nms_utils = iu
    sys.modules[iu.__name__] = iu
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
    from pcdet.datasets.augmentor import augmentor_utils, database_sampler
    from pcdet.utils import box_utils, common_utils
    return database_sampler, augmentor_utils, common_utils, box_utils


class Recorder:
    """Wraps np.random.permutation / choice / uniform: records every draw; choice returns scripted flip coins."""

    def __init__(self, coins):
        self.coins = list(coins)
        self.log = []
        self._perm, self._choice, self._uniform = np.random.permutation, np.random.choice, np.random.uniform

    def __enter__(self):
        def permutation(n):
            v = self._perm(n)
            self.log.append(('permutation', v.copy()))
            return v

        def choice(*a, **k):
            v = self.coins.pop(0)
            self.log.append(('choice', v))
            return v

        def uniform(lo, hi, *a, **k):
            v = self._uniform(lo, hi, *a, **k)
            self.log.append(('uniform', v))
            return v
        np.random.permutation, np.random.choice, np.random.uniform = permutation, choice, uniform
        return self

    def __exit__(self, *exc):
        np.random.permutation, np.random.choice, np.random.uniform = self._perm, self._choice, self._uniform


def make_database(rng, root):
    """Database entries by class with deliberate placements (lidar frame, z ~ -1)."""
    spec = {
        'Car': [(20.0, 5.0), (20.3, 5.4), (30.0, -10.0), (40.0, 12.0), (69.9, 0.0)],   # 0/1 collide; 2 on a scene box
        'Pedestrian': [(40.2, 12.3), (15.0, -3.0), (25.0, 15.0), (50.0, -20.0)],      # 0 on Car 3
        'Cyclist': [(10.0, 10.0), (60.0, 25.0), (35.0, -30.0)],
        'Van': [(12.0, -15.0)],
    }
    sizes = {'Car': (3.9, 1.6, 1.56), 'Pedestrian': (0.8, 0.6, 1.73), 'Cyclist': (1.76, 0.6, 1.73), 'Van': (5.0, 2.0, 2.2)}
    (root / 'gt_database').mkdir(parents=True, exist_ok=True)
    infos, k = {}, 0
    for name, locs in spec.items():
        infos[name] = []
        for (x, y) in locs:
            dims = np.array(sizes[name], np.float32) * rng.uniform(0.95, 1.05, 3).astype(np.float32)
            box = np.array([x, y, -1.0 + rng.uniform(-0.1, 0.1), *dims, rng.uniform(-np.pi, np.pi)], np.float32)
            n = int(rng.integers(6, 14))
            rel = (rng.uniform(-0.45, 0.45, (n, 3)) * dims).astype(np.float32)
            c, s = np.cos(box[6]), np.sin(box[6])
            rel[:, :2] = np.stack([rel[:, 0] * c - rel[:, 1] * s, rel[:, 0] * s + rel[:, 1] * c], 1).astype(np.float32)
            pts = np.concatenate([rel, rng.uniform(0, 1, (n, 1)).astype(np.float32)], 1).astype(np.float32)
            path = f'gt_database/{k:04d}_{name}.bin'
            pts.tofile(str(root / path))
            infos[name].append({'name': name, 'path': path, 'box3d_lidar': box, 'num_points_in_gt': n,
                                'difficulty': int(k % 3), 'gt_idx': k})
            k += 1
    with open(root / 'dbinfos_train.pkl', 'wb') as f:
        pickle.dump(infos, f)
    return infos


def make_scene(rng, infos, boxes_spec):
    """Scene points: uniform (partly outside the range) + clusters at every database box; boxes_spec [(name, box)]."""
    pts = [np.stack([rng.uniform(-5, 80, 400), rng.uniform(-50, 50, 400), rng.uniform(-2.5, 0.5, 400),
                     rng.uniform(0, 1, 400)], 1)]
    for name in infos:
        for info in infos[name]:
            b = info['box3d_lidar']
            q = rng.uniform(-0.7, 0.7, (15, 3)) * (b[3:6] + 0.6)
            pts.append(np.concatenate([q + b[:3], rng.uniform(0, 1, (15, 1))], 1))
    pts = np.concatenate(pts, 0).astype(np.float32)
    # drop points within 1e-4 of any (enlarged) database box face
    ok = np.ones(len(pts), bool)
    for name in infos:
        for info in infos[name]:
            for extra in (0.0, 0.2):
                b = info['box3d_lidar'].astype(np.float64)
                c, s = np.cos(-b[6]), np.sin(-b[6])
                sx, sy = pts[:, 0] - b[0], pts[:, 1] - b[1]
                lx, ly = sx * c - sy * s, sx * s + sy * c
                for d, half in ((np.abs(lx), (b[3] + extra) / 2 + 0.01), (np.abs(ly), (b[4] + extra) / 2 + 0.01),
                                (np.abs(pts[:, 2] - b[2]), b[5] / 2)):
                    ok &= np.abs(d - half) > 1e-4
    pts = pts[ok]
    names = np.array([n for n, _ in boxes_spec])
    gt = np.array([bx for _, bx in boxes_spec], np.float32).reshape(-1, 7)
    return pts, gt, names


CONFIGS = {
    'A': {'sampler': {'SAMPLE_GROUPS': ['Car:3', 'Pedestrian:2', 'Cyclist:2'], 'LIMIT_WHOLE_SCENE': False,
                      'REMOVE_EXTRA_WIDTH': [0.2, 0.2, 0.0]},
          'flip': ['x'], 'rot': [-0.78539816, 0.78539816], 'scale': [0.95, 1.05]},
    'B': {'sampler': {'SAMPLE_GROUPS': ['Car:4', 'Pedestrian:2'], 'LIMIT_WHOLE_SCENE': True,
                      'REMOVE_EXTRA_WIDTH': [0.0, 0.0, 0.0]},
          'flip': ['x', 'y'], 'rot': [-0.3, 0.3], 'scale': [1.0, 1.0005]},
}


def run_config(mods, root, infos, key, cfg, scenes, coins):
    database_sampler, augmentor_utils, common_utils, box_utils = mods
    scfg = EasyDict({'DB_INFO_PATH': ['dbinfos_train.pkl'], 'PREPARE': {'filter_by_difficulty': [-1],
                     'filter_by_min_points': ['Car:5', 'Pedestrian:5']}, 'NUM_POINT_FEATURES': C,
                     'DATABASE_WITH_FAKELIDAR': False, **cfg['sampler']})
    sampler = database_sampler.DataBaseSampler(root_path=Path(root), sampler_cfg=scfg, class_names=CLASS_NAMES)
    db_rows = {c: [info['gt_idx'] for info in sampler.db_infos[c]] for c in CLASS_NAMES}
    rec_sampled = []
    orig = sampler.sample_with_fixed_number

    def sample_with_fixed_number(class_name, group):
        out = orig(class_name, group)
        rec_sampled[-1].append((class_name, [db_rows[class_name].index(i['gt_idx']) for i in out]))
        return out
    sampler.sample_with_fixed_number = sample_with_fixed_number
    res = []
    with Recorder(coins) as rec:
        for pts, gt, names in scenes:
            rec_sampled.append([])
            mask = np.array([n in CLASS_NAMES for n in names], dtype=np.bool_)
            d = sampler({'points': pts.copy(), 'gt_boxes': gt.copy(), 'gt_names': names.copy(), 'gt_boxes_mask': mask})
            gb, p = d['gt_boxes'], d['points']
            gnames = d['gt_names']
            flips = []
            for ax in cfg['flip']:
                gb, p, en = getattr(augmentor_utils, 'random_flip_along_%s' % ax)(gb, p, return_flip=True)
                flips.append(bool(en))
            n_log = len(rec.log)
            gb, p, angle = augmentor_utils.global_rotation(gb, p, cfg['rot'], return_rot=True)
            r = augmentor_utils.global_scaling(gb, p, cfg['scale'], return_scale=True)
            gb, p = r[0], r[1]
            scale = r[2] if len(r) == 3 else None
            assert len(rec.log) == n_log + (2 if scale is not None else 1)
            gb[:, 6] = common_utils.limit_period(gb[:, 6], offset=0.5, period=2 * np.pi)
            sel = np.array([n in CLASS_NAMES for n in gnames], dtype=bool)
            gb, gnames = gb[sel], gnames[sel]
            cls = np.array([CLASS_NAMES.index(n) + 1 for n in gnames], np.float32)
            gb = np.concatenate([gb[:, :7], cls[:, None]], 1).astype(np.float32)
            p = p[common_utils.mask_points_by_range(p, PC_RANGE)]
            gb = gb[box_utils.mask_boxes_outside_range_numpy(gb, PC_RANGE, 1, True)]
            res.append({'points': np.asarray(p, np.float32), 'boxes': gb, 'flip': flips, 'angle': float(angle),
                        'scale': scale, 'n_accepted': len(d['gt_names']) - int(mask.sum()) if len(d['gt_names']) != len(names)
                        else 0})
    return sampler, db_rows, rec_sampled, res, rec.log


def scene_boxes(infos):
    car2 = infos['Car'][2]['box3d_lidar'].copy()
    car2[0] += 0.5
    return [
        [('Car', car2), ('Van', np.array([12, -15, -1, 5, 2, 2.2, 0.3], np.float32)),
         ('Pedestrian', np.array([75.0, 2, -1, 0.8, 0.6, 1.7, 0.0], np.float32))],          # out of range
        [('Cyclist', np.array([8.0, -25, -1, 1.8, 0.6, 1.7, 1.0], np.float32)),
         ('Car', np.array([55.0, 30, -1, 3.9, 1.6, 1.5, -0.5], np.float32))],
        [('Car', np.array([15.0, 20, -1, 4.0, 1.7, 1.5, 0.2], np.float32)),
         ('Car', np.array([45.0, -5, -1, 4.0, 1.7, 1.5, 2.0], np.float32))],
        [('Van', np.array([60.0, -35, -1, 5, 2, 2.2, 0.3], np.float32))],
    ]


def to_arrays(infos):
    """The database in GTDatabase order (class_names order, reference file order within a class)."""
    pts, offs, boxes, cids = [], [0], [], []
    for k, c in enumerate(CLASS_NAMES):
        for info in infos[c]:
            p = info['points']
            pts.append(p)
            offs.append(offs[-1] + len(p))
            boxes.append(info['box3d_lidar'])
            cids.append(k)
    return np.concatenate(pts, 0), np.asarray(offs, np.int64), np.asarray(boxes, np.float32), np.asarray(cids, np.int64)


def main():
    mods = install_reference()
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        rng = np.random.default_rng(7)
        infos = make_database(rng, Path(tmp))
        for c in infos:
            for info in infos[c]:
                info['points'] = np.fromfile(os.path.join(tmp, info['path']), np.float32).reshape(-1, C)
        scenes = [make_scene(rng, infos, spec) for spec in scene_boxes(infos)]
        for key, cfg in CONFIGS.items():
            np.random.seed({'A': 3, 'B': 11}[key])
            coins = [True, False, False, True, True, True, False, False, True, False]
            sampler, db_rows, rec_sampled, res, log = run_config(mods, tmp, infos, key, cfg, scenes, coins)
            filt = {c: [i for i in infos[c] if i['gt_idx'] in db_rows[c]] for c in CLASS_NAMES}
            for c in CLASS_NAMES:
                assert [i['gt_idx'] for i in filt[c]] == db_rows[c]
            dbp, dbo, dbb, dbc = to_arrays(filt)
            first = np.concatenate([[0], np.cumsum([len(filt[c]) for c in CLASS_NAMES])[:-1]])
            groups = [(CLASS_NAMES.index(g.split(':')[0]), int(g.split(':')[1])) for g in cfg['sampler']['SAMPLE_GROUPS']]
            K = sum(n for _, n in groups)
            B = len(scenes)
            sampled = np.full((B, K), -1, np.int32)
            for b, lst in enumerate(rec_sampled):
                for cname, idx in lst:
                    t = [g[0] for g in groups].index(CLASS_NAMES.index(cname))
                    slot = sum(n for _, n in groups[:t])
                    sampled[b, slot:slot + len(idx)] = first[CLASS_NAMES.index(cname)] + np.asarray(idx)
            pre = f'{key}_'
            out[pre + 'db_points'], out[pre + 'db_offsets'], out[pre + 'db_boxes'], out[pre + 'db_class'] = dbp, dbo, dbb, dbc
            out[pre + 'groups'] = np.asarray(groups, np.int32)
            out[pre + 'sampled'] = sampled
            fl = np.zeros(B, np.int32)
            for b, r in enumerate(res):
                for ax, en in zip(cfg['flip'], r['flip']):
                    fl[b] |= (1 if ax == 'x' else 2) if en else 0
            out[pre + 'flip'] = fl
            out[pre + 'angle'] = np.asarray([r['angle'] for r in res], np.float32)
            out[pre + 'scale'] = np.asarray([1.0 if r['scale'] is None else r['scale'] for r in res], np.float32)
            out[pre + 'scale_skipped'] = np.asarray([r['scale'] is None for r in res])
            out[pre + 'extra'] = np.asarray(cfg['sampler']['REMOVE_EXTRA_WIDTH'], np.float32)
            out[pre + 'limit'] = np.asarray(cfg['sampler']['LIMIT_WHOLE_SCENE'])
            out[pre + 'ops'] = np.asarray([1 if a == 'x' else 2 for a in cfg['flip']] + [3] +
                                          ([4] if cfg['scale'][1] - cfg['scale'][0] >= 1e-3 else []), np.int32)
            out[pre + 'out_counts'] = np.asarray([len(r['points']) for r in res], np.int32)
            out[pre + 'out_points'] = np.concatenate([r['points'] for r in res], 0)
            out[pre + 'box_counts'] = np.asarray([len(r['boxes']) for r in res], np.int32)
            out[pre + 'out_boxes'] = np.concatenate([r['boxes'] for r in res], 0)
            out[pre + 'permutations'] = np.asarray([len(v) for k_, v in log if k_ == 'permutation'], np.int32)
            print(key, 'sampled', sampled.tolist(), 'flip', fl.tolist(), 'counts', out[pre + 'out_counts'].tolist(),
                  'boxes', out[pre + 'box_counts'].tolist())
        out['in_counts'] = np.asarray([len(s[0]) for s in scenes], np.int32)
        out['in_points'] = np.concatenate([s[0] for s in scenes], 0)
        M = max(len(s[1]) for s in scenes)
        gt = np.zeros((len(scenes), M, 8), np.float32)
        for b, (_, g, names) in enumerate(scenes):
            gt[b, :len(g), :7] = g
            gt[b, :len(g), 7] = [CLASS_NAMES.index(n) + 1 if n in CLASS_NAMES else -1 for n in names]
        out['in_boxes'] = gt
        out['pc_range'] = PC_RANGE
    np.savez_compressed(os.path.join(HERE, 'ref_augment.npz'), **out)
    print('wrote', os.path.join(HERE, 'ref_augment.npz'), os.path.getsize(os.path.join(HERE, 'ref_augment.npz')), 'bytes')


if __name__ == '__main__':
    main()

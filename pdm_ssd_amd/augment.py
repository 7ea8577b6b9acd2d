"""Batched training augmentation on the device: the reference's DataAugmentor.forward with
the KITTI recipe's gt_sampling, random_world_flip, random_world_rotation and random_world_scaling
(pcdet/datasets/augmentor/data_augmentor.py:290-318, database_sampler.py:130-147 / :365-443 / :445-502,
augmentor_utils.py:8-92), limit_period, and the data processor's range mask with the class column
(data_processor.py:79-93, dataset.py:158-215) for a whole batch of raw ragged clouds already in HBM.  The result
chains into input_path.sample_points_batch and PDMSSD.forward in train mode; there is no per-scene host loop.

Two stages, four native calls (csrc/augment.hip): draw (state + seed -> per-scene parameters: sampled database
indices, flip bits, angle, scale) and apply (collision select -> box outputs; scene count -> scan -> fill -> rows).
The reference draws from numpy's global RNG in each dataloader worker, which nothing can replay; here every draw is
a documented function of (seed, state, scene, group) and the per-group (epoch, pointer) state of
sample_with_fixed_number lives in a small device tensor that the draw kernel advances, so the padded form needs no
host synchronisation and replays correctly from a captured graph.  There is no CPU fallback.

Box rows are (B, M, 8) [x, y, z, dx, dy, dz, heading, class]: class > 0 is a target (class index + 1), < 0 a
non-target box (Van, ...) that blocks candidates and is then dropped, 0 padding.
"""
import ctypes
import os
import pickle

import numpy as np
import torch

from . import _native
from .input_path import sample_points_batch

MAX_B, MAX_GROUPS, MAX_SLOTS, MAX_BOXES = 1024, 8, 256, 256
OP_FLIP_X, OP_FLIP_Y, OP_ROT, OP_SCALE = 1, 2, 3, 4
SUPPORTED = ('gt_sampling', 'random_world_flip', 'random_world_rotation', 'random_world_scaling')


def _get(cfg, key, default=None):
    return cfg.get(key, default) if isinstance(cfg, dict) else getattr(cfg, key, default)


def _ptr(t):
    return None if t is None else t.data_ptr()


class GTDatabase:
    """Device-resident ground-truth database: object points (P, C) fp32 relative to their box centre, offsets (N + 1)
    int64 (entry i owns rows offsets[i]:offsets[i + 1]), boxes (N, 7) fp32, class ids (N) int (0-based into
    class_names).  Entries are grouped by class in class_names order, each class keeping its input order, so that
    index j of a class's permutation is the class's j-th entry (db_infos[class][j] of the reference)."""

    def __init__(self, points, offsets, boxes, class_ids, class_names, device):
        self.class_names = list(class_names)
        cid = np.asarray(class_ids, dtype=np.int64)
        order = np.argsort(cid, kind='stable')
        offs = np.asarray(offsets, dtype=np.int64)
        pts = np.asarray(points, dtype=np.float32)
        lens = offs[1:] - offs[:-1]
        if pts.ndim != 2 or pts.shape[1] < 3 or offs[0] != 0 or offs[-1] != pts.shape[0] or (lens < 0).any():
            raise ValueError("GTDatabase: points (P, C >= 3) with offsets (N + 1) from 0 to P expected")
        if cid.size and (cid.min() < 0 or cid.max() >= len(self.class_names)):
            raise ValueError("GTDatabase: class id outside class_names")
        rows = np.concatenate([np.arange(offs[i], offs[i + 1]) for i in order]) if len(order) else np.zeros(0, np.int64)
        self.num_point_features = int(pts.shape[1])
        new_offs = np.concatenate([[0], np.cumsum(lens[order])]).astype(np.int64)
        self.class_ids = cid[order]
        self.counts = np.bincount(self.class_ids, minlength=len(self.class_names)).astype(np.int64)
        self.first = np.concatenate([[0], np.cumsum(self.counts)[:-1]]).astype(np.int64)
        dev = torch.device(device)
        self.points = torch.from_numpy(np.ascontiguousarray(pts[rows].reshape(-1, pts.shape[1]))).to(dev)
        self.offsets = torch.from_numpy(new_offs).to(dev)
        self.boxes = torch.from_numpy(np.ascontiguousarray(np.asarray(boxes, dtype=np.float32).reshape(-1, 7)[order])).to(dev)
        self.host_offsets = new_offs

    def __len__(self):
        return int(self.class_ids.shape[0])

    @classmethod
    def from_arrays(cls, points, offsets, boxes, class_ids, class_names, device):
        """points (P, C) relative to the box centres, offsets (N + 1), boxes (N, 7), class ids (N)."""
        return cls(points, offsets, boxes, class_ids, class_names, device)

    @classmethod
    def from_reference_infos(cls, root, db_info_paths, class_names, prepare, num_point_features, device):
        """The reference's `*_dbinfos_*.pkl` + `gt_database/*.bin` (DataBaseSampler.__init__, database_sampler.py:17-64):
        the infos of class_names in file order, PREPARE's filter_by_difficulty / filter_by_min_points applied once here
        (in PREPARE's order), each object's points read as float32 and, when the count does not match
        num_points_in_gt, as float64 (database_sampler.py:395-398; converted to float32 here)."""
        infos = {c: [] for c in class_names}
        for p in db_info_paths:
            with open(os.path.join(str(root), str(p)), 'rb') as f:
                d = pickle.load(f)
            for c in class_names:
                infos[c].extend(d.get(c, []))
        for name, val in (prepare or {}).items():
            if name == 'filter_by_difficulty':
                infos = {k: [i for i in v if i['difficulty'] not in val] for k, v in infos.items()}
            elif name == 'filter_by_min_points':
                for name_num in val:
                    n, m = name_num.split(':')
                    if int(m) > 0 and n in infos:
                        infos[n] = [i for i in infos[n] if i['num_points_in_gt'] >= int(m)]
            else:
                raise ValueError(f"PREPARE.{name} is not supported")
        pts, offs, boxes, cids = [], [0], [], []
        for k, c in enumerate(class_names):
            for info in infos[c]:
                path = os.path.join(str(root), info['path'])
                p = np.fromfile(path, dtype=np.float32).reshape(-1, num_point_features)
                if p.shape[0] != info['num_points_in_gt']:
                    p = np.fromfile(path, dtype=np.float64).reshape(-1, num_point_features)
                if p.shape[0] != info['num_points_in_gt']:
                    raise ValueError(f"{path}: {p.shape[0]} points, num_points_in_gt {info['num_points_in_gt']}")
                pts.append(p.astype(np.float32))
                offs.append(offs[-1] + p.shape[0])
                boxes.append(np.asarray(info['box3d_lidar'], dtype=np.float32)[:7])
                cids.append(k)
        pts = np.concatenate(pts, 0) if pts else np.zeros((0, num_point_features), np.float32)
        return cls(pts, np.asarray(offs), np.asarray(boxes, np.float32).reshape(-1, 7), cids, class_names, device)


def parse_config(aug_cfg, class_names):
    """DATA_AUGMENTOR (dict with AUG_CONFIG_LIST / DISABLE_AUG_LIST, or the bare list) -> plan dict.  Raises ValueError
    naming the key for anything this augmentor does not implement."""
    if isinstance(aug_cfg, (list, tuple)):
        entries, disabled = list(aug_cfg), []
    else:
        entries, disabled = list(_get(aug_cfg, 'AUG_CONFIG_LIST') or []), list(_get(aug_cfg, 'DISABLE_AUG_LIST') or [])
    plan = {'ops': [], 'sampling': None, 'flip_axes': 0, 'rot': None, 'scale': None}
    seen = set()
    for e in entries:
        name = _get(e, 'NAME')
        if name in disabled:
            continue
        if name not in SUPPORTED:
            raise ValueError(f"{name}: not supported by the device augmentor (supported: {', '.join(SUPPORTED)})")
        if name in seen:
            raise ValueError(f"{name}: configured twice")
        seen.add(name)
        if name == 'gt_sampling':
            if plan['ops']:
                raise ValueError("gt_sampling: must come before the world transforms")
            for key in ('USE_ROAD_PLANE', 'FILTER_OBJ_POINTS_BY_TIMESTAMP', 'DATABASE_WITH_FAKELIDAR'):
                if _get(e, key, False):
                    raise ValueError(f"{key}: not supported by the device augmentor")
            if _get(e, 'IMG_AUG_TYPE', None) is not None:
                raise ValueError("IMG_AUG_TYPE: image copy-paste is not supported by the device augmentor")
            groups = []
            for g in _get(e, 'SAMPLE_GROUPS'):
                cname, num = str(g).split(':')
                if cname in class_names and int(num) > 0 and cname not in [x[0] for x in groups]:
                    groups.append((cname, int(num)))
            extra = [float(x) for x in (_get(e, 'REMOVE_EXTRA_WIDTH') or [0.0, 0.0, 0.0])]
            plan['sampling'] = {'groups': groups, 'limit': bool(_get(e, 'LIMIT_WHOLE_SCENE', False)), 'extra': extra}
        elif name == 'random_world_flip':
            for ax in _get(e, 'ALONG_AXIS_LIST'):
                if ax not in ('x', 'y'):
                    raise ValueError(f"ALONG_AXIS_LIST: axis {ax!r}")
                op = OP_FLIP_X if ax == 'x' else OP_FLIP_Y
                if op not in plan['ops']:
                    plan['ops'].append(op)
                    plan['flip_axes'] |= 1 if ax == 'x' else 2
        elif name == 'random_world_rotation':
            r = _get(e, 'WORLD_ROT_ANGLE')
            if not isinstance(r, (list, tuple)):
                r = [-r, r]
            plan['rot'] = (float(r[0]), float(r[1]))
            plan['ops'].append(OP_ROT)
        else:
            r = _get(e, 'WORLD_SCALE_RANGE')
            if r[1] - r[0] >= 1e-3:          # global_scaling returns without a draw otherwise
                plan['scale'] = (float(r[0]), float(r[1]))
                plan['ops'].append(OP_SCALE)
    plan['ops_code'] = sum(op << (4 * k) for k, op in enumerate(plan['ops']))
    return plan


class BatchAugmentor:
    """aug_cfg: the reference's DATA_AUGMENTOR (dict / list form); point_cloud_range: 6 floats; database: GTDatabase
    (needed with gt_sampling); seed: 32-bit key of every draw.  `state` (int32 device tensor [step, (epoch, pointer)
    per group]) starts as the reference's sampler does (pointer = class size: the first draw permutes)."""

    def __init__(self, aug_cfg, point_cloud_range, class_names, database=None, seed=0, remove_outside_boxes=True,
                 device=None):
        self.class_names = list(class_names)
        self.plan = parse_config(aug_cfg, self.class_names)
        self.range = [float(x) for x in point_cloud_range]
        if len(self.range) != 6:
            raise ValueError("point_cloud_range: 6 values expected")
        self.seed = int(seed) & 0xffffffff
        self.remove_outside = bool(remove_outside_boxes)
        smp = self.plan['sampling']
        self.database = database
        groups = smp['groups'] if smp else []
        if smp is not None:
            if database is None:
                raise ValueError("gt_sampling: a GTDatabase is required")
            if database.class_names != self.class_names:
                raise ValueError("gt_sampling: the database's class_names differ from the augmentor's")
        if len(groups) > MAX_GROUPS or sum(n for _, n in groups) > MAX_SLOTS:
            raise ValueError(f"SAMPLE_GROUPS: at most {MAX_GROUPS} groups and {MAX_SLOTS} samples per scene")
        self.g_cls = [self.class_names.index(c) for c, _ in groups]
        self.g_num = [n for _, n in groups]
        self.g_len = [int(database.counts[k]) for k in self.g_cls] if groups else []
        self.g_first = [int(database.first[k]) for k in self.g_cls] if groups else []
        for (c, _), n in zip(groups, self.g_len):
            if n == 0:
                raise ValueError(f"SAMPLE_GROUPS: the database holds no {c} entries")
        self.K = sum(self.g_num)
        self.extra = smp['extra'] if smp else [0.0, 0.0, 0.0]
        self.limit = bool(smp['limit']) if smp else False
        dev = database.points.device if database is not None else torch.device(device or 'cuda')
        self.device = dev
        self.state = torch.tensor([0] + sum([[-1, n] for n in self.g_len], []), dtype=torch.int32, device=dev)
        if database is None:   # empty stand-ins so that every pointer handed to the kernels is valid
            self._db = (torch.zeros((1, 3), dtype=torch.float32, device=dev), torch.zeros((1,), dtype=torch.int64, device=dev),
                        torch.zeros((1, 7), dtype=torch.float32, device=dev), 0)
        else:
            self._db = (database.points, database.offsets, database.boxes, len(database))
        self._ws = None

    def workspace(self, B):
        n = int(_native.lib().pdm_augment_workspace_bytes(B, self.K))
        if self._ws is None or self._ws.numel() < n:
            self._ws = torch.empty((max(n, 256),), dtype=torch.uint8, device=self.device)
        return self._ws

    def _check(self, raw, counts, gt_boxes):
        assert raw.is_cuda and raw.dtype == torch.float32 and raw.is_contiguous() and raw.dim() == 2
        assert counts.is_cuda and counts.dtype == torch.int32 and counts.is_contiguous() and counts.dim() == 1
        assert gt_boxes.is_cuda and gt_boxes.dtype == torch.float32 and gt_boxes.is_contiguous() and gt_boxes.dim() == 3
        B, M = gt_boxes.shape[0], gt_boxes.shape[1]
        if B != counts.numel() or gt_boxes.shape[2] != 8:
            raise ValueError("gt_boxes must be (B, M, 8) with B = counts.numel()")
        if not 1 <= B <= MAX_B or M > MAX_BOXES:
            raise ValueError(f"B={B}, M={M}: at most {MAX_B} scenes of {MAX_BOXES} boxes")
        if self.database is not None and self.K and raw.shape[1] != self.database.num_point_features:
            raise ValueError(f"scene points have {raw.shape[1]} features, the database {self.database.num_point_features}")
        return B, M

    def draw(self, counts, gt_boxes):
        """state + seed -> params dict {'sampled' (B, K) int32, 'flip' (B) int32, 'angle' (B), 'scale' (B)}; advances
        self.state (the step counter and every group's epoch / pointer)."""
        B, M = gt_boxes.shape[0], gt_boxes.shape[1]
        dev = gt_boxes.device
        p = {'sampled': torch.empty((B, self.K), dtype=torch.int32, device=dev),
             'flip': torch.empty((B,), dtype=torch.int32, device=dev),
             'angle': torch.empty((B,), dtype=torch.float32, device=dev),
             'scale': torch.empty((B,), dtype=torch.float32, device=dev)}
        ws = self.workspace(B)
        rot = self.plan['rot'] or (0.0, 0.0)
        sc = self.plan['scale'] or (1.0, 1.0)
        G = len(self.g_num)
        g_cls, g_num, g_len, g_first = (_native.host_array(ctypes.c_int, v) for v in (self.g_cls, self.g_num, self.g_len, self.g_first))
        _native.call("pdm_augment_draw", _native.stream(dev), B, G, g_cls, g_num, g_len, g_first, 1 if self.limit else 0, M,
                     gt_boxes.data_ptr(), self.seed, self.state.data_ptr(), self.plan['flip_axes'],
                     1 if self.plan['rot'] else 0, rot[0], rot[1], 1 if self.plan['scale'] else 0, sc[0], sc[1], self.K,
                     _ptr(p['sampled']) if self.K else None, p['flip'].data_ptr(), p['angle'].data_ptr(),
                     p['scale'].data_ptr(), ws.data_ptr(), ws.numel())
        return p

    def _apply_boxes(self, gt_boxes, params):
        B, M = gt_boxes.shape[0], gt_boxes.shape[1]
        dev = gt_boxes.device
        M_out = M + self.K
        out = {'boxes': torch.empty((B, M_out, 8), dtype=torch.float32, device=dev),
               'box_counts': torch.empty((B,), dtype=torch.int32, device=dev),
               'accepted': torch.empty((B, self.K), dtype=torch.int32, device=dev),
               'num_accepted': torch.empty((B,), dtype=torch.int32, device=dev)}
        ws = self.workspace(B)
        pts, offs, boxes, n = self._db
        _native.call("pdm_augment_select", _native.stream(dev), B, M, gt_boxes.data_ptr(),
                     len(self.g_num), _native.host_array(ctypes.c_int, self.g_cls), _native.host_array(ctypes.c_int, self.g_num), n,
                     boxes.data_ptr(), offs.data_ptr(),
                     self.K, _ptr(params['sampled']) if self.K else None, params['flip'].data_ptr(),
                     params['angle'].data_ptr(), params['scale'].data_ptr(), self.plan['ops_code'],
                     _native.host_array(ctypes.c_float, self.range), 1 if self.remove_outside else 0, M_out, out['boxes'].data_ptr(),
                     out['box_counts'].data_ptr(), _ptr(out['accepted']) if self.K else None,
                     out['num_accepted'].data_ptr(), ws.data_ptr(), ws.numel())
        return out

    def _scene(self, fn, raw, counts, out, capacity, rows):
        B = counts.numel()
        ws = self.workspace(B)
        pts, offs, boxes, _ = self._db
        _native.call(fn, _native.stream(raw.device), B, raw.shape[1], raw.data_ptr(),
                     counts.data_ptr(), pts.data_ptr(), offs.data_ptr(), boxes.data_ptr(), self.K,
                     _ptr(out['accepted']) if self.K else None, out['num_accepted'].data_ptr(),
                     out['params']['flip'].data_ptr(), out['params']['angle'].data_ptr(), out['params']['scale'].data_ptr(),
                     self.plan['ops_code'], _native.host_array(ctypes.c_float, self.range),
                     _native.host_array(ctypes.c_float, self.extra), int(capacity),
                     out['counts'].data_ptr(), out['overflow'].data_ptr(), _ptr(rows), ws.data_ptr(), ws.numel())

    def _front(self, raw, counts, gt_boxes, params):
        B, M = self._check(raw, counts, gt_boxes)
        if params is None:
            params = self.draw(counts, gt_boxes)
        else:
            params = self._given(params, B)
        out = self._apply_boxes(gt_boxes, params)
        out['params'] = params
        out['counts'] = torch.empty((B,), dtype=torch.int32, device=raw.device)
        out['overflow'] = torch.empty((1,), dtype=torch.int32, device=raw.device)
        return out

    def _given(self, params, B):
        dev = self.device
        p = {'sampled': torch.as_tensor(params.get('sampled', np.full((B, self.K), -1)), dtype=torch.int32, device=dev),
             'flip': torch.as_tensor(params.get('flip', np.zeros(B)), dtype=torch.int32, device=dev),
             'angle': torch.as_tensor(params.get('angle', np.zeros(B)), dtype=torch.float32, device=dev),
             'scale': torch.as_tensor(params.get('scale', np.ones(B)), dtype=torch.float32, device=dev)}
        p = {k: v.contiguous() for k, v in p.items()}
        if tuple(p['sampled'].shape) != (B, self.K) or any(p[k].shape != (B,) for k in ('flip', 'angle', 'scale')):
            raise ValueError(f"params: sampled (B, {self.K}) and flip / angle / scale (B,) expected")
        return p

    def augment_padded(self, raw, counts, gt_boxes, capacity_rows, params=None, out_rows=None):
        """No host synchronisation; capturable in a torch.cuda.graph.  raw (sum counts, C) fp32, counts (B) int32 and
        gt_boxes (B, M, 8) on the device -> dict of device tensors:
          rows (capacity_rows, C)   the augmented clouds, scene after scene (counts[b] rows each)
          counts (B) int32          rows per scene (the true counts, also when they overflow the capacity)
          boxes (B, M + K, 8)       [target boxes] + [accepted samples], zero-padded; box_counts (B) int32
          accepted (B, K) int32     database index of each accepted sample, in acceptance order, -1 padded;
          num_accepted (B) int32;   params: the draws used (or the given ones)
          overflow (1) int32        1: the rows did not fit; nothing was written past capacity_rows.
        params: optional dict of explicit draws (sampled database indices (B, K) -1 padded, each group owning its
        SAMPLE_NUM slots in config order; flip (B) bits 1 = x, 2 = y; angle (B); scale (B)); the state is not advanced.
        out_rows: optional contiguous (>= capacity_rows, C) fp32 device buffer for the rows."""
        out = self._front(raw, counts, gt_boxes, params)
        if out_rows is not None:
            assert out_rows.is_contiguous() and out_rows.dtype == torch.float32 and out_rows.shape[1] == raw.shape[1]
            assert out_rows.shape[0] >= capacity_rows
            rows = out_rows
        else:
            rows = torch.empty((max(int(capacity_rows), 1), raw.shape[1]), dtype=torch.float32, device=raw.device)
        self._scene("pdm_augment_scene_count", raw, counts, out, capacity_rows, rows)
        self._scene("pdm_augment_scene_fill", raw, counts, out, capacity_rows, rows)
        out['rows'] = rows[:int(capacity_rows)]
        return out

    def __call__(self, raw, counts, gt_boxes, params=None):
        """As augment_padded, sized exactly after ONE device-to-host read (row counts and box counts together):
        rows (sum counts, C), boxes (B, max box count, 8), and host_counts (list)."""
        out = self._front(raw, counts, gt_boxes, params)
        self._scene("pdm_augment_scene_count", raw, counts, out, 0, None)
        fetched = torch.cat([out['counts'], out['box_counts']]).cpu().tolist()
        B = counts.numel()
        host_counts, nbox = fetched[:B], max(fetched[B:] + [0])
        total = sum(host_counts)
        rows = torch.empty((max(total, 1), raw.shape[1]), dtype=torch.float32, device=raw.device)
        self._scene("pdm_augment_scene_fill", raw, counts, out, total, rows)
        out['rows'] = rows[:total]
        out['boxes'] = out['boxes'][:, :nbox].contiguous()
        out['host_counts'] = host_counts
        out['overflow'].zero_()
        return out

    def augment_and_sample(self, raw, counts, gt_boxes, num_points, sample_seed=0, params=None):
        """-> (points (B * num_points, 1 + C) [scene, x, y, z, ...], gt_boxes (B, max boxes, 8)) ready for
        PDMSSD.forward in train mode: __call__ followed by input_path.sample_points_batch."""
        out = self(raw, counts, gt_boxes, params=params)
        points = sample_points_batch(out['rows'], out['counts'], num_points, seed=sample_seed, host_counts=out['host_counts'])
        return points, out['boxes']

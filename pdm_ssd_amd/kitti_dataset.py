"""KITTI dataset front end: from a KITTI directory to the info pickles, the ground-truth
database and detector-ready batches, with the per-point work on the device (csrc/kitti_data.hip, `pdm_kitti_data_*`).

What the reference does per frame on CPU workers (pcdet/datasets/kitti/kitti_dataset.py: get_infos :150-222,
create_groundtruth_database :224-275, __getitem__ :371-428, create_kitti_infos :431-470) is done here for a batch of
frames at once: files are read by a small thread pool, the clouds go to the device in one upload, and the FOV flags, the
per-object point counts and the database points come from count -> scan -> fill kernels without atomics.  The files
written (kitti_infos_*.pkl, kitti_dbinfos_*.pkl, gt_database/*.bin) have the reference's names, keys, order and dtypes
and load with nothing but numpy, so either side can read the other's.  There is no CPU fallback for the device work.

    python -m pdm_ssd_amd.kitti_dataset create_kitti_infos ROOT [SAVE_PATH]
"""
import concurrent.futures as futures
import copy
import os
import pickle
import struct
import sys

import numpy as np
import torch

from . import _native
from .augment import MAX_BOXES, BatchAugmentor, GTDatabase
from .input_path import read_velodyne_bin, sample_points_batch, upload_raw
from .kitti_eval import stack_calib

MAX_WORKERS = 16          # file readers are I/O-bound: a fixed ceiling, never sized by os.cpu_count()
DEFAULT_CFG = {'FOV_POINTS_ONLY': True, 'NUM_POINT_FEATURES': 4,
               'POINT_CLOUD_RANGE': [0.0, -40.0, -3.0, 70.4, 40.0, 1.0],
               'INFO_PATH': {'train': ['kitti_infos_train.pkl'], 'val': ['kitti_infos_val.pkl'],
                             'trainval': ['kitti_infos_trainval.pkl'], 'test': ['kitti_infos_test.pkl']}}


def pool_size(num_workers):
    """size of the file-reading thread pool: the request clipped to [1, MAX_WORKERS]"""
    return max(1, min(int(num_workers), MAX_WORKERS))


# ---- files -------------------------------------------------------------------------------------------------------------

class Calibration:
    """KITTI calibration: a calib/*.txt file or a dict with P2 (3, 4), R0 (3, 3), Tr_velo2cam (3, 4); float32 fields as
    calibration_kitti.get_calib_from_file reads them (lines 3-6 of the file: P2, P3, R0_rect, Tr_velo_to_cam)."""

    def __init__(self, calib):
        if not isinstance(calib, dict):
            with open(str(calib)) as f:
                lines = f.readlines()

            def row(k, shape):
                return np.array(lines[k].strip().split(' ')[1:], dtype=np.float32).reshape(shape)
            calib = {'P2': row(2, (3, 4)), 'P3': row(3, (3, 4)), 'R0': row(4, (3, 3)), 'Tr_velo2cam': row(5, (3, 4))}
        self.P2 = calib['P2']
        self.R0 = calib['R0']
        self.V2C = calib['Tr_velo2cam'] if 'Tr_velo2cam' in calib else calib['V2C']
        self.P3 = calib.get('P3')

    @staticmethod
    def _hom(pts):
        return np.hstack((pts, np.ones((pts.shape[0], 1), dtype=np.float32)))

    def _ext(self):
        R0 = np.zeros((4, 4), dtype=np.float32)
        R0[:3, :3] = self.R0
        R0[3, 3] = 1
        V2C = np.zeros((4, 4), dtype=np.float32)
        V2C[:3] = self.V2C
        V2C[3, 3] = 1
        return R0, V2C

    def lidar_to_rect(self, pts_lidar):
        return np.dot(self._hom(pts_lidar), np.dot(self.V2C.T, self.R0.T))

    def rect_to_lidar(self, pts_rect):
        R0, V2C = self._ext()
        return np.dot(self._hom(pts_rect), np.linalg.inv(np.dot(R0, V2C).T))[:, 0:3]

    def rect_to_img(self, pts_rect):
        hom = self._hom(pts_rect)
        img = np.dot(hom, self.P2.T)
        return (img[:, 0:2].T / hom[:, 2]).T, img[:, 2] - self.P2.T[3, 2]

    def lidar_to_img(self, pts_lidar):
        return self.rect_to_img(self.lidar_to_rect(pts_lidar))

    def corners3d_to_img_boxes(self, corners3d):
        """(N, 8, 3) rect corners -> (boxes (N, 4) [x1, y1, x2, y2], corners (N, 8, 2)) in the image"""
        hom = np.concatenate((corners3d, np.ones((corners3d.shape[0], 8, 1))), axis=2)
        img = np.matmul(hom, self.P2.T)
        x, y = img[:, :, 0] / img[:, :, 2], img[:, :, 1] / img[:, :, 2]
        boxes = np.stack((x.min(1), y.min(1), x.max(1), y.max(1)), axis=1)
        return boxes, np.stack((x, y), axis=2)


def fov_flag_numpy(points_xyz, calib, image_shape):
    """get_fov_flag in float64 in the device's operation order (csrc/kitti_data.hip): the restatement the device equals
    bit for bit.  points (N, 3) float32, image_shape [height, width]."""
    p = np.asarray(points_xyz, dtype=np.float32).astype(np.float64)
    V, R, P = (np.asarray(m, dtype=np.float32).astype(np.float64) for m in (calib.V2C, calib.R0, calib.P2))
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    cam = [((V[j, 0] * x + V[j, 1] * y) + V[j, 2] * z) + V[j, 3] for j in range(3)]
    rect = [(R[i, 0] * cam[0] + R[i, 1] * cam[1]) + R[i, 2] * cam[2] for i in range(3)]
    hom = [((P[k, 0] * rect[0] + P[k, 1] * rect[1]) + P[k, 2] * rect[2]) + P[k, 3] for k in range(3)]
    with np.errstate(divide='ignore', invalid='ignore'):
        u, v = hom[0] / rect[2], hom[1] / rect[2]
    depth = hom[2] - P[2, 3]
    h, w = float(image_shape[0]), float(image_shape[1])
    return (u >= 0) & (u < w) & (v >= 0) & (v < h) & (depth >= 0)


def kitti_obj_level(bbox, truncation, occlusion):
    """get_kitti_obj_level: 0 easy, 1 moderate, 2 hard, -1 unknown"""
    height = float(bbox[3]) - float(bbox[1]) + 1
    if height >= 40 and truncation <= 0.15 and occlusion <= 0:
        return 0
    if height >= 25 and truncation <= 0.3 and occlusion <= 1:
        return 1
    if height >= 25 and truncation <= 0.5 and occlusion <= 2:
        return 2
    return -1


def read_label(path):
    """a label_2/*.txt file -> the label fields of the reference's annotation dict, dtype for dtype: name (str),
    truncated / occluded / alpha / rotation_y / score (float64), bbox (n, 4) and location (n, 3) float32, dimensions
    (n, 3) float64 [l, h, w], difficulty int32."""
    with open(str(path)) as f:
        rows = [line.strip().split(' ') for line in f.readlines()]
    n = len(rows)
    out = {'name': np.array([r[0] for r in rows]),
           'truncated': np.array([float(r[1]) for r in rows]),
           'occluded': np.array([float(r[2]) for r in rows]),
           'alpha': np.array([float(r[3]) for r in rows]),
           'bbox': np.array([[float(v) for v in r[4:8]] for r in rows], dtype=np.float32).reshape(n, 4),
           'dimensions': np.array([[float(r[10]), float(r[8]), float(r[9])] for r in rows]).reshape(n, 3),
           'location': np.array([[float(v) for v in r[11:14]] for r in rows], dtype=np.float32).reshape(n, 3),
           'rotation_y': np.array([float(r[14]) for r in rows]),
           'score': np.array([float(r[15]) if len(r) == 16 else -1.0 for r in rows])}
    out['difficulty'] = np.array([kitti_obj_level(out['bbox'][k], out['truncated'][k], out['occluded'][k]) for k in range(n)],
                                 np.int32)
    return out


def image_shape(path):
    """[height, width] int32 of a PNG, read from its IHDR chunk (no image library)"""
    with open(str(path), 'rb') as f:
        head = f.read(24)
    if len(head) < 24 or head[:8] != b'\x89PNG\r\n\x1a\n' or head[12:16] != b'IHDR':
        raise ValueError(f"{path}: not a PNG file")
    w, h = struct.unpack('>II', head[16:24])
    return np.array([h, w], dtype=np.int32)


def read_split(root, split):
    """ImageSets/<split>.txt -> list of frame ids, or None when the file is absent"""
    path = os.path.join(str(root), 'ImageSets', split + '.txt')
    if not os.path.exists(path):
        return None
    with open(path) as f:
        return [x.strip() for x in f.readlines()]


def boxes3d_kitti_camera_to_lidar(boxes3d_camera, calib):
    """(N, 7) [x, y, z, l, h, w, r] in rect camera coordinates -> [x, y, z, dx, dy, dz, heading], z the box centre"""
    b = np.array(boxes3d_camera, copy=True)
    xyz = calib.rect_to_lidar(b[:, 0:3])
    xyz[:, 2] += b[:, 4] / 2
    return np.concatenate([xyz, b[:, 3:4], b[:, 5:6], b[:, 4:5], -(b[:, 6:7] + np.pi / 2)], axis=-1)


def class_column(names, class_names):
    """BatchAugmentor's convention: > 0 target (class index + 1), < 0 a known non-target name"""
    return np.array([class_names.index(n) + 1 if n in class_names else -1 for n in names], dtype=np.float32)


def _calib_of_info(info):
    c = info['calib']
    return Calibration({'P2': np.asarray(c['P2'], dtype=np.float32)[:3], 'R0': np.asarray(c['R0_rect'], dtype=np.float32)[:3, :3],
                        'Tr_velo2cam': np.asarray(c['Tr_velo_to_cam'], dtype=np.float32)[:3]})


# ---- device calls ------------------------------------------------------------------------------------------------------

def _check_frames(raw, counts, calib, shape):
    assert raw.is_cuda and raw.dtype == torch.float32 and raw.is_contiguous() and raw.dim() == 2
    assert counts.is_cuda and counts.dtype == torch.int32 and counts.is_contiguous() and counts.dim() == 1
    B = counts.numel()
    if not 1 <= B <= 1024:
        raise ValueError(f"B={B}: 1 to 1024 frames per call")
    assert shape.is_cuda and shape.dtype == torch.int32 and shape.is_contiguous() and tuple(shape.shape) == (B, 2)
    for k, s in (('V2C', (B, 3, 4)), ('R0', (B, 3, 3)), ('P2', (B, 3, 4))):
        m = calib[k]
        assert m.is_cuda and m.dtype == torch.float32 and m.is_contiguous() and tuple(m.shape) == s, k
    return B


def _frame_args(raw, counts, calib, shape):
    return (counts.numel(), raw.shape[1], raw.shape[0], raw.data_ptr(), counts.data_ptr(), calib['V2C'].data_ptr(),
            calib['R0'].data_ptr(), calib['P2'].data_ptr(), shape.data_ptr())


def fov_workspace(B, device):
    n = int(_native.lib().pdm_kitti_data_fov_workspace_bytes(B))
    return torch.empty((max(n, 256),), dtype=torch.uint8, device=device)


def boxes_workspace(B, M, device):
    n = int(_native.lib().pdm_kitti_data_boxes_workspace_bytes(B, M))
    return torch.empty((max(n, 256),), dtype=torch.uint8, device=device)


def fov_crop_padded(raw, counts, calib, image_shape, capacity_rows=None, out_rows=None, workspace=None, flags=False):
    """FOV_POINTS_ONLY for a batch, without host synchronisation (capturable in a torch.cuda.graph): raw (sum counts, C)
    fp32, counts (B) int32, calib {'V2C', 'R0', 'P2'} (kitti_eval.stack_calib) and image_shape (B, 2) int32 on the
    device -> {'rows' (capacity_rows, C): the kept rows, frame after frame in input order, packed as the augmentor reads
    them; 'counts' (B) int32: kept rows per frame; 'overflow' (1) int32: the total exceeds capacity_rows (nothing is
    written past it); 'flags' (sum counts) uint8 when asked}.  capacity_rows defaults to raw.shape[0], which a crop
    cannot exceed."""
    B = _check_frames(raw, counts, calib, image_shape)
    dev = raw.device
    cap = int(raw.shape[0] if capacity_rows is None else capacity_rows)
    if out_rows is not None:
        assert out_rows.is_contiguous() and out_rows.dtype == torch.float32 and out_rows.shape[1] == raw.shape[1]
        assert out_rows.shape[0] >= cap
        rows = out_rows
    else:
        rows = torch.empty((max(cap, 1), raw.shape[1]), dtype=torch.float32, device=dev)
    ws = workspace if workspace is not None else fov_workspace(B, dev)
    out = {'counts': torch.empty((B,), dtype=torch.int32, device=dev),
           'overflow': torch.empty((1,), dtype=torch.int32, device=dev)}
    fl = torch.empty((max(raw.shape[0], 1),), dtype=torch.uint8, device=dev) if flags else None
    args = _frame_args(raw, counts, calib, image_shape) + (cap, out['counts'].data_ptr(), out['overflow'].data_ptr())
    _native.call("pdm_kitti_data_fov_count", _native.stream(raw), *args, None if fl is None else fl.data_ptr(), ws.data_ptr(), ws.numel())
    _native.call("pdm_kitti_data_fov_fill", _native.stream(raw), *args, rows.data_ptr(), ws.data_ptr(), ws.numel())
    out['rows'] = rows[:cap]
    if flags:
        out['flags'] = fl[:raw.shape[0]]
    return out


def fov_crop(raw, counts, calib, image_shape, workspace=None, flags=False):
    """As fov_crop_padded, sized exactly after ONE device-to-host read of the kept counts: rows (sum kept, C), counts
    (B) int32 on the device and host_counts (list)."""
    B = _check_frames(raw, counts, calib, image_shape)
    dev = raw.device
    ws = workspace if workspace is not None else fov_workspace(B, dev)
    out = {'counts': torch.empty((B,), dtype=torch.int32, device=dev),
           'overflow': torch.empty((1,), dtype=torch.int32, device=dev)}
    fl = torch.empty((max(raw.shape[0], 1),), dtype=torch.uint8, device=dev) if flags else None
    front = _frame_args(raw, counts, calib, image_shape)
    tail = (out['counts'].data_ptr(), out['overflow'].data_ptr())
    _native.call("pdm_kitti_data_fov_count", _native.stream(raw), *front, 0, *tail, None if fl is None else fl.data_ptr(), ws.data_ptr(),
                 ws.numel())
    host = out['counts'].cpu().tolist()
    total = sum(host)
    rows = torch.empty((max(total, 1), raw.shape[1]), dtype=torch.float32, device=dev)
    _native.call("pdm_kitti_data_fov_fill", _native.stream(raw), *front, total, *tail, rows.data_ptr(), ws.data_ptr(), ws.numel())
    out['rows'] = rows[:total]
    out['host_counts'] = host
    out['overflow'].zero_()
    if flags:
        out['flags'] = fl[:raw.shape[0]]
    return out


def pad_boxes(boxes_per_frame, device):
    """list of (n_i, 7) float64 lidar boxes (gt_boxes_lidar of the infos) -> (boxes (B, M, 7) fp32: what the membership
    tests see, box_count (B) int32, centres (B, M, 3) float64: what the object points are shifted by), on the device."""
    B = len(boxes_per_frame)
    M = max([len(b) for b in boxes_per_frame] + [1])
    if M > MAX_BOXES:
        raise ValueError(f"{M} boxes in a frame: at most {MAX_BOXES}")
    b32 = np.zeros((B, M, 7), dtype=np.float32)
    ctr = np.zeros((B, M, 3), dtype=np.float64)
    for k, b in enumerate(boxes_per_frame):
        b = np.asarray(b, dtype=np.float64).reshape(-1, 7)
        b32[k, :len(b)] = b.astype(np.float32)
        ctr[k, :len(b)] = b[:, :3]
    cnt = np.array([len(b) for b in boxes_per_frame], dtype=np.int32)
    return torch.from_numpy(b32).to(device), torch.from_numpy(cnt).to(device), torch.from_numpy(ctr).to(device)


class BoxMembership:
    """num_points_in_gt and the ground-truth database of a batch of frames (pdm_kitti_data_boxes_count / _fill).

        m = BoxMembership(raw, counts, calib, image_shape, boxes, box_count)      # count pass, no synchronisation
        m.num_points_in_gt, m.db_count                                            # (B, M) int32 device tensors
        points, offsets, out_boxes = m.gather(centres)                            # one host read (the totals), then fill
    """

    def __init__(self, raw, counts, calib, image_shape, boxes, box_count, workspace=None):
        B = _check_frames(raw, counts, calib, image_shape)
        assert boxes.is_cuda and boxes.dtype == torch.float32 and boxes.is_contiguous() and boxes.dim() == 3
        assert boxes.shape[0] == B and boxes.shape[2] == 7
        assert box_count.is_cuda and box_count.dtype == torch.int32 and box_count.is_contiguous() and box_count.shape == (B,)
        M = boxes.shape[1]
        if M > MAX_BOXES:
            raise ValueError(f"M={M}: at most {MAX_BOXES} boxes per frame")
        dev = raw.device
        self.raw, self.counts, self.calib, self.shape, self.boxes, self.box_count = raw, counts, calib, image_shape, boxes, box_count
        self.ws = workspace if workspace is not None else boxes_workspace(B, M, dev)
        self.num_points_in_gt = torch.empty((B, M), dtype=torch.int32, device=dev)
        self.db_count = torch.empty((B, M), dtype=torch.int32, device=dev)
        self.totals = torch.empty((2,), dtype=torch.int64, device=dev)
        _native.call("pdm_kitti_data_boxes_count", _native.stream(raw), *self._args(), *self._outs(), self.ws.data_ptr(), self.ws.numel())

    def _args(self):
        return _frame_args(self.raw, self.counts, self.calib, self.shape) + (
            self.boxes.shape[1], self.boxes.data_ptr(), self.box_count.data_ptr())

    def _outs(self):
        return (self.num_points_in_gt.data_ptr(), self.db_count.data_ptr(), self.totals.data_ptr())

    def gather(self, centres, totals=None):
        """centres (B, M, 3) float64 -> (points (P, C) fp32 relative to the centres, offsets (N + 1) int64, boxes (N, 7))
        on the device: GTDatabase's layout, entries frame after frame, box after box.  totals: (P, N) if already read."""
        assert centres.is_cuda and centres.dtype == torch.float64 and centres.is_contiguous()
        assert tuple(centres.shape) == (self.boxes.shape[0], self.boxes.shape[1], 3)
        P, N = (int(v) for v in (self.totals.cpu().tolist() if totals is None else totals))
        dev, C = self.raw.device, self.raw.shape[1]
        points = torch.empty((max(P, 1), C), dtype=torch.float32, device=dev)
        offsets = torch.empty((N + 1,), dtype=torch.int64, device=dev)
        out_boxes = torch.empty((max(N, 1), 7), dtype=torch.float32, device=dev)
        a = self._args()
        _native.call("pdm_kitti_data_boxes_fill", _native.stream(self.raw), *a, centres.data_ptr(), *self._outs(), P, N, points.data_ptr(),
                     offsets.data_ptr(), out_boxes.data_ptr(), self.ws.data_ptr(), self.ws.numel())
        return points[:P], offsets, out_boxes[:N]


# ---- the dataset -------------------------------------------------------------------------------------------------------

class KittiDataset:
    """root: the KITTI directory (ImageSets/, training/, testing/); class_names: the target classes; split: 'train' |
    'val' | 'trainval' | 'test'; cfg: DEFAULT_CFG keys (FOV_POINTS_ONLY, NUM_POINT_FEATURES, POINT_CLOUD_RANGE,
    INFO_PATH).  Info pickles of the split found under root are loaded into self.infos."""

    def __init__(self, root, class_names, split='train', cfg=None, device=None, load_infos=True):
        self.root = str(root)
        self.class_names = list(class_names)
        self.cfg = dict(DEFAULT_CFG)
        self.cfg.update(cfg or {})
        self.device = torch.device(device) if device is not None else torch.device('cuda:0')
        self.num_point_features = int(self.cfg['NUM_POINT_FEATURES'])
        self.infos = []
        self.set_split(split)
        if load_infos:
            for p in (self.cfg['INFO_PATH'] or {}).get(split, []):
                path = os.path.join(self.root, p)
                if os.path.exists(path):
                    with open(path, 'rb') as f:
                        self.infos.extend(pickle.load(f))

    def set_split(self, split):
        self.split = split
        self.split_dir = os.path.join(self.root, 'training' if split != 'test' else 'testing')
        self.sample_id_list = read_split(self.root, split)

    def __len__(self):
        return len(self.infos)

    def lidar_path(self, idx):
        return os.path.join(self.split_dir, 'velodyne', '%s.bin' % idx)

    def get_lidar(self, idx):
        return read_velodyne_bin(self.lidar_path(idx), self.num_point_features)

    def get_calib(self, idx):
        return Calibration(os.path.join(self.split_dir, 'calib', '%s.txt' % idx))

    def get_label(self, idx):
        return read_label(os.path.join(self.split_dir, 'label_2', '%s.txt' % idx))

    def get_image_shape(self, idx):
        return image_shape(os.path.join(self.split_dir, 'image_2', '%s.png' % idx))

    # -- infos
    def _host_info(self, idx, has_label, read_points):
        """everything of one frame's info that needs no point: one pool task"""
        info = {'point_cloud': {'num_features': 4, 'lidar_idx': idx},
                'image': {'image_idx': idx, 'image_shape': self.get_image_shape(idx)}}
        calib = self.get_calib(idx)
        last = np.array([[0., 0., 0., 1.]])
        R0 = np.zeros([4, 4], dtype=calib.R0.dtype)
        R0[3, 3] = 1.
        R0[:3, :3] = calib.R0
        info['calib'] = {'P2': np.concatenate([calib.P2, last], axis=0), 'R0_rect': R0,
                         'Tr_velo_to_cam': np.concatenate([calib.V2C, last], axis=0)}
        if has_label:
            annos = self.get_label(idx)
            num_gt = len(annos['name'])
            num_objects = int((annos['name'] != 'DontCare').sum()) if num_gt else 0
            annos['index'] = np.array(list(range(num_objects)) + [-1] * (num_gt - num_objects), dtype=np.int32)
            loc, dims, rots = annos['location'][:num_objects], annos['dimensions'][:num_objects], annos['rotation_y'][:num_objects]
            loc_lidar = calib.rect_to_lidar(loc)
            l, h, w = dims[:, 0:1], dims[:, 1:2], dims[:, 2:3]
            loc_lidar[:, 2] += h[:, 0] / 2
            annos['gt_boxes_lidar'] = np.concatenate([loc_lidar, l, w, h, -(np.pi / 2 + rots[..., np.newaxis])], axis=1)
            info['annos'] = annos
        points = self.get_lidar(idx) if read_points else None
        return info, calib, points

    def get_infos(self, num_workers=4, has_label=True, count_inside_pts=True, sample_id_list=None, batch_frames=16):
        """The reference's info dicts, key for key and dtype for dtype.  Files are read by a pool of at most 16 threads;
        with count_inside_pts the frames go to the device batch_frames at a time, one launch sequence and one host read
        (the counts) per batch."""
        ids = list(sample_id_list if sample_id_list is not None else self.sample_id_list)
        count = bool(has_label and count_inside_pts)
        infos = []
        with futures.ThreadPoolExecutor(pool_size(num_workers)) as pool:
            for lo in range(0, len(ids), max(int(batch_frames), 1)):
                batch = list(pool.map(lambda i: self._host_info(i, has_label, count), ids[lo:lo + max(int(batch_frames), 1)]))
                if count:
                    nums = self._count_batch(batch)
                    for (info, _, _), n in zip(batch, nums):
                        info['annos']['num_points_in_gt'] = n
                infos.extend(info for info, _, _ in batch)
        return infos

    def _frames_to_device(self, clouds, calibs, shapes):
        raw, counts, _ = upload_raw(clouds, self.device)
        calib = stack_calib(calibs, self.device)
        shape = torch.from_numpy(np.stack([np.asarray(s, dtype=np.int32) for s in shapes])).to(self.device)
        return raw, counts, calib, shape

    def _count_batch(self, batch):
        raw, counts, calib, shape = self._frames_to_device([p for _, _, p in batch], [c for _, c, _ in batch],
                                                           [i['image']['image_shape'] for i, _, _ in batch])
        boxes, box_count, _ = pad_boxes([i['annos']['gt_boxes_lidar'] for i, _, _ in batch], self.device)
        m = BoxMembership(raw, counts, calib, shape, boxes, box_count)
        got = m.num_points_in_gt.cpu().numpy()
        out = []
        for k, (info, _, _) in enumerate(batch):
            num_gt = len(info['annos']['name'])
            num_objects = len(info['annos']['gt_boxes_lidar'])
            n = -np.ones(num_gt, dtype=np.int32)
            n[:num_objects] = got[k, :num_objects]
            out.append(n)
        return out

    # -- the ground-truth database
    def _database_batches(self, infos, batch_frames, num_workers):
        """per batch of infos: (infos, host points (P, C), host offsets (N + 1)) with entries frame after frame"""
        step = max(int(batch_frames), 1)
        with futures.ThreadPoolExecutor(pool_size(num_workers)) as pool:
            for lo in range(0, len(infos), step):
                part = infos[lo:lo + step]
                clouds = list(pool.map(lambda i: self.get_lidar(i['point_cloud']['lidar_idx']), part))
                raw, counts, calib, shape = self._frames_to_device(clouds, [_calib_of_info(i) for i in part],
                                                                   [i['image']['image_shape'] for i in part])
                boxes, box_count, centres = pad_boxes([i['annos']['gt_boxes_lidar'] for i in part], self.device)
                m = BoxMembership(raw, counts, calib, shape, boxes, box_count)
                points, offsets, _ = m.gather(centres)
                yield part, points.cpu().numpy(), offsets.cpu().numpy()       # the batch's one read of the result

    def create_groundtruth_database(self, info_path=None, used_classes=None, split='train', batch_frames=16, num_workers=4):
        """gt_database/<idx>_<name>_<i>.bin and kitti_dbinfos_<split>.pkl with the reference's names, keys and order"""
        db_dir = os.path.join(self.root, 'gt_database' if split == 'train' else 'gt_database_%s' % split)
        os.makedirs(db_dir, exist_ok=True)
        with open(str(info_path), 'rb') as f:
            infos = pickle.load(f)
        all_db_infos = {}
        for part, points, offsets in self._database_batches(infos, batch_frames, num_workers):
            e = 0
            for info in part:
                idx = info['point_cloud']['lidar_idx']
                annos = info['annos']
                gt_boxes = annos['gt_boxes_lidar']
                for i in range(gt_boxes.shape[0]):
                    name = annos['name'][i]
                    filename = '%s_%s_%d.bin' % (idx, name, i)
                    obj = points[offsets[e]:offsets[e + 1]]
                    e += 1
                    obj.tofile(os.path.join(db_dir, filename))
                    if used_classes is None or name in used_classes:
                        db_info = {'name': name, 'path': os.path.join(os.path.basename(db_dir), filename), 'image_idx': idx,
                                   'gt_idx': i, 'box3d_lidar': gt_boxes[i], 'num_points_in_gt': int(obj.shape[0]),
                                   'difficulty': annos['difficulty'][i], 'bbox': annos['bbox'][i], 'score': annos['score'][i]}
                        all_db_infos.setdefault(name, []).append(db_info)
        with open(os.path.join(self.root, 'kitti_dbinfos_%s.pkl' % split), 'wb') as f:
            pickle.dump(all_db_infos, f)
        return all_db_infos

    def build_gt_database(self, infos=None, used_classes=None, batch_frames=16, num_workers=4):
        """infos -> GTDatabase of the objects of class_names (and used_classes), as GTDatabase.from_reference_infos
        builds it from the files create_groundtruth_database writes, without touching the disk"""
        infos = self.infos if infos is None else infos
        pts, offs, boxes, cids = [], [0], [], []
        for part, points, offsets in self._database_batches(infos, batch_frames, num_workers):
            e = 0
            for info in part:
                gt_boxes = info['annos']['gt_boxes_lidar']
                for i in range(gt_boxes.shape[0]):
                    name = info['annos']['name'][i]
                    if name in self.class_names and (used_classes is None or name in used_classes):
                        obj = points[offsets[e]:offsets[e + 1]]
                        pts.append(obj)
                        offs.append(offs[-1] + len(obj))
                        boxes.append(gt_boxes[i].astype(np.float32))
                        cids.append(self.class_names.index(name))
                    e += 1
        C = self.num_point_features
        pts = np.concatenate(pts, 0) if pts else np.zeros((0, C), np.float32)
        return GTDatabase.from_arrays(pts, np.asarray(offs), np.asarray(boxes, np.float32).reshape(-1, 7), cids,
                                      self.class_names, self.device)

    def gt_annos(self):
        """the frames' annotation dicts (copies, with 'frame_id') for KittiEvaluator.evaluate"""
        out = []
        for info in self.infos:
            a = copy.deepcopy(info['annos'])
            a['frame_id'] = info['point_cloud']['lidar_idx']
            out.append(a)
        return out


def create_kitti_infos(root, save_path=None, class_names=('Car', 'Pedestrian', 'Cyclist'), workers=4, cfg=None, device=None,
                       batch_frames=16):
    """The four info pickles and the train database (kitti_dataset.py:431-470)."""
    save_path = str(root if save_path is None else save_path)
    ds = KittiDataset(root, list(class_names), split='train', cfg=cfg, device=device, load_infos=False)
    names = {s: os.path.join(save_path, 'kitti_infos_%s.pkl' % s) for s in ('train', 'val', 'trainval', 'test')}
    got = {}
    for split in ('train', 'val'):
        ds.set_split(split)
        got[split] = ds.get_infos(num_workers=workers, has_label=True, count_inside_pts=True, batch_frames=batch_frames)
        with open(names[split], 'wb') as f:
            pickle.dump(got[split], f)
    with open(names['trainval'], 'wb') as f:
        pickle.dump(got['train'] + got['val'], f)
    ds.set_split('test')
    test = ds.get_infos(num_workers=workers, has_label=False, count_inside_pts=False, batch_frames=batch_frames)
    with open(names['test'], 'wb') as f:
        pickle.dump(test, f)
    ds.set_split('train')
    ds.create_groundtruth_database(names['train'], split='train', batch_frames=batch_frames, num_workers=workers)
    return names


# ---- batches -----------------------------------------------------------------------------------------------------------

class KittiBatches:
    """Iterator of detector-ready batches over dataset.infos.

    Per batch: the frames' .bin files are read by the thread pool (the next batch is prefetched while the current one
    is on the device), uploaded once (upload_raw), cropped to the FOV on the device when FOV_POINTS_ONLY, and the boxes
    of the annotations become (B, M, 8) lidar boxes with BatchAugmentor's class column (host numpy, float32, as
    __getitem__: a few dozen boxes; DontCare dropped).  training: augmentor.augment_and_sample -> {'batch_size',
    'points', 'gt_boxes', 'frame_id'}; evaluation: sample_points_batch -> {'batch_size', 'points', 'frame_id', 'calib'
    (stacked, ready for KittiEvaluator.add_batch), 'image_shape' (B, 2) int32 on the device, 'gt_boxes'}."""

    def __init__(self, dataset, batch_size, training, augmentor=None, num_points=16384, shuffle_seed=None, num_workers=4,
                 sample_seed=0, drop_last=False):
        self.ds, self.B, self.training = dataset, int(batch_size), bool(training)
        self.num_points, self.seed, self.sample_seed = int(num_points), shuffle_seed, int(sample_seed)
        self.workers = pool_size(num_workers)
        self.drop_last = bool(drop_last)
        self.epoch = 0
        if self.training and augmentor is None:      # no augmentation: still the range mask and the class column
            augmentor = BatchAugmentor([], dataset.cfg['POINT_CLOUD_RANGE'], dataset.class_names, device=dataset.device)
        self.augmentor = augmentor

    def __len__(self):
        n = len(self.ds.infos)
        return n // self.B if self.drop_last else (n + self.B - 1) // self.B

    def frame_boxes(self, info):
        """(n, 8) float32 [lidar box, class column] of a frame, DontCare dropped; (calib, n == 0 without annotations)"""
        calib = _calib_of_info(info)
        if 'annos' not in info:
            return calib, np.zeros((0, 8), np.float32)
        a = info['annos']
        keep = np.array([i for i, x in enumerate(a['name']) if x != 'DontCare'], dtype=np.int64)
        cam = np.concatenate([a['location'][keep], a['dimensions'][keep], a['rotation_y'][keep][..., np.newaxis]],
                             axis=1).astype(np.float32)
        lidar = boxes3d_kitti_camera_to_lidar(cam, calib).astype(np.float32)
        return calib, np.concatenate([lidar, class_column(list(a['name'][keep]), self.ds.class_names)[:, None]], 1)

    def _load(self, pool, infos):
        clouds = list(pool.map(lambda i: self.ds.get_lidar(i['point_cloud']['lidar_idx']), infos))
        meta = [self.frame_boxes(i) for i in infos]
        return infos, clouds, meta

    def __iter__(self):
        order = np.arange(len(self.ds.infos))
        if self.seed is not None:
            order = np.random.default_rng([int(self.seed), self.epoch]).permutation(len(order))
        self.epoch += 1
        chunks = [order[k:k + self.B] for k in range(0, len(order), self.B)]
        if self.drop_last:
            chunks = [c for c in chunks if len(c) == self.B]
        with futures.ThreadPoolExecutor(self.workers) as pool, futures.ThreadPoolExecutor(1) as ahead:
            nxt = ahead.submit(self._load, pool, [self.ds.infos[i] for i in chunks[0]]) if chunks else None
            for k in range(len(chunks)):
                infos, clouds, meta = nxt.result()
                nxt = ahead.submit(self._load, pool, [self.ds.infos[i] for i in chunks[k + 1]]) if k + 1 < len(chunks) else None
                yield self._batch(infos, clouds, meta, k)

    def _batch(self, infos, clouds, meta, k):
        ds = self.ds
        dev = ds.device
        B = len(infos)
        raw, counts, calib, shape = ds._frames_to_device(clouds, [c for c, _ in meta], [i['image']['image_shape'] for i in infos])
        host_counts = [len(c) for c in clouds]
        M = max([len(b) for _, b in meta] + [1])
        gt = np.zeros((B, M, 8), np.float32)
        for j, (_, b) in enumerate(meta):
            gt[j, :len(b)] = b
        gt = torch.from_numpy(gt).to(dev)
        if ds.cfg['FOV_POINTS_ONLY']:
            crop = fov_crop(raw, counts, calib, shape)
            raw, counts, host_counts = crop['rows'], crop['counts'], crop['host_counts']
        seed = self.sample_seed + k
        ids = [i['point_cloud']['lidar_idx'] for i in infos]
        if self.training:
            points, boxes = self.augmentor.augment_and_sample(raw, counts, gt, self.num_points, sample_seed=seed)
            return {'batch_size': B, 'points': points, 'gt_boxes': boxes, 'frame_id': ids}
        points = sample_points_batch(raw, counts, self.num_points, seed=seed, host_counts=host_counts)
        return {'batch_size': B, 'points': points, 'frame_id': ids, 'calib': calib, 'image_shape': shape, 'gt_boxes': gt}


def main(argv=None):
    argv = sys.argv[1:] if argv is None else list(argv)
    if len(argv) < 2 or argv[0] != 'create_kitti_infos':
        print(__doc__.strip().splitlines()[-1].strip(), file=sys.stderr)
        return 2
    names = create_kitti_infos(argv[1], argv[2] if len(argv) > 2 else None)
    for k, v in names.items():
        print('kitti info %s file is saved to %s' % (k, v))
    return 0


if __name__ == '__main__':
    sys.exit(main())

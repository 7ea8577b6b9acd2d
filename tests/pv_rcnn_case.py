"""The reduced PV-RCNN case shared by tests/golden/gen_pv_rcnn_fixtures.py (which runs the reference's own VoxelSetAbstraction,
PointHeadSimple and PVRCNNHead under it) and tests/test_pv_rcnn_host.py / test_pv_rcnn_gpu.py.  A helper module: no tests, no
fixtures.

Geometry: voxel_rcnn_case's range [0, -4, -3, 10.5, 4, 1] with voxels of 0.5 x 0.5 x 0.1 m, B = 3, every sample non-empty (the
reference divides by a sample's point count: an empty one has no reference answer), sample 1 with fewer points (30) than
NUM_KEYPOINTS (48).  Two levels stand for the sparse backbone's: the occupied cells of the points at strides 1 and 4 with seeded
features; the BEV map is 8 channels on 4 x 6 cells at stride 4.  Widths are reduced; every NSAMPLE is 16 so that the fused
set-abstraction kernels serve the modules.
"""
import copy

import numpy as np

import voxel_rcnn_case as vcase

RANGE = list(vcase.RANGE)
VOXEL = list(vcase.VOXEL)
B = 3
COUNTS = (90, 30, 70)
NUM_KEYPOINTS = 48
BEV_SHAPE = (8, 4, 6)           # (C, H, W): 8 channels, so that every source's column offset (8, 24, 40 of 60) is a multiple of 4
                                # and the encoder writes in place, as at the published widths
BEV_STRIDE = 4
LEVELS = (('x_conv1', 1, 4), ('x_conv3', 4, 8))      # name, stride, channels
GRID_SIZES = (2, 3)

PFE_CFG = {'NAME': 'VoxelSetAbstraction', 'POINT_SOURCE': 'raw_points', 'NUM_KEYPOINTS': NUM_KEYPOINTS, 'NUM_OUTPUT_FEATURES': 16,
           'SAMPLE_METHOD': 'FPS', 'FEATURES_SOURCE': ['bev', 'x_conv1', 'x_conv3', 'raw_points'],
           'SA_LAYER': {'raw_points': {'MLPS': [[8, 8], [8, 8]], 'POOL_RADIUS': [0.9, 1.8], 'NSAMPLE': [16, 16]},
                        'x_conv1': {'DOWNSAMPLE_FACTOR': 1, 'MLPS': [[4, 8], [4, 8]], 'POOL_RADIUS': [0.9, 1.8], 'NSAMPLE': [16, 16]},
                        'x_conv3': {'DOWNSAMPLE_FACTOR': 4, 'MLPS': [[8, 8], [8, 12]], 'POOL_RADIUS': [1.7, 3.4], 'NSAMPLE': [16, 16]}}}
POINT_HEAD_CFG = {'NAME': 'PointHeadSimple', 'CLS_FC': [16], 'CLASS_AGNOSTIC': True, 'USE_POINT_FEATURES_BEFORE_FUSION': True,
                  # read by the REFERENCE's constructor only (its loss modules)
                  'LOSS_CONFIG': {'LOSS_REG': 'smooth-l1', 'LOSS_WEIGHTS': {'point_cls_weight': 1.0}}}
HEAD_CFG = {'NAME': 'PVRCNNHead', 'CLASS_AGNOSTIC': True,
            'SHARED_FC': [32, 32], 'CLS_FC': [32, 32], 'REG_FC': [32, 32], 'DP_RATIO': 0.3,
            'NMS_CONFIG': {'TRAIN': {'NMS_TYPE': 'nms_gpu', 'MULTI_CLASSES_NMS': False, 'NMS_PRE_MAXSIZE': 512, 'NMS_POST_MAXSIZE': 16, 'NMS_THRESH': 0.8},
                           'TEST': {'NMS_TYPE': 'nms_gpu', 'MULTI_CLASSES_NMS': False, 'NMS_PRE_MAXSIZE': 512, 'NMS_POST_MAXSIZE': 16, 'NMS_THRESH': 0.7}},
            'ROI_GRID_POOL': {'GRID_SIZE': 2, 'MLPS': [[8, 8], [8, 12]], 'POOL_RADIUS': [1.1, 2.2], 'NSAMPLE': [16, 16], 'POOL_METHOD': 'max_pool'},
            'TARGET_CONFIG': {'BOX_CODER': 'ResidualCoder'},
            # read by the REFERENCE's constructor only (its loss modules); this repository's head ignores it
            'LOSS_CONFIG': {'LOSS_WEIGHTS': {'code_weights': [1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0]}}}
NUM_RAWPOINT_FEATURES = 4
NUM_BEFORE_FUSION = BEV_SHAPE[0] + 16 + 16 + 20        # bev, raw_points, x_conv1, x_conv3: the reference's column order


def pfe_cfg():
    return copy.deepcopy(PFE_CFG)


def head_cfg(grid_size):
    cfg = copy.deepcopy(HEAD_CFG)
    cfg['ROI_GRID_POOL']['GRID_SIZE'] = grid_size
    return cfg


def points(seed):
    """(sum COUNTS, 5) fp32 rows (b, x, y, z, intensity), sample-major; clustered so that balls are empty, partly filled and full"""
    rng = np.random.default_rng(seed)
    rows = []
    for b, n in enumerate(COUNTS):
        centres = np.stack([rng.uniform(1.5, 9.0, 4), rng.uniform(-3.0, 3.0, 4), rng.uniform(-2.0, 0.0, 4)], 1)
        xyz = centres[rng.integers(0, 4, n)] + rng.normal(0, [0.7, 0.7, 0.25], (n, 3))
        xyz = np.clip(xyz, [0.05, -3.95, -2.95], [10.45, 3.95, 0.95])
        rows.append(np.concatenate([np.full((n, 1), b), xyz, rng.uniform(0, 1, (n, 1))], 1))
    return np.concatenate(rows).astype(np.float32)


def levels(pts):
    """-> {name: dict(indices (P, 4) int32 (b, z, y, x) sample-major, features (P, C) fp32, stride)}: the occupied cells of the
    points at the level's stride"""
    out = {}
    cell = np.floor((pts[:, 1:4] - np.float32(RANGE[:3])) / np.float32(VOXEL)).astype(np.int64)      # (x, y, z)
    for name, stride, channels in LEVELS:
        rows = np.concatenate([pts[:, :1].astype(np.int64), (cell // stride)[:, [2, 1, 0]]], 1)
        idx = np.unique(rows, axis=0).astype(np.int32)                                                # sorted: sample-major
        rng = np.random.default_rng(31 + stride)
        out[name] = dict(indices=idx, stride=stride,
                         features=np.maximum(rng.normal(0.3, 0.6, (len(idx), channels)), 0).astype(np.float32))
    return out


def bev_features():
    return np.random.default_rng(41).normal(0.2, 0.7, (B,) + BEV_SHAPE).astype(np.float32)


rois = vcase.rois                   # (B, 5, 7): three boxes inside (one with heading 0), one over a border, a zero padding row
fill_module = vcase.fill_module     # seeded parameters: outputs of order 1

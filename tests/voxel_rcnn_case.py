"""The reduced Voxel R-CNN second-stage case shared by tests/golden/gen_voxel_rcnn_fixtures.py (which runs the reference's own
NeighborVoxelSAModuleMSG and VoxelRCNNHead under it) and tests/test_voxel_rcnn_host.py / test_voxel_rcnn_gpu.py.  A helper
module: no tests, no fixtures.

Geometry: sparse_conv_reference.V1's range [0, -4, -3, 10.5, 4, 1] with voxels of 0.5 x 0.5 x 0.1 m, B = 3, sample 1 empty.  The
levels are sparse_conv_reference.b1_voxels carried through the numpy rulebook of the backbone's three strided convolutions:
strides 2, 4, 8 on the grids (21, 8, 11), (11, 4, 6), (5, 2, 3) as (D, H, W).
"""
import copy

import numpy as np

import sparse_conv_reference as scr

RANGE = [0.0, -4.0, -3.0, 10.5, 4.0, 1.0]
VOXEL = [0.5, 0.5, 0.1]
B = 3
LEVEL_GEOMETRY = (('x_conv2', 2, 'k3s2p1'), ('x_conv3', 4, 'k3s2p1'), ('x_conv4', 8, 'k3s2p011'))
BACKBONE_CHANNELS = {'x_conv1': 16, 'x_conv2': 32, 'x_conv3': 64, 'x_conv4': 64}

# two source levels, an anisotropic window and a full 9 x 9 x 9 one, NSAMPLE 4 so that groups overflow, FC widths 32; DP_RATIO
# 0.3 with two widths per stack, so that the Dropout modules shift the child indices as in the full head
HEAD_CFG = {'NAME': 'VoxelRCNNHead', 'CLASS_AGNOSTIC': True,
            'SHARED_FC': [32, 32], 'CLS_FC': [32, 32], 'REG_FC': [32, 32], 'DP_RATIO': 0.3,
            'NMS_CONFIG': {'TRAIN': {'NMS_TYPE': 'nms_gpu', 'MULTI_CLASSES_NMS': False, 'NMS_PRE_MAXSIZE': 512, 'NMS_POST_MAXSIZE': 16, 'NMS_THRESH': 0.8},
                           'TEST': {'NMS_TYPE': 'nms_gpu', 'MULTI_CLASSES_NMS': False, 'NMS_PRE_MAXSIZE': 512, 'NMS_POST_MAXSIZE': 16, 'NMS_THRESH': 0.7}},
            'ROI_GRID_POOL': {'FEATURES_SOURCE': ['x_conv2', 'x_conv4'], 'GRID_SIZE': 2,
                              'POOL_LAYERS': {'x_conv2': {'MLPS': [[16, 16]], 'QUERY_RANGES': [[1, 2, 3]], 'POOL_RADIUS': [1.6], 'NSAMPLE': [4],
                                                          'POOL_METHOD': 'max_pool'},
                                              'x_conv4': {'MLPS': [[16, 32]], 'QUERY_RANGES': [[4, 4, 4]], 'POOL_RADIUS': [5.0], 'NSAMPLE': [4],
                                                          'POOL_METHOD': 'max_pool'}}},
            'TARGET_CONFIG': {'BOX_CODER': 'ResidualCoder'},
            # read by the REFERENCE's constructor only (its loss modules); this repository's head ignores it
            'LOSS_CONFIG': {'LOSS_WEIGHTS': {'code_weights': [1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0]}}}
GRID_SIZES = (2, 3)


def head_cfg(grid_size):
    cfg = copy.deepcopy(HEAD_CFG)
    cfg['ROI_GRID_POOL']['GRID_SIZE'] = grid_size
    return cfg


def levels():
    """-> {name: dict(indices (P, 4) int32 (b, z, y, x) in ascending key order, shape (D, H, W), stride)}"""
    idx, _ = scr.b1_voxels(4)
    shape = (scr.B1_GRID[2] + 1, scr.B1_GRID[1], scr.B1_GRID[0])
    out = {}
    for name, stride, geo in LEVEL_GEOMETRY:
        idx, _, shape = scr.rulebook(idx, B, shape, *scr.GEOMETRIES[geo])
        out[name] = dict(indices=idx, shape=tuple(int(v) for v in shape), stride=stride)
    return out


def level_features(name, rows, seed=17):
    """seeded fp32 features of a level, BACKBONE_CHANNELS[name] wide, non-negative as behind the backbone's ReLU"""
    rng = np.random.default_rng(seed + int(name[-1]))
    return np.maximum(rng.normal(0.3, 0.6, (rows, BACKBONE_CHANNELS[name])), 0).astype(np.float32)


def rois(rng):
    """(B, 5, 7) fp32: per sample three boxes inside the range with random headings (the first with heading exactly 0), one partly
    below the range minimum on x and y (negative cells), or hanging over the far border on x, and an all-zero padding row"""
    r = np.zeros((B, 5, 7), dtype=np.float32)
    for b in range(B):
        r[b, 0:3, 0] = rng.uniform(2.0, 8.5, 3)
        r[b, 0:3, 1] = rng.uniform(-2.5, 2.5, 3)
        r[b, 0:3, 2] = rng.uniform(-2.0, 0.0, 3)
        r[b, 0:3, 3:6] = rng.uniform([1.5, 1.0, 1.0], [4.0, 2.0, 1.8], (3, 3))
        r[b, 1:3, 6] = rng.uniform(-np.pi, np.pi, 2)
        if b % 2 == 0:
            r[b, 3] = [rng.uniform(0.2, 0.6), rng.uniform(-3.9, -3.5), rng.uniform(-2.9, -2.6), 3.0, 2.0, 1.6, rng.uniform(-np.pi, np.pi)]
        else:
            r[b, 3] = [rng.uniform(9.8, 10.3), rng.uniform(-1.0, 1.0), rng.uniform(0.3, 0.8), 3.5, 1.8, 1.6, rng.uniform(-np.pi, np.pi)]
    return r


def fill_module(module, seed):
    """seeded parameters of a pool layer or head (generator and tests alike): weights normal, BatchNorm with set statistics"""
    import torch
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, t in sorted(module.state_dict().items()):
            if name.endswith('num_batches_tracked'):
                continue
            if name.endswith('running_var'):
                v = torch.rand(t.shape, generator=g) + 0.5
            elif name.endswith('running_mean'):
                v = torch.randn(t.shape, generator=g) * 0.1
            elif t.dim() > 1:
                fan_in = int(np.prod(t.shape[1:]))
                v = torch.randn(t.shape, generator=g) * float(1.0 / np.sqrt(fan_in))
                if 'mlps_pos' in name:      # offsets reach several metres: keep the position term of the features' size
                    v = v * 0.3
            elif name.endswith('weight'):
                v = torch.rand(t.shape, generator=g) * 0.4 + 0.8
            else:
                v = torch.randn(t.shape, generator=g) * 0.2
            t.copy_(v.to(t.dtype))

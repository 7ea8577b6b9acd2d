"""The PV-RCNN++ cases shared by tests/golden/gen_pv_rcnn_pp_fixtures.py, tests/test_pv_rcnn_pp_host.py and test_pv_rcnn_pp_gpu.py.
A helper module: no tests, no fixtures.

partition_case(counts): stacked points and rois for pdm_spc_partition with S = 6, K = 50, radius 1.6, built point by point so that
what is planted is known, and reject-sampled so that no verdict rests on a last-ulp difference between the host and the device:
|d_min - (roi_max_dim + r)| >= 1e-4, a second-nearest roi within 1e-4 gives the same verdict, and the sector quotient is at least
1e-4 from an integer (the planted axis point excepted).
  sample 0   exactly 25 kept rows (N' < K): 7 near a roi in sector 0, 9 in sector 2, 8 in sector 3 and the point (-3, 0.0, z), whose
             sector index is whatever fp32 makes of 2 PI_F / SIZE_F; sectors 1, 4 and 5 are empty
  sample 1   37 rows, none near a roi: the fallback point
  sample 2   no rows
  sample 3   (the four-sample case) exactly 100 kept rows spread over its tiles, 28 of them in sector 0: with K = 50 the double
             evaluation ceil(28 / 100 * 50) is 15 where the integer form ceil(28 * 50 / 100) is 14
  (a first sample of 700 rows, in the four-sample case, gets 120 more kept rows around its rois on top of sample 0's plan)
"""
import numpy as np

import pv_rcnn_pp_reference as ppr

S, K, RADIUS = 6, 50, 1.6
SMALL = (300, 37, 0)
LARGE = (700, 37, 0, 1500)
AXIS_POINT = (-3.0, 0.0, -1.0)

# (cx, cy, cz, dx, dy, dz, heading): centres far from each other and from the sector borders; a zero padding row last
ROIS = np.array([[-20.0, -12.0, -1.0, 3.9, 1.6, 1.5, 0.3],       # angle + pi = 31 deg: sector 0
                 [15.0, -15.0, -1.0, 4.2, 1.7, 1.6, -1.1],       # 135 deg: sector 2
                 [20.0, 12.0, -1.0, 0.8, 0.7, 1.8, 2.0],         # 211 deg: sector 3
                 [-6.0, 0.0, -1.0, 4.0, 2.0, 2.0, 0.0],          # holds the axis point alone
                 [0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0]], dtype=np.float32)


def _clear(xyz, rois, sectors=True):
    mask, clearance, second = ppr.keep_mask(xyz, rois, RADIUS)
    ok = (clearance >= 1e-4) & (second == mask)
    if sectors:
        ok &= ppr.sector_index(xyz, S)[1] >= 1e-4
    return ok, mask


def _draw(rng, rois, near, far):
    """`near[j]` rows within 0.6 m of roi j's centre (kept) and `far` rows more than a metre beyond every roi's reach, all clear"""
    reach = np.linalg.norm(rois[:, 3:6] / 2, axis=1) + RADIUS
    rows = []
    for j, count in enumerate(near):
        while count:
            p = (rois[j, 0:3] + rng.uniform(-0.6, 0.6, 3)).astype(np.float32)[None]
            ok, mask = _clear(p, rois)
            if ok[0] and mask[0]:
                rows.append(p[0])
                count -= 1
    while far:
        p = np.array([rng.uniform(-40, 40), rng.uniform(-40, 40), rng.uniform(-3, 1)], dtype=np.float32)[None]
        ok, mask = _clear(p, rois)
        if ok[0] and not mask[0] and (np.linalg.norm(p - rois[:, 0:3], axis=1) > reach + 1.0).all():
            rows.append(p[0])
            far -= 1
    return rows


def partition_case(counts, seed=7):
    """-> (xyz (N, 3) fp32, counts, rois (B, 5, 7) fp32)"""
    rng = np.random.default_rng(seed)
    B = len(counts)
    rois = np.stack([ROIS] * B).copy()
    rois[1:, :4, 0:2] += rng.uniform(-2, 2, (B - 1, 4, 2)).astype(np.float32)     # other samples: other rois
    out = []
    for b, n in enumerate(counts):
        if n == 0:
            continue
        if b == 0:
            extra = n - 300
            assert extra == 0 or extra >= 120
            rows = _draw(rng, rois[0], [7, 9, 8, 0, 0], 275)
            rows.append(np.array(AXIS_POINT, dtype=np.float32))
            rows = [rows[k] for k in rng.permutation(len(rows))]
            if extra:                                                             # appended: the first 300 rows keep their plan
                more = _draw(rng, rois[0], [40, 40, 40, 0, 0], extra - 120)
                rows += [more[k] for k in rng.permutation(len(more))]
        elif b == 3:
            rows = _draw(rng, rois[b], [28, 30, 42, 0, 0], n - 100)
            rows = [rows[k] for k in rng.permutation(len(rows))]
        else:
            rows = _draw(rng, rois[b], [0, 0, 0, 0, 0], n)
        assert len(rows) == n
        out.append(np.stack(rows))
    xyz = np.concatenate(out).astype(np.float32)
    return xyz, tuple(counts), rois


# ------------------------------------------------------------------------------------------------------------ module case
# The reduced PV-RCNN++ modules on pv_rcnn_case's geometry (B = 3, counts 90 / 30 / 70, two backbone levels, an 8-channel BEV map,
# 5 rois a sample with one all-zero row): SPC sampling with S = 6 and K = 50 (sample 1 keeps fewer rows than K), one plain
# StackSAModuleMSG source without a filter and two filtered VectorPool sources, a VectorPool RoI-grid pool.
import copy  # noqa: E402

import pv_rcnn_case as pcase  # noqa: E402

B, COUNTS, RANGE, VOXEL = pcase.B, pcase.COUNTS, pcase.RANGE, pcase.VOXEL
BEV_SHAPE, BEV_STRIDE, LEVELS, NUM_RAWPOINT_FEATURES = pcase.BEV_SHAPE, pcase.BEV_STRIDE, pcase.LEVELS, pcase.NUM_RAWPOINT_FEATURES
GRID = 2


def _vp(kind, reduced, post, cells, distances, nsample, width):
    cfg = {'NAME': 'VectorPoolAggregationModuleMSG', 'NUM_GROUPS': 2, 'LOCAL_AGGREGATION_TYPE': kind, 'NUM_REDUCED_CHANNELS': reduced,
           'NUM_CHANNELS_OF_LOCAL_AGGREGATION': 4, 'MSG_POST_MLPS': [post]}
    for k in range(2):
        cfg[f'GROUP_CFG_{k}'] = {'NUM_LOCAL_VOXEL': list(cells[k]), 'MAX_NEIGHBOR_DISTANCE': distances[k], 'NEIGHBOR_NSAMPLE': nsample,
                                 'POST_MLPS': [width]}
    return cfg


PFE_CFG = {'NAME': 'VoxelSetAbstractionSPC', 'POINT_SOURCE': 'raw_points', 'NUM_KEYPOINTS': K, 'NUM_OUTPUT_FEATURES': 16,
           'SAMPLE_METHOD': 'SPC', 'SPC_SAMPLING': {'NUM_SECTORS': S, 'SAMPLE_RADIUS_WITH_ROI': RADIUS},
           'FEATURES_SOURCE': ['bev', 'x_conv1', 'x_conv3', 'raw_points'],
           'SA_LAYER': {
               'raw_points': dict(_vp('local_interpolation', 1, 8, ([2, 2, 2], [3, 3, 2]), (0.5, 0.9), -1, 8),
                                  FILTER_NEIGHBOR_WITH_ROI=True, RADIUS_OF_NEIGHBOR_WITH_ROI=2.4),
               'x_conv1': {'DOWNSAMPLE_FACTOR': 1, 'MLPS': [[4, 8], [4, 8]], 'POOL_RADIUS': [0.9, 1.8], 'NSAMPLE': [16, 16]},
               'x_conv3': dict(_vp('local_interpolation', 4, 12, ([2, 2, 2], [3, 3, 2]), (1.2, 2.4), -1, 8),
                               DOWNSAMPLE_FACTOR=4, INPUT_CHANNELS=8, FILTER_NEIGHBOR_WITH_ROI=True, RADIUS_OF_NEIGHBOR_WITH_ROI=3.0)}}
FILTER_RADII = {'raw_points': 2.4, 'x_conv3': 3.0}
NUM_BEFORE_FUSION = BEV_SHAPE[0] + 8 + 16 + 12          # bev, raw_points, x_conv1, x_conv3: the reference's column order
POINT_HEAD_CFG = pcase.POINT_HEAD_CFG
HEAD_CFG = copy.deepcopy(pcase.HEAD_CFG)
HEAD_CFG['ROI_GRID_POOL'] = dict(_vp('voxel_random_choice', 8, 12, ([2, 2, 2], [3, 3, 2]), (1.1, 2.2), 16, 8), GRID_SIZE=GRID)


def pfe_cfg():
    return copy.deepcopy(PFE_CFG)


def head_cfg():
    return copy.deepcopy(HEAD_CFG)


def level_xyz(level):
    """voxel centres of a level (pv_rcnn_case.levels): get_voxel_centers in fp32"""
    xyz = level['indices'][:, [3, 2, 1]].astype(np.float32)
    return ((xyz + np.float32(0.5)) * (np.float32(VOXEL) * np.float32(level['stride'])) + np.float32(RANGE[:3])).astype(np.float32)


def partition_is_clear(xyz, counts, rois, radius, sectors):
    """every verdict of the keep rule at this radius (and, for `sectors`, every sector index) is at least 1e-4 from flipping"""
    start = 0
    for b, n in enumerate(counts):
        if n:
            mask, clearance, second = ppr.keep_mask(xyz[start:start + n], rois[b], radius)
            if (clearance < 1e-4).any() or (second != mask).any():
                return False
            if sectors and (ppr.sector_index(xyz[start:start + n], S)[1] < 1e-4).any():
                return False
        start += n
    return True

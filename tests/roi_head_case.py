"""The reduced PointRCNN second-stage configurations shared by tests/golden/gen_roi_fixtures.py (which runs the
reference's own head under them) and tests/test_roi_pool_host.py / test_roi_head_gpu.py."""
import copy

from pdm_ssd_amd.detector_config import POINT_RCNN_CFG

# fixtures (c), (d), (e): 16 input channels, 32 sampled points, three small SA levels (nsample 8: the torch path of the SA
# modules, whose fused kernels have tests of their own)
HEAD_CFG = {'NAME': 'PointRCNNHead', 'CLASS_AGNOSTIC': True,
            'ROI_POINT_POOL': {'POOL_EXTRA_WIDTH': [0.1, 0.1, 0.1], 'NUM_SAMPLED_POINTS': 32, 'DEPTH_NORMALIZER': 70.0},
            'XYZ_UP_LAYER': [16, 16], 'CLS_FC': [32], 'REG_FC': [32], 'DP_RATIO': 0, 'USE_BN': False,
            'SA_CONFIG': {'NPOINTS': [16, 4, -1], 'RADIUS': [0.4, 0.8, 100], 'NSAMPLE': [8, 8, 8],
                          'MLPS': [[16, 16], [16, 32], [32, 32]]},
            'NMS_CONFIG': copy.deepcopy(POINT_RCNN_CFG['ROI_HEAD']['NMS_CONFIG']),
            'TARGET_CONFIG': {'BOX_CODER': 'ResidualCoder'},
            # read by the REFERENCE's constructor only (its loss modules); this repository's head ignores it
            'LOSS_CONFIG': {'LOSS_WEIGHTS': {'code_weights': [1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0]}}}
HEAD_INPUT_CHANNELS = 16

# the full detector with a three-level backbone, a narrow point head and a small second stage
REDUCED_POINT_RCNN_CFG = copy.deepcopy(POINT_RCNN_CFG)
REDUCED_POINT_RCNN_CFG['BACKBONE_3D'] = {
    'NAME': 'PointNet2MSG',
    'SA_CONFIG': {'NPOINTS': [256, 64, 16], 'RADIUS': [[0.5, 1.0], [1.0, 2.0], [2.0, 4.0]], 'NSAMPLE': [[16, 32], [16, 32], [16, 32]],
                  'MLPS': [[[16, 16, 32], [16, 16, 32]], [[32, 32, 64], [32, 32, 64]], [[64, 64, 128], [64, 64, 128]]]},
    'FP_MLPS': [[32, 32], [64, 64], [128, 128]]}
REDUCED_POINT_RCNN_CFG['POINT_HEAD'].update(CLS_FC=[32], REG_FC=[32])
REDUCED_POINT_RCNN_CFG['ROI_HEAD'].update(
    ROI_POINT_POOL={'POOL_EXTRA_WIDTH': [0.0, 0.0, 0.0], 'NUM_SAMPLED_POINTS': 64, 'DEPTH_NORMALIZER': 70.0},
    XYZ_UP_LAYER=[32, 32], CLS_FC=[32], REG_FC=[32],
    SA_CONFIG={'NPOINTS': [16, 4, -1], 'RADIUS': [0.4, 0.8, 100], 'NSAMPLE': [16, 16, 16], 'MLPS': [[32, 32], [32, 64], [64, 64]]})
REDUCED_POINT_RCNN_CFG['ROI_HEAD']['NMS_CONFIG']['TEST'].update(NMS_PRE_MAXSIZE=512, NMS_POST_MAXSIZE=16)

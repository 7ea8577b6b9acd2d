"""The PDM-SSD model configuration the benchmark and tests build (key names as an OpenPCDet YAML would hold them; the
reference's own YAML files are git-ignored and absent).  Backbone = upstream pointrcnn.yaml's
PointNet2MSG; point head = its PointHeadBox settings; neck / heat-map head = this repo's spec."""
import copy
from types import SimpleNamespace

from . import synthetic
from .config import cfg_from_dict
from .pointnet2_backbone import POINTRCNN_MSG_CFG

CLASS_NAMES = ['Car', 'Pedestrian', 'Cyclist']
VOXEL_SIZE = [0.05, 0.05, 0.1]
GRID_SIZE = [1408, 1600, 40]

PDM_SSD_CFG = {
    'NAME': 'PDMSSD',
    'BACKBONE_3D': dict(POINTRCNN_MSG_CFG),
    'MAP_TO_BEV': {'NAME': 'PDMNeck', 'SOURCE_LAYER': 2, 'FEATURE_DIM': 128, 'DILATION': [7, 7, 1], 'SH_DEGREE': 2,
                   'BEV_STRIDE': 8, 'HEIGHT_BINS': 1, 'INPUT_CHANNELS': 256, 'NORMALIZE': True},
    'DENSE_HEAD': {'NAME': 'PDMHeatmapHead', 'CLASS_AGNOSTIC': False, 'SHARED_CONV_CHANNEL': 64, 'NUM_CONTEXT_CONV': 1, 'CONTEXT_CONV': 'separable',
                   'TARGET_ASSIGNER_CONFIG': {'FEATURE_MAP_STRIDE': 8, 'GAUSSIAN_OVERLAP': 0.1, 'MIN_RADIUS': 2},
                   'LOSS_CONFIG': {'LOSS_WEIGHTS': {'cls_weight': 1.0}}},
    'POINT_HEAD': {'NAME': 'PointHeadBox', 'CLS_FC': [256, 256], 'REG_FC': [256, 256], 'CLASS_AGNOSTIC': False,
                   'USE_POINT_FEATURES_BEFORE_FUSION': False,
                   'TARGET_CONFIG': {'GT_EXTRA_WIDTH': [0.2, 0.2, 0.2], 'BOX_CODER': 'PointResidualCoder',
                                     'BOX_CODER_CONFIG': {'use_mean_size': True,
                                                          'mean_size': [[3.9, 1.6, 1.56], [0.8, 0.6, 1.73], [1.76, 0.6, 1.73]]}},
                   'LOSS_CONFIG': {'LOSS_REG': 'WeightedSmoothL1Loss',
                                   'LOSS_WEIGHTS': {'point_cls_weight': 1.0, 'point_box_weight': 1.0,
                                                    'code_weights': [1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0]}}},
    'POST_PROCESSING': {'RECALL_THRESH_LIST': [0.3, 0.5, 0.7], 'SCORE_THRESH': 0.1, 'OUTPUT_RAW_SCORE': False,
                        'NMS_CONFIG': {'MULTI_CLASSES_NMS': False, 'NMS_TYPE': 'nms_gpu', 'NMS_THRESH': 0.1,
                                       'NMS_PRE_MAXSIZE': 4096, 'NMS_POST_MAXSIZE': 500}},
}

# PointRCNN: the upstream project's published settings (its tools/cfgs/kitti_models/pointrcnn.yaml) restated as a dict — the
# snapshot this repository was modelled on holds no YAML.  First stage = the backbone and point head above;
# a second stage built from this dict runs in eval mode only: of TARGET_CONFIG it holds the box coder alone, and a RoI head
# without the proposal-target sampler's settings has no training half (POINT_RCNN_TRAIN_CFG below adds them).
POINT_RCNN_CFG = {
    'NAME': 'PointRCNN',
    'BACKBONE_3D': dict(POINTRCNN_MSG_CFG),
    'POINT_HEAD': dict(PDM_SSD_CFG['POINT_HEAD']),
    'ROI_HEAD': {'NAME': 'PointRCNNHead', 'CLASS_AGNOSTIC': True,
                 'ROI_POINT_POOL': {'POOL_EXTRA_WIDTH': [0.0, 0.0, 0.0], 'NUM_SAMPLED_POINTS': 512, 'DEPTH_NORMALIZER': 70.0},
                 'XYZ_UP_LAYER': [128, 128], 'CLS_FC': [256, 256], 'REG_FC': [256, 256], 'DP_RATIO': 0.0, 'USE_BN': False,
                 'SA_CONFIG': {'NPOINTS': [128, 32, -1], 'RADIUS': [0.2, 0.4, 100], 'NSAMPLE': [16, 16, 16],
                               'MLPS': [[128, 128, 128], [128, 128, 256], [256, 256, 512]]},
                 'NMS_CONFIG': {'TRAIN': {'NMS_TYPE': 'nms_gpu', 'MULTI_CLASSES_NMS': False, 'NMS_PRE_MAXSIZE': 9000,
                                          'NMS_POST_MAXSIZE': 512, 'NMS_THRESH': 0.8},
                                'TEST': {'NMS_TYPE': 'nms_gpu', 'MULTI_CLASSES_NMS': False, 'NMS_PRE_MAXSIZE': 9000,
                                         'NMS_POST_MAXSIZE': 100, 'NMS_THRESH': 0.85}},
                 'TARGET_CONFIG': {'BOX_CODER': 'ResidualCoder'}},
    'POST_PROCESSING': {'RECALL_THRESH_LIST': [0.3, 0.5, 0.7], 'SCORE_THRESH': 0.1, 'OUTPUT_RAW_SCORE': False,
                        'NMS_CONFIG': {'MULTI_CLASSES_NMS': False, 'NMS_TYPE': 'nms_gpu', 'NMS_THRESH': 0.1,
                                       'NMS_PRE_MAXSIZE': 4096, 'NMS_POST_MAXSIZE': 500}},
}

# POINT_RCNN_CFG plus the upstream file's proposal-target sampler (TARGET_CONFIG) and rcnn loss settings (LOSS_CONFIG),
# restated: a RoI head built from this dict has the training half (ProposalTargetLayer, assign_targets, get_loss).
POINT_RCNN_TRAIN_CFG = copy.deepcopy(POINT_RCNN_CFG)
POINT_RCNN_TRAIN_CFG['ROI_HEAD']['TARGET_CONFIG'].update(
    ROI_PER_IMAGE=128, FG_RATIO=0.5, SAMPLE_ROI_BY_EACH_CLASS=True, CLS_SCORE_TYPE='cls', CLS_FG_THRESH=0.6, CLS_BG_THRESH=0.45,
    CLS_BG_THRESH_LO=0.1, HARD_BG_RATIO=0.8, REG_FG_THRESH=0.55)
POINT_RCNN_TRAIN_CFG['ROI_HEAD']['LOSS_CONFIG'] = {
    'CLS_LOSS': 'BinaryCrossEntropy', 'REG_LOSS': 'smooth-l1', 'CORNER_LOSS_REGULARIZATION': True,
    'LOSS_WEIGHTS': {'rcnn_cls_weight': 1.0, 'rcnn_reg_weight': 1.0, 'rcnn_corner_weight': 1.0, 'code_weights': [1.0] * 7}}

# CenterPoint on the PDM neck: PointNet2MSG -> PDMNeck -> CenterHead.  The head and post-processing values are the upstream
# project's published KITTI settings (the dense head of its tools/cfgs/kitti_models/centerpoint.yaml) restated as a dict;
# the neck's map (128 channels, 200 x 176 cells of 0.4 m) stands where that file's 2-D backbone would.
CENTER_PDM_CFG = {
    'NAME': 'CenterPoint',
    'BACKBONE_3D': dict(POINTRCNN_MSG_CFG),
    'MAP_TO_BEV': dict(PDM_SSD_CFG['MAP_TO_BEV']),
    'DENSE_HEAD': {'NAME': 'CenterHead', 'CLASS_AGNOSTIC': False, 'CLASS_NAMES_EACH_HEAD': [['Car', 'Pedestrian', 'Cyclist']],
                   'SHARED_CONV_CHANNEL': 64, 'USE_BIAS_BEFORE_NORM': True, 'NUM_HM_CONV': 2,
                   'SEPARATE_HEAD_CFG': {'HEAD_ORDER': ['center', 'center_z', 'dim', 'rot'],
                                         'HEAD_DICT': {'center': {'out_channels': 2, 'num_conv': 2},
                                                       'center_z': {'out_channels': 1, 'num_conv': 2},
                                                       'dim': {'out_channels': 3, 'num_conv': 2},
                                                       'rot': {'out_channels': 2, 'num_conv': 2}}},
                   'TARGET_ASSIGNER_CONFIG': {'FEATURE_MAP_STRIDE': 8, 'NUM_MAX_OBJS': 500, 'GAUSSIAN_OVERLAP': 0.1, 'MIN_RADIUS': 2},
                   'LOSS_CONFIG': {'LOSS_WEIGHTS': {'cls_weight': 1.0, 'loc_weight': 2.0,
                                                    'code_weights': [1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0]}},
                   'POST_PROCESSING': {'SCORE_THRESH': 0.1, 'POST_CENTER_LIMIT_RANGE': [-75.2, -75.2, -2, 75.2, 75.2, 4],
                                       'MAX_OBJ_PER_SAMPLE': 500,
                                       'NMS_CONFIG': {'MULTI_CLASSES_NMS': False, 'NMS_TYPE': 'nms_gpu', 'NMS_THRESH': 0.01,
                                                      'NMS_PRE_MAXSIZE': 4096, 'NMS_POST_MAXSIZE': 500}}},
    'POST_PROCESSING': {'RECALL_THRESH_LIST': [0.3, 0.5, 0.7], 'SCORE_THRESH': 0.1, 'OUTPUT_RAW_SCORE': False, 'EVAL_METRIC': 'kitti',
                        'NMS_CONFIG': {'MULTI_CLASSES_NMS': False, 'NMS_TYPE': 'nms_gpu', 'NMS_THRESH': 0.01,
                                       'NMS_PRE_MAXSIZE': 4096, 'NMS_POST_MAXSIZE': 500}},
}

# CenterPoint on dynamic pillars: DynamicPillarVFE -> PointPillarScatter -> BaseBEVBackbone -> CenterHead.  The 2-D backbone
# holds the upstream project's published KITTI PointPillars values (its tools/cfgs/kitti_models/pointpillar.yaml) restated
# as a dict; the head is CENTER_PDM_CFG's on that backbone's map (248 x 216 cells of 0.32 m: FEATURE_MAP_STRIDE 2).
PILLAR_RANGE = [0, -39.68, -3, 69.12, 39.68, 1]
PILLAR_VOXEL_SIZE = [0.16, 0.16, 4]
PILLAR_GRID_SIZE = [432, 496, 1]
CENTER_PILLAR_CFG = {
    'NAME': 'CenterPoint',
    'VFE': {'NAME': 'DynamicPillarVFE', 'USE_NORM': True, 'WITH_DISTANCE': False, 'USE_ABSLOTE_XYZ': True, 'NUM_FILTERS': [64]},
    'MAP_TO_BEV': {'NAME': 'PointPillarScatter', 'NUM_BEV_FEATURES': 64},
    'BACKBONE_2D': {'NAME': 'BaseBEVBackbone', 'LAYER_NUMS': [3, 5, 5], 'LAYER_STRIDES': [2, 2, 2], 'NUM_FILTERS': [64, 128, 256],
                    'UPSAMPLE_STRIDES': [1, 2, 4], 'NUM_UPSAMPLE_FILTERS': [128, 128, 128]},
    'DENSE_HEAD': copy.deepcopy(CENTER_PDM_CFG['DENSE_HEAD']),
    'POST_PROCESSING': copy.deepcopy(CENTER_PDM_CFG['POST_PROCESSING']),
}
CENTER_PILLAR_CFG['DENSE_HEAD']['TARGET_ASSIGNER_CONFIG']['FEATURE_MAP_STRIDE'] = 2

# PointPillars: DynamicPillarVFE -> PointPillarScatter -> BaseBEVBackbone -> AnchorHeadSingle on the 384-channel map.  VFE,
# scatter and 2-D backbone are CENTER_PILLAR_CFG's; the head values are the upstream project's published KITTI PointPillars
# settings (the dense head of its tools/cfgs/kitti_models/pointpillar.yaml) restated as a dict: 248 x 216 cells x 6 anchors =
# 321 408 anchors per sample.
POINT_PILLAR_CFG = {
    'NAME': 'PointPillar',
    'VFE': copy.deepcopy(CENTER_PILLAR_CFG['VFE']),
    'MAP_TO_BEV': copy.deepcopy(CENTER_PILLAR_CFG['MAP_TO_BEV']),
    'BACKBONE_2D': copy.deepcopy(CENTER_PILLAR_CFG['BACKBONE_2D']),
    'DENSE_HEAD': {'NAME': 'AnchorHeadSingle', 'CLASS_AGNOSTIC': False, 'USE_DIRECTION_CLASSIFIER': True, 'DIR_OFFSET': 0.78539,
                   'DIR_LIMIT_OFFSET': 0.0, 'NUM_DIR_BINS': 2,
                   'ANCHOR_GENERATOR_CONFIG': [
                       {'class_name': 'Car', 'anchor_sizes': [[3.9, 1.6, 1.56]], 'anchor_rotations': [0, 1.57],
                        'anchor_bottom_heights': [-1.78], 'align_center': False, 'feature_map_stride': 2,
                        'matched_threshold': 0.6, 'unmatched_threshold': 0.45},
                       {'class_name': 'Pedestrian', 'anchor_sizes': [[0.8, 0.6, 1.73]], 'anchor_rotations': [0, 1.57],
                        'anchor_bottom_heights': [-0.6], 'align_center': False, 'feature_map_stride': 2,
                        'matched_threshold': 0.5, 'unmatched_threshold': 0.35},
                       {'class_name': 'Cyclist', 'anchor_sizes': [[1.76, 0.6, 1.73]], 'anchor_rotations': [0, 1.57],
                        'anchor_bottom_heights': [-0.6], 'align_center': False, 'feature_map_stride': 2,
                        'matched_threshold': 0.5, 'unmatched_threshold': 0.35}],
                   'TARGET_ASSIGNER_CONFIG': {'NAME': 'AxisAlignedTargetAssigner', 'POS_FRACTION': -1.0, 'SAMPLE_SIZE': 512,
                                              'NORM_BY_NUM_EXAMPLES': False, 'MATCH_HEIGHT': False, 'BOX_CODER': 'ResidualCoder'},
                   'LOSS_CONFIG': {'LOSS_WEIGHTS': {'cls_weight': 1.0, 'loc_weight': 2.0, 'dir_weight': 0.2,
                                                    'code_weights': [1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0]}}},
    'POST_PROCESSING': copy.deepcopy(CENTER_PILLAR_CFG['POST_PROCESSING']),
}

# SECOND: DynamicMeanVFE -> VoxelBackBone8x -> HeightCompression -> BaseBEVBackbone -> AnchorHeadSingle on the KITTI voxel grid
# (VOXEL_SIZE, GRID_SIZE, range [0, -40, -3, 70.4, 40, 1]): the encoded tensor is 128 channels x 2 heights on 200 x 176 cells
# of 0.4 m (stride 8).  The 2-D backbone and head values are the upstream project's published KITTI SECOND settings (its
# tools/cfgs/kitti_models/second.yaml) restated as a dict; the anchors are POINT_PILLAR_CFG's at feature_map_stride 8.
SECOND_CFG = {
    'NAME': 'SECONDNet',
    'VFE': {'NAME': 'DynamicMeanVFE'},
    'BACKBONE_3D': {'NAME': 'VoxelBackBone8x'},
    'MAP_TO_BEV': {'NAME': 'HeightCompression', 'NUM_BEV_FEATURES': 256},
    'BACKBONE_2D': {'NAME': 'BaseBEVBackbone', 'LAYER_NUMS': [5, 5], 'LAYER_STRIDES': [1, 2], 'NUM_FILTERS': [128, 256],
                    'UPSAMPLE_STRIDES': [1, 2], 'NUM_UPSAMPLE_FILTERS': [256, 256]},
    'DENSE_HEAD': copy.deepcopy(POINT_PILLAR_CFG['DENSE_HEAD']),
    'POST_PROCESSING': copy.deepcopy(POINT_PILLAR_CFG['POST_PROCESSING']),
}
for _anchor_cfg in SECOND_CFG['DENSE_HEAD']['ANCHOR_GENERATOR_CONFIG']:
    _anchor_cfg['feature_map_stride'] = 8

# The same two detectors on HARD voxels, what the upstream project's published KITTI models were trained on: at most
# MAX_POINTS_PER_VOXEL points a cell and MAX_NUMBER_OF_VOXELS cells a sample (its transform_points_to_voxels values: 32 and 5
# points, 16000 / 40000 voxels), voxelized on the device by the encoder itself.  Every other detector on SECOND_CFG's or
# POINT_PILLAR_CFG's front end takes the same one-line change of its VFE entry.
HARD_MAX_NUMBER_OF_VOXELS = {'train': 16000, 'test': 40000}
POINT_PILLAR_HARD_CFG = copy.deepcopy(POINT_PILLAR_CFG)
POINT_PILLAR_HARD_CFG['VFE'].update(NAME='HardPillarVFE', MAX_POINTS_PER_VOXEL=32, MAX_NUMBER_OF_VOXELS=dict(HARD_MAX_NUMBER_OF_VOXELS))
SECOND_HARD_CFG = copy.deepcopy(SECOND_CFG)
SECOND_HARD_CFG['VFE'].update(NAME='HardMeanVFE', MAX_POINTS_PER_VOXEL=5, MAX_NUMBER_OF_VOXELS=dict(HARD_MAX_NUMBER_OF_VOXELS))

# CenterPoint on voxels: SECOND_CFG's front with the residual backbone, then CenterHead at FEATURE_MAP_STRIDE 8 (the head of
# CENTER_PDM_CFG, whose map has the same 200 x 176 cells).
CENTER_VOXEL_CFG = {
    'NAME': 'CenterPoint',
    'VFE': {'NAME': 'DynamicMeanVFE'},
    'BACKBONE_3D': {'NAME': 'VoxelResBackBone8x'},
    'MAP_TO_BEV': {'NAME': 'HeightCompression', 'NUM_BEV_FEATURES': 256},
    'BACKBONE_2D': copy.deepcopy(SECOND_CFG['BACKBONE_2D']),
    'DENSE_HEAD': copy.deepcopy(CENTER_PDM_CFG['DENSE_HEAD']),
    'POST_PROCESSING': copy.deepcopy(CENTER_PDM_CFG['POST_PROCESSING']),
}

# Voxel R-CNN: SECOND_CFG's front as it is, plus VoxelRCNNHead on the backbone's x_conv2 / x_conv3 / x_conv4 levels.  The
# snapshot this repository was modelled on holds no YAML for this detector, so the ROI_HEAD values are BUILD-DEFINED: they
# restate the upstream project's KITTI setting for Voxel R-CNN as far as it is remembered here (class-agnostic head, 6 x 6 x 6
# grid, one scale of 32 -> 32 channels per level with a 9 x 9 x 9 window and 16 samples, radii 0.4 / 0.8 / 1.6 m, three FC
# stacks of 256 -> 256, dropout 0.3, 100 test-time proposals at NMS 0.7) and were not checked against that file.  Of
# TARGET_CONFIG it holds the box coder alone, so its second stage has no training half (VOXEL_RCNN_TRAIN_CFG below adds it).
_VOXEL_RCNN_POOL = {'MLPS': [[32, 32]], 'QUERY_RANGES': [[4, 4, 4]], 'NSAMPLE': [16], 'POOL_METHOD': 'max_pool'}
VOXEL_RCNN_CFG = copy.deepcopy(SECOND_CFG)
VOXEL_RCNN_CFG['NAME'] = 'VoxelRCNN'
VOXEL_RCNN_CFG['ROI_HEAD'] = {
    'NAME': 'VoxelRCNNHead', 'CLASS_AGNOSTIC': True,
    'SHARED_FC': [256, 256], 'CLS_FC': [256, 256], 'REG_FC': [256, 256], 'DP_RATIO': 0.3,
    'NMS_CONFIG': {'TRAIN': {'NMS_TYPE': 'nms_gpu', 'MULTI_CLASSES_NMS': False, 'NMS_PRE_MAXSIZE': 9000,
                             'NMS_POST_MAXSIZE': 512, 'NMS_THRESH': 0.8},
                   'TEST': {'NMS_TYPE': 'nms_gpu', 'MULTI_CLASSES_NMS': False, 'NMS_PRE_MAXSIZE': 2048,
                            'NMS_POST_MAXSIZE': 100, 'NMS_THRESH': 0.7}},
    'ROI_GRID_POOL': {'FEATURES_SOURCE': ['x_conv2', 'x_conv3', 'x_conv4'], 'GRID_SIZE': 6,
                      'POOL_LAYERS': {'x_conv2': dict(copy.deepcopy(_VOXEL_RCNN_POOL), POOL_RADIUS=[0.4]),
                                      'x_conv3': dict(copy.deepcopy(_VOXEL_RCNN_POOL), POOL_RADIUS=[0.8]),
                                      'x_conv4': dict(copy.deepcopy(_VOXEL_RCNN_POOL), POOL_RADIUS=[1.6])}},
    'TARGET_CONFIG': {'BOX_CODER': 'ResidualCoder'}}

# VOXEL_RCNN_CFG plus the proposal-target sampler (TARGET_CONFIG) and the rcnn loss settings (LOSS_CONFIG): a head built from
# this dict has the training half, and build_voxel_rcnn(VOXEL_RCNN_TRAIN_CFG) takes training steps.  BUILD-DEFINED like the
# dict above: the values restate the upstream project's KITTI setting for Voxel R-CNN as remembered (IoU-graded class targets
# between 0.25 and 0.75, regression on proposals above 0.55) and were not checked against that file.
VOXEL_RCNN_TRAIN_CFG = copy.deepcopy(VOXEL_RCNN_CFG)
VOXEL_RCNN_TRAIN_CFG['ROI_HEAD']['TARGET_CONFIG'].update(
    ROI_PER_IMAGE=128, FG_RATIO=0.5, SAMPLE_ROI_BY_EACH_CLASS=True, CLS_SCORE_TYPE='roi_iou', CLS_FG_THRESH=0.75, CLS_BG_THRESH=0.25,
    CLS_BG_THRESH_LO=0.1, HARD_BG_RATIO=0.8, REG_FG_THRESH=0.55)
VOXEL_RCNN_TRAIN_CFG['ROI_HEAD']['LOSS_CONFIG'] = {
    'CLS_LOSS': 'BinaryCrossEntropy', 'REG_LOSS': 'smooth-l1', 'CORNER_LOSS_REGULARIZATION': True,
    'LOSS_WEIGHTS': {'rcnn_cls_weight': 1.0, 'rcnn_reg_weight': 1.0, 'rcnn_corner_weight': 1.0, 'code_weights': [1.0] * 7}}

# SECOND-IoU: SECOND_CFG's front as it is, plus SECONDHead on the 2-D backbone's 512-channel map (stride 8).  The snapshot this
# repository was modelled on holds no YAML for this detector, so the ROI_HEAD values are BUILD-DEFINED and were not checked
# against any file: class-agnostic head, a 7 x 7 crop of the 512 channels at DOWNSAMPLE_RATIO 8, FC stacks of 256 -> 256, dropout
# 0.3, 512 train proposals at NMS 0.8, 100 test proposals at NMS 0.7.  Of TARGET_CONFIG it holds the box coder alone, so its second
# stage has no training half (SECOND_IOU_TRAIN_CFG below adds it).  POST_PROCESSING scores the boxes by the predicted IoU.
SECOND_IOU_CFG = copy.deepcopy(SECOND_CFG)
SECOND_IOU_CFG['NAME'] = 'SECONDNetIoU'
SECOND_IOU_CFG['ROI_HEAD'] = {
    'NAME': 'SECONDHead', 'CLASS_AGNOSTIC': True,
    'SHARED_FC': [256, 256], 'IOU_FC': [256, 256], 'DP_RATIO': 0.3,
    'NMS_CONFIG': {'TRAIN': {'NMS_TYPE': 'nms_gpu', 'MULTI_CLASSES_NMS': False, 'NMS_PRE_MAXSIZE': 9000,
                             'NMS_POST_MAXSIZE': 512, 'NMS_THRESH': 0.8},
                   'TEST': {'NMS_TYPE': 'nms_gpu', 'MULTI_CLASSES_NMS': False, 'NMS_PRE_MAXSIZE': 2048,
                            'NMS_POST_MAXSIZE': 100, 'NMS_THRESH': 0.7}},
    'ROI_GRID_POOL': {'GRID_SIZE': 7, 'IN_CHANNEL': 512, 'DOWNSAMPLE_RATIO': 8},
    'TARGET_CONFIG': {'BOX_CODER': 'ResidualCoder'}}
SECOND_IOU_CFG['POST_PROCESSING']['NMS_CONFIG']['SCORE_TYPE'] = 'iou'

# SECOND_IOU_CFG plus the proposal-target sampler (TARGET_CONFIG) and the IoU loss settings (LOSS_CONFIG): a head built from this
# dict has the training half, and build_second_iou(SECOND_IOU_TRAIN_CFG) takes training steps.  BUILD-DEFINED like the dict above:
# 128 rois a sample, 'roi_iou' labels graded between 0.25 and 0.75, the binary cross-entropy IoU loss.  code_weights is what
# RoIHeadTemplate.build_losses reads; this head regresses no box, so they weigh nothing.
SECOND_IOU_TRAIN_CFG = copy.deepcopy(SECOND_IOU_CFG)
SECOND_IOU_TRAIN_CFG['ROI_HEAD']['TARGET_CONFIG'].update(
    ROI_PER_IMAGE=128, FG_RATIO=0.5, SAMPLE_ROI_BY_EACH_CLASS=True, CLS_SCORE_TYPE='roi_iou', CLS_FG_THRESH=0.75, CLS_BG_THRESH=0.25,
    CLS_BG_THRESH_LO=0.1, HARD_BG_RATIO=0.8, REG_FG_THRESH=0.55)
SECOND_IOU_TRAIN_CFG['ROI_HEAD']['LOSS_CONFIG'] = {
    'IOU_LOSS': 'BinaryCrossEntropy', 'LOSS_WEIGHTS': {'rcnn_iou_weight': 1.0, 'code_weights': [1.0] * 7}}

# PV-RCNN: SECOND_CFG's front as it is, plus the voxel set abstraction (PFE), the keypoint segmentation head and PVRCNNHead.  The
# snapshot this repository was modelled on holds no YAML for this detector, so the PFE, POINT_HEAD and ROI_HEAD values are
# BUILD-DEFINED: they restate the upstream project's published KITTI setting for PV-RCNN as far as it is remembered here (2048
# keypoints by FPS of the raw points, 128 fused features; two-scale set abstraction over the raw points and the four levels of
# the backbone; a 6 x 6 x 6 RoI grid over the keypoints at radii 0.8 / 1.6 m; FC stacks of 256, dropout 0.3, 100 test-time
# proposals at NMS 0.7) and were not checked against that file.  Eval only: TARGET_CONFIG holds the box coder alone.
PV_RCNN_CFG = copy.deepcopy(SECOND_CFG)
PV_RCNN_CFG['NAME'] = 'PVRCNN'
PV_RCNN_CFG['PFE'] = {
    'NAME': 'VoxelSetAbstraction', 'POINT_SOURCE': 'raw_points', 'NUM_KEYPOINTS': 2048, 'NUM_OUTPUT_FEATURES': 128, 'SAMPLE_METHOD': 'FPS',
    'FEATURES_SOURCE': ['bev', 'x_conv1', 'x_conv2', 'x_conv3', 'x_conv4', 'raw_points'],
    'SA_LAYER': {'raw_points': {'MLPS': [[16, 16], [16, 16]], 'POOL_RADIUS': [0.4, 0.8], 'NSAMPLE': [16, 16]},
                 'x_conv1': {'DOWNSAMPLE_FACTOR': 1, 'MLPS': [[16, 16], [16, 16]], 'POOL_RADIUS': [0.4, 0.8], 'NSAMPLE': [16, 16]},
                 'x_conv2': {'DOWNSAMPLE_FACTOR': 2, 'MLPS': [[32, 32], [32, 32]], 'POOL_RADIUS': [0.8, 1.2], 'NSAMPLE': [16, 32]},
                 'x_conv3': {'DOWNSAMPLE_FACTOR': 4, 'MLPS': [[64, 64], [64, 64]], 'POOL_RADIUS': [1.2, 2.4], 'NSAMPLE': [16, 32]},
                 'x_conv4': {'DOWNSAMPLE_FACTOR': 8, 'MLPS': [[64, 64], [64, 64]], 'POOL_RADIUS': [2.4, 4.8], 'NSAMPLE': [16, 32]}}}
PV_RCNN_CFG['POINT_HEAD'] = {'NAME': 'PointHeadSimple', 'CLS_FC': [256, 256], 'CLASS_AGNOSTIC': True,
                             'USE_POINT_FEATURES_BEFORE_FUSION': True}
PV_RCNN_CFG['ROI_HEAD'] = {
    'NAME': 'PVRCNNHead', 'CLASS_AGNOSTIC': True,
    'SHARED_FC': [256, 256], 'CLS_FC': [256, 256], 'REG_FC': [256, 256], 'DP_RATIO': 0.3,
    'NMS_CONFIG': {'TRAIN': {'NMS_TYPE': 'nms_gpu', 'MULTI_CLASSES_NMS': False, 'NMS_PRE_MAXSIZE': 9000,
                             'NMS_POST_MAXSIZE': 512, 'NMS_THRESH': 0.8},
                   'TEST': {'NMS_TYPE': 'nms_gpu', 'MULTI_CLASSES_NMS': False, 'NMS_PRE_MAXSIZE': 1024,
                            'NMS_POST_MAXSIZE': 100, 'NMS_THRESH': 0.7}},
    'ROI_GRID_POOL': {'GRID_SIZE': 6, 'MLPS': [[64, 64], [64, 64]], 'POOL_RADIUS': [0.8, 1.6], 'NSAMPLE': [16, 16],
                      'POOL_METHOD': 'max_pool'},
    'TARGET_CONFIG': {'BOX_CODER': 'ResidualCoder'}}

# Part-A2 (the anchor-based variant): SECOND_CFG's 2-D half on the sparse UNet, plus the intra-object part head on the UNet's
# per-voxel features and PartA2FCHead.  The snapshot this repository was modelled on holds no YAML for this detector, so the
# POINT_HEAD and ROI_HEAD values are BUILD-DEFINED: they restate the upstream project's published KITTI setting for Part-A2 as
# far as it is remembered here (a 12 x 12 x 12 RoI-aware grid of 128 features with at most 128 points a cell, three shared FC
# layers of 256, class and box stacks of 256 -> 256, dropout 0.3, points scoring under 0.3 masked out of the part features,
# point stacks of 256 -> 256, ground truth enlarged by 0.2 m for the point targets, 100 test-time proposals at NMS 0.7) and were
# not checked against that file.  Eval only: TARGET_CONFIG holds the box coder alone.  ROI_AWARE_POOL.FUSED selects the batched
# sparse pooling + sparse FC over the reference's composed formulation.
PART_A2_CFG = copy.deepcopy(SECOND_CFG)
PART_A2_CFG['NAME'] = 'PartA2Net'
PART_A2_CFG['BACKBONE_3D'] = {'NAME': 'UNetV2', 'RETURN_ENCODED_TENSOR': True}
PART_A2_CFG['POINT_HEAD'] = {'NAME': 'PointIntraPartOffsetHead', 'CLS_FC': [256, 256], 'PART_FC': [256, 256], 'CLASS_AGNOSTIC': True,
                             'TARGET_CONFIG': {'GT_EXTRA_WIDTH': [0.2, 0.2, 0.2]}}
PART_A2_CFG['ROI_HEAD'] = {
    'NAME': 'PartA2FCHead', 'CLASS_AGNOSTIC': True,
    'SHARED_FC': [256, 256, 256], 'CLS_FC': [256, 256], 'REG_FC': [256, 256], 'DP_RATIO': 0.3,
    'DISABLE_PART': False, 'SEG_MASK_SCORE_THRESH': 0.3,
    'NMS_CONFIG': {'TRAIN': {'NMS_TYPE': 'nms_gpu', 'MULTI_CLASSES_NMS': False, 'NMS_PRE_MAXSIZE': 9000,
                             'NMS_POST_MAXSIZE': 512, 'NMS_THRESH': 0.8},
                   'TEST': {'NMS_TYPE': 'nms_gpu', 'MULTI_CLASSES_NMS': False, 'NMS_PRE_MAXSIZE': 1024,
                            'NMS_POST_MAXSIZE': 100, 'NMS_THRESH': 0.7}},
    'ROI_AWARE_POOL': {'POOL_SIZE': 12, 'NUM_FEATURES': 128, 'MAX_POINTS_PER_VOXEL': 128, 'FUSED': True},
    'TARGET_CONFIG': {'BOX_CODER': 'ResidualCoder'}}


# PV-RCNN++: PV_RCNN_CFG with the proposals first, sectorized proposal-centric keypoint sampling and VectorPool aggregation.
# BUILD-DEFINED, not taken from a YAML (the snapshot this repository was modelled on holds none for this detector): 4096 keypoints
# by SPC over 6 sectors of the raw points within 1.6 m of a proposal, 90 fused features; bev, x_conv3, x_conv4 and the raw points,
# each filtered to the neighbourhood of the proposals (4.0 / 6.4 / 2.4 m) and gathered by two-scale local_interpolation VectorPool
# layers of 3 x 3 x 3 cells (2 x 2 x 2 at the raw points' first scale); a 6 x 6 x 6 RoI grid pooled by voxel_random_choice
# VectorPool layers at 0.8 / 1.6 m with 32 samples.  Eval only.
def _vector_pool(kind, reduced, post, cells, distances, nsample, widths):
    cfg = {'NAME': 'VectorPoolAggregationModuleMSG', 'NUM_GROUPS': 2, 'LOCAL_AGGREGATION_TYPE': kind, 'NUM_REDUCED_CHANNELS': reduced,
           'NUM_CHANNELS_OF_LOCAL_AGGREGATION': 32, 'MSG_POST_MLPS': [post]}
    for k in range(2):
        cfg[f'GROUP_CFG_{k}'] = {'NUM_LOCAL_VOXEL': list(cells[k]), 'MAX_NEIGHBOR_DISTANCE': distances[k], 'NEIGHBOR_NSAMPLE': nsample,
                                 'POST_MLPS': list(widths)}
    return cfg


PV_RCNN_PP_CFG = copy.deepcopy(PV_RCNN_CFG)
PV_RCNN_PP_CFG['NAME'] = 'PVRCNNPlusPlus'
PV_RCNN_PP_CFG['PFE'] = {
    'NAME': 'VoxelSetAbstractionSPC', 'POINT_SOURCE': 'raw_points', 'NUM_KEYPOINTS': 4096, 'NUM_OUTPUT_FEATURES': 90, 'SAMPLE_METHOD': 'SPC',
    'SPC_SAMPLING': {'NUM_SECTORS': 6, 'SAMPLE_RADIUS_WITH_ROI': 1.6},
    'FEATURES_SOURCE': ['bev', 'x_conv3', 'x_conv4', 'raw_points'],
    'SA_LAYER': {
        'raw_points': dict(_vector_pool('local_interpolation', 1, 32, ([2, 2, 2], [3, 3, 3]), (0.2, 0.4), -1, [32, 32]),
                           FILTER_NEIGHBOR_WITH_ROI=True, RADIUS_OF_NEIGHBOR_WITH_ROI=2.4),
        'x_conv3': dict(_vector_pool('local_interpolation', 32, 128, ([3, 3, 3], [3, 3, 3]), (1.2, 2.4), -1, [64, 64]),
                        DOWNSAMPLE_FACTOR=4, INPUT_CHANNELS=64, FILTER_NEIGHBOR_WITH_ROI=True, RADIUS_OF_NEIGHBOR_WITH_ROI=4.0),
        'x_conv4': dict(_vector_pool('local_interpolation', 32, 128, ([3, 3, 3], [3, 3, 3]), (2.4, 4.8), -1, [64, 64]),
                        DOWNSAMPLE_FACTOR=8, INPUT_CHANNELS=64, FILTER_NEIGHBOR_WITH_ROI=True, RADIUS_OF_NEIGHBOR_WITH_ROI=6.4)}}
PV_RCNN_PP_CFG['ROI_HEAD']['ROI_GRID_POOL'] = dict(
    _vector_pool('voxel_random_choice', 30, 128, ([3, 3, 3], [3, 3, 3]), (0.8, 1.6), 32, [64, 64]), GRID_SIZE=6)

# PillarNet: DynamicPillarVFESimple2D -> PillarBackBone8x -> BaseBEVBackboneV1 -> CenterHead.  The snapshot this repository was
# modelled on holds no YAML for this detector, so the values are BUILD-DEFINED and were not checked against any file: the KITTI
# voxel range with pillars of 0.05 x 0.05 x 4 m (grid 1408 x 1600 x 1), one PFN layer of 32 filters, the sparse 2-D backbone's
# 256-channel x_conv4 (stride 8, 200 x 176 cells) and x_conv5 (stride 16) through five 256-wide convolutions each and up to two
# 128-channel maps, and CENTER_PDM_CFG's CenterHead at FEATURE_MAP_STRIDE 8 with batched post-processing.  The reference's head for
# this detector also predicts an IoU (an `iou` head, IOU_REG_LOSS, USE_IOU_TO_RECTIFY_SCORE), which CenterHead here refuses: it is
# not part of this build.  PILLARNET_TRAIN_CFG is the same dict: CenterHead carries its training half, so
# build_pillarnet(PILLARNET_TRAIN_CFG) takes training steps; the name marks the intent, as the other *_TRAIN_CFG dicts do.
PILLARNET_RANGE = [0, -40, -3, 70.4, 40, 1]
PILLARNET_VOXEL_SIZE = [0.05, 0.05, 4]
PILLARNET_GRID_SIZE = [1408, 1600, 1]
PILLARNET_CFG = {
    'NAME': 'PillarNet',
    'VFE': {'NAME': 'DynamicPillarVFESimple2D', 'USE_NORM': True, 'WITH_DISTANCE': False, 'USE_ABSLOTE_XYZ': True, 'NUM_FILTERS': [32]},
    'BACKBONE_3D': {'NAME': 'PillarBackBone8x'},
    'BACKBONE_2D': {'NAME': 'BaseBEVBackboneV1', 'LAYER_NUMS': [5, 5], 'NUM_FILTERS': [256, 256], 'UPSAMPLE_STRIDES': [1, 2],
                    'NUM_UPSAMPLE_FILTERS': [128, 128]},
    'DENSE_HEAD': copy.deepcopy(CENTER_PDM_CFG['DENSE_HEAD']),
    'POST_PROCESSING': copy.deepcopy(CENTER_PDM_CFG['POST_PROCESSING']),
}
PILLARNET_CFG['DENSE_HEAD']['TARGET_ASSIGNER_CONFIG']['FEATURE_MAP_STRIDE'] = 8
PILLARNET_CFG['DENSE_HEAD']['POST_PROCESSING']['BATCHED'] = True
PILLARNET_TRAIN_CFG = copy.deepcopy(PILLARNET_CFG)

# TransFusion-L: the LiDAR branch of the upstream project's BEVFusion recipe for nuScenes, restated as far as it is remembered
# here and not checked against any file (the snapshot this repository was modelled on holds no YAML): ten classes, range
# [-54, 54] m x [-54, 54] m x [-5, 3] m on 0.075 x 0.075 x 0.2 m voxels (grid 1440 x 1440 x 40, a 180 x 180 map at stride 8),
# mean VFE -> VoxelResBackBone8x -> HeightCompression -> BaseBEVBackbone (512 channels out) -> TransFusionHead with 200 queries,
# 128 hidden channels, 8 attention heads, a 256-wide feed-forward block and a 3 x 3 local-maximum filter.  The encoder is
# DynamicMeanVFE, as in every voxel detector of this build (the plain NAME MeanVFE stays refused, vfe/__init__.py).  This dict
# is eval only: its head reads neither LOSS_CONFIG nor the assigner values; TRANSFUSION_LIDAR_TRAIN_CFG below adds the training half.
TRANSFUSION_CLASS_NAMES = ['car', 'truck', 'construction_vehicle', 'bus', 'trailer', 'barrier', 'motorcycle', 'bicycle',
                           'pedestrian', 'traffic_cone']
TRANSFUSION_RANGE = [-54.0, -54.0, -5.0, 54.0, 54.0, 3.0]
TRANSFUSION_VOXEL_SIZE = [0.075, 0.075, 0.2]
TRANSFUSION_GRID_SIZE = [1440, 1440, 40]
TRANSFUSION_LIDAR_CFG = {
    'NAME': 'TransFusion',
    'VFE': {'NAME': 'DynamicMeanVFE'},
    'BACKBONE_3D': {'NAME': 'VoxelResBackBone8x'},
    'MAP_TO_BEV': {'NAME': 'HeightCompression', 'NUM_BEV_FEATURES': 256},
    'BACKBONE_2D': {'NAME': 'BaseBEVBackbone', 'LAYER_NUMS': [5, 5], 'LAYER_STRIDES': [1, 2], 'NUM_FILTERS': [128, 256],
                    'UPSAMPLE_STRIDES': [1, 2], 'NUM_UPSAMPLE_FILTERS': [256, 256]},
    'DENSE_HEAD': {
        'NAME': 'TransFusionHead', 'CLASS_AGNOSTIC': False, 'USE_BIAS_BEFORE_NORM': False,
        'NUM_PROPOSALS': 200, 'HIDDEN_CHANNEL': 128, 'NUM_CLASSES': 10, 'NUM_HEADS': 8, 'NMS_KERNEL_SIZE': 3, 'FFN_CHANNEL': 256,
        'DROPOUT': 0.1, 'BN_MOMENTUM': 0.1, 'ACTIVATION': 'relu', 'NUM_HM_CONV': 2,
        'SEPARATE_HEAD_CFG': {'HEAD_ORDER': ['center', 'height', 'dim', 'rot', 'vel'],
                              'HEAD_DICT': {'center': {'out_channels': 2, 'num_conv': 2}, 'height': {'out_channels': 1, 'num_conv': 2},
                                            'dim': {'out_channels': 3, 'num_conv': 2}, 'rot': {'out_channels': 2, 'num_conv': 2},
                                            'vel': {'out_channels': 2, 'num_conv': 2}}},
        'TARGET_ASSIGNER_CONFIG': {'FEATURE_MAP_STRIDE': 8, 'DATASET': 'nuScenes', 'GAUSSIAN_OVERLAP': 0.1, 'MIN_RADIUS': 2,
                                   'HUNGARIAN_ASSIGNER': {'cls_cost': {'gamma': 2.0, 'alpha': 0.25, 'weight': 0.15},
                                                          'reg_cost': {'weight': 0.25}, 'iou_cost': {'weight': 0.25}}},
        'LOSS_CONFIG': {'LOSS_WEIGHTS': {'cls_weight': 1.0, 'bbox_weight': 0.25, 'hm_weight': 1.0,
                                         'code_weights': [1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 0.2, 0.2]},
                        'LOSS_CLS': {'use_sigmoid': True, 'gamma': 2.0, 'alpha': 0.25}},
        'POST_PROCESSING': {'SCORE_THRESH': 0.0, 'POST_CENTER_RANGE': [-61.2, -61.2, -10.0, 61.2, 61.2, 10.0]}},
    'POST_PROCESSING': {'RECALL_THRESH_LIST': [0.3, 0.5, 0.7], 'SCORE_THRESH': 0.1, 'OUTPUT_RAW_SCORE': False},
}
# the same detector with the head's training half: ASSIGN_ON_DEVICE is a key of this build (the reference has none like it);
# with it the head builds its HungarianAssigner3D and reads LOSS_CONFIG, without it the head is the eval-only one above
TRANSFUSION_LIDAR_TRAIN_CFG = copy.deepcopy(TRANSFUSION_LIDAR_CFG)
TRANSFUSION_LIDAR_TRAIN_CFG['DENSE_HEAD']['TARGET_ASSIGNER_CONFIG']['ASSIGN_ON_DEVICE'] = True
# ... and with the decoder's two attentions trained through attention_ops.mha_qkv / mha_kv (the fused forward with dropout and
# its HIP backward) instead of nn.MultiheadAttention: FUSED_ATTENTION_TRAIN is a key of this build too, opt-in; the attention
# dropout then draws from the head's ATTENTION_DROPOUT_SEED (default 0) and a device step counter, not from torch's generator
TRANSFUSION_LIDAR_FUSED_TRAIN_CFG = copy.deepcopy(TRANSFUSION_LIDAR_TRAIN_CFG)
TRANSFUSION_LIDAR_FUSED_TRAIN_CFG['DENSE_HEAD']['FUSED_ATTENTION_TRAIN'] = True


def synthetic_dataset(num_point_features=4):
    """The attributes Detector3DTemplate.build_networks reads from a dataset (detector3d_template.py:36-43)."""
    return SimpleNamespace(class_names=CLASS_NAMES, grid_size=GRID_SIZE, voxel_size=VOXEL_SIZE,
                           point_cloud_range=list(synthetic.KITTI_RANGE),
                           point_feature_encoder=SimpleNamespace(num_point_features=num_point_features))


def build_pdm_ssd(model_cfg=None, num_point_features=4):
    from .detectors import build_network
    cfg = cfg_from_dict(PDM_SSD_CFG if model_cfg is None else model_cfg)
    return build_network(cfg, num_class=len(CLASS_NAMES), dataset=synthetic_dataset(num_point_features))


def build_point_rcnn(model_cfg=None, num_point_features=4):
    """PointRCNN from POINT_RCNN_CFG (eval mode only), POINT_RCNN_TRAIN_CFG (with the second stage's training half) or a
    dict like them."""
    from .detectors import build_network
    cfg = cfg_from_dict(copy.deepcopy(POINT_RCNN_CFG if model_cfg is None else model_cfg))   # (the SA constructors edit MLPS)
    return build_network(cfg, num_class=len(CLASS_NAMES), dataset=synthetic_dataset(num_point_features))


def build_center_pdm(model_cfg=None, num_point_features=4):
    """CenterPoint from CENTER_PDM_CFG (or a dict like it): PointNet2MSG -> PDMNeck -> CenterHead."""
    from .detectors import build_network
    cfg = cfg_from_dict(copy.deepcopy(CENTER_PDM_CFG if model_cfg is None else model_cfg))
    return build_network(cfg, num_class=len(CLASS_NAMES), dataset=synthetic_dataset(num_point_features))


def pillar_dataset(num_point_features=4, point_cloud_range=None, voxel_size=None, grid_size=None):
    """The pillar detectors' dataset namespace: the KITTI PointPillars range, 0.16 m pillars over the whole height."""
    return SimpleNamespace(class_names=CLASS_NAMES, grid_size=list(PILLAR_GRID_SIZE if grid_size is None else grid_size),
                           voxel_size=list(PILLAR_VOXEL_SIZE if voxel_size is None else voxel_size),
                           point_cloud_range=list(PILLAR_RANGE if point_cloud_range is None else point_cloud_range),
                           point_feature_encoder=SimpleNamespace(num_point_features=num_point_features))


def build_center_pillar(model_cfg=None, num_point_features=4, dataset=None):
    """CenterPoint from CENTER_PILLAR_CFG (or a dict like it): DynamicPillarVFE -> PointPillarScatter -> BaseBEVBackbone ->
    CenterHead, on pillar_dataset() unless another dataset namespace is given."""
    from .detectors import build_network
    cfg = cfg_from_dict(copy.deepcopy(CENTER_PILLAR_CFG if model_cfg is None else model_cfg))
    return build_network(cfg, num_class=len(CLASS_NAMES), dataset=pillar_dataset(num_point_features) if dataset is None else dataset)


def build_point_pillar(model_cfg=None, num_point_features=4, dataset=None):
    """PointPillar from POINT_PILLAR_CFG (or a dict like it): DynamicPillarVFE -> PointPillarScatter -> BaseBEVBackbone ->
    AnchorHeadSingle, on pillar_dataset() unless another dataset namespace is given.  POINT_PILLAR_HARD_CFG puts HardPillarVFE
    (hard voxels) in front instead."""
    from .detectors import build_network
    cfg = cfg_from_dict(copy.deepcopy(POINT_PILLAR_CFG if model_cfg is None else model_cfg))
    return build_network(cfg, num_class=len(CLASS_NAMES), dataset=pillar_dataset(num_point_features) if dataset is None else dataset)


def voxel_dataset(num_point_features=4, point_cloud_range=None, voxel_size=None, grid_size=None):
    """The voxel detectors' dataset namespace: the KITTI range on VOXEL_SIZE / GRID_SIZE unless other values are given."""
    return SimpleNamespace(class_names=CLASS_NAMES, grid_size=list(GRID_SIZE if grid_size is None else grid_size),
                           voxel_size=list(VOXEL_SIZE if voxel_size is None else voxel_size),
                           point_cloud_range=list(synthetic.KITTI_RANGE if point_cloud_range is None else point_cloud_range),
                           point_feature_encoder=SimpleNamespace(num_point_features=num_point_features))


def build_second(model_cfg=None, num_point_features=4, dataset=None):
    """SECONDNet from SECOND_CFG (or a dict like it): DynamicMeanVFE -> VoxelBackBone8x -> HeightCompression -> BaseBEVBackbone ->
    AnchorHeadSingle, on voxel_dataset() unless another dataset namespace is given.  Runs in eval mode and takes training steps.
    SECOND_HARD_CFG puts HardMeanVFE (hard voxels) in front instead."""
    from .detectors import build_network
    cfg = cfg_from_dict(copy.deepcopy(SECOND_CFG if model_cfg is None else model_cfg))
    return build_network(cfg, num_class=len(CLASS_NAMES), dataset=voxel_dataset(num_point_features) if dataset is None else dataset)


def build_center_voxel(model_cfg=None, num_point_features=4, dataset=None):
    """CenterPoint from CENTER_VOXEL_CFG (or a dict like it): DynamicMeanVFE -> VoxelResBackBone8x -> HeightCompression ->
    BaseBEVBackbone -> CenterHead, on voxel_dataset() unless another dataset namespace is given.  Runs in eval mode and takes
    training steps."""
    from .detectors import build_network
    cfg = cfg_from_dict(copy.deepcopy(CENTER_VOXEL_CFG if model_cfg is None else model_cfg))
    return build_network(cfg, num_class=len(CLASS_NAMES), dataset=voxel_dataset(num_point_features) if dataset is None else dataset)


def build_voxel_rcnn(model_cfg=None, num_point_features=4, dataset=None):
    """VoxelRCNN from VOXEL_RCNN_CFG, VOXEL_RCNN_TRAIN_CFG (with the second stage's training half) or a dict like them:
    DynamicMeanVFE -> VoxelBackBone8x -> HeightCompression -> BaseBEVBackbone -> AnchorHeadSingle -> VoxelRCNNHead, on
    voxel_dataset() unless another dataset namespace is given.  Runs in eval mode and, from the training dict, takes training steps."""
    from .detectors import build_network
    cfg = cfg_from_dict(copy.deepcopy(VOXEL_RCNN_CFG if model_cfg is None else model_cfg))
    return build_network(cfg, num_class=len(CLASS_NAMES), dataset=voxel_dataset(num_point_features) if dataset is None else dataset)


def build_second_iou(model_cfg=None, num_point_features=4, dataset=None):
    """SECONDNetIoU from SECOND_IOU_CFG, SECOND_IOU_TRAIN_CFG (with the second stage's training half) or a dict like them:
    DynamicMeanVFE -> VoxelBackBone8x -> HeightCompression -> BaseBEVBackbone -> AnchorHeadSingle -> SECONDHead, on voxel_dataset()
    unless another dataset namespace is given.  Runs in eval mode and, from the training dict, takes training steps."""
    from .detectors import build_network
    cfg = cfg_from_dict(copy.deepcopy(SECOND_IOU_CFG if model_cfg is None else model_cfg))
    return build_network(cfg, num_class=len(CLASS_NAMES), dataset=voxel_dataset(num_point_features) if dataset is None else dataset)


def build_pv_rcnn(model_cfg=None, num_point_features=4, dataset=None):
    """PVRCNN from PV_RCNN_CFG (or a dict like it): DynamicMeanVFE -> VoxelBackBone8x -> HeightCompression -> VoxelSetAbstraction ->
    BaseBEVBackbone -> AnchorHeadSingle -> PointHeadSimple -> PVRCNNHead (the reference's module order), on voxel_dataset() unless
    another dataset namespace is given.  Runs in eval mode only."""
    from .detectors import build_network
    cfg = cfg_from_dict(copy.deepcopy(PV_RCNN_CFG if model_cfg is None else model_cfg))   # (the SA constructors edit MLPS)
    return build_network(cfg, num_class=len(CLASS_NAMES), dataset=voxel_dataset(num_point_features) if dataset is None else dataset)


def build_part_a2(model_cfg=None, num_point_features=4, dataset=None):
    """PartA2Net from PART_A2_CFG (or a dict like it): DynamicMeanVFE -> UNetV2 -> HeightCompression -> BaseBEVBackbone ->
    AnchorHeadSingle -> PointIntraPartOffsetHead -> PartA2FCHead, on voxel_dataset() unless another dataset namespace is given.
    Runs in eval mode only."""
    from .detectors import build_network
    cfg = cfg_from_dict(copy.deepcopy(PART_A2_CFG if model_cfg is None else model_cfg))
    return build_network(cfg, num_class=len(CLASS_NAMES), dataset=voxel_dataset(num_point_features) if dataset is None else dataset)


def build_pv_rcnn_plusplus(model_cfg=None, num_point_features=4, dataset=None):
    """PVRCNNPlusPlus from PV_RCNN_PP_CFG (or a dict like it): the modules of build_pv_rcnn() with VoxelSetAbstractionSPC as the pfe
    (DynamicMeanVFE -> VoxelBackBone8x -> HeightCompression -> VoxelSetAbstractionSPC -> BaseBEVBackbone -> AnchorHeadSingle ->
    PointHeadSimple -> PVRCNNHead in the template's build order; the detector's forward runs the proposal layer before the pfe), on
    voxel_dataset() unless another dataset namespace is given.  Runs in eval mode only."""
    from .detectors import build_network
    cfg = cfg_from_dict(copy.deepcopy(PV_RCNN_PP_CFG if model_cfg is None else model_cfg))
    return build_network(cfg, num_class=len(CLASS_NAMES), dataset=voxel_dataset(num_point_features) if dataset is None else dataset)


def pillarnet_dataset(num_point_features=4, point_cloud_range=None, voxel_size=None, grid_size=None):
    """PillarNet's dataset namespace: the KITTI voxel range on 0.05 m pillars over the whole height unless other values are given."""
    return SimpleNamespace(class_names=CLASS_NAMES, grid_size=list(PILLARNET_GRID_SIZE if grid_size is None else grid_size),
                           voxel_size=list(PILLARNET_VOXEL_SIZE if voxel_size is None else voxel_size),
                           point_cloud_range=list(PILLARNET_RANGE if point_cloud_range is None else point_cloud_range),
                           point_feature_encoder=SimpleNamespace(num_point_features=num_point_features))


def build_pillarnet(model_cfg=None, num_point_features=4, dataset=None):
    """PillarNet from PILLARNET_CFG, PILLARNET_TRAIN_CFG or a dict like them: DynamicPillarVFESimple2D -> PillarBackBone8x (or
    PillarRes18BackBone8x) -> BaseBEVBackboneV1 -> CenterHead, on pillarnet_dataset() unless another dataset namespace is given.
    Runs in eval mode and takes training steps."""
    from .detectors import build_network
    cfg = cfg_from_dict(copy.deepcopy(PILLARNET_CFG if model_cfg is None else model_cfg))
    return build_network(cfg, num_class=len(CLASS_NAMES), dataset=pillarnet_dataset(num_point_features) if dataset is None else dataset)


def transfusion_dataset(num_point_features=5, point_cloud_range=None, voxel_size=None, grid_size=None):
    """TransFusion-L's dataset namespace: ten nuScenes class names on the 108 m x 108 m x 8 m range with 0.075 m voxels unless
    other values are given; points carry (x, y, z, intensity, time lag)."""
    return SimpleNamespace(class_names=list(TRANSFUSION_CLASS_NAMES),
                           grid_size=list(TRANSFUSION_GRID_SIZE if grid_size is None else grid_size),
                           voxel_size=list(TRANSFUSION_VOXEL_SIZE if voxel_size is None else voxel_size),
                           point_cloud_range=list(TRANSFUSION_RANGE if point_cloud_range is None else point_cloud_range),
                           point_feature_encoder=SimpleNamespace(num_point_features=num_point_features))


def build_transfusion_lidar(model_cfg=None, num_point_features=5, dataset=None):
    """TransFusion from TRANSFUSION_LIDAR_CFG (eval mode only), TRANSFUSION_LIDAR_TRAIN_CFG (with the head's training half),
    TRANSFUSION_LIDAR_FUSED_TRAIN_CFG (training through the fused attention as well) or a dict like them: DynamicMeanVFE -> VoxelResBackBone8x -> HeightCompression -> BaseBEVBackbone -> TransFusionHead, on
    transfusion_dataset() unless another dataset namespace is given."""
    from .detectors import build_network
    cfg = cfg_from_dict(copy.deepcopy(TRANSFUSION_LIDAR_CFG if model_cfg is None else model_cfg))
    dataset = transfusion_dataset(num_point_features) if dataset is None else dataset
    return build_network(cfg, num_class=len(dataset.class_names), dataset=dataset)


# DSVT-Pillar: DynamicPillarVFE -> DSVT -> PointPillarScatter3d -> BaseBEVResBackbone -> CenterHead under the CenterPoint
# detector.  The reference ships no yaml for it, so the values are build-defined, after the published pillar model: 192 channels in
# 8 heads (d = 24), sets of 36, one stage of 4 blocks, 12 x 12 x 1 windows with hybrid factor 2 x 2 x 1, a 468 x 468 x 1 grid of
# 0.32 m pillars, FFN 384 with gelu.  The head is CENTER_PDM_CFG's on the backbone's stride-1 map.  Eval only for the fused
# operators; CenterHead's iou branch, USE_IOU_TO_RECTIFY_SCORE and class_specific_nms are not built.
DSVT_RANGE = [-74.88, -74.88, -2, 74.88, 74.88, 4.0]
DSVT_VOXEL_SIZE = [0.32, 0.32, 6]
DSVT_GRID_SIZE = [468, 468, 1]
DSVT_PILLAR_CFG = {
    'NAME': 'CenterPoint',
    'VFE': {'NAME': 'DynamicPillarVFE', 'USE_NORM': True, 'WITH_DISTANCE': False, 'USE_ABSLOTE_XYZ': True, 'NUM_FILTERS': [192, 192]},
    'BACKBONE_3D': {'NAME': 'DSVT',
                    'INPUT_LAYER': {'sparse_shape': [468, 468, 1], 'downsample_stride': [], 'd_model': [192], 'set_info': [[36, 4]],
                                    'window_shape': [[12, 12, 1]], 'hybrid_factor': [2, 2, 1], 'shifts_list': [[[0, 0, 0], [6, 6, 0]]],
                                    'normalize_pos': False},
                    'block_name': ['DSVTBlock'], 'set_info': [[36, 4]], 'd_model': [192], 'nhead': [8], 'dim_feedforward': [384],
                    'dropout': 0.0, 'activation': 'gelu', 'output_shape': [468, 468], 'conv_out_channel': 192},
    'MAP_TO_BEV': {'NAME': 'PointPillarScatter3d', 'INPUT_SHAPE': [468, 468, 1], 'NUM_BEV_FEATURES': 192},
    'BACKBONE_2D': {'NAME': 'BaseBEVResBackbone', 'LAYER_NUMS': [1, 2, 2], 'LAYER_STRIDES': [1, 2, 2], 'NUM_FILTERS': [128, 128, 256],
                    'UPSAMPLE_STRIDES': [1, 2, 4], 'NUM_UPSAMPLE_FILTERS': [128, 128, 128]},
    'DENSE_HEAD': copy.deepcopy(CENTER_PDM_CFG['DENSE_HEAD']),
    'POST_PROCESSING': copy.deepcopy(CENTER_PDM_CFG['POST_PROCESSING']),
}
DSVT_PILLAR_CFG['DENSE_HEAD']['TARGET_ASSIGNER_CONFIG']['FEATURE_MAP_STRIDE'] = 1
DSVT_PILLAR_CFG['DENSE_HEAD']['POST_PROCESSING']['POST_CENTER_LIMIT_RANGE'] = [-80, -80, -10.0, 80, 80, 10.0]


def dsvt_dataset(num_point_features=4, point_cloud_range=None, voxel_size=None, grid_size=None):
    """DSVT-Pillar's dataset namespace: a 149.76 m square of 0.32 m pillars over the whole height unless other values are given."""
    return SimpleNamespace(class_names=CLASS_NAMES, grid_size=list(DSVT_GRID_SIZE if grid_size is None else grid_size),
                           voxel_size=list(DSVT_VOXEL_SIZE if voxel_size is None else voxel_size),
                           point_cloud_range=list(DSVT_RANGE if point_cloud_range is None else point_cloud_range),
                           point_feature_encoder=SimpleNamespace(num_point_features=num_point_features))


def build_dsvt_pillar(model_cfg=None, num_point_features=4, dataset=None):
    """CenterPoint from DSVT_PILLAR_CFG (or a dict like it): DynamicPillarVFE -> DSVT -> PointPillarScatter3d ->
    BaseBEVResBackbone -> CenterHead, on dsvt_dataset() unless another dataset namespace is given.  The backbone's sparse_shape
    and the scatter's INPUT_SHAPE must be the dataset's grid."""
    from .detectors import build_network
    cfg = cfg_from_dict(copy.deepcopy(DSVT_PILLAR_CFG if model_cfg is None else model_cfg))
    return build_network(cfg, num_class=len(CLASS_NAMES), dataset=dsvt_dataset(num_point_features) if dataset is None else dataset)

"""Detector assembly: the spconv-free equivalent of the reference's Detector3DTemplate for the point path.

Contract restated from /root/reference/pcdet/models/detectors/detector3d_template.py:14-139 (module topology, one
`build_<slot>` per slot, modules chosen by `NAME` from registry dicts, `model_info_dict` threading channel counts),
:178-263 (post_processing: per-sample class-agnostic NMS over the head's boxes) and :330-359 (shape-filtered
checkpoint loading).  The reference's template cannot be imported on this platform (it pulls in spconv,
pcdet/utils/spconv_utils.py:3).  The vfe, backbone_3d, map_to_bev and backbone_2d slots build the pillar family
(DynamicPillarVFE -> PointPillarScatter -> BaseBEVBackbone) and the voxel family (DynamicMeanVFE ->
VoxelBackBone8x / VoxelResBackBone8x -> HeightCompression -> BaseBEVBackbone) on this package's own sparse convolution, each also
on hard voxels (HardPillarVFE / HardMeanVFE, which voxelize on the device with the two sizes of their own config); a NAME outside
the registries (the plain MeanVFE and PillarVFE among them, ...) is refused.  The sparse pillar family (DynamicPillarVFESimple2D ->
PillarBackBone8x / PillarRes18BackBone8x -> BaseBEVBackboneV1, PillarNet) has no map_to_bev module: its 2-D backbone reads the dense
levels the sparse 2-D backbone leaves, and is refused without one.  The pfe slot builds PV-RCNN's VoxelSetAbstraction or PV-RCNN++'s
VoxelSetAbstractionSPC, the roi_head slot the RoI heads of roi_heads/ (PointRCNN's second stage, Voxel R-CNN's, PV-RCNN's in eval
mode).
"""
import torch
import torch.nn as nn

from .. import backbones_2d, backbones_3d, dense_heads, roi_heads, vfe
from ..backbones_2d import map_to_bev
from ..backbones_3d import pfe
from ..iou3d_nms import iou3d_nms_utils
from ..pdm_neck import PDMNeck
from ..pointnet2_backbone import PointNet2MSG

# registries keyed by NAME, as pcdet/models/backbones_3d/__init__.py:10-22 and map_to_bev/__init__.py:5-10
BACKBONES_3D = {'PointNet2MSG': PointNet2MSG, **backbones_3d.__all__}
MAP_TO_BEV = {'PDMNeck': PDMNeck, **map_to_bev.__all__}
VFE = {k: v for k, v in vfe.__all__.items() if k != 'VFETemplate'}
BACKBONES_2D = dict(backbones_2d.__all__)


def _get(cfg, key, default=None):
    return cfg.get(key, default) if isinstance(cfg, dict) else getattr(cfg, key, default)


class Detector3DTemplate(nn.Module):
    def __init__(self, model_cfg, num_class, dataset):
        """dataset: an object with class_names, point_feature_encoder.num_point_features, grid_size,
        point_cloud_range, voxel_size (the attributes build_networks reads, ref :36-43)."""
        super().__init__()
        self.model_cfg = model_cfg
        self.num_class = num_class
        self.dataset = dataset
        self.class_names = dataset.class_names
        self.register_buffer('global_step', torch.LongTensor(1).zero_())
        self.module_topology = ['vfe', 'backbone_3d', 'map_to_bev_module', 'pfe', 'backbone_2d', 'dense_head',
                                'point_head', 'roi_head']

    @property
    def mode(self):
        return 'TRAIN' if self.training else 'TEST'

    def update_global_step(self):
        self.global_step += 1

    def build_networks(self):
        model_info_dict = {
            'module_list': [],
            'num_rawpoint_features': self.dataset.point_feature_encoder.num_point_features,
            'num_point_features': self.dataset.point_feature_encoder.num_point_features,
            'grid_size': self.dataset.grid_size,
            'point_cloud_range': self.dataset.point_cloud_range,
            'voxel_size': self.dataset.voxel_size,
        }
        for module_name in self.module_topology:
            module, model_info_dict = getattr(self, 'build_%s' % module_name)(model_info_dict=model_info_dict)
            self.add_module(module_name, module)
        return model_info_dict['module_list']

    def _registered(self, key, registry):
        """the slot's config, or None; a NAME outside the registry is one of the reference's spconv / voxel modules"""
        cfg = _get(self.model_cfg, key, None)
        assert cfg is None or _get(cfg, 'NAME') in registry, \
            f"{key} {_get(cfg, 'NAME')} needs spconv / voxel modules: not built here (have {sorted(registry)})"
        return cfg

    def build_vfe(self, model_info_dict):
        """ref :62-77: the encoder's output width becomes num_point_features"""
        cfg = self._registered('VFE', VFE)
        if cfg is None:
            return None, model_info_dict
        module = VFE[_get(cfg, 'NAME')](
            model_cfg=cfg, num_point_features=model_info_dict['num_rawpoint_features'],
            point_cloud_range=model_info_dict['point_cloud_range'], voxel_size=model_info_dict['voxel_size'],
            grid_size=model_info_dict['grid_size'])
        model_info_dict['num_point_features'] = module.get_output_feature_dim()
        model_info_dict['module_list'].append(module)
        return module, model_info_dict

    def build_pfe(self, model_info_dict):
        """ref :109-125: the point feature encoder (PV-RCNN's VoxelSetAbstraction); its widths become num_point_features and
        num_point_features_before_fusion"""
        cfg = self._registered('PFE', pfe.__all__)
        if cfg is None:
            return None, model_info_dict
        module = pfe.__all__[_get(cfg, 'NAME')](
            model_cfg=cfg, voxel_size=model_info_dict['voxel_size'], point_cloud_range=model_info_dict['point_cloud_range'],
            num_bev_features=model_info_dict['num_bev_features'], num_rawpoint_features=model_info_dict['num_rawpoint_features'])
        model_info_dict['module_list'].append(module)
        model_info_dict['num_point_features'] = module.num_point_features
        model_info_dict['num_point_features_before_fusion'] = module.num_point_features_before_fusion
        return module, model_info_dict

    def build_backbone_2d(self, model_info_dict):
        """ref :106-117: reads num_bev_features of the map_to_bev module and replaces it with its own"""
        cfg = self._registered('BACKBONE_2D', BACKBONES_2D)
        if cfg is None:
            return None, model_info_dict
        if _get(cfg, 'NAME') == 'BaseBEVBackboneV1':
            # it reads multi_scale_2d_features['x_conv4' / 'x_conv5']: the model's BACKBONE_3D must have published those two widths
            channels = model_info_dict.get('backbone_channels', None) or {}
            assert 'x_conv4' in channels and 'x_conv5' in channels, \
                ('BACKBONE_2D BaseBEVBackboneV1 needs a sparse 2-D (spconv-style) BACKBONE_3D such as PillarBackBone8x, whose dense '
                 f'x_conv4 / x_conv5 maps it reads; this model\'s backbone published {sorted(channels)}')
        module = BACKBONES_2D[_get(cfg, 'NAME')](model_cfg=cfg, input_channels=model_info_dict.get('num_bev_features', None))
        model_info_dict['module_list'].append(module)
        model_info_dict['num_bev_features'] = module.num_bev_features
        return module, model_info_dict

    def build_roi_head(self, model_info_dict):
        """ref :159-176: built by NAME from roi_heads.__all__; backbone_channels, point_cloud_range and voxel_size are what the
        voxel-based head (VoxelRCNNHead) reads, the point-based ones take them as unused keywords."""
        cfg = _get(self.model_cfg, 'ROI_HEAD', None)
        if cfg is None:
            return None, model_info_dict
        module = roi_heads.__all__[_get(cfg, 'NAME')](
            model_cfg=cfg, input_channels=model_info_dict['num_point_features'],
            backbone_channels=model_info_dict.get('backbone_channels', {}), point_cloud_range=model_info_dict['point_cloud_range'],
            voxel_size=model_info_dict['voxel_size'],
            num_class=self.num_class if not _get(cfg, 'CLASS_AGNOSTIC', False) else 1)
        model_info_dict['module_list'].append(module)
        return module, model_info_dict

    def build_backbone_3d(self, model_info_dict):
        cfg = _get(self.model_cfg, 'BACKBONE_3D', None)
        if cfg is None:
            return None, model_info_dict
        module = BACKBONES_3D[_get(cfg, 'NAME')](
            model_cfg=cfg, input_channels=model_info_dict['num_point_features'], grid_size=model_info_dict['grid_size'],
            voxel_size=model_info_dict['voxel_size'], point_cloud_range=model_info_dict['point_cloud_range'])
        model_info_dict['module_list'].append(module)
        model_info_dict['num_point_features'] = module.num_point_features
        model_info_dict['backbone_channels'] = getattr(module, 'backbone_channels', None)
        return module, model_info_dict

    def build_map_to_bev_module(self, model_info_dict):
        cfg = _get(self.model_cfg, 'MAP_TO_BEV', None)
        if cfg is None:
            return None, model_info_dict
        # (the reference passes model_cfg and grid_size only, ref :89-92; the PDM neck also needs the metric grid)
        module = MAP_TO_BEV[_get(cfg, 'NAME')](
            model_cfg=cfg, grid_size=model_info_dict['grid_size'], voxel_size=model_info_dict['voxel_size'],
            point_cloud_range=model_info_dict['point_cloud_range'])
        model_info_dict['module_list'].append(module)
        model_info_dict['num_bev_features'] = module.num_bev_features
        return module, model_info_dict

    def build_dense_head(self, model_info_dict):
        cfg = _get(self.model_cfg, 'DENSE_HEAD', None)
        if cfg is None:
            return None, model_info_dict
        module = dense_heads.__all__[_get(cfg, 'NAME')](
            model_cfg=cfg, input_channels=model_info_dict.get('num_bev_features', None),
            num_class=self.num_class if not _get(cfg, 'CLASS_AGNOSTIC', False) else 1, class_names=self.class_names,
            grid_size=model_info_dict['grid_size'], point_cloud_range=model_info_dict['point_cloud_range'],
            predict_boxes_when_training=_get(self.model_cfg, 'ROI_HEAD', False),
            voxel_size=model_info_dict.get('voxel_size', False))
        model_info_dict['module_list'].append(module)
        return module, model_info_dict

    def build_point_head(self, model_info_dict):
        cfg = _get(self.model_cfg, 'POINT_HEAD', None)
        if cfg is None:
            return None, model_info_dict
        before_fusion = _get(cfg, 'USE_POINT_FEATURES_BEFORE_FUSION', False) and 'num_point_features_before_fusion' in model_info_dict
        module = dense_heads.__all__[_get(cfg, 'NAME')](
            model_cfg=cfg, input_channels=model_info_dict['num_point_features_before_fusion' if before_fusion else 'num_point_features'],
            num_class=self.num_class if not _get(cfg, 'CLASS_AGNOSTIC', False) else 1,
            predict_boxes_when_training=_get(self.model_cfg, 'ROI_HEAD', False))
        model_info_dict['module_list'].append(module)
        return module, model_info_dict

    def forward(self, **kwargs):
        raise NotImplementedError

    def post_processing(self, batch_dict):
        """batch_cls_preds (N1 + N2 + ..., num_class | 1) logits, batch_box_preds (.., 7), batch_index (..) ->
        ([{'pred_boxes', 'pred_scores', 'pred_labels'}] per sample, recall_dict) as the reference (ref :178-263).

        The default is the reference's per-sample loop.  POST_PROCESSING.BATCHED (absent = False) runs the whole batch
        through pdm_post_process on the device (post_process.py) with identical results; it falls back to the loop,
        with a one-time warning, for a list of cls_preds, has_class_labels, rois, NMS_PRE_MAXSIZE > 16384,
        NMS_THRESH < 0 or a batch_index that is not sample-major."""
        cfg = _get(self.model_cfg, 'POST_PROCESSING')
        if _get(cfg, 'BATCHED', False):
            from .. import post_process
            nms_cfg = _get(cfg, 'NMS_CONFIG')
            reason = None
            if isinstance(batch_dict['batch_cls_preds'], list):
                reason = 'a list of cls_preds'
            elif batch_dict.get('has_class_labels', False):
                reason = 'has_class_labels'
            elif 'rois' in batch_dict:
                reason = 'rois'
            elif int(_get(nms_cfg, 'NMS_PRE_MAXSIZE')) > post_process.MAX_PRE:
                reason = f'NMS_PRE_MAXSIZE > {post_process.MAX_PRE}'
            elif float(_get(nms_cfg, 'NMS_THRESH')) < 0:
                reason = 'NMS_THRESH < 0'
            if reason is None:
                out = post_process.batched_post_processing(batch_dict, cfg, self.num_class,
                                                           gt_boxes=batch_dict.get('gt_boxes', None))
                if out is not None:
                    return out
                reason = 'batch_index is not sample-major'
            post_process.warn_once(reason)
        return self.post_processing_loop(batch_dict)

    def post_processing_loop(self, batch_dict):
        """The reference's per-sample loop (ref :178-263): sigmoid, then either
        - class-agnostic NMS: arg-max class, score threshold, top NMS_PRE_MAXSIZE, rotated NMS (HIP kernels of
          iou3d_nms.hip), first NMS_POST_MAXSIZE; OUTPUT_RAW_SCORE reports the raw maximum instead; or
        - MULTI_CLASSES_NMS: the same per class column (iou3d_nms_utils.multi_classes_nms), survivors class after class.
          The reference's line builds the label mapping as torch.arange(1, self.num_class), which fails its own
          `assert cur_cls_preds.shape[1] == len(cur_label_mapping)` for num_class columns; the evident intent, labels
          1 .. num_class, is implemented here (a list of cls_preds with multihead_label_mapping is not supported).
        and generate_recall_record when batch_dict holds gt_boxes."""
        cfg = _get(self.model_cfg, 'POST_PROCESSING')
        nms_cfg = _get(cfg, 'NMS_CONFIG')
        assert not isinstance(batch_dict['batch_cls_preds'], list), 'a list of cls_preds is not part of the point path'
        recall_dict = {}
        pred_dicts = []
        for index in range(batch_dict['batch_size']):
            if batch_dict.get('batch_index', None) is not None:
                assert batch_dict['batch_box_preds'].dim() == 2
                batch_mask = batch_dict['batch_index'] == index
            else:
                assert batch_dict['batch_box_preds'].dim() == 3
                batch_mask = index
            box_preds = batch_dict['batch_box_preds'][batch_mask]
            src_box_preds = box_preds
            cls_preds = batch_dict['batch_cls_preds'][batch_mask]
            src_cls_preds = cls_preds
            assert cls_preds.shape[1] in [1, self.num_class]
            if not batch_dict['cls_preds_normalized']:
                cls_preds = torch.sigmoid(cls_preds)
            if _get(nms_cfg, 'MULTI_CLASSES_NMS', False):
                label_mapping = torch.arange(1, self.num_class + 1, device=cls_preds.device)
                assert cls_preds.shape[1] == len(label_mapping)
                final_scores, final_labels, final_boxes = iou3d_nms_utils.multi_classes_nms(
                    cls_scores=cls_preds, box_preds=box_preds, nms_config=nms_cfg, score_thresh=_get(cfg, 'SCORE_THRESH'))
                final_labels = label_mapping[final_labels]
            else:
                cls_preds, label_preds = torch.max(cls_preds, dim=-1)
                if batch_dict.get('has_class_labels', False):
                    label_key = 'roi_labels' if 'roi_labels' in batch_dict else 'batch_pred_labels'
                    label_preds = batch_dict[label_key][index]
                else:
                    label_preds = label_preds + 1
                selected, selected_scores = iou3d_nms_utils.class_agnostic_nms(
                    box_scores=cls_preds, box_preds=box_preds, nms_config=nms_cfg, score_thresh=_get(cfg, 'SCORE_THRESH'))
                if _get(cfg, 'OUTPUT_RAW_SCORE', False):
                    selected_scores = torch.max(src_cls_preds, dim=-1)[0][selected]
                final_scores, final_labels, final_boxes = selected_scores, label_preds[selected], box_preds[selected]
            recall_dict = self.generate_recall_record(
                box_preds=final_boxes if 'rois' not in batch_dict else src_box_preds, recall_dict=recall_dict,
                batch_index=index, data_dict=batch_dict, thresh_list=_get(cfg, 'RECALL_THRESH_LIST'))
            pred_dicts.append({'pred_boxes': final_boxes, 'pred_scores': final_scores, 'pred_labels': final_labels})
        return pred_dicts, recall_dict

    @staticmethod
    def generate_recall_record(box_preds, recall_dict, batch_index, data_dict=None, thresh_list=None):
        """ref :265-300: counts of gt boxes ('gt') and of gt boxes whose best 3-D IoU with a kept box exceeds each
        threshold ('rcnn_<t>'; 'roi_<t>' for the rois, when batch_dict holds any), accumulated over the samples.
        Trailing gt rows whose sum is 0 are padding."""
        if 'gt_boxes' not in data_dict:
            return recall_dict
        rois = data_dict['rois'][batch_index] if 'rois' in data_dict else None
        gt_boxes = data_dict['gt_boxes'][batch_index]
        if len(recall_dict) == 0:
            recall_dict = {'gt': 0}
            for cur_thresh in thresh_list:
                recall_dict['roi_%s' % (str(cur_thresh))] = 0
                recall_dict['rcnn_%s' % (str(cur_thresh))] = 0
        cur_gt = gt_boxes
        k = cur_gt.__len__() - 1
        while k >= 0 and cur_gt[k].sum() == 0:
            k -= 1
        cur_gt = cur_gt[:k + 1]
        if cur_gt.shape[0] > 0:
            if box_preds.shape[0] > 0:
                iou3d_rcnn = iou3d_nms_utils.boxes_iou3d_gpu(box_preds[:, 0:7], cur_gt[:, 0:7])
            else:
                iou3d_rcnn = torch.zeros((0, cur_gt.shape[0]))
            if rois is not None:
                iou3d_roi = iou3d_nms_utils.boxes_iou3d_gpu(rois[:, 0:7], cur_gt[:, 0:7])
            for cur_thresh in thresh_list:
                if iou3d_rcnn.shape[0] > 0:
                    recall_dict['rcnn_%s' % str(cur_thresh)] += (iou3d_rcnn.max(dim=0)[0] > cur_thresh).sum().item()
                if rois is not None:
                    recall_dict['roi_%s' % str(cur_thresh)] += (iou3d_roi.max(dim=0)[0] > cur_thresh).sum().item()
            recall_dict['gt'] += cur_gt.shape[0]
        return recall_dict

    def load_params_from_state_dict(self, model_state_disk, strict=True):
        """Copy every entry whose key and shape match (ref :330-359, without the spconv weight re-layout).  As in the
        reference (:354-358): strict=True loads ONLY the matching entries, strictly — a checkpoint that lacks a
        parameter of this model (or holds it with another shape) raises; strict=False keeps this model's own values
        for those.  Returns the keys that were not taken from the checkpoint."""
        state = self.state_dict()
        update = {k: v for k, v in model_state_disk.items() if k in state and state[k].shape == v.shape}
        if strict:
            self.load_state_dict(update)
        else:
            state.update(update)
            self.load_state_dict(state)
        return [k for k in state if k not in update]

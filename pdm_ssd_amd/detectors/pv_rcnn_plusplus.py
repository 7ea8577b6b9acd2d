"""PVRCNNPlusPlus: PV-RCNN with the proposals made BEFORE the keypoints, so that the voxel set abstraction (VoxelSetAbstractionSPC)
samples and gathers around them: the forward of the reference's pcdet/models/detectors/pv_rcnn_plusplus.py on this repository's
template, in eval mode: vfe -> backbone_3d -> map_to_bev -> backbone_2d -> dense_head -> roi_head.proposal_layer(TEST) -> pfe ->
point_head -> roi_head -> post_processing (the template's).  The head's own proposal_layer call then finds the rois in place and
returns.  Training raises NotImplementedError, as for PVRCNN.
"""
from ..config import cfg_get as _get
from .detector3d_template import Detector3DTemplate


class PVRCNNPlusPlus(Detector3DTemplate):
    def __init__(self, model_cfg, num_class, dataset):
        super().__init__(model_cfg=model_cfg, num_class=num_class, dataset=dataset)
        self.module_list = self.build_networks()

    def forward(self, batch_dict):
        """eval: (pred_dicts, recall_dict)"""
        if self.training:
            raise NotImplementedError('PVRCNNPlusPlus runs in eval mode only: the training half of the keypoint path (proposal and '
                                      'point targets, the gradients of the keypoint operators) is not built')
        batch_dict = self.vfe(batch_dict)
        batch_dict = self.backbone_3d(batch_dict)
        batch_dict = self.map_to_bev_module(batch_dict)
        batch_dict = self.backbone_2d(batch_dict)
        batch_dict = self.dense_head(batch_dict)
        batch_dict = self.roi_head.proposal_layer(batch_dict, nms_config=_get(self.roi_head.model_cfg, 'NMS_CONFIG')['TEST'])
        batch_dict = self.pfe(batch_dict)
        batch_dict = self.point_head(batch_dict)
        batch_dict = self.roi_head(batch_dict)
        return self.post_processing(batch_dict)

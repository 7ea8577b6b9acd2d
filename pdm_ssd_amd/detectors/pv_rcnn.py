"""PVRCNN: SECOND's front, the voxel set abstraction on its levels and its BEV map (pfe), the 2-D backbone and anchor head, the
keypoint segmentation head and PVRCNNHead: the forward of the reference's pcdet/models/detectors/pv_rcnn.py on this repository's
template, in eval mode; post_processing is the template's.  Training raises NotImplementedError: proposal targets for this head,
point targets and the gradients of the two keypoint operators are not built.
"""
from .detector3d_template import Detector3DTemplate


class PVRCNN(Detector3DTemplate):
    def __init__(self, model_cfg, num_class, dataset):
        super().__init__(model_cfg=model_cfg, num_class=num_class, dataset=dataset)
        self.module_list = self.build_networks()

    def forward(self, batch_dict):
        """eval: (pred_dicts, recall_dict)"""
        if self.training:
            raise NotImplementedError('PVRCNN runs in eval mode only: the training half of the keypoint path (proposal and point '
                                      'targets, the gradients of pdm_bev_interpolate and of the RoI-grid pooling) is not built')
        for cur_module in self.module_list:
            batch_dict = cur_module(batch_dict)
        return self.post_processing(batch_dict)

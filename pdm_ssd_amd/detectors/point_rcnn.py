"""PointRCNN: PointNet2MSG backbone -> PointHeadBox (proposals) -> PointRCNNHead (refinement), the forward loop of
/root/reference/pcdet/models/detectors/point_rcnn.py:9-30.  Eval mode only: the RoI head's training half (proposal
targets, rcnn losses) is not built, and it says so when called in training mode.
"""
from .detector3d_template import Detector3DTemplate


class PointRCNN(Detector3DTemplate):
    def __init__(self, model_cfg, num_class, dataset):
        super().__init__(model_cfg=model_cfg, num_class=num_class, dataset=dataset)
        self.module_list = self.build_networks()

    def forward(self, batch_dict):
        """eval: (pred_dicts, recall_dict) of post_processing over the RoI head's refined boxes"""
        if self.training:
            raise NotImplementedError('PointRCNN training: ProposalTargetLayer and the rcnn losses are not built')
        for module in self.module_list:
            batch_dict = module(batch_dict)
        return self.post_processing(batch_dict)

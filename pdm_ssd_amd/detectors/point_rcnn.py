"""PointRCNN: PointNet2MSG backbone -> PointHeadBox (proposals) -> PointRCNNHead (refinement), the forward loop and
get_training_loss of /root/reference/pcdet/models/detectors/point_rcnn.py:9-30.  Training needs a RoI head with a
training half (POINT_RCNN_TRAIN_CFG); one built from POINT_RCNN_CFG says so when called in training mode.
"""
from .detector3d_template import Detector3DTemplate


class PointRCNN(Detector3DTemplate):
    def __init__(self, model_cfg, num_class, dataset):
        super().__init__(model_cfg=model_cfg, num_class=num_class, dataset=dataset)
        self.module_list = self.build_networks()

    def forward(self, batch_dict):
        """eval: (pred_dicts, recall_dict) of post_processing over the RoI head's refined boxes;
        training: ({'loss': loss}, tb_dict, disp_dict), tb_dict holding detached 0-dim tensors (no host read)"""
        if self.training and not self.roi_head.has_training_half:
            self.roi_head._require_training_half('PointRCNN')
        for module in self.module_list:
            batch_dict = module(batch_dict)
        if self.training:
            loss, tb_dict, disp_dict = self.get_training_loss()
            return {'loss': loss}, tb_dict, disp_dict
        return self.post_processing(batch_dict)

    def get_training_loss(self):
        disp_dict = {}
        loss_point, tb_dict = self.point_head.get_loss()
        loss_rcnn, tb_dict = self.roi_head.get_loss(tb_dict)
        return loss_point + loss_rcnn, tb_dict, disp_dict

"""VoxelRCNN: SECOND's front (dynamic mean VFE -> sparse 3-D backbone -> height compression -> 2-D backbone -> anchor head) and
VoxelRCNNHead on the backbone's multi-scale levels: the forward and get_training_loss of the reference's
pcdet/models/detectors/voxel_rcnn.py on this repository's template; post_processing is the template's.
"""
from .detector3d_template import Detector3DTemplate


class VoxelRCNN(Detector3DTemplate):
    def __init__(self, model_cfg, num_class, dataset):
        super().__init__(model_cfg=model_cfg, num_class=num_class, dataset=dataset)
        self.module_list = self.build_networks()

    def forward(self, batch_dict):
        """eval: (pred_dicts, recall_dict); training: ({'loss': loss}, tb_dict, disp_dict)"""
        from .. import fused_bn
        with fused_bn.counter_scope():      # the BatchNorm step counters of every stack: one multi-tensor add
            for cur_module in self.module_list:
                batch_dict = cur_module(batch_dict)
        if self.training:
            loss, tb_dict, disp_dict = self.get_training_loss()
            return {'loss': loss}, tb_dict, disp_dict
        return self.post_processing(batch_dict)

    def get_training_loss(self):
        disp_dict = {}
        loss_rpn, tb_dict = self.dense_head.get_loss()
        loss_rcnn, tb_dict = self.roi_head.get_loss(tb_dict)
        loss = loss_rpn + loss_rcnn
        if hasattr(self.backbone_3d, 'get_loss'):
            loss_backbone3d, tb_dict = self.backbone_3d.get_loss(tb_dict)
            loss = loss + loss_backbone3d
        return loss, tb_dict, disp_dict

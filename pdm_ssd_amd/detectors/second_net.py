"""SECONDNet: dynamic mean VFE -> sparse 3-D backbone -> height compression -> 2-D backbone -> anchor head, the forward and
get_training_loss of the reference's pcdet/models/detectors/second_net.py on this repository's template; post_processing is
the template's.  The voxel backbone trains through the sparse convolution's autograd node (spconv/__init__.py).
"""
from .detector3d_template import Detector3DTemplate


class SECONDNet(Detector3DTemplate):
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
        tb_dict = {'loss_rpn': loss_rpn.detach(), **tb_dict}
        return loss_rpn, tb_dict, disp_dict

"""CenterPoint: backbone -> BEV neck -> CenterHead, the forward, get_training_loss and post_processing of the
reference's pcdet/models/detectors/centerpoint.py on this repository's template.  The head has already decoded and
suppressed its boxes (final_box_dicts); post_processing only adds the recall record.
"""
from .detector3d_template import Detector3DTemplate, _get


class CenterPoint(Detector3DTemplate):
    def __init__(self, model_cfg, num_class, dataset):
        super().__init__(model_cfg=model_cfg, num_class=num_class, dataset=dataset)
        self.module_list = self.build_networks()

    def forward(self, batch_dict):
        """eval: (pred_dicts, recall_dict); training: ({'loss': loss}, tb_dict, disp_dict), tb_dict holding detached
        0-dim tensors (no host read)"""
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

    def post_processing(self, batch_dict):
        thresh_list = _get(_get(self.model_cfg, 'POST_PROCESSING'), 'RECALL_THRESH_LIST')
        final_pred_dict = batch_dict['final_box_dicts']
        recall_dict = {}
        for index in range(batch_dict['batch_size']):
            recall_dict = self.generate_recall_record(box_preds=final_pred_dict[index]['pred_boxes'], recall_dict=recall_dict,
                                                      batch_index=index, data_dict=batch_dict, thresh_list=thresh_list)
        return final_pred_dict, recall_dict

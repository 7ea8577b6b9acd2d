"""TransFusion (LiDAR branch): voxel backbone -> BEV neck -> TransFusionHead, the forward, get_training_loss and
post_processing of the reference's pcdet/models/detectors/transfusion.py on this repository's template.  The head has
already decoded its boxes (final_box_dicts; a transformer head needs no NMS); post_processing only adds the recall record.
Training needs a head built with TARGET_ASSIGNER_CONFIG.ASSIGN_ON_DEVICE (detector_config.TRANSFUSION_LIDAR_TRAIN_CFG);
without it the head refuses training mode (dense_heads/transfusion_head.py).  The training forward reads nothing back to
the host: the loss and every entry of tb_dict are tensors on the device.
"""
from .detector3d_template import Detector3DTemplate, _get


class TransFusion(Detector3DTemplate):
    def __init__(self, model_cfg, num_class, dataset):
        super().__init__(model_cfg=model_cfg, num_class=num_class, dataset=dataset)
        self.module_list = self.build_networks()

    def forward(self, batch_dict):
        """eval: (pred_dicts, recall_dict); training: ({'loss': loss}, tb_dict, disp_dict)"""
        for cur_module in self.module_list:
            batch_dict = cur_module(batch_dict)
        if self.training:       # (a head without the training half has raised already)
            loss, tb_dict, disp_dict = self.get_training_loss(batch_dict)
            return {'loss': loss}, tb_dict, disp_dict
        return self.post_processing(batch_dict)

    def get_training_loss(self, batch_dict):
        loss_trans, tb_dict = batch_dict['loss'], batch_dict['tb_dict']
        tb_dict = {'loss_trans': loss_trans.detach(), **tb_dict}
        return loss_trans, tb_dict, {}

    def post_processing(self, batch_dict):
        thresh_list = _get(_get(self.model_cfg, 'POST_PROCESSING'), 'RECALL_THRESH_LIST')
        final_pred_dict = batch_dict['final_box_dicts']
        recall_dict = {}
        for index in range(batch_dict['batch_size']):
            recall_dict = self.generate_recall_record(box_preds=final_pred_dict[index]['pred_boxes'], recall_dict=recall_dict,
                                                      batch_index=index, data_dict=batch_dict, thresh_list=thresh_list)
        return final_pred_dict, recall_dict

"""TransFusion (LiDAR branch): voxel backbone -> BEV neck -> TransFusionHead, the forward and post_processing of the
reference's pcdet/models/detectors/transfusion.py on this repository's template.  The head has already decoded its boxes
(final_box_dicts; a transformer head needs no NMS); post_processing only adds the recall record.  Eval mode only: the head
has no training half yet (dense_heads/transfusion_head.py).
"""
from .detector3d_template import Detector3DTemplate, _get


class TransFusion(Detector3DTemplate):
    def __init__(self, model_cfg, num_class, dataset):
        super().__init__(model_cfg=model_cfg, num_class=num_class, dataset=dataset)
        self.module_list = self.build_networks()

    def forward(self, batch_dict):
        """eval: (pred_dicts, recall_dict)"""
        for cur_module in self.module_list:
            batch_dict = cur_module(batch_dict)
        if self.training:       # (the head has raised already)
            raise NotImplementedError('TransFusion runs in eval mode only')
        return self.post_processing(batch_dict)

    def post_processing(self, batch_dict):
        thresh_list = _get(_get(self.model_cfg, 'POST_PROCESSING'), 'RECALL_THRESH_LIST')
        final_pred_dict = batch_dict['final_box_dicts']
        recall_dict = {}
        for index in range(batch_dict['batch_size']):
            recall_dict = self.generate_recall_record(box_preds=final_pred_dict[index]['pred_boxes'], recall_dict=recall_dict,
                                                      batch_index=index, data_dict=batch_dict, thresh_list=thresh_list)
        return final_pred_dict, recall_dict

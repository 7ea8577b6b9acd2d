"""PartA2Net: DynamicMeanVFE -> UNetV2 -> HeightCompression -> BaseBEVBackbone -> AnchorHeadSingle -> PointIntraPartOffsetHead ->
PartA2FCHead: the forward of the reference's pcdet/models/detectors/PartA2_net.py on this repository's template, in eval mode;
post_processing is the template's.  Training raises NotImplementedError.
"""
from .detector3d_template import Detector3DTemplate


class PartA2Net(Detector3DTemplate):
    def __init__(self, model_cfg, num_class, dataset):
        super().__init__(model_cfg=model_cfg, num_class=num_class, dataset=dataset)
        self.module_list = self.build_networks()

    def forward(self, batch_dict):
        """eval: (pred_dicts, recall_dict)"""
        if self.training:
            raise NotImplementedError('PartA2Net runs in eval mode only: the point part targets and losses, proposal targets for '
                                      'PartA2FCHead, and the gradients of the inverse sparse convolution, of pdm_roiaware_pool_sparse '
                                      'and of pdm_sparse_fc are not built')
        for cur_module in self.module_list:
            batch_dict = cur_module(batch_dict)
        return self.post_processing(batch_dict)

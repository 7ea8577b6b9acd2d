"""HeightCompression of the reference's pcdet/models/backbones_2d/map_to_bev/height_compression.py: the encoded sparse tensor's
dense canvas (B, C, D, H, W), written in one launch, viewed as the BEV map (B, C D, H, W).  No host read."""
import torch.nn as nn

from ...config import cfg_get as _get


class HeightCompression(nn.Module):
    def __init__(self, model_cfg, **kwargs):
        super().__init__()
        self.model_cfg = model_cfg
        self.num_bev_features = _get(model_cfg, 'NUM_BEV_FEATURES')

    def forward(self, batch_dict):
        spatial_features = batch_dict['encoded_spconv_tensor'].dense()
        N, C, D, H, W = spatial_features.shape
        batch_dict['spatial_features'] = spatial_features.view(N, C * D, H, W)
        batch_dict['spatial_features_stride'] = batch_dict['encoded_spconv_tensor_stride']
        return batch_dict

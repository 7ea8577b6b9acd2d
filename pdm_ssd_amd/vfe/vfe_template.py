"""The reference's pcdet/models/backbones_3d/vfe/vfe_template.py, restated."""
import torch.nn as nn


class VFETemplate(nn.Module):
    def __init__(self, model_cfg, **kwargs):
        super().__init__()
        self.model_cfg = model_cfg

    def get_output_feature_dim(self):
        raise NotImplementedError

    def forward(self, **kwargs):
        """-> batch_dict with voxel_features (num_voxels, C)"""
        raise NotImplementedError

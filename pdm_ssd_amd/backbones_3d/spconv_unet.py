"""UNetV2 of the reference's pcdet/models/backbones_3d/spconv_unet.py (Part-A2's sparse UNet) on this package's spconv stand-in:
same constructor signature, config keys (RETURN_ENCODED_TENSOR, last_pad), module names and state_dict keys, and batch_dict
outputs: encoded_spconv_tensor (stride 8) for the detection head, point_features (P, 16) and point_coords (P, 4) rows
(b, x, y, z) at the voxel centres for the point head, in the input voxels' row order.

The encoder is VoxelBackBone8x's; the decoder walks back up: per level a SparseBasicBlock on the lateral tensor, cat with the
tensor from below, a submanifold block, a channel reduction added back (plain torch on the features), then the INVERSE of the
level's strided convolution (spconv.SparseInverseConv3d over the rulebook that convolution stored under its indice_key), which
lands on the level above's own rows.  In eval mode without grad every conv -> BatchNorm1d -> ReLU run is one launch.  The
inverse convolutions have no gradients yet, so training mode raises NotImplementedError there.
"""
from functools import partial

import torch
import torch.nn as nn

from .. import spconv
from ..config import cfg_get as _get
from ..utils import common_utils
from .spconv_backbone import SparseBasicBlock, post_act_block


class UNetV2(nn.Module):
    def __init__(self, model_cfg, input_channels, grid_size, voxel_size, point_cloud_range, **kwargs):
        super().__init__()
        self.model_cfg = model_cfg
        self.sparse_shape = [int(v) for v in list(grid_size)[::-1]]
        self.sparse_shape[0] += 1       # grid_size[::-1] + [1, 0, 0]
        self.voxel_size = voxel_size
        self.point_cloud_range = point_cloud_range
        norm_fn = partial(nn.BatchNorm1d, eps=1e-3, momentum=0.01)
        self.conv_input = spconv.SparseSequential(
            spconv.SubMConv3d(input_channels, 16, 3, padding=1, bias=False, indice_key='subm1'), norm_fn(16), nn.ReLU())
        block = post_act_block
        self.conv1 = spconv.SparseSequential(block(16, 16, 3, norm_fn=norm_fn, padding=1, indice_key='subm1'))
        self.conv2 = spconv.SparseSequential(      # [1600, 1408, 41] -> [800, 704, 21]
            block(16, 32, 3, norm_fn=norm_fn, stride=2, padding=1, indice_key='spconv2', conv_type='spconv'),
            block(32, 32, 3, norm_fn=norm_fn, padding=1, indice_key='subm2'),
            block(32, 32, 3, norm_fn=norm_fn, padding=1, indice_key='subm2'))
        self.conv3 = spconv.SparseSequential(      # [800, 704, 21] -> [400, 352, 11]
            block(32, 64, 3, norm_fn=norm_fn, stride=2, padding=1, indice_key='spconv3', conv_type='spconv'),
            block(64, 64, 3, norm_fn=norm_fn, padding=1, indice_key='subm3'),
            block(64, 64, 3, norm_fn=norm_fn, padding=1, indice_key='subm3'))
        self.conv4 = spconv.SparseSequential(      # [400, 352, 11] -> [200, 176, 5]
            block(64, 64, 3, norm_fn=norm_fn, stride=2, padding=(0, 1, 1), indice_key='spconv4', conv_type='spconv'),
            block(64, 64, 3, norm_fn=norm_fn, padding=1, indice_key='subm4'),
            block(64, 64, 3, norm_fn=norm_fn, padding=1, indice_key='subm4'))
        if _get(model_cfg, 'RETURN_ENCODED_TENSOR', True):
            last_pad = _get(model_cfg, 'last_pad', 0)
            self.conv_out = spconv.SparseSequential(   # [200, 176, 5] -> [200, 176, 2]
                spconv.SparseConv3d(64, 128, (3, 1, 1), stride=(2, 1, 1), padding=last_pad, bias=False, indice_key='spconv_down2'),
                norm_fn(128), nn.ReLU())
        else:
            self.conv_out = None
        # decoder
        self.conv_up_t4 = SparseBasicBlock(64, 64, bias=False, indice_key='subm4', norm_fn=norm_fn)
        self.conv_up_m4 = block(128, 64, 3, norm_fn=norm_fn, padding=1, indice_key='subm4')
        self.inv_conv4 = block(64, 64, 3, norm_fn=norm_fn, indice_key='spconv4', conv_type='inverseconv')
        self.conv_up_t3 = SparseBasicBlock(64, 64, bias=False, indice_key='subm3', norm_fn=norm_fn)
        self.conv_up_m3 = block(128, 64, 3, norm_fn=norm_fn, padding=1, indice_key='subm3')
        self.inv_conv3 = block(64, 32, 3, norm_fn=norm_fn, indice_key='spconv3', conv_type='inverseconv')
        self.conv_up_t2 = SparseBasicBlock(32, 32, bias=False, indice_key='subm2', norm_fn=norm_fn)
        self.conv_up_m2 = block(64, 32, 3, norm_fn=norm_fn, indice_key='subm2')
        self.inv_conv2 = block(32, 16, 3, norm_fn=norm_fn, indice_key='spconv2', conv_type='inverseconv')
        self.conv_up_t1 = SparseBasicBlock(16, 16, bias=False, indice_key='subm1', norm_fn=norm_fn)
        self.conv_up_m1 = block(32, 16, 3, norm_fn=norm_fn, indice_key='subm1')
        self.conv5 = spconv.SparseSequential(block(16, 16, 3, norm_fn=norm_fn, padding=1, indice_key='subm1'))
        self.num_point_features = 16
        self.backbone_channels = {'x_conv1': 16, 'x_conv2': 32, 'x_conv3': 64, 'x_conv4': 64}

    def UR_block_forward(self, x_lateral, x_bottom, conv_t, conv_m, conv_inv):
        x_trans = conv_t(x_lateral)
        x = x_trans.replace_feature(torch.cat((x_bottom.features, x_trans.features), dim=1))
        x_m = conv_m(x)
        x = self.channel_reduction(x, x_m.features.shape[1])
        x = x.replace_feature(x_m.features + x.features)
        return conv_inv(x)

    @staticmethod
    def channel_reduction(x, out_channels):
        """features (N, C1) -> (N, C2), C1 a multiple of C2: the sum of each run of C1 / C2 consecutive channels"""
        features = x.features
        n, in_channels = features.shape
        assert in_channels % out_channels == 0 and in_channels >= out_channels
        return x.replace_feature(features.view(n, out_channels, -1).sum(dim=2))

    def forward(self, batch_dict):
        input_sp_tensor = spconv.SparseConvTensor(features=batch_dict['voxel_features'], indices=batch_dict['voxel_coords'].int(),
                                                  spatial_shape=self.sparse_shape, batch_size=batch_dict['batch_size'])
        x = self.conv_input(input_sp_tensor)
        x_conv1 = self.conv1(x)
        x_conv2 = self.conv2(x_conv1)
        x_conv3 = self.conv3(x_conv2)
        x_conv4 = self.conv4(x_conv3)
        if self.conv_out is not None:       # for the detection head: [200, 176, 5] -> [200, 176, 2]
            batch_dict['encoded_spconv_tensor'] = self.conv_out(x_conv4)
            batch_dict['encoded_spconv_tensor_stride'] = 8
        # for the segmentation head
        x_up4 = self.UR_block_forward(x_conv4, x_conv4, self.conv_up_t4, self.conv_up_m4, self.inv_conv4)
        x_up3 = self.UR_block_forward(x_conv3, x_up4, self.conv_up_t3, self.conv_up_m3, self.inv_conv3)
        x_up2 = self.UR_block_forward(x_conv2, x_up3, self.conv_up_t2, self.conv_up_m2, self.inv_conv2)
        x_up1 = self.UR_block_forward(x_conv1, x_up2, self.conv_up_t1, self.conv_up_m1, self.conv5)
        batch_dict['point_features'] = x_up1.features
        centres = common_utils.get_voxel_centers(x_up1.indices[:, 1:], downsample_times=1, voxel_size=self.voxel_size,
                                                 point_cloud_range=self.point_cloud_range)
        batch_dict['point_coords'] = torch.cat((x_up1.indices[:, 0:1].float(), centres), dim=1)
        return batch_dict

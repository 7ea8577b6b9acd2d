"""PillarBackBone8x and PillarRes18BackBone8x of the reference's pcdet/models/backbones_3d/spconv_backbone_2d.py on this package's
spconv stand-in: the sparse 2-D pillar backbones of PillarNet.  Same constructor signatures, state_dict keys and batch_dict outputs
(multi_scale_2d_features, multi_scale_2d_strides) as the reference's; backbone_channels is published to the template.

conv1 to conv4 are sparse 2-D layers (spconv.SubMConv2d / SparseConv2d: the 3-D operators on a depth-1 grid through the wide
entries, since conv4 is 128 -> 256 and 256 -> 256); conv5 is dense torch on x_conv4.dense().  In eval mode without grad every
conv -> BatchNorm1d -> ReLU run is one launch and a SparseBasicBlock two; in training each convolution is an autograd node
(spconv/__init__.py).  The three strided sparse convolutions each read their output-site count on the host: three host reads per
forward.  As in the reference, multi_scale_2d_features['x_conv4'] is the DENSE (B, 256, H / 8, W / 8) map; the sparse tensor it
came from is left under 'encoded_spconv_tensor' (stride 8), which the reference does not publish.
SparseInverseConv2d is not built: conv_type='inverseconv' raises NotImplementedError.
"""
from functools import partial

import torch.nn as nn

from .. import spconv


def post_act_block(in_channels, out_channels, kernel_size, indice_key=None, stride=1, padding=0, conv_type='subm', norm_fn=None):
    if conv_type == 'subm':
        conv = spconv.SubMConv2d(in_channels, out_channels, kernel_size, bias=False, indice_key=indice_key)
    elif conv_type == 'spconv':
        conv = spconv.SparseConv2d(in_channels, out_channels, kernel_size, stride=stride, padding=padding, bias=False, indice_key=indice_key)
    elif conv_type == 'inverseconv':
        raise NotImplementedError('SparseInverseConv2d is not built (conv_type inverseconv)')
    else:
        raise NotImplementedError(conv_type)
    return spconv.SparseSequential(conv, norm_fn(out_channels), nn.ReLU())


def post_act_block_dense(in_channels, out_channels, kernel_size, stride=1, padding=0, dilation=1, norm_fn=None):
    return nn.Sequential(nn.Conv2d(in_channels, out_channels, kernel_size, stride, padding=padding, dilation=dilation, bias=False),
                         norm_fn(out_channels), nn.ReLU())


class SparseBasicBlock(spconv.SparseModule):
    expansion = 1

    def __init__(self, inplanes, planes, stride=1, norm_fn=None, downsample=None, indice_key=None):
        super().__init__()
        assert norm_fn is not None
        bias = norm_fn is not None
        self.conv1 = spconv.SubMConv2d(inplanes, planes, kernel_size=3, stride=stride, padding=1, bias=bias, indice_key=indice_key)
        self.bn1 = norm_fn(planes)
        self.relu = nn.ReLU()
        self.conv2 = spconv.SubMConv2d(planes, planes, kernel_size=3, stride=stride, padding=1, bias=bias, indice_key=indice_key)
        self.bn2 = norm_fn(planes)
        self.downsample = downsample
        self.stride = stride

    def forward(self, x):
        """conv1 + bn1 + relu, then conv2 + bn2 + identity + relu: two launches in eval mode without grad"""
        identity = x if self.downsample is None else self.downsample(x)
        out = self.conv1(x, norm=self.bn1, relu=True)
        return self.conv2(out, norm=self.bn2, relu=True, residual=identity.features)


class BasicBlock(nn.Module):
    expansion = 1

    def __init__(self, inplanes, planes, stride=1, norm_fn=None, downsample=None):
        super().__init__()
        assert norm_fn is not None
        bias = norm_fn is not None
        self.conv1 = nn.Conv2d(inplanes, planes, 3, stride=stride, padding=1, bias=bias)
        self.bn1 = norm_fn(planes)
        self.relu = nn.ReLU()
        self.conv2 = nn.Conv2d(planes, planes, 3, stride=stride, padding=1, bias=bias)
        self.bn2 = norm_fn(planes)
        self.downsample = downsample
        self.stride = stride

    def forward(self, x):
        identity = x if self.downsample is None else self.downsample(x)
        out = self.relu(self.bn1(self.conv1(x)))
        out = self.bn2(self.conv2(out))
        return self.relu(out + identity)


class _PillarBackBone(nn.Module):
    """what the two backbones share: the input tensor, the level walk and the batch_dict outputs"""

    def _init_common(self, model_cfg, grid_size):
        self.model_cfg = model_cfg
        self.sparse_shape = [int(grid_size[1]), int(grid_size[0])]      # grid_size[[1, 0]]: (H, W) = (ny, nx)
        self.num_point_features = 256
        self.backbone_channels = {'x_conv1': 32, 'x_conv2': 64, 'x_conv3': 128, 'x_conv4': 256, 'x_conv5': 256}

    def forward(self, batch_dict):
        """pillar_features (P, 32), pillar_coords (P, 3) (b, y, x), batch_size -> multi_scale_2d_features: x_conv1 to x_conv3
        sparse, x_conv4 and x_conv5 dense"""
        input_sp_tensor = spconv.SparseConvTensor(features=batch_dict['pillar_features'], indices=batch_dict['pillar_coords'].int(),
                                                  spatial_shape=self.sparse_shape, batch_size=batch_dict['batch_size'])
        x_conv1 = self.conv1(input_sp_tensor)
        x_conv2 = self.conv2(x_conv1)
        x_conv3 = self.conv3(x_conv2)
        x_conv4_sparse = self.conv4(x_conv3)
        x_conv4 = x_conv4_sparse.dense()
        x_conv5 = self.conv5(x_conv4)
        batch_dict.update({'encoded_spconv_tensor': x_conv4_sparse, 'encoded_spconv_tensor_stride': 8})
        batch_dict.update({'multi_scale_2d_features': {'x_conv1': x_conv1, 'x_conv2': x_conv2, 'x_conv3': x_conv3, 'x_conv4': x_conv4,
                                                       'x_conv5': x_conv5}})
        batch_dict.update({'multi_scale_2d_strides': {'x_conv1': 1, 'x_conv2': 2, 'x_conv3': 4, 'x_conv4': 8, 'x_conv5': 16}})
        return batch_dict


class PillarBackBone8x(_PillarBackBone):
    def __init__(self, model_cfg, input_channels, grid_size, **kwargs):
        super().__init__()
        self._init_common(model_cfg, grid_size)
        norm_fn = partial(nn.BatchNorm1d, eps=1e-3, momentum=0.01)
        block = post_act_block
        dense_block = post_act_block_dense
        self.conv1 = spconv.SparseSequential(
            block(32, 32, 3, norm_fn=norm_fn, padding=1, indice_key='subm1'),
            block(32, 32, 3, norm_fn=norm_fn, padding=1, indice_key='subm1'))
        self.conv2 = spconv.SparseSequential(      # [1600, 1408] -> [800, 704]
            block(32, 64, 3, norm_fn=norm_fn, stride=2, padding=1, indice_key='spconv2', conv_type='spconv'),
            block(64, 64, 3, norm_fn=norm_fn, padding=1, indice_key='subm2'),
            block(64, 64, 3, norm_fn=norm_fn, padding=1, indice_key='subm2'))
        self.conv3 = spconv.SparseSequential(      # [800, 704] -> [400, 352]
            block(64, 128, 3, norm_fn=norm_fn, stride=2, padding=1, indice_key='spconv3', conv_type='spconv'),
            block(128, 128, 3, norm_fn=norm_fn, padding=1, indice_key='subm3'),
            block(128, 128, 3, norm_fn=norm_fn, padding=1, indice_key='subm3'))
        self.conv4 = spconv.SparseSequential(      # [400, 352] -> [200, 176]
            block(128, 256, 3, norm_fn=norm_fn, stride=2, padding=1, indice_key='spconv4', conv_type='spconv'),
            block(256, 256, 3, norm_fn=norm_fn, padding=1, indice_key='subm4'),
            block(256, 256, 3, norm_fn=norm_fn, padding=1, indice_key='subm4'))
        norm_fn = partial(nn.BatchNorm2d, eps=1e-3, momentum=0.01)
        self.conv5 = nn.Sequential(                # [200, 176] -> [100, 88]
            dense_block(256, 256, 3, norm_fn=norm_fn, stride=2, padding=1),
            dense_block(256, 256, 3, norm_fn=norm_fn, padding=1),
            dense_block(256, 256, 3, norm_fn=norm_fn, padding=1))


class PillarRes18BackBone8x(_PillarBackBone):
    def __init__(self, model_cfg, input_channels, grid_size, **kwargs):
        super().__init__()
        self._init_common(model_cfg, grid_size)
        norm_fn = partial(nn.BatchNorm1d, eps=1e-3, momentum=0.01)
        block = post_act_block
        dense_block = post_act_block_dense
        self.conv1 = spconv.SparseSequential(
            SparseBasicBlock(32, 32, norm_fn=norm_fn, indice_key='res1'),
            SparseBasicBlock(32, 32, norm_fn=norm_fn, indice_key='res1'))
        self.conv2 = spconv.SparseSequential(
            block(32, 64, 3, norm_fn=norm_fn, stride=2, padding=1, indice_key='spconv2', conv_type='spconv'),
            SparseBasicBlock(64, 64, norm_fn=norm_fn, indice_key='res2'),
            SparseBasicBlock(64, 64, norm_fn=norm_fn, indice_key='res2'))
        self.conv3 = spconv.SparseSequential(
            block(64, 128, 3, norm_fn=norm_fn, stride=2, padding=1, indice_key='spconv3', conv_type='spconv'),
            SparseBasicBlock(128, 128, norm_fn=norm_fn, indice_key='res3'),
            SparseBasicBlock(128, 128, norm_fn=norm_fn, indice_key='res3'))
        self.conv4 = spconv.SparseSequential(
            block(128, 256, 3, norm_fn=norm_fn, stride=2, padding=1, indice_key='spconv4', conv_type='spconv'),
            SparseBasicBlock(256, 256, norm_fn=norm_fn, indice_key='res4'),
            SparseBasicBlock(256, 256, norm_fn=norm_fn, indice_key='res4'))
        norm_fn = partial(nn.BatchNorm2d, eps=1e-3, momentum=0.01)
        self.conv5 = nn.Sequential(
            dense_block(256, 256, 3, norm_fn=norm_fn, stride=2, padding=1),
            BasicBlock(256, 256, norm_fn=norm_fn),
            BasicBlock(256, 256, norm_fn=norm_fn))

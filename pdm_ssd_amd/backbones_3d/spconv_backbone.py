"""VoxelBackBone8x, VoxelResBackBone8x and SparseBasicBlock of the reference's pcdet/models/backbones_3d/spconv_backbone.py on
this package's spconv stand-in (hand-written HIP sparse convolution and its gradients): same constructor signatures, config keys
(last_pad, USE_BIAS), state_dict keys and batch_dict outputs (encoded_spconv_tensor and its stride, multi_scale_3d_features,
multi_scale_3d_strides).  In eval mode without grad every conv -> BatchNorm1d -> ReLU run is one launch; a SparseBasicBlock is
two (conv1 + bn1 + relu, conv2 + bn2 + identity + relu).  In training mode, or on features that require grad, each convolution
is an autograd node and BatchNorm1d, the residual and ReLU run in torch behind it (spconv/__init__.py).  The four strided convolutions each read their output-site count on the host: four host reads
per forward; the submanifold layers read nothing and share one rulebook per indice_key.
"""
from functools import partial

import torch.nn as nn

from .. import spconv
from ..config import cfg_get as _get


def post_act_block(in_channels, out_channels, kernel_size, indice_key=None, stride=1, padding=0, conv_type='subm', norm_fn=None):
    if conv_type == 'subm':
        conv = spconv.SubMConv3d(in_channels, out_channels, kernel_size, bias=False, indice_key=indice_key)
    elif conv_type == 'spconv':
        conv = spconv.SparseConv3d(in_channels, out_channels, kernel_size, stride=stride, padding=padding, bias=False, indice_key=indice_key)
    elif conv_type == 'inverseconv':
        conv = spconv.SparseInverseConv3d(in_channels, out_channels, kernel_size, indice_key=indice_key, bias=False)
    else:
        raise NotImplementedError(conv_type)
    return spconv.SparseSequential(conv, norm_fn(out_channels), nn.ReLU())


class SparseBasicBlock(spconv.SparseModule):
    expansion = 1

    def __init__(self, inplanes, planes, stride=1, bias=None, norm_fn=None, downsample=None, indice_key=None):
        super().__init__()
        assert norm_fn is not None
        if bias is None:
            bias = norm_fn is not None
        self.conv1 = spconv.SubMConv3d(inplanes, planes, kernel_size=3, stride=stride, padding=1, bias=bias, indice_key=indice_key)
        self.bn1 = norm_fn(planes)
        self.relu = nn.ReLU()
        self.conv2 = spconv.SubMConv3d(planes, planes, kernel_size=3, stride=stride, padding=1, bias=bias, indice_key=indice_key)
        self.bn2 = norm_fn(planes)
        self.downsample = downsample
        self.stride = stride

    def forward(self, x):
        """conv1 + bn1 + relu, then conv2 + bn2 + identity + relu: two launches in eval mode without grad, the autograd path of
        SparseConvolution.forward otherwise"""
        identity = x if self.downsample is None else self.downsample(x)
        out = self.conv1(x, norm=self.bn1, relu=True)
        return self.conv2(out, norm=self.bn2, relu=True, residual=identity.features)


class _VoxelBackBone(nn.Module):
    """what the two backbones share: the input tensor, the level walk and the batch_dict outputs"""

    def _init_common(self, model_cfg, grid_size, channels):
        self.model_cfg = model_cfg
        self.sparse_shape = [int(v) for v in list(grid_size)[::-1]]
        self.sparse_shape[0] += 1       # grid_size[::-1] + [1, 0, 0]
        self.num_point_features = 128
        self.backbone_channels = dict(zip(('x_conv1', 'x_conv2', 'x_conv3', 'x_conv4'), channels))

    def forward(self, batch_dict):
        """voxel_features (P, C), voxel_coords (P, 4) (b, z, y, x), batch_size -> encoded_spconv_tensor (stride 8) and the
        four levels' tensors"""
        input_sp_tensor = spconv.SparseConvTensor(features=batch_dict['voxel_features'], indices=batch_dict['voxel_coords'].int(),
                                                  spatial_shape=self.sparse_shape, batch_size=batch_dict['batch_size'])
        x = self.conv_input(input_sp_tensor)
        x_conv1 = self.conv1(x)
        x_conv2 = self.conv2(x_conv1)
        x_conv3 = self.conv3(x_conv2)
        x_conv4 = self.conv4(x_conv3)
        out = self.conv_out(x_conv4)        # for the detection head: [200, 176, 5] -> [200, 176, 2]
        batch_dict.update({'encoded_spconv_tensor': out, 'encoded_spconv_tensor_stride': 8})
        batch_dict.update({'multi_scale_3d_features': {'x_conv1': x_conv1, 'x_conv2': x_conv2, 'x_conv3': x_conv3, 'x_conv4': x_conv4}})
        batch_dict.update({'multi_scale_3d_strides': {'x_conv1': 1, 'x_conv2': 2, 'x_conv3': 4, 'x_conv4': 8}})
        return batch_dict


class VoxelBackBone8x(_VoxelBackBone):
    def __init__(self, model_cfg, input_channels, grid_size, **kwargs):
        super().__init__()
        self._init_common(model_cfg, grid_size, (16, 32, 64, 64))
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
        last_pad = _get(model_cfg, 'last_pad', 0)
        self.conv_out = spconv.SparseSequential(   # [200, 176, 5] -> [200, 176, 2]
            spconv.SparseConv3d(64, 128, (3, 1, 1), stride=(2, 1, 1), padding=last_pad, bias=False, indice_key='spconv_down2'),
            norm_fn(128), nn.ReLU())


class VoxelResBackBone8x(_VoxelBackBone):
    def __init__(self, model_cfg, input_channels, grid_size, **kwargs):
        super().__init__()
        self._init_common(model_cfg, grid_size, (16, 32, 64, 128))
        use_bias = _get(model_cfg, 'USE_BIAS', None)
        norm_fn = partial(nn.BatchNorm1d, eps=1e-3, momentum=0.01)
        self.conv_input = spconv.SparseSequential(
            spconv.SubMConv3d(input_channels, 16, 3, padding=1, bias=False, indice_key='subm1'), norm_fn(16), nn.ReLU())
        block = post_act_block
        self.conv1 = spconv.SparseSequential(
            SparseBasicBlock(16, 16, bias=use_bias, norm_fn=norm_fn, indice_key='res1'),
            SparseBasicBlock(16, 16, bias=use_bias, norm_fn=norm_fn, indice_key='res1'))
        self.conv2 = spconv.SparseSequential(
            block(16, 32, 3, norm_fn=norm_fn, stride=2, padding=1, indice_key='spconv2', conv_type='spconv'),
            SparseBasicBlock(32, 32, bias=use_bias, norm_fn=norm_fn, indice_key='res2'),
            SparseBasicBlock(32, 32, bias=use_bias, norm_fn=norm_fn, indice_key='res2'))
        self.conv3 = spconv.SparseSequential(
            block(32, 64, 3, norm_fn=norm_fn, stride=2, padding=1, indice_key='spconv3', conv_type='spconv'),
            SparseBasicBlock(64, 64, bias=use_bias, norm_fn=norm_fn, indice_key='res3'),
            SparseBasicBlock(64, 64, bias=use_bias, norm_fn=norm_fn, indice_key='res3'))
        self.conv4 = spconv.SparseSequential(
            block(64, 128, 3, norm_fn=norm_fn, stride=2, padding=(0, 1, 1), indice_key='spconv4', conv_type='spconv'),
            SparseBasicBlock(128, 128, bias=use_bias, norm_fn=norm_fn, indice_key='res4'),
            SparseBasicBlock(128, 128, bias=use_bias, norm_fn=norm_fn, indice_key='res4'))
        last_pad = _get(model_cfg, 'last_pad', 0)
        self.conv_out = spconv.SparseSequential(
            spconv.SparseConv3d(128, 128, (3, 1, 1), stride=(2, 1, 1), padding=last_pad, bias=False, indice_key='spconv_down2'),
            norm_fn(128), nn.ReLU())

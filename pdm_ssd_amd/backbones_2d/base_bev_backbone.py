"""BaseBEVBackbone of the reference's pcdet/models/backbones_2d/base_bev_backbone.py, restated: plain torch
convolutions (MIOpen on the GPU), the same config keys and state_dict keys (blocks.{i}.{j}.*, deblocks.{i}.{j}.*).
The reference's `np.round(1 / stride).astype(np.int)` (np.int no longer exists) is int(round(1 / stride)).

BaseBEVBackboneV1 is the 2-D backbone of the sparse pillar family (PillarNet): it reads the dense x_conv4 and x_conv5 maps a sparse
2-D backbone left in multi_scale_2d_features, not spatial_features.

BaseBEVResBackbone is the residual 2-D backbone behind DSVT: every level is a strided BasicBlock with a 1 x 1 shortcut followed
by LAYER_NUMS plain ones (keys blocks.{i}.{j}.conv1 / bn1 / conv2 / bn2 / downsample_layer.{0, 1}.*, deblocks.{i}.{0, 1}.*)."""
import torch
import torch.nn as nn

from ..config import cfg_get as _get


class BaseBEVBackbone(nn.Module):
    def __init__(self, model_cfg, input_channels):
        super().__init__()
        self.model_cfg = model_cfg
        if _get(model_cfg, 'LAYER_NUMS', None) is not None:
            layer_nums, layer_strides = list(_get(model_cfg, 'LAYER_NUMS')), list(_get(model_cfg, 'LAYER_STRIDES'))
            num_filters = list(_get(model_cfg, 'NUM_FILTERS'))
            assert len(layer_nums) == len(layer_strides) == len(num_filters)
        else:
            layer_nums = layer_strides = num_filters = []
        if _get(model_cfg, 'UPSAMPLE_STRIDES', None) is not None:
            upsample_strides, num_upsample_filters = list(_get(model_cfg, 'UPSAMPLE_STRIDES')), list(_get(model_cfg, 'NUM_UPSAMPLE_FILTERS'))
            assert len(upsample_strides) == len(num_upsample_filters)
        else:
            upsample_strides = num_upsample_filters = []
        conv_for_no_stride = _get(model_cfg, 'USE_CONV_FOR_NO_STRIDE', False)

        def bn(c):
            return nn.BatchNorm2d(c, eps=1e-3, momentum=0.01)

        num_levels = len(layer_nums)
        c_in_list = [input_channels, *num_filters[:-1]]
        self.blocks = nn.ModuleList()
        self.deblocks = nn.ModuleList()
        for idx in range(num_levels):
            # the first convolution pads with an explicit ZeroPad2d and strides (keys blocks.{idx}.1.*, .2.*)
            cur_layers = [nn.ZeroPad2d(1),
                          nn.Conv2d(c_in_list[idx], num_filters[idx], kernel_size=3, stride=layer_strides[idx], padding=0, bias=False),
                          bn(num_filters[idx]), nn.ReLU()]
            for _ in range(layer_nums[idx]):
                cur_layers.extend([nn.Conv2d(num_filters[idx], num_filters[idx], kernel_size=3, padding=1, bias=False),
                                   bn(num_filters[idx]), nn.ReLU()])
            self.blocks.append(nn.Sequential(*cur_layers))
            if len(upsample_strides) > 0:
                stride = upsample_strides[idx]
                if stride > 1 or (stride == 1 and not conv_for_no_stride):
                    up = nn.ConvTranspose2d(num_filters[idx], num_upsample_filters[idx], stride, stride=stride, bias=False)
                else:
                    stride = int(round(1 / stride))
                    up = nn.Conv2d(num_filters[idx], num_upsample_filters[idx], stride, stride=stride, bias=False)
                self.deblocks.append(nn.Sequential(up, bn(num_upsample_filters[idx]), nn.ReLU()))
        c_in = sum(num_upsample_filters)
        if len(upsample_strides) > num_levels:      # one more deblock over the concatenation
            self.deblocks.append(nn.Sequential(
                nn.ConvTranspose2d(c_in, c_in, upsample_strides[-1], stride=upsample_strides[-1], bias=False), bn(c_in), nn.ReLU()))
        self.num_bev_features = c_in

    def forward(self, data_dict):
        """spatial_features (B, C, H, W) -> spatial_features_2d, and spatial_features_{s}x per level (the reference
        collects those in a dict it then drops; here they are written to data_dict)"""
        spatial_features = data_dict['spatial_features']
        ups = []
        x = spatial_features
        for i in range(len(self.blocks)):
            x = self.blocks[i](x)
            stride = int(spatial_features.shape[2] / x.shape[2])
            data_dict['spatial_features_%dx' % stride] = x
            ups.append(self.deblocks[i](x) if len(self.deblocks) > 0 else x)
        if len(ups) > 1:
            x = torch.cat(ups, dim=1)
        elif len(ups) == 1:
            x = ups[0]
        if len(self.deblocks) > len(self.blocks):
            x = self.deblocks[-1](x)
        data_dict['spatial_features_2d'] = x
        return data_dict


class BaseBEVBackboneV1(nn.Module):
    def __init__(self, model_cfg, **kwargs):
        super().__init__()
        self.model_cfg = model_cfg
        layer_nums, num_filters = list(_get(model_cfg, 'LAYER_NUMS')), list(_get(model_cfg, 'NUM_FILTERS'))
        assert len(layer_nums) == len(num_filters) == 2
        num_upsample_filters, upsample_strides = list(_get(model_cfg, 'NUM_UPSAMPLE_FILTERS')), list(_get(model_cfg, 'UPSAMPLE_STRIDES'))
        assert len(num_upsample_filters) == len(upsample_strides)

        def bn(c):
            return nn.BatchNorm2d(c, eps=1e-3, momentum=0.01)

        num_levels = len(layer_nums)
        self.blocks = nn.ModuleList()
        self.deblocks = nn.ModuleList()
        for idx in range(num_levels):
            cur_layers = [nn.ZeroPad2d(1), nn.Conv2d(num_filters[idx], num_filters[idx], kernel_size=3, stride=1, padding=0, bias=False),
                          bn(num_filters[idx]), nn.ReLU()]
            for _ in range(layer_nums[idx]):
                cur_layers.extend([nn.Conv2d(num_filters[idx], num_filters[idx], kernel_size=3, padding=1, bias=False),
                                   bn(num_filters[idx]), nn.ReLU()])
            self.blocks.append(nn.Sequential(*cur_layers))
            if len(upsample_strides) > 0:
                stride = upsample_strides[idx]
                if stride >= 1:
                    up = nn.ConvTranspose2d(num_filters[idx], num_upsample_filters[idx], stride, stride=stride, bias=False)
                else:
                    stride = int(round(1 / stride))
                    up = nn.Conv2d(num_filters[idx], num_upsample_filters[idx], stride, stride=stride, bias=False)
                self.deblocks.append(nn.Sequential(up, bn(num_upsample_filters[idx]), nn.ReLU()))
        c_in = sum(num_upsample_filters)
        if len(upsample_strides) > num_levels:
            self.deblocks.append(nn.Sequential(
                nn.ConvTranspose2d(c_in, c_in, upsample_strides[-1], stride=upsample_strides[-1], bias=False), bn(c_in), nn.ReLU()))
        self.num_bev_features = c_in

    def forward(self, data_dict):
        """multi_scale_2d_features['x_conv4'] (B, C4, H, W) and ['x_conv5'] (B, C5, H / 2, W / 2), both dense ->
        spatial_features_2d: blocks[0] over the concatenation of deblocks[0](x_conv4) and deblocks[1](blocks[1](x_conv5))"""
        feats = data_dict['multi_scale_2d_features']
        ups = [self.deblocks[0](feats['x_conv4'])]
        ups.append(self.deblocks[1](self.blocks[1](feats['x_conv5'])))
        data_dict['spatial_features_2d'] = self.blocks[0](torch.cat(ups, dim=1))
        return data_dict


class BasicBlock(nn.Module):
    expansion = 1

    def __init__(self, inplanes, planes, stride=1, padding=1, downsample=False):
        super().__init__()
        self.conv1 = nn.Conv2d(inplanes, planes, kernel_size=3, stride=stride, padding=padding, bias=False)
        self.bn1 = nn.BatchNorm2d(planes, eps=1e-3, momentum=0.01)
        self.relu1 = nn.ReLU()
        self.conv2 = nn.Conv2d(planes, planes, kernel_size=3, padding=1, bias=False)
        self.bn2 = nn.BatchNorm2d(planes, eps=1e-3, momentum=0.01)
        self.relu2 = nn.ReLU()
        self.downsample = downsample
        if downsample:
            self.downsample_layer = nn.Sequential(nn.Conv2d(inplanes, planes, kernel_size=1, stride=stride, padding=0, bias=False),
                                                  nn.BatchNorm2d(planes, eps=1e-3, momentum=0.01))
        self.stride = stride

    def forward(self, x):
        out = self.bn2(self.conv2(self.relu1(self.bn1(self.conv1(x)))))
        return self.relu2(out + (self.downsample_layer(x) if self.downsample else x))


class BaseBEVResBackbone(nn.Module):
    def __init__(self, model_cfg, input_channels):
        super().__init__()
        self.model_cfg = model_cfg
        if _get(model_cfg, 'LAYER_NUMS', None) is not None:
            layer_nums, layer_strides = list(_get(model_cfg, 'LAYER_NUMS')), list(_get(model_cfg, 'LAYER_STRIDES'))
            num_filters = list(_get(model_cfg, 'NUM_FILTERS'))
            assert len(layer_nums) == len(layer_strides) == len(num_filters)
        else:
            layer_nums = layer_strides = num_filters = []
        if _get(model_cfg, 'UPSAMPLE_STRIDES', None) is not None:
            upsample_strides, num_upsample_filters = list(_get(model_cfg, 'UPSAMPLE_STRIDES')), list(_get(model_cfg, 'NUM_UPSAMPLE_FILTERS'))
            assert len(upsample_strides) == len(num_upsample_filters)
        else:
            upsample_strides = num_upsample_filters = []

        def bn(c):
            return nn.BatchNorm2d(c, eps=1e-3, momentum=0.01)

        num_levels = len(layer_nums)
        c_in_list = [input_channels, *num_filters[:-1]]
        self.blocks = nn.ModuleList()
        self.deblocks = nn.ModuleList()
        for idx in range(num_levels):
            layers = [BasicBlock(c_in_list[idx], num_filters[idx], layer_strides[idx], 1, True)]
            layers.extend(BasicBlock(num_filters[idx], num_filters[idx]) for _ in range(layer_nums[idx]))
            self.blocks.append(nn.Sequential(*layers))
            if len(upsample_strides) > 0:
                stride = upsample_strides[idx]
                if stride >= 1:
                    up = nn.ConvTranspose2d(num_filters[idx], num_upsample_filters[idx], stride, stride=stride, bias=False)
                else:
                    stride = int(round(1 / stride))
                    up = nn.Conv2d(num_filters[idx], num_upsample_filters[idx], stride, stride=stride, bias=False)
                self.deblocks.append(nn.Sequential(up, bn(num_upsample_filters[idx]), nn.ReLU()))
        c_in = sum(num_upsample_filters) if len(num_upsample_filters) > 0 else sum(num_filters)
        if len(upsample_strides) > num_levels:
            self.deblocks.append(nn.Sequential(
                nn.ConvTranspose2d(c_in, c_in, upsample_strides[-1], stride=upsample_strides[-1], bias=False), bn(c_in), nn.ReLU()))
        self.num_bev_features = c_in

    forward = BaseBEVBackbone.forward

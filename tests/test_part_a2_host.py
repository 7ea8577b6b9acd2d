"""Part-A2 without a GPU: hand-derived known answers of the numpy inverse sparse convolution (tests/part_a2_reference.py), the
activity rule and row order of the sparse RoI-aware pooling's restatement, the configuration and the module registries."""
import numpy as np
import pytest
import torch

import part_a2_reference as par
import sparse_conv_reference as scr


def test_inverse_conv_known_answer_on_a_line():
    """Grid (D, H, W) = (5, 1, 1), all five sites z = 0 .. 4 active, kernel (3, 1, 1), stride (2, 1, 1), no padding: the strided
    convolution has two output sites, o0 reading z = 0, 1, 2 and o1 reading z = 2, 3, 4 under the offsets k = 0, 1, 2.  With one
    channel, W[k] = (1, 10, 100) and the output-site values y = (1, 2), the inverse puts W[k] y[o] on the input row that o reads under
    k: z0 = 1, z1 = 10, z2 = 100 * 1 + 1 * 2 = 102 (read by both, under k = 2 and k = 0: same offset index, no flip), z3 = 20, z4 = 200."""
    idx = np.array([[0, z, 0, 0] for z in range(5)], dtype=np.int32)
    out_idx, nbr, oshape = scr.rulebook(idx, 1, (5, 1, 1), (3, 1, 1), (2, 1, 1), (0, 0, 0), False)
    assert oshape == (2, 1, 1) and nbr.tolist() == [[0, 1, 2], [2, 3, 4]]
    w = np.array([1.0, 10.0, 100.0]).reshape(1, 3, 1, 1, 1)
    got = par.inverse_conv_reference(np.array([[1.0], [2.0]]), nbr, w, 5)
    assert got[:, 0].tolist() == [1.0, 10.0, 102.0, 20.0, 200.0]


def test_inverse_conv_known_answer_with_a_missing_site_and_two_channels():
    """the same line without z = 3 (rows z = 0, 1, 2, 4): o1 reads rows 2, -, 3.  Two input channels (y, 2 y) with weights
    W[c_out = 0][k] = (1, 10, 100) on channel 0 and zero on channel 1, W[c_out = 1][k] = 1 on channel 1 only: channel 0 as before
    without z3, channel 1 = 2 * (sum of the y that read the row)."""
    idx = np.array([[0, z, 0, 0] for z in (0, 1, 2, 4)], dtype=np.int32)
    _, nbr, _ = scr.rulebook(idx, 1, (5, 1, 1), (3, 1, 1), (2, 1, 1), (0, 0, 0), False)
    assert nbr.tolist() == [[0, 1, 2], [2, -1, 3]]
    w = np.zeros((2, 3, 1, 1, 2))
    w[0, :, 0, 0, 0] = [1, 10, 100]
    w[1, :, 0, 0, 1] = 1
    y = np.array([[1.0, 2.0], [2.0, 4.0]])
    got = par.inverse_conv_reference(y, nbr, w, 4)
    assert got.tolist() == [[1.0, 2.0], [10.0, 2.0], [102.0, 6.0], [200.0, 4.0]]


def test_active_cells_rule_and_order():
    """active = the fp32 sum of the four part channels, added in ascending channel order, is non-zero: a cell of zeros is not,
    a cell whose channels cancel exactly is not, and 2^24 + 1 - 2^24 (0 in fp32 ascending order, 1 in exact arithmetic) is not;
    rows ascend in ((roi Sx + x) Sy + y) Sz + z"""
    p = np.zeros((2, 2, 3, 2, 4), dtype=np.float32)
    p[1, 0, 2, 1] = [0.5, 0, 0, 0]
    p[0, 1, 0, 0] = [0, 0, 0, 1e-30]
    p[0, 0, 1, 1] = [1, -1, 0, 0]                       # cancels
    p[0, 1, 2, 0] = [2.0 ** 24, 1, -2.0 ** 24, 0]       # the 1 is lost in fp32: inactive by the rule
    p[1, 1, 1, 0] = [1, 2.0 ** 24, -2.0 ** 24, 0]       # ascending: (1 + 2^24) = 2^24 in fp32, then 0: inactive as well
    p[0, 0, 0, 1] = [-2.0 ** 24, 2.0 ** 24, 1, 0]       # 0, then + 1: active
    got = par.active_cells(p)
    assert got.dtype == np.int32 and got.tolist() == [[0, 0, 0, 1], [0, 1, 0, 0], [1, 0, 2, 1]]


def test_config_builds_and_registries():
    from pdm_ssd_amd import backbones_3d, dense_heads, detector_config as dc, detectors, roi_heads, spconv
    assert 'SparseInverseConv3d' in spconv.__all__ and issubclass(spconv.SparseInverseConv3d, spconv.SparseModule)
    assert 'UNetV2' in backbones_3d.__all__ and 'PointIntraPartOffsetHead' in dense_heads.__all__
    assert 'PartA2FCHead' in roi_heads.__all__ and 'PartA2Net' in detectors.__all__
    roi = dc.PART_A2_CFG['ROI_HEAD']
    assert roi['ROI_AWARE_POOL'] == {'POOL_SIZE': 12, 'NUM_FEATURES': 128, 'MAX_POINTS_PER_VOXEL': 128, 'FUSED': True}
    assert roi['SHARED_FC'] == [256, 256, 256] and roi['CLS_FC'] == [256, 256] and roi['REG_FC'] == [256, 256]
    assert roi['DP_RATIO'] == 0.3 and roi['SEG_MASK_SCORE_THRESH'] == 0.3 and roi['NMS_CONFIG']['TEST']['NMS_POST_MAXSIZE'] == 100
    ph = dc.PART_A2_CFG['POINT_HEAD']
    assert ph['CLS_FC'] == [256, 256] and ph['PART_FC'] == [256, 256] and ph['TARGET_CONFIG']['GT_EXTRA_WIDTH'] == [0.2, 0.2, 0.2]
    import copy
    cfg = copy.deepcopy(dc.PART_A2_CFG)
    cfg['ROI_HEAD']['ROI_AWARE_POOL']['POOL_SIZE'] = 2      # (the published 12 makes a 226 MB first FC: not for a host test)
    model = dc.build_part_a2(cfg)
    keys = list(model.state_dict())
    for k in ('backbone_3d.inv_conv4.0.weight', 'backbone_3d.conv_up_t4.conv1.weight', 'backbone_3d.conv_up_m1.0.weight', 'backbone_3d.conv5.0.0.weight',
              'backbone_3d.conv_out.0.weight', 'point_head.cls_layers.0.weight', 'point_head.part_reg_layers.6.bias',
              'roi_head.conv_part.0.0.weight', 'roi_head.conv_rpn.1.0.weight', 'roi_head.shared_fc_layer.8.weight', 'roi_head.reg_layers.7.bias'):
        assert k in keys, k
    assert not any(k.startswith('point_head.box_layers') for k in keys)
    inv = model.backbone_3d.inv_conv3[0]
    assert type(inv).__name__ == 'SparseInverseConv3d' and inv.indice_key == 'spconv3' and tuple(inv.weight.shape) == (32, 3, 3, 3, 64)
    assert 'backbone_3d.conv_up_t4.conv1.bias' not in keys and 'backbone_3d.conv_up_t4.bn1.bias' in keys      # the UNet's blocks: no conv bias
    with pytest.raises(NotImplementedError):
        model.train()({'batch_size': 1, 'points': torch.zeros((1, 5))})
    with pytest.raises(NotImplementedError):
        model.point_head.get_loss()

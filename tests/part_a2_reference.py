"""What the Part-A2 operators' tests share (a helper module like sparse_conv_reference.py: no tests, no fixtures, nothing from
pdm_ssd_amd):

  * inverse_conv_reference: a numpy restatement in float64 of the inverse sparse convolution over a rulebook of
    sparse_conv_reference.rulebook: out[i] = sum over the pairs nbr[j, k] = i of W[:, k, :] x[j], same offset index k, no flip.
  * the case of tests/golden/ref_part_a2.npz (gen_part_a2_fixtures.py): seeds and the reduced head configurations.
  * active_cells: the activity rule and row order of the batched sparse RoI-aware pooling, restated on the dense pooled
    tensors of the composed formulation: a cell is active where the fp32 sum of its averaged part channels, added in ascending
    channel order, is non-zero; rows ascend in ((roi S_x + x) S_y + y) S_z + z.
"""
import numpy as np

import sparse_conv_reference as scr  # noqa: F401  (the rulebooks the inverse walks come from there)


def inverse_conv_reference(x, nbr, weight, num_in_rows):
    """x (P_out, Cin) the rows of the paired convolution's OUTPUT, nbr (P_out, kvol) that convolution's table (its input row
    under every offset or -1), weight (Cout, kz, ky, kx, Cin) -> (num_in_rows, Cout) float64 on the convolution's INPUT rows"""
    x = np.asarray(x, dtype=np.float64)
    nbr = np.asarray(nbr)
    w = np.asarray(weight, dtype=np.float64)
    w = w.reshape(w.shape[0], -1, w.shape[-1])                   # (Cout, kvol, Cin)
    out = np.zeros((int(num_in_rows), w.shape[0]))
    for j in range(nbr.shape[0]):
        for k in range(nbr.shape[1]):
            i = int(nbr[j, k])
            if i >= 0:
                out[i] += w[:, k, :] @ x[j]
    return out


def active_cells(pooled_part):
    """pooled_part (R, Sx, Sy, Sz, 4) fp32, the 'avg' pooling of the part features -> coords (Q, 4) int32 rows (roi, x, y, z) of
    the active cells in ascending ((roi Sx + x) Sy + y) Sz + z"""
    p = np.asarray(pooled_part, dtype=np.float32)
    s = p[..., 0]
    for c in range(1, p.shape[-1]):
        s = (s + p[..., c]).astype(np.float32)                   # one fp32 rounding per addition, ascending channels
    return np.argwhere(s != 0).astype(np.int32)                  # argwhere walks in C order: the key's order


# ---- the fixture's case: UNetV2 on sparse_conv_reference.b1_voxels with fill_backbone(UNET_SEED, UNET_GAIN), heads at reduced widths
UNET_SEED, UNET_GAIN = 47, 0.7
GEO = scr.V1            # the range and voxel size of B1_GRID
POINT_CFG = {'CLS_FC': [32], 'PART_FC': [32], 'CLASS_AGNOSTIC': True, 'TARGET_CONFIG': {'GT_EXTRA_WIDTH': [0.2, 0.2, 0.2]},
             'LOSS_CONFIG': {'LOSS_REG': 'smooth-l1', 'LOSS_WEIGHTS': {'point_cls_weight': 1.0, 'point_part_weight': 1.0}}}
ROI_CFG = {'CLASS_AGNOSTIC': True, 'SHARED_FC': [32, 32], 'CLS_FC': [32], 'REG_FC': [32], 'DP_RATIO': 0.3, 'DISABLE_PART': False,
           'SEG_MASK_SCORE_THRESH': 0.3,
           'NMS_CONFIG': {'TEST': {'NMS_TYPE': 'nms_gpu', 'MULTI_CLASSES_NMS': False, 'NMS_PRE_MAXSIZE': 64, 'NMS_POST_MAXSIZE': 5, 'NMS_THRESH': 0.7}},
           'ROI_AWARE_POOL': {'POOL_SIZE': 3, 'NUM_FEATURES': 32, 'MAX_POINTS_PER_VOXEL': 4},
           'TARGET_CONFIG': {'BOX_CODER': 'ResidualCoder'},
           'LOSS_CONFIG': {'CLS_LOSS': 'BinaryCrossEntropy', 'REG_LOSS': 'smooth-l1', 'CORNER_LOSS_REGULARIZATION': True,      # (read by the
                           'LOSS_WEIGHTS': {'rcnn_cls_weight': 1.0, 'rcnn_reg_weight': 1.0, 'rcnn_corner_weight': 1.0,                # reference's constructor)
                                            'code_weights': [1.0] * 7}}}

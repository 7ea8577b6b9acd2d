"""Shared inputs of the CenterHead tests: the reference fixture (tests/golden/gen_center_head_fixtures.py), its head
configuration restated, and the builders and comparisons both the CPU and the GPU tests use."""
import json
import os

import numpy as np
import torch

from pdm_ssd_amd.config import cfg_from_dict
from pdm_ssd_amd.dense_heads import CenterHead

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
B, H, W, CIN = 2, 12, 20, 8
CLASS_NAMES = ['Car', 'Pedestrian', 'Cyclist']
PC_RANGE = [0.0, -2.4, -3.0, 8.0, 2.4, 1.0]
VOXEL = [0.05, 0.05, 0.1]
STRIDE = 8
LIMIT = [0.5, -2.0, -2.0, 7.5, 2.0, 1.0]
MARGIN = 1e-3
TOL = 1e-4                        # the project's standing tolerance for floats against a reference
HEADS = {'one': [['Car', 'Pedestrian', 'Cyclist']], 'two': [['Car'], ['Pedestrian', 'Cyclist']]}
MAPS = ('center', 'center_z', 'dim', 'rot')
TARGET_KEYS = ('heatmaps', 'target_boxes', 'inds', 'masks', 'target_boxes_src')

_fixture = None


def fixture():
    global _fixture
    if _fixture is None:
        with np.load(os.path.join(G, "ref_center_head.npz")) as z:
            _fixture = {k: z[k] for k in z.files}
    return _fixture


def manifest():
    with open(os.path.join(G, "ref_center_head_manifest.json")) as f:
        return json.load(f)


def head_cfg(class_names_each_head, **post):
    """as tests/golden/gen_center_head_fixtures.py"""
    return {'CLASS_NAMES_EACH_HEAD': class_names_each_head, 'SHARED_CONV_CHANNEL': 16, 'USE_BIAS_BEFORE_NORM': True, 'NUM_HM_CONV': 2,
            'SEPARATE_HEAD_CFG': {'HEAD_ORDER': ['center', 'center_z', 'dim', 'rot'],
                                  'HEAD_DICT': {'center': {'out_channels': 2, 'num_conv': 2}, 'center_z': {'out_channels': 1, 'num_conv': 2},
                                                'dim': {'out_channels': 3, 'num_conv': 2}, 'rot': {'out_channels': 2, 'num_conv': 2}}},
            'TARGET_ASSIGNER_CONFIG': {'FEATURE_MAP_STRIDE': STRIDE, 'NUM_MAX_OBJS': 6, 'GAUSSIAN_OVERLAP': 0.1, 'MIN_RADIUS': 2},
            'LOSS_CONFIG': {'LOSS_WEIGHTS': {'cls_weight': 1.0, 'loc_weight': 2.0,
                                             'code_weights': [1.0, 1.0, 0.5, 1.0, 1.0, 1.0, 2.0, 1.0]}},
            'POST_PROCESSING': dict({'SCORE_THRESH': 0.1, 'POST_CENTER_LIMIT_RANGE': LIMIT, 'MAX_OBJ_PER_SAMPLE': 10,
                                     'NMS_CONFIG': {'NMS_TYPE': 'nms_gpu', 'NMS_THRESH': 0.1, 'NMS_PRE_MAXSIZE': 100, 'NMS_POST_MAXSIZE': 10}},
                                    **post)}


def build_head(class_names_each_head, tag=None, as_config=True, edit=None, **kw):
    """a CenterHead at the fixture's shapes; tag 'one' | 'two' loads the reference's parameters; edit(cfg) changes the dict"""
    cfg = head_cfg(class_names_each_head)
    if edit is not None:
        edit(cfg)
    head = CenterHead(model_cfg=cfg_from_dict(cfg) if as_config else cfg, input_channels=CIN, num_class=3, class_names=CLASS_NAMES,
                      grid_size=np.array([160, 96, 40]), point_cloud_range=PC_RANGE, voxel_size=VOXEL,
                      predict_boxes_when_training=False, **kw)
    if tag is not None:
        fx = fixture()
        state = {k[len(tag) + 7:]: torch.from_numpy(v) for k, v in fx.items() if k.startswith(f'{tag}.state.')}
        head.load_state_dict(state, strict=True)
    return head


def close(a, b, tol=TOL):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    if a.size:
        err = np.abs(a - b).max()
        assert err <= tol * max(1.0, float(np.abs(b).max())), err


def check_targets(td, prefix, heads=None):
    """td: an assign_targets dict -> compared with the fixture's record: integers exactly, floats at TOL"""
    fx = fixture()
    n = len(td['heatmaps'])
    assert n == sum(1 for k in fx if k.startswith(f'{prefix}.inds.'))
    for h in range(n):
        for key in TARGET_KEYS:
            got, want = td[key][h].detach().cpu().numpy(), fx[f'{prefix}.{key}.{h}']
            if key in ('inds', 'masks'):
                assert got.dtype == np.int64 and np.array_equal(got, want), (key, h)
            else:
                close(got, want)


def check_decode_conditions(logits, K, thresh, ranked_boxes):
    """The conditions on the decode fixture's inputs, re-asserted: consecutive scores among the top K + 1 of every sample
    differ by at least MARGIN, and no candidate lies within MARGIN of the score threshold or of a limit-range bound."""
    scores = 1.0 / (1.0 + np.exp(-logits.astype(np.float64).reshape(logits.shape[0], -1)))
    top = np.sort(scores, axis=1)[:, ::-1][:, :min(K + 1, scores.shape[1])]
    assert (top[:, :-1] - top[:, 1:]).min() >= MARGIN
    assert np.abs(top[:, :K] - thresh).min() >= MARGIN
    lim = np.array(LIMIT, dtype=np.float64)
    xyz = np.asarray(ranked_boxes, dtype=np.float64)[..., :3]
    assert min(np.abs(xyz - lim[:3]).min(), np.abs(xyz - lim[3:]).min()) >= MARGIN


def decode_maps(device='cpu', dtype=torch.float32):
    fx = fixture()
    return {k: torch.from_numpy(fx[f'dec_{k}']).to(device=device, dtype=dtype) for k in ('hm',) + MAPS}


def interleaved_expectation():
    """[['Car', 'Cyclist'], ['Pedestrian']] on the fixture's boxes, derived by hand: head 0 takes rows 0 (Car), 3 (Cyclist -> its
    class 2), 4 (Car, dx = 0: a used, empty slot) and 6 (Car, far edge); head 1 rows 2 and 7 (Pedestrian -> its class 1).  The
    reference would hand head 1 row 0, 4 and 6 as well: head 0 relabels Car to 1 in the caller's tensor, and 1 is Pedestrian."""
    gt = fixture()['gt_boxes']
    rows = {0: [(0, 1), (3, 2), (4, 1), (6, 1)], 1: [(2, 1), (7, 1)]}
    cells = {0: (5, 3), 3: (13, 7), 6: (19, 11), 2: (13, 7), 7: (2, 0)}       # (x, y) = trunc((x - 0) / 0.4), trunc((y + 2.4) / 0.4)
    out = {}
    for h, picks in rows.items():
        src = np.zeros((B, 6, 8), dtype=np.float32)
        inds = np.zeros((B, 6), dtype=np.int64)
        mask = np.zeros((B, 6), dtype=np.int64)
        for k, (r, local) in enumerate(picks):
            src[0, k] = gt[0, r]
            src[0, k, 7] = local
            if r in cells:
                inds[0, k] = cells[r][1] * W + cells[r][0]
                mask[0, k] = 1
        out[h] = (src, inds, mask)
    return out

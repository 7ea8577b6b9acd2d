"""Shared inputs of the anchor-head tests: the reference fixture (tests/golden/gen_anchor_head_fixtures.py), its head
configuration restated, and the builders, box draws and comparisons both the CPU and the GPU tests use."""
import json
import os

import numpy as np
import torch

from center_head_case import TOL, close  # noqa: F401  (the standing tolerance and its rule)
from pdm_ssd_amd.config import cfg_from_dict
from pdm_ssd_amd.dense_heads import AnchorHeadSingle

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
B, H, W, CIN = 2, 12, 20, 8
A_LOC = 6
CLASS_NAMES = ['Car', 'Pedestrian', 'Cyclist']
GRID_SIZE = [40, 24, 1]
PC_RANGE = [0.0, -9.6, -3.0, 32.0, 9.6, 1.0]
MARGIN = 1e-3
SETS = [('Car', [3.9, 1.6, 1.56], -1.78, 0.6, 0.45), ('Pedestrian', [0.8, 0.6, 1.73], -0.6, 0.5, 0.35),
        ('Cyclist', [1.76, 0.6, 1.73], -0.6, 0.5, 0.35)]
MAPS = ('cls_preds', 'box_preds', 'dir_cls_preds')

_fixture = None


def fixture():
    global _fixture
    if _fixture is None:
        with np.load(os.path.join(G, "ref_anchor_head.npz")) as z:
            _fixture = {k: z[k] for k in z.files}
    return _fixture


def manifest():
    with open(os.path.join(G, "ref_anchor_head_manifest.json")) as f:
        return json.load(f)


def head_cfg(align_center=False, direction=True, norm=False):
    """as tests/golden/gen_anchor_head_fixtures.py"""
    cfg = {'NAME': 'AnchorHeadSingle', 'CLASS_AGNOSTIC': False, 'DIR_OFFSET': 0.78539, 'DIR_LIMIT_OFFSET': 0.0, 'NUM_DIR_BINS': 2,
           'ANCHOR_GENERATOR_CONFIG': [
               {'class_name': n, 'anchor_sizes': [size], 'anchor_rotations': [0, 1.57], 'anchor_bottom_heights': [z],
                'align_center': align_center, 'feature_map_stride': 2, 'matched_threshold': hi, 'unmatched_threshold': lo}
               for n, size, z, hi, lo in SETS],
           'TARGET_ASSIGNER_CONFIG': {'NAME': 'AxisAlignedTargetAssigner', 'POS_FRACTION': -1.0, 'SAMPLE_SIZE': 512,
                                      'NORM_BY_NUM_EXAMPLES': norm, 'MATCH_HEIGHT': False, 'BOX_CODER': 'ResidualCoder'},
           'LOSS_CONFIG': {'LOSS_WEIGHTS': {'cls_weight': 1.0, 'loc_weight': 2.0, 'dir_weight': 0.2, 'code_weights': [1.0] * 7}}}
    if direction:
        cfg['USE_DIRECTION_CLASSIFIER'] = True
    return cfg


def build_head(state=None, num_class=3, grid_size=GRID_SIZE, pc_range=PC_RANGE, edit=None, as_config=True, **cfg_kw):
    """an AnchorHeadSingle at the fixture's shapes (or on another grid); state '' | 'nodir.' | 'nc1.' loads the reference's
    parameters; edit(cfg) changes the dict"""
    cfg = head_cfg(**cfg_kw)
    if edit is not None:
        edit(cfg)
    head = AnchorHeadSingle(model_cfg=cfg_from_dict(cfg) if as_config else cfg, input_channels=CIN, num_class=num_class,
                            class_names=CLASS_NAMES, grid_size=np.array(grid_size), point_cloud_range=np.array(pc_range),
                            predict_boxes_when_training=False)
    if state is not None:
        fx = fixture()
        prefix = f'{state}state.'
        head.load_state_dict({k[len(prefix):]: torch.from_numpy(v) for k, v in fx.items() if k.startswith(prefix)}, strict=True)
    return head


def check_margins(ious, sets=SETS):
    """The conditions on the boxes, asserted on {(sample, set): (anchors of the set, boxes of its class) IoUs}: no IoU within
    MARGIN of a threshold; every box's best IoU at least MARGIN above the next lower one — where several IoUs lie within MARGIN
    of the best without being the same bits (the fixture's square box: its two rotations differ by 1.8e-6), all of them lie
    at least MARGIN above the matched threshold, positive with or without being forced.  Raises AssertionError."""
    for (b, s), m in ious.items():
        m = np.asarray(m, dtype=np.float64)
        if m.size == 0:
            continue
        for th in sets[s][3:5]:
            assert np.abs(m - th).min() >= MARGIN, (b, s, 'threshold')
        for j in range(m.shape[1]):
            col = m[:, j]
            best = col.max()
            if best > 0:
                group = col[col > best - MARGIN]
                assert len(np.unique(group)) == 1 or group.min() >= sets[s][3] + MARGIN, (b, s, j, 'runner-up')
                assert best - col[col <= best - MARGIN].max() >= MARGIN


def ious_of(head, gt):
    """{(b, s): IoUs} of a head's anchors against gt (B, M, 8) on the CPU, by the torch formulation"""
    from pdm_ssd_amd.utils import box_utils
    out = {}
    gt = torch.as_tensor(gt).float().cpu()
    for b in range(gt.shape[0]):
        for s, a in enumerate(head.anchors):
            mine = gt[b][gt[b, :, 7] == s + 1]
            out[(b, s)] = box_utils.boxes3d_nearest_bev_iou(a.cpu().view(-1, 7), mine[:, :7]).numpy() if len(mine) else np.zeros((0, 0))
    return out


SIZES = np.array([s[1] for s in SETS], dtype=np.float32)


def draw_boxes(head, Bn, M, seed, classes=(1, 2, 3), fill=0.8, x_hi=32.0, y_half=9.6, cap=50):
    """(Bn, M, 8) seeded boxes with padding rows scattered through the list.  Both margin conditions are properties of one box
    against its set's anchors, so every box is re-drawn on its own until it meets them; the loop is capped at `cap` draws a
    box and raises when the cap is reached."""
    from pdm_ssd_amd.utils import box_utils
    rng = np.random.default_rng(seed)
    flat = [a.cpu().view(-1, 7) for a in head.anchors]
    gt = np.zeros((Bn, M, 8), dtype=np.float32)
    for b in range(Bn):
        for r in range(M):
            if rng.uniform() > fill:
                continue
            cls = int(classes[int(rng.integers(0, len(classes)))])
            for _ in range(cap):
                box = np.array([rng.uniform(0.5, x_hi - 0.5), rng.uniform(-y_half + 0.5, y_half - 0.5), rng.uniform(-1.2, -0.6),
                                *(SIZES[cls - 1] * rng.uniform(0.85, 1.15, 3)), rng.uniform(-3.1, 3.1)], dtype=np.float32)
                iou = box_utils.boxes3d_nearest_bev_iou(flat[cls - 1], torch.from_numpy(box[None])).numpy()
                try:
                    check_margins({(b, cls - 1): iou})
                except AssertionError:
                    continue
                break
            else:
                raise AssertionError(f'sample {b} row {r}: no draw out of {cap} meets the margin conditions')
            gt[b, r, :7] = box
            gt[b, r, 7] = cls
    check_margins(ious_of(head, gt))
    return gt


TIE_GRID, TIE_RANGE = [34, 18, 1], [0.0, -8.0, -3.0, 32.0, 8.0, 1.0]     # stride 2: a 9 x 17 map of cells exactly 2 m apart


def tie_head(**kw):
    """a head whose Car anchors are 4 x 2 m on cell centres with exact coordinates (x = 0, 2, .., y = -8, -6, ..)"""
    def edit(cfg):
        cfg['ANCHOR_GENERATOR_CONFIG'][0]['anchor_sizes'] = [[4.0, 2.0, 1.5]]
    return build_head(grid_size=TIE_GRID, pc_range=TIE_RANGE, edit=edit, **kw)


def tie_boxes():
    """one 4 x 2 m Car at (5, 1), between the cells (4 | 6, 0 | 2): against each of their rotation-1.57 anchors the overlap is
    2 x 2 of a union of 12, every operand exact, so the four IoUs of 1/3 are the same bits; the rotation-0 anchors reach 3/13"""
    gt = np.zeros((1, 2, 8), dtype=np.float32)
    gt[0, 0] = [5.0, 1.0, -1.0, 4.0, 2.0, 1.5, 0.0, 1]
    return gt


def check_targets(td, tag):
    """td: an assign_targets dict -> compared with the fixture's record: labels and num_pos exactly, floats at TOL"""
    fx = fixture()
    labels = td['box_cls_labels'].cpu().numpy()
    assert labels.dtype == np.int32 and np.array_equal(labels, fx[f'targets.{tag}.labels'])
    assert td['num_pos'].dtype == torch.int32 and td['num_pos'].cpu().tolist() == (fx[f'targets.{tag}.labels'] > 0).sum(1).tolist()
    close(td['box_reg_targets'].cpu().numpy(), fx[f'targets.{tag}.reg'])
    close(td['reg_weights'].cpu().numpy(), fx[f'targets.{tag}.weights'])


def same_targets(got, want):
    """two assign_targets dicts (any devices): labels and num_pos exactly, floats at TOL"""
    assert torch.equal(got['box_cls_labels'].cpu(), want['box_cls_labels'].cpu())
    assert torch.equal(got['num_pos'].cpu(), want['num_pos'].cpu())
    close(got['box_reg_targets'].cpu().numpy(), want['box_reg_targets'].cpu().numpy())
    close(got['reg_weights'].cpu().numpy(), want['reg_weights'].cpu().numpy())


def close_grad(got, want):
    """gradients at TOL relative to the map's largest reference gradient"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    err, scale = np.abs(got - want).max(), np.abs(want).max()
    assert err <= TOL * scale, (err, scale)


def torch_losses(head, maps, targets):
    """the torch formulation on fp32 leaves made from `maps` (any device/dtype) moved to the CPU -> ((cls, loc, dir | None)
    terms, gradients in map order)"""
    cpu = copy_head_cpu(head)
    leaves = [None if t is None else t.detach().float().cpu().requires_grad_(True) for t in maps]
    cpu.forward_ret_dict = {k: v for k, v in zip(MAPS, leaves) if v is not None}
    cpu.forward_ret_dict.update({k: v.detach().cpu() for k, v in targets.items()})
    cls_loss, _ = cpu.get_cls_layer_loss()
    box_loss, tb = cpu.get_box_reg_layer_loss()
    (cls_loss + box_loss).backward()
    return (cls_loss.detach(), tb['rpn_loss_loc'], tb.get('rpn_loss_dir')), [None if t is None else t.grad for t in leaves]


def copy_head_cpu(head):
    import copy
    kept, head.forward_ret_dict = head.forward_ret_dict, {}          # (tensors inside a graph do not deep-copy)
    try:
        cpu = copy.deepcopy(head).cpu()
    finally:
        head.forward_ret_dict = kept
    cpu.use_fused = False
    return cpu

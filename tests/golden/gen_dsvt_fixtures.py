#!/usr/bin/env python3
"""Generates tests/golden/ref_dsvt.npz (+ ref_dsvt_manifest.json) by running the REFERENCE's own DSVT in eval mode on the CPU:
pcdet/models/backbones_3d/dsvt.py with models/model_utils/dsvt_utils.py, and PointPillarScatter3d and BaseBEVResBackbone of
backbones_2d, imported from where they lie, nothing copied, with the stubs of gen_head_fixtures.install_reference and one
more: pcdet.ops.ingroup_inds.ingroup_inds_op.ingroup_inds (a CUDA extension in the reference) as a stable numbering of the
voxels of each window in row order.  The reference's result does not depend on which valid numbering that function returns.
The installed torch refuses the all-zero INT key_padding_mask the reference hands its attention reduction: the generator
passes it on as bool (it masks nothing either way).
Run in the authoring container only; the outputs hold numbers and key names only.

Cases, occupancies, inputs and the seeded fill: tests/dsvt_case.py.  No weights are stored.

Conditions asserted on the reference's own output (batch_win_inds and the set indices it returns):
  case a: some window holds exactly 1 voxel (all slots of its set but the first are masked), some exactly ss and some 3 ss
          (nothing masked), some ss + 1; the second input (a_empty) has a sample with no voxel;
  case b: 1, ss and ss + 1;
  case c: the same, and some voxel lies in a window that exists only through the shift's extra border window, in x and in z;
  every case: the two shifts have different set counts, and every voxel fills exactly one unmasked slot per partition.

Parity bound: a float64 twin of the reference (built with default dtype float64, the same seeded values) runs on the same
inputs.  With these weights the reference's float32 run lies 1.5e-6 to 3.4e-6 from its float64 run at an output scale of 4 to 6
(LayerNorm outputs); parity_abs = 2e-5 leaves a second float32 implementation with another summation order a few times that
distance, and the generator fails unless float32 and float64 agree within a quarter of it.
"""
import importlib
import json
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from gen_center_head_fixtures import EasyDict  # noqa: E402
from gen_head_fixtures import REF, install_reference  # noqa: E402
import dsvt_case as dc  # noqa: E402

PARITY_ABS = 2e-5


def ingroup_inds(group_inds):
    """a valid in-window numbering: the voxels of a window numbered 0, 1, ... in row order"""
    order = torch.argsort(group_inds, stable=True)
    sorted_g = group_inds[order]
    start = torch.ones_like(sorted_g, dtype=torch.bool)
    start[1:] = sorted_g[1:] != sorted_g[:-1]
    first = torch.cummax(torch.where(start, torch.arange(len(sorted_g)), torch.zeros_like(sorted_g)), 0).values
    out = torch.empty_like(group_inds)
    out[order] = torch.arange(len(sorted_g)) - first
    return out


def install_dsvt():
    install_reference()
    for name in ('pcdet.ops.ingroup_inds', 'pcdet.ops.ingroup_inds.ingroup_inds_op'):
        sys.modules[name] = types.ModuleType(name)
    sys.modules['pcdet.ops.ingroup_inds.ingroup_inds_op'].ingroup_inds = ingroup_inds
    for name in ('pcdet.models.backbones_3d', 'pcdet.models.backbones_2d', 'pcdet.models.backbones_2d.map_to_bev'):
        m = types.ModuleType(name)                  # package __init__ not run (it imports spconv)
        m.__path__ = [f'{REF}/' + name.replace('.', '/')]
        sys.modules[name] = m
    dsvt = importlib.import_module('pcdet.models.backbones_3d.dsvt')
    reduce = dsvt.Stage_ReductionAtt_Block.forward
    dsvt.Stage_ReductionAtt_Block.forward = lambda self, x, key_padding_mask: reduce(self, x, key_padding_mask.bool())
    return (dsvt,
            importlib.import_module('pcdet.models.backbones_2d.map_to_bev.pointpillar_scatter'),
            importlib.import_module('pcdet.models.backbones_2d.base_bev_backbone'))


def window_counts(win):
    return np.unique(win.numpy(), return_counts=True)[1]


def run_case(ref, name, models):
    c = dc.CASES[name]
    coords = dc.coords(name)
    feats = dc.features(name, len(coords))
    key = c.get('model', name)
    if key not in models:
        pair = []
        for dtype in (torch.float32, torch.float64):
            torch.set_default_dtype(dtype)
            m = ref.DSVT(EasyDict(dc.model_cfg(key)))
            torch.set_default_dtype(torch.float32)
            total = dc.fill(m)
            pair.append(m.eval())
        models[key] = (pair, total)
    (m32, m64), total = models[key]
    with torch.no_grad():
        info = m32.input_layer({'voxel_features': feats, 'voxel_coords': torch.from_numpy(coords)})
        out32 = m32({'voxel_features': feats, 'voxel_coords': torch.from_numpy(coords)})
        torch.set_default_dtype(torch.float64)      # (the reference's position embedding builds float tensors of the default dtype)
        out64 = m64({'voxel_features': feats.double(), 'voxel_coords': torch.from_numpy(coords)})
        torch.set_default_dtype(torch.float32)
    arrays = {'coords': coords, 'out': out32['voxel_features'].numpy(), 'out_coords': out32['voxel_coords'].numpy().astype(np.int32)}
    stages = c.get('stages', 1)
    sets = []
    for s in range(stages):
        for i in range(2):
            inds, mask = info[f'set_voxel_inds_stage{s}_shift{i}'], info[f'set_voxel_mask_stage{s}_shift{i}']
            n = len(info[f'voxel_coors_stage{s}'])
            for ax in range(2):                     # every voxel fills exactly one unmasked slot
                live = inds[ax][~mask[ax]].numpy()
                assert len(live) == n and len(np.unique(live)) == n, (name, s, i, ax)
            arrays[f'inds.{s}.{i}'] = inds.numpy().astype(np.int32)
            arrays[f'mask.{s}.{i}'] = mask.numpy()
            arrays[f'ciw.{s}.{i}'] = info[f'coors_in_win_stage{s}_shift{i}'].numpy().astype(np.int16)
            sets.append(int(inds.shape[1]))
        assert sets[-2] != sets[-1], (name, sets)
        if s:
            arrays[f'coords.{s}'] = info[f'voxel_coors_stage{s}'].numpy().astype(np.int32)
    # the hand-placed conditions, on the reference's window ids
    counts = [window_counts(info[f'batch_win_inds_stage0_shift{i}']) for i in range(2)]
    if 'empty' in c:
        assert not (coords[:, 0] == c['empty']).any()
    else:
        want = dc.hand_counts(name)
        ss = c['ss']
        for n in (1, ss, ss + 1) + ((3 * ss,) if 3 * ss in want else ()):
            assert (counts[0] == n).any(), (name, n)
        m0 = arrays['mask.0.0']
        assert (m0[0].sum(1) == ss - 1).any() and (m0[0].sum(1) == 0).any()
    if name == 'a':
        assert (counts[0] == 36).any()
    if name == 'c':
        (sx, sy, sz), (wx, wy, wz), (hx, hy, hz) = c['shape'], c['window'], c['shift']
        assert (coords[:, 3] + hx >= -(-sx // (2 * wx)) * 2 * wx).any() and (coords[:, 1] + hz >= -(-sz // wz) * wz).any()
    gap = float(np.abs(out64['voxel_features'].numpy() - arrays['out']).max())
    assert gap <= PARITY_ABS / 4, (name, gap)
    meta = {'n': int(len(coords)), 'sets': sets, 'float32_to_float64_gap': gap, 'scale': float(np.abs(arrays['out']).max()),
            'weight_sum': total, 'state': {k: list(v.shape) for k, v in m32.state_dict().items()}}
    return arrays, meta


def main():
    ref, ref_scatter, ref_bev = install_dsvt()
    out, manifest, models = {}, {'parity_abs': PARITY_ABS, 'seed': dc.SEED, 'cases': {}}, {}
    for name in dc.CASES:
        arrays, meta = run_case(ref, name, models)
        for k, v in arrays.items():
            out[f'{name}.{k}'] = v
        manifest['cases'][name] = meta
    for tag, c in dc.SCATTER_CASES.items():
        rows, feats = dc.scatter_input(tag)
        assert (rows[:, 0] == dc.B - 1).any()       # (the reference takes the batch size from the largest sample id)
        m = ref_scatter.PointPillarScatter3d(EasyDict({'INPUT_SHAPE': list(c['shape']), 'NUM_BEV_FEATURES': c['C'] * c['shape'][2]}), None)
        res = m({'pillar_features': torch.from_numpy(feats), 'voxel_coords': torch.from_numpy(rows)})
        out[f'scatter.{tag}'] = res['spatial_features'].numpy()
    bev = ref_bev.BaseBEVResBackbone(EasyDict(dc.BEV_CFG), dc.BEV_INPUT[1])
    manifest['bev_weight_sum'] = dc.fill(bev)
    manifest['bev_state'] = {k: list(v.shape) for k, v in bev.state_dict().items()}
    with torch.no_grad():
        out['bev.out'] = bev.eval()({'spatial_features': torch.from_numpy(dc.bev_input())})['spatial_features_2d'].numpy()
    np.savez_compressed(os.path.join(HERE, 'ref_dsvt.npz'), **out)
    with open(os.path.join(HERE, 'ref_dsvt_manifest.json'), 'w') as f:
        json.dump(manifest, f, indent=1, sort_keys=True)
    print('wrote', len(out), 'arrays;', {k: (v['n'], v['sets'], v['float32_to_float64_gap'], v['scale']) for k, v in manifest['cases'].items()})


if __name__ == '__main__':
    main()

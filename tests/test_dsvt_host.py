"""DSVT on the CPU against tests/golden/ref_dsvt.npz, which holds what the reference's own DSVT, PointPillarScatter3d and
BaseBEVResBackbone computed (tests/golden/gen_dsvt_fixtures.py): state_dict keys, the set partition exactly, the torch path's
features within the manifest's parity_abs (a small multiple of the reference's own float32-to-float64 gap, written there by the
generator), the scatter exactly, the residual 2-D backbone within parity_abs.  Weights are not stored: dsvt_case.fill seeds
them on both sides."""
import json
import os

import numpy as np
import pytest
import torch

import dsvt_case as dc
from pdm_ssd_amd import dsvt_ops
from pdm_ssd_amd.config import cfg_from_dict

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


def load():
    """(arrays, manifest) of the fixture, read once"""
    if not hasattr(load, 'cache'):
        with open(os.path.join(GOLDEN, 'ref_dsvt_manifest.json')) as f:
            manifest = json.load(f)
        load.cache = (dict(np.load(os.path.join(GOLDEN, 'ref_dsvt.npz'))), manifest)
    return load.cache


def build(name):
    """our DSVT of a case, seeded as the generator seeded the reference's, in eval mode on the CPU"""
    from pdm_ssd_amd.backbones_3d.dsvt import DSVT
    net = DSVT(cfg_from_dict(dc.model_cfg(dc.CASES[name].get('model', name))))
    total = dc.fill(net)
    return net.eval(), total


def stage_coords(arrays, name, s):
    return torch.from_numpy(arrays[f'{name}.coords' if s == 0 else f'{name}.coords.{s}'])


def geometry(name, s):
    """(sparse shape, two windows, two shifts, set size) of stage s"""
    layer = dc.model_cfg(name)['INPUT_LAYER']
    shape = list(layer['sparse_shape'])
    for stride in layer['downsample_stride'][:s]:
        shape = [-(-shape[c] // stride[c]) for c in range(3)]
    w = layer['window_shape'][s]
    return shape, [w, [w[c] * layer['hybrid_factor'][c] for c in range(3)]], layer['shifts_list'][s], layer['set_info'][s][0]


def check_partition(arrays, name, s, part):
    for i in range(2):
        assert torch.equal(part.coors_in_win[i].long().cpu(), torch.from_numpy(arrays[f'{name}.ciw.{s}.{i}']).long()), (name, s, i)
        assert part.set_voxel_inds[i].dtype == torch.int64 and part.set_voxel_mask[i].dtype == torch.bool
        assert torch.equal(part.set_voxel_inds[i].cpu(), torch.from_numpy(arrays[f'{name}.inds.{s}.{i}']).long()), (name, s, i)
        assert torch.equal(part.set_voxel_mask[i].cpu(), torch.from_numpy(arrays[f'{name}.mask.{s}.{i}'])), (name, s, i)


@pytest.mark.parametrize('name', list(dc.CASES))
def test_state_dict_keys_and_shapes(name):
    _, manifest = load()
    net, total = build(name)
    meta = manifest['cases'][name]
    assert {k: list(v.shape) for k, v in net.state_dict().items()} == meta['state']
    assert abs(total - meta['weight_sum']) <= 1e-9 * max(1.0, abs(meta['weight_sum']))


@pytest.mark.parametrize('name', list(dc.CASES))
def test_set_partition_torch_is_the_reference_partition(name):
    arrays, manifest = load()
    assert np.array_equal(arrays[f'{name}.coords'], dc.coords(name))
    for s in range(dc.CASES[name].get('stages', 1)):
        part = dsvt_ops.set_partition_torch(stage_coords(arrays, name, s), *geometry(name, s))
        check_partition(arrays, name, s, part)
        assert [int(i.shape[1]) for i in part.set_voxel_inds] == manifest['cases'][name]['sets'][2 * s:2 * s + 2]


@pytest.mark.parametrize('name', list(dc.CASES))
def test_torch_path_is_within_the_parity_bound(name):
    arrays, manifest = load()
    net, _ = build(name)
    coords = torch.from_numpy(arrays[f'{name}.coords'])
    with torch.no_grad():
        out = net({'batch_size': dc.B, 'voxel_features': dc.features(name, len(coords)), 'voxel_coords': coords})
    want = arrays[f'{name}.out']
    err = float(np.abs(out['voxel_features'].numpy() - want).max())
    print(f'dsvt {name}: torch path |err| {err:.3e}, parity_abs {manifest["parity_abs"]:.1e}, '
          f'the reference\'s own fp32-to-fp64 gap {manifest["cases"][name]["float32_to_float64_gap"]:.3e}')
    assert out['pillar_features'] is out['voxel_features'] and out['voxel_features'].shape == want.shape
    assert err <= manifest['parity_abs']
    assert np.array_equal(out['voxel_coords'].numpy().astype(np.int64), arrays[f'{name}.out_coords'].astype(np.int64))


def test_training_mode_runs_the_differentiable_formulation():
    net, _ = build('b')
    net.train()
    coords = torch.from_numpy(dc.coords('b'))
    feats = dc.features('b', len(coords)).requires_grad_(True)
    out = net({'batch_size': dc.B, 'voxel_features': feats, 'voxel_coords': coords})['voxel_features']
    out.square().mean().backward()
    assert feats.grad is not None and bool(torch.isfinite(feats.grad).all()) and float(feats.grad.abs().max()) > 0
    assert all(p.grad is not None for n, p in net.named_parameters() if 'stage_0' in n)


def test_set_attention_torch_refuses_unsupported_sizes():
    inds = torch.zeros((1, 4), dtype=torch.long)
    for C, H, ss in ((40, 2, 4), (512, 16, 4), (32, 2, 129)):
        x = torch.zeros((3, C))
        with pytest.raises(ValueError):
            dsvt_ops.set_attention_torch(x, x, x, torch.zeros((1, ss), dtype=torch.long) if ss != 4 else inds, H)


@pytest.mark.parametrize('tag', list(dc.SCATTER_CASES))
def test_point_pillar_scatter_3d(tag):
    from pdm_ssd_amd.backbones_2d.map_to_bev import PointPillarScatter3d
    arrays, _ = load()
    c = dc.SCATTER_CASES[tag]
    rows, feats = dc.scatter_input(tag)
    m = PointPillarScatter3d(cfg_from_dict({'INPUT_SHAPE': list(c['shape']), 'NUM_BEV_FEATURES': c['C'] * c['shape'][2]}), None)
    out = m({'batch_size': dc.B, 'pillar_features': torch.from_numpy(feats), 'voxel_coords': torch.from_numpy(rows)})
    assert np.array_equal(out['spatial_features'].numpy(), arrays[f'scatter.{tag}'])


def test_base_bev_res_backbone():
    from pdm_ssd_amd.backbones_2d import BaseBEVResBackbone
    arrays, manifest = load()
    net = BaseBEVResBackbone(cfg_from_dict(dc.BEV_CFG), dc.BEV_INPUT[1])
    total = dc.fill(net)
    assert {k: list(v.shape) for k, v in net.state_dict().items()} == manifest['bev_state']
    assert abs(total - manifest['bev_weight_sum']) <= 1e-9 * max(1.0, abs(total))
    with torch.no_grad():
        out = net.eval()({'spatial_features': torch.from_numpy(dc.bev_input())})['spatial_features_2d'].numpy()
    assert out.shape == arrays['bev.out'].shape
    assert float(np.abs(out - arrays['bev.out']).max()) <= manifest['parity_abs']


def test_build_dsvt_pillar_constructs():
    from pdm_ssd_amd import detector_config
    net = detector_config.build_dsvt_pillar()
    names = [type(m).__name__ for m in (net.vfe, net.backbone_3d, net.map_to_bev_module, net.backbone_2d, net.dense_head)]
    assert names == ['DynamicPillarVFE', 'DSVT', 'PointPillarScatter3d', 'BaseBEVResBackbone', 'CenterHead']
    assert type(net).__name__ == 'CenterPoint' and net.backbone_3d.set_info == [[36, 4]]
    assert net.backbone_3d.stage_0[0].encoder_list[0].win_attn.self_attn.head_dim == 24

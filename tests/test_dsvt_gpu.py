"""DSVT on the GPU: the set partition operator, the fused set attention, the backbone's fused path and a small DSVT-Pillar detector.

Partition: exact equality, with the reference's partition in tests/golden/ref_dsvt.npz and with dsvt_ops.set_partition_torch on
random occupancies.

Set attention: err_fused <= 8 * err_torch, both maximum absolute errors against a float64 evaluation of
dsvt_ops.set_attention_torch on the CPU, err_torch the error of the same formulation in fp32 on the device with the same inputs.
The factor is the one test_attention_gpu.py and test_attention_train_gpu.py allow the other fused attention.  The ratios are
printed (DESIGN.md quotes them).

Backbone: the fused path within the manifest's parity_abs of the reference's features, a bound the generator wrote from the
reference's own fp32-to-fp64 gap.
"""
import copy
import ctypes

import numpy as np
import pytest
import torch

import dsvt_case as dc
import test_dsvt_host as host
from arena import Arena
from pdm_ssd_amd import _native, dsvt_ops
from pdm_ssd_amd.config import cfg_from_dict

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
FACTOR = 8.0


# ---- 1. the partition operator ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', list(dc.CASES))
def test_partition_is_the_reference_partition(name):
    arrays, manifest = host.load()
    for s in range(dc.CASES[name].get('stages', 1)):
        coords = host.stage_coords(arrays, name, s).to(DEV)
        part = dsvt_ops.set_partition(coords, dc.B, *host.geometry(name, s))
        assert part.coors_in_win.dtype == torch.int32
        host.check_partition(arrays, name, s, part)
        again = dsvt_ops.set_partition(coords, dc.B, *host.geometry(name, s))
        for a, b in zip(part.set_voxel_inds + part.set_voxel_mask, again.set_voxel_inds + again.set_voxel_mask):
            assert torch.equal(a, b)


def random_coords(seed, B, shape, density, empty=None):
    rng = np.random.default_rng(seed)
    sx, sy, sz = shape
    occ = rng.random((B, sz, sy, sx)) < density
    if empty is not None:
        occ[empty] = False
    rows = np.argwhere(occ).astype(np.int32)
    return torch.from_numpy(rows[rng.permutation(len(rows))])


RANDOM = {
    # name: (B, sparse shape, windows, shifts, set size, coords)
    'dense 2-d, windows that do not divide the grid': (3, (37, 23, 1), [[5, 4, 1], [10, 8, 1]], [[0, 0, 0], [2, 3, 0]], 7, dict(density=0.6)),
    'sparse 3-d, several scan tiles of bitmap groups and of windows': (2, (130, 126, 5), [[3, 3, 2], [6, 6, 2]], [[0, 0, 0], [1, 2, 1]], 36,
                                                                       dict(density=0.02)),
    'an empty sample in the middle': (3, (30, 30, 1), [[6, 6, 1], [12, 12, 1]], [[0, 0, 0], [6, 6, 0]], 5, dict(density=0.3, empty=1)),
    'a set size above the window': (1, (16, 16, 1), [[4, 4, 1], [8, 8, 1]], [[0, 0, 0], [4, 4, 0]], 90, dict(density=0.9)),
    'set size 1': (2, (16, 12, 2), [[4, 4, 2], [8, 8, 2]], [[0, 0, 0], [2, 2, 0]], 1, dict(density=0.4)),
}


@pytest.mark.parametrize('name', list(RANDOM))
def test_partition_equals_the_torch_formulation(name):
    B, shape, windows, shifts, ss, kw = RANDOM[name]
    coords = random_coords(len(name), B, shape, **kw)
    want = dsvt_ops.set_partition_torch(coords, shape, windows, shifts, ss)
    got = dsvt_ops.set_partition(coords.to(DEV), B, shape, windows, shifts, ss)
    assert torch.equal(got.coors_in_win.long().cpu(), want.coors_in_win)
    for i in range(2):
        assert torch.equal(got.set_voxel_inds[i].cpu(), want.set_voxel_inds[i]), (name, i)
        assert torch.equal(got.set_voxel_mask[i].cpu(), want.set_voxel_mask[i]), (name, i)


@pytest.mark.parametrize('n', [0, 1])
def test_partition_of_one_voxel_and_of_none(n):
    coords = torch.tensor([[1, 0, 27, 39]], dtype=torch.int32)[:n]
    geo = ((40, 28, 1), [[6, 6, 1], [12, 12, 1]], [[0, 0, 0], [3, 3, 0]], 12)
    got = dsvt_ops.set_partition(coords.to(DEV), 2, *geo)
    want = dsvt_ops.set_partition_torch(coords, *geo)
    for i in range(2):
        assert got.set_voxel_inds[i].shape == (2, n, 12)
        assert torch.equal(got.set_voxel_inds[i].cpu(), want.set_voxel_inds[i]) and torch.equal(got.set_voxel_mask[i].cpu(), want.set_voxel_mask[i])
    if n:
        assert not got.set_voxel_inds[0].any() and bool(got.set_voxel_mask[0][:, :, 1:].all()) and not got.set_voxel_mask[0][:, :, 0].any()


def test_partition_refusals():
    geo = ((40, 28, 1), [[6, 6, 1], [12, 12, 1]], [[0, 0, 0], [3, 3, 0]])
    good = torch.from_numpy(dc.coords('a')).to(DEV)
    for row in ([0, 0, 28, 3], [0, 1, 3, 3], [2, 0, 3, 3], [0, 0, 3, 40], [0, 0, -1, 3]):
        bad = good.clone()
        bad[5] = torch.tensor(row, dtype=torch.int32)
        with pytest.raises(_native.NativeLibraryError, match='code -1.*outside the sparse shape'):
            dsvt_ops.set_partition(bad, dc.B, *geo, 12)
    with pytest.raises(_native.NativeLibraryError, match='set_size'):
        dsvt_ops.set_partition(good, dc.B, *geo, 0)
    # a workspace sized for 6 x 6 and 12 x 12 windows does not hold the bitmap of windows sixteen times the volume
    lib = _native.lib()
    sized_for = lib.pdm_dsvt_partition_workspace_bytes(len(good), dc.B, 40, 28, 1, _native.host_array(ctypes.c_int, [6, 6, 1, 12, 12, 1]))
    large = ((40, 28, 1), [[24, 24, 1], [48, 48, 1]], [[0, 0, 0], [3, 3, 0]])
    assert 0 < sized_for < lib.pdm_dsvt_partition_workspace_bytes(len(good), dc.B, 40, 28, 1, _native.host_array(ctypes.c_int, [24, 24, 1, 48, 48, 1]))
    with pytest.raises(_native.NativeLibraryError, match='window volumes'):
        dsvt_ops.set_partition(good, dc.B, *large, 12, workspace=torch.empty(sized_for, dtype=torch.uint8, device=DEV))
    # the C entry refuses by itself, before any launch
    rc = lib.pdm_dsvt_partition_count(None, 4, None, 2, 40, 28, 1, None, None, 12, None, None, None, 0)
    assert rc == -1 and b'null pointer' in lib.pdm_last_error()
    assert lib.pdm_dsvt_partition_workspace_bytes(4, 2, 40, 28, 0, _native.host_array(ctypes.c_int, [6, 6, 1, 12, 12, 1])) == 0


@pytest.mark.parametrize('off', [0, 4, 12])
def test_partition_in_a_poisoned_arena(off):
    name = 'c'
    shape, windows, shifts, ss = host.geometry(name, 0)
    coords0 = torch.from_numpy(dc.coords(name))
    want = dsvt_ops.set_partition_torch(coords0, shape, windows, shifts, ss)
    N = len(coords0)
    arena = Arena(DEV, nbytes=8 << 20)
    coords = arena.put(coords0, off, poison=[0, 0, 0, 0])            # a stray read finds an in-range voxel
    lib = _native.lib()
    win = _native.host_array(ctypes.c_int, [v for w in windows for v in w])
    sh = _native.host_array(ctypes.c_int, [v for h in shifts for v in h])
    nbytes = lib.pdm_dsvt_partition_workspace_bytes(N, dc.B, *shape, win)
    ws = arena.carve(nbytes, torch.uint8, 8)
    ws.fill_(0xFF)                                                     # nothing relies on what a workspace held
    ciw = arena.carve((2, N, 3), torch.int32, (off + 4) % 16)
    counts = _native.host_array(ctypes.c_int, [0, 0])
    geom = (N, coords.data_ptr(), dc.B, *shape, win, sh, ss)
    _native.call('pdm_dsvt_partition_count', _native.stream(coords), *geom, ciw.data_ptr(), counts, ws.data_ptr(), nbytes)
    S = [int(counts[0]), int(counts[1])]
    assert S == [int(i.shape[1]) for i in want.set_voxel_inds]
    inds = [arena.carve((2, s, ss), torch.int64, 8 if off else 0) for s in S]
    mask = [arena.carve((2, s, ss), torch.uint8, (off + 1) % 16) for s in S]
    _native.call('pdm_dsvt_partition', _native.stream(coords), *geom, S[0], S[1], inds[0].data_ptr(), mask[0].data_ptr(), inds[1].data_ptr(),
                 mask[1].data_ptr(), ws.data_ptr(), nbytes)
    assert torch.equal(ciw.long().cpu(), want.coors_in_win)
    for i in range(2):
        assert torch.equal(inds[i].cpu(), want.set_voxel_inds[i]) and torch.equal(mask[i].bool().cpu(), want.set_voxel_mask[i])
    arena.check()


# ---- 2. the fused set attention --------------------------------------------------------------------------------------------------------
SHAPES = [(12, 48, 2), (36, 192, 8), (90, 128, 8), (20, 32, 2), (1, 32, 2), (128, 256, 8)]
SETS = [1, 3, 130]


def sets_of(S, ss, seed):
    """(set_voxel_inds (S, ss), N): set s holds n_s distinct voxels of its own, slot k the voxel floor(k n_s / ss) of them, as the
    partition builds them.  Set 0 (of 3 and 130) is all duplicates of one voxel, set 1 has none; a single set has none."""
    rng = np.random.default_rng(seed)
    n = rng.integers(1, ss + 1, S)
    if S == 1:
        n[0] = ss
    else:
        n[0], n[1] = 1, ss
    base = np.concatenate([[0], np.cumsum(n)])
    perm = rng.permutation(int(base[-1]))                              # the voxels' rows in any order
    inds = np.stack([perm[base[s] + (np.arange(ss) * n[s]) // ss] for s in range(S)])
    return torch.from_numpy(inds.astype(np.int64)), int(base[-1])


def attention_inputs(S, ss, C, seed):
    inds, N = sets_of(S, ss, seed)
    qkv = torch.randn((N, 3 * C), generator=torch.Generator().manual_seed(seed + 1))
    return inds, N, qkv


_reference = {}


def reference64(S, ss, C, H, seed):
    """the float64 evaluation on the CPU, computed once a shape and left unchanged"""
    key = (S, ss, C, H, seed)
    if key not in _reference:
        inds, N, qkv = attention_inputs(S, ss, C, seed)
        q, k, v = (qkv[:, i * C:(i + 1) * C].double() for i in range(3))
        _reference[key] = dsvt_ops.set_attention_torch(q, k, v, inds, H)
    return _reference[key]


@pytest.mark.parametrize('S', SETS)
@pytest.mark.parametrize('ss, C, H', SHAPES)
def test_set_attention_against_float64(ss, C, H, S):
    seed = 1000 + 7 * ss + S
    inds, N, qkv = attention_inputs(S, ss, C, seed)
    want = reference64(S, ss, C, H, seed)
    qkv_d, inds_d = qkv.to(DEV), inds.to(DEV)
    q, k, v = (qkv_d[:, i * C:(i + 1) * C] for i in range(3))          # strided: the thirds of one (N, 3C) tensor
    out = torch.full((N, C), float('nan'), device=DEV)
    got = dsvt_ops.set_attention(q, k, v, inds_d, H, out=out)
    assert got.data_ptr() == out.data_ptr()
    assert not bool(torch.isnan(got).any()), 'a row of out was not written'
    base = dsvt_ops.set_attention_torch(q, k, v, inds_d, H)
    err_fused = float((got.double().cpu() - want).abs().max())
    err_torch = float((base.double().cpu() - want).abs().max())
    print(f'set attention ss {ss} C {C} H {H} S {S}: err_fused {err_fused:.3e} err_torch {err_torch:.3e} ratio {err_fused / max(err_torch, 1e-300):.3f}')
    assert err_fused <= FACTOR * err_torch
    # contiguous operands give the same bits as the strided ones, and a second run the same as the first
    again = dsvt_ops.set_attention(q.contiguous(), k.contiguous(), v.contiguous(), inds_d, H)
    assert torch.equal(again, got)
    if ss > 1 and S > 1:                                               # set 0 is one voxel ss times: its row is its own v row
        assert torch.equal(got[inds_d[0, 0]], v[inds_d[0, 0]])


def test_set_attention_refuses_unsupported_sizes():
    inds = torch.zeros((1, 4), dtype=torch.long, device=DEV)
    for C, H, ss in ((40, 2, 4), (16, 2, 4), (512, 16, 4), (32, 2, 129)):
        x = torch.zeros((3, C), device=DEV)
        with pytest.raises(ValueError):
            dsvt_ops.set_attention(x, x, x, torch.zeros((1, ss), dtype=torch.long, device=DEV) if ss != 4 else inds, H)
    lib = _native.lib()
    for C, H, ss in ((40, 2, 4), (512, 16, 4), (32, 2, 129), (32, 2, 0)):
        assert lib.pdm_set_attention(None, 1, ss, 3, C, H, None, C, None, C, None, C, None, None) == -1
        assert b'set_size' in lib.pdm_last_error()
    assert lib.pdm_set_attention(None, 1, 4, 3, 32, 2, None, 16, None, 32, None, 32, None, None) == -1 and b'stride' in lib.pdm_last_error()
    x = torch.zeros((3, 32), device=DEV)
    with pytest.raises(ValueError, match='strides'):
        dsvt_ops.set_attention(x.t().contiguous().t(), x, x, inds, 2)


def test_set_attention_graph_replay_gives_the_eager_bits():
    ss, C, H, S = 36, 192, 8, 130
    inds, N, qkv = attention_inputs(S, ss, C, 77)
    qkv, inds = qkv.to(DEV), inds.to(DEV)
    q, k, v = (qkv[:, i * C:(i + 1) * C] for i in range(3))
    eager = dsvt_ops.set_attention(q, k, v, inds, H)                   # (the warm-up call as well)
    out = torch.zeros((N, C), device=DEV)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        dsvt_ops.set_attention(q, k, v, inds, H, out=out)
    out.fill_(float('nan'))
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)


@pytest.mark.parametrize('off', [4, 8, 12])
def test_set_attention_in_a_poisoned_arena(off):
    ss, C, H, S = 20, 48, 2, 37                                        # d = 24, a partly filled second tile
    inds0, N, qkv0 = attention_inputs(S, ss, C, 91)
    want = dsvt_ops.set_attention(*(qkv0[:, i * C:(i + 1) * C].to(DEV).contiguous() for i in range(3)), inds0.to(DEV), H)
    arena = Arena(DEV, nbytes=8 << 20)
    nan = float('nan')
    q, k, v = (arena.put(qkv0[:, i * C:(i + 1) * C].contiguous(), (off + 4 * i) % 16, nan) for i in range(3))
    inds = arena.put(inds0, 8, poison=[0])
    out = arena.carve((N, C), torch.float32, off)
    got = dsvt_ops.set_attention(q, k, v, inds, H, out=out)
    assert torch.equal(got, want)
    arena.check()


# ---- 3. the backbone -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', list(dc.CASES))
def test_backbone_fused_path(name):
    arrays, manifest = host.load()
    net, _ = host.build(name)
    net = net.to(DEV)
    coords = torch.from_numpy(arrays[f'{name}.coords']).to(DEV)
    feats = dc.features(name, len(coords)).to(DEV)
    want = arrays[f'{name}.out']
    outs = {}
    for fused in (True, False):
        net.use_fused = fused
        reads = dsvt_ops.HOST_READS
        with torch.no_grad():
            out = net({'batch_size': dc.B, 'voxel_features': feats.clone(), 'voxel_coords': coords.clone()})
        assert dsvt_ops.HOST_READS - reads == (dc.CASES[name].get('stages', 1) if fused else 0)      # one host read a stage
        outs[fused] = out['voxel_features'].cpu().numpy()
        assert np.array_equal(out['voxel_coords'].cpu().numpy().astype(np.int64), arrays[f'{name}.out_coords'].astype(np.int64))
    err = {f: float(np.abs(o - want).max()) for f, o in outs.items()}
    print(f'dsvt {name}: |fused - reference| {err[True]:.3e}, |torch - reference| {err[False]:.3e}, '
          f'|fused - torch| {float(np.abs(outs[True] - outs[False]).max()):.3e}, parity_abs {manifest["parity_abs"]:.1e}')
    assert err[True] <= manifest['parity_abs'] and err[False] <= manifest['parity_abs']
    assert float(np.abs(outs[True] - outs[False]).max()) <= manifest['parity_abs']


# ---- 4. the detector -------------------------------------------------------------------------------------------------------------------
def small_detector(seed):
    """build_dsvt_pillar with 48 channels in 2 heads on a 96 x 96 grid of 0.2 m pillars, every parameter and BatchNorm statistic
    seeded by dsvt_case.fill (unit-gain matrices: with the constructors' initialisation the heat-map is flat)"""
    from pdm_ssd_amd import detector_config
    cfg = copy.deepcopy(detector_config.DSVT_PILLAR_CFG)
    cfg['VFE']['NUM_FILTERS'] = [48, 48]
    b3 = cfg['BACKBONE_3D']
    b3['INPUT_LAYER'].update(sparse_shape=[96, 96, 1], d_model=[48], set_info=[[36, 2]])
    b3.update(set_info=[[36, 2]], d_model=[48], nhead=[2], dim_feedforward=[96], output_shape=[96, 96], conv_out_channel=48)
    cfg['MAP_TO_BEV'].update(INPUT_SHAPE=[96, 96, 1], NUM_BEV_FEATURES=48)
    cfg['BACKBONE_2D'] = {'NAME': 'BaseBEVResBackbone', 'LAYER_NUMS': [1, 1], 'LAYER_STRIDES': [1, 2], 'NUM_FILTERS': [32, 64],
                          'UPSAMPLE_STRIDES': [1, 2], 'NUM_UPSAMPLE_FILTERS': [32, 32]}
    cfg['DENSE_HEAD']['POST_PROCESSING'].update(SCORE_THRESH=0.0, POST_CENTER_LIMIT_RANGE=[-20.0, -20.0, -10.0, 20.0, 20.0, 10.0])
    ds = detector_config.dsvt_dataset(4, [-9.6, -9.6, -3.0, 9.6, 9.6, 3.0], [0.2, 0.2, 6.0], [96, 96, 1])
    net = detector_config.build_dsvt_pillar(cfg, dataset=ds)
    dc.fill(net, seed)
    return net.to(DEV).eval()


def synthetic_points(seed, B=2, n=6000):
    rng = np.random.default_rng(seed)
    rows = []
    for b in range(B):
        xy = rng.uniform(-9.5, 9.5, (n, 2))
        z = np.clip(-1.0 + 1.2 * np.sin(0.9 * xy[:, 0]) * np.cos(0.7 * xy[:, 1]) + rng.normal(0, 0.15, n), -2.8, 2.8)
        rows.append(np.concatenate([np.full((n, 1), b), xy, z[:, None], rng.uniform(0, 1, (n, 1))], 1))
    return torch.from_numpy(np.concatenate(rows).astype(np.float32)).to(DEV)


def test_detector_returns_boxes_and_the_two_paths_agree():
    net = small_detector(5)
    pts = synthetic_points(5)
    res = {}
    for fused in (False, True):
        net.backbone_3d.use_fused = fused
        with torch.no_grad():
            res[fused], _ = net({'batch_size': 2, 'points': pts.clone()})
    assert len(res[True]) == 2
    for f, p in zip(res[True], res[False]):
        n = len(f['pred_boxes'])
        assert n > 0 and f['pred_boxes'].shape == (n, 7)
        assert int(f['pred_labels'].min()) >= 1 and int(f['pred_labels'].max()) <= 3
        assert torch.equal(f['pred_labels'], p['pred_labels'])
        # the backbones' features agree within the fixture's parity_abs = 2e-5; behind them lie a dozen unit-gain convolutions
        # (each may double a perturbation's maximum at the worst) and the decode, whose sizes pass through exp: 50 x for the
        # boxes; a score is a sigmoid, slope <= 1 / 4
        d_box = float((f['pred_boxes'] - p['pred_boxes']).abs().max())
        d_score = float((f['pred_scores'] - p['pred_scores']).abs().max())
        print(f'dsvt detector: {n} boxes, |boxes| {d_box:.3e}, |scores| {d_score:.3e}')
        assert d_box <= 1e-3 and d_score <= 2.5e-4

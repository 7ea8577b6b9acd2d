"""The DSVT cases shared by tests/golden/gen_dsvt_fixtures.py (which runs the reference on them) and the DSVT tests: the
configs, the hand-placed occupancies, the seeded inputs and the seeded fill of every parameter and BatchNorm statistic.
No weights are stored anywhere: both sides call fill() on modules with the same state_dict keys.  A helper module like
transfusion_case.py: no tests here.

Cases
  a         2-D, B = 2, sparse shape 40 x 28 x 1, C = 48, 2 heads (d = 24), set size 12, window 6 x 6 x 1, hybrid 2 x 2 x 1,
            shifts [0, 0, 0] and [3, 3, 0], 2 blocks
  a_empty   case a's model on a second input whose sample 0 has no voxel at all
  b         d = 16: C = 32, 2 heads, set size 20
  c         3-D: sparse shape 24 x 20 x 4, window 6 x 6 x 2 (does not span z; the position embedding has 3 inputs), shift
            [3, 3, 1], C = 48, set size 16
  d_linear, d_maxpool, d_attention   two stages of one block with downsample_stride [[2, 2, 1]], once per reduction type

Sample 1 of every occupancy is placed by hand: under shift 0 its windows (0, 0), (1, 0), (2, 0), (3, 0) hold exactly 1, ss,
min(3 ss, the window) and ss + 1 voxels; the rest of both samples is a seeded scatter.
"""
import numpy as np
import torch

SEED = 20
CASES = {
    'a': dict(shape=(40, 28, 1), C=48, H=2, ss=12, window=(6, 6, 1), shift=(3, 3, 0), blocks=2, density=0.16),
    'a_empty': dict(shape=(40, 28, 1), C=48, H=2, ss=12, window=(6, 6, 1), shift=(3, 3, 0), blocks=2, density=0.16, empty=0, model='a'),
    'b': dict(shape=(40, 28, 1), C=32, H=2, ss=20, window=(6, 6, 1), shift=(3, 3, 0), blocks=2, density=0.16),
    'c': dict(shape=(24, 20, 4), C=48, H=2, ss=16, window=(6, 6, 2), shift=(3, 3, 1), blocks=2, density=0.07),
    'd_linear': dict(shape=(40, 28, 1), C=48, H=2, ss=12, window=(6, 6, 1), shift=(3, 3, 0), blocks=1, density=0.16, stages=2, reduction='linear'),
    'd_maxpool': dict(shape=(40, 28, 1), C=48, H=2, ss=12, window=(6, 6, 1), shift=(3, 3, 0), blocks=1, density=0.16, stages=2, reduction='maxpool'),
    'd_attention': dict(shape=(40, 28, 1), C=48, H=2, ss=12, window=(6, 6, 1), shift=(3, 3, 0), blocks=1, density=0.16, stages=2,
                        reduction='attention'),
}
SINGLE_STAGE = ('a', 'a_empty', 'b', 'c')
B = 2


def model_cfg(name):
    """the DSVT model_cfg of a case, a plain dict (wrap it in the config class of whoever builds the module)"""
    c = CASES[name]
    stages = c.get('stages', 1)
    return {
        'NAME': 'DSVT',
        'INPUT_LAYER': {'sparse_shape': list(c['shape']), 'downsample_stride': [[2, 2, 1]] * (stages - 1), 'd_model': [c['C']] * stages,
                        'set_info': [[c['ss'], c['blocks']]] * stages, 'window_shape': [list(c['window'])] * stages,
                        'hybrid_factor': [2, 2, 1], 'shifts_list': [[[0, 0, 0], list(c['shift'])]] * stages, 'normalize_pos': False},
        'block_name': ['DSVTBlock'] * stages, 'set_info': [[c['ss'], c['blocks']]] * stages, 'd_model': [c['C']] * stages,
        'nhead': [c['H']] * stages, 'dim_feedforward': [2 * c['C']] * stages, 'dropout': 0.0, 'activation': 'gelu',
        'reduction_type': c.get('reduction', 'attention'), 'output_shape': [c['shape'][1], c['shape'][0]], 'conv_out_channel': c['C'],
    }


def hand_counts(name):
    c = CASES[name]
    volume = c['window'][0] * c['window'][1] * c['window'][2]
    return [1, c['ss'], min(3 * c['ss'], volume), c['ss'] + 1]


def coords(name):
    """(N, 4) int32 rows (b, z, y, x), distinct, in a seeded random row order"""
    c = CASES[name]
    sx, sy, sz = c['shape']
    wx, wy, wz = c['window']
    rng = np.random.default_rng(SEED + sorted(CASES).index(name))
    occ = rng.random((B, sz, sy, sx)) < c['density']
    occ[1, :wz, :wy, :4 * wx] = False                                   # the four hand-placed windows of sample 1
    for g, n in enumerate(hand_counts(name)):
        cells = [(z, y, g * wx + x) for y in range(wy) for x in range(wx) for z in range(wz)][:n]
        for z, y, x in cells:
            occ[1, z, y, x] = True
    if 'empty' in c:
        occ[c['empty']] = False
    rows = np.argwhere(occ).astype(np.int32)
    return rows[rng.permutation(len(rows))]


def features(name, n):
    c = CASES[name]
    g = torch.Generator().manual_seed(SEED + 100 + sorted(CASES).index(name))
    return torch.randn((n, c['C']), generator=g)


def fill(module, seed=SEED):
    """Every floating entry of module.state_dict(), in sorted key order, from one seeded generator: matrices normal with
    standard deviation 1 / sqrt(fan-in), BatchNorm variances in [0.5, 1.5], other vectors named weight 1 + 0.1 normal, the rest
    0.1 normal.  Returns the sum of all values in float64 (the manifest's check sum)."""
    g = torch.Generator().manual_seed(seed)
    total = 0.0
    state = module.state_dict()
    with torch.no_grad():
        for key in sorted(state):
            t = state[key]
            if not t.is_floating_point():
                continue
            r = torch.randn(t.shape, generator=g, dtype=torch.float32)
            if key.endswith('running_var'):
                v = 0.5 + torch.rand(t.shape, generator=g, dtype=torch.float32)
            elif t.dim() > 1:
                v = r / float(np.sqrt(t.shape[-1] if t.dim() == 2 else np.prod(t.shape[1:])))
            elif key.endswith('weight'):
                v = 1.0 + 0.1 * r
            else:
                v = 0.1 * r
            t.copy_(v.to(t.dtype))
            total += float(v.double().sum())
    return total


# the small reference-run pieces around the backbone
SCATTER_CASES = {'nz1': dict(shape=(9, 7, 1), C=4), 'nz2': dict(shape=(9, 7, 2), C=3)}
BEV_CFG = {'LAYER_NUMS': [1, 1], 'LAYER_STRIDES': [1, 2], 'NUM_FILTERS': [8, 16], 'UPSAMPLE_STRIDES': [1, 2], 'NUM_UPSAMPLE_FILTERS': [8, 8]}
BEV_INPUT = (2, 6, 12, 16)


def scatter_input(tag):
    c = SCATTER_CASES[tag]
    nx, ny, nz = c['shape']
    rng = np.random.default_rng(SEED + 50 + nz)
    occ = rng.random((B, nz, ny, nx)) < 0.3
    rows = np.argwhere(occ).astype(np.int32)
    rows = rows[rng.permutation(len(rows))]
    feats = rng.standard_normal((len(rows), c['C'])).astype(np.float32)
    return rows, feats


def bev_input():
    return np.random.default_rng(SEED + 60).standard_normal(BEV_INPUT).astype(np.float32)

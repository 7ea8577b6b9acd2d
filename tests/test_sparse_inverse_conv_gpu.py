"""spconv.SparseInverseConv3d (pdm_sparse_conv over the transposed table of the paired strided convolution) against the numpy
restatement of tests/part_a2_reference.py.

Geometries: B = 2 with sample 1 empty on the grid (D, H, W) = (5, 6, 7), kernel 3, stride 2, padding (0, 1, 1) (spconv4's
asymmetric case), and kernel (3, 1, 1), stride (2, 1, 1), no padding.  Channels 64 -> 32 and 16 -> 16.

Exact: the output indices (the paired convolution's input rows, row for row) and grid; two runs.
Bounded: the values, by the bound tests/test_sparse_conv_gpu.py holds pdm_sparse_conv to (it is the same kernel):
|err| <= 2 n 2^-24 A, n = kvol Cin, A the float64 inverse convolution of |x| with |w| (times |scale| when a norm is folded), plus
the one rounding of the epilogue's multiply-add, 2^-24 |y scale + shift|.  ReLU is 1-Lipschitz and keeps the bound.
"""
import numpy as np
import pytest
import torch
import torch.nn as nn

import part_a2_reference as par
import sparse_conv_reference as scr
from arena import Arena
from pdm_ssd_amd import spconv

pytestmark = pytest.mark.gpu
SHAPE, B = (5, 6, 7), 2
GEOS = {'k3s2p011': ((3, 3, 3), (2, 2, 2), (0, 1, 1)), 'k311s211p0': ((3, 1, 1), (2, 1, 1), (0, 0, 0))}
U = 2.0 ** -24


@pytest.fixture(scope="module")
def arena(dev):
    return Arena(dev)


def sites(seed):
    """a shuffled 60 % of sample 0's cells; sample 1 stays empty"""
    rng = np.random.default_rng(seed)
    D, H, W = SHAPE
    cells = np.stack(np.meshgrid(np.arange(D), np.arange(H), np.arange(W), indexing='ij'), -1).reshape(-1, 3)
    keep = rng.permutation(len(cells))[: int(0.6 * len(cells))]
    return np.concatenate([np.zeros((len(keep), 1), dtype=np.int64), cells[keep]], 1).astype(np.int32)


def build(dev, arena, geo, cin, cout, seed):
    """the paired convolution (8 -> cin) run on the device, then the inverse layer cin -> cout"""
    kernel, stride, padding = GEOS[geo]
    rng = np.random.default_rng(seed)
    idx = sites(seed)
    arena.reset()
    feats = arena.put(rng.uniform(-1, 1, (len(idx), 16)).astype(np.float32), misalign_bytes=4, poison=float('nan'))
    x0 = spconv.SparseConvTensor(feats, torch.from_numpy(idx).to(dev), SHAPE, B)
    torch.manual_seed(seed)
    down = spconv.SparseConv3d(16, cin, kernel, stride=stride, padding=padding, bias=False, indice_key='down').to(dev).eval()
    inv = spconv.SparseInverseConv3d(cin, cout, kernel, indice_key='down', bias=True).to(dev).eval()
    with torch.no_grad():
        y = down(x0)
    return idx, x0, y, inv


@pytest.mark.parametrize("cin, cout", [(64, 32), (16, 16)])
@pytest.mark.parametrize("geo", list(GEOS))
def test_inverse_conv_rows_and_values(dev, arena, geo, cin, cout):
    kernel, stride, padding = GEOS[geo]
    idx, x0, y, inv = build(dev, arena, geo, cin, cout, seed=cin + cout)
    out_idx, nbr, oshape = scr.rulebook(idx, B, SHAPE, kernel, stride, padding, False)
    assert np.array_equal(y.indices.cpu().numpy(), out_idx) and tuple(y.spatial_shape) == tuple(oshape)
    assert 0 < len(out_idx) < len(idx)
    with torch.no_grad():
        z = inv(y)
        z2 = inv(y)
    torch.cuda.synchronize()
    arena.check()
    # rows: the paired convolution's input indices, row for row, on its input grid
    assert torch.equal(z.indices, x0.indices) and list(z.spatial_shape) == list(SHAPE) and z.batch_size == B
    assert torch.equal(z.features, z2.features), 'two runs differ'
    assert ('down', 'nbr_t') in y.indice_dict, 'the transposed table is kept under the slot the data gradient uses'
    yx, w, bias = y.features.cpu().numpy(), inv.weight.detach().cpu().numpy(), inv.bias.detach().cpu().numpy().astype(np.float64)
    want = par.inverse_conv_reference(yx, nbr, w, len(idx))
    A = par.inverse_conv_reference(np.abs(yx), nbr, np.abs(w), len(idx))
    n = kernel[0] * kernel[1] * kernel[2] * cin
    got = z.features.cpu().numpy()
    assert got.shape == (len(idx), cout)
    ratio = np.abs(got - (want + bias)) / (2 * n * U * A + U * np.abs(want + bias) + 1e-300)
    print(geo, cin, cout, 'rows', len(idx), '<-', len(out_idx), 'max err / bound', float(ratio.max()))
    assert np.isfinite(got).all() and (ratio <= 1.0).all()
    # rows no output site reads stay at the bias
    unread = np.setdiff1d(np.arange(len(idx)), nbr[nbr >= 0])
    assert np.array_equal(got[unread], np.broadcast_to(inv.bias.detach().cpu().numpy(), (len(unread), cout)))


@pytest.mark.parametrize("geo", list(GEOS))
def test_inverse_conv_folds_norm_and_relu_in_a_sequential(dev, arena, geo):
    kernel, stride, padding = GEOS[geo]
    cin, cout = 64, 32
    idx, x0, y, inv = build(dev, arena, geo, cin, cout, seed=7)
    _, nbr, _ = scr.rulebook(idx, B, SHAPE, kernel, stride, padding, False)
    bn = nn.BatchNorm1d(cout, eps=1e-3).to(dev)
    rng = np.random.default_rng(11)
    with torch.no_grad():
        bn.weight.copy_(torch.from_numpy(rng.uniform(0.5, 1.5, cout) * rng.choice([-1, 1], cout)).float())
        bn.bias.copy_(torch.from_numpy(rng.uniform(-0.5, 0.5, cout)).float())
        bn.running_mean.copy_(torch.from_numpy(rng.uniform(-0.2, 0.2, cout)).float())
        bn.running_var.copy_(torch.from_numpy(rng.uniform(0.5, 2.0, cout)).float())
    seq = spconv.SparseSequential(inv, bn, nn.ReLU()).eval()
    with torch.no_grad():
        z = seq(y)
    assert torch.equal(z.indices, x0.indices)
    yx, w = y.features.cpu().numpy(), inv.weight.detach().cpu().numpy()
    raw = par.inverse_conv_reference(yx, nbr, w, len(idx))
    A = par.inverse_conv_reference(np.abs(yx), nbr, np.abs(w), len(idx))
    # the (scale, shift) the launch is handed: conv bias -> eval BatchNorm as one multiply-add, folded in fp32 on the device
    with torch.no_grad():
        sc, sh = (t.cpu().numpy().astype(np.float64) for t in spconv.fold_norm(bn, inv.bias, cout, inv.weight))
    post = raw * sc + sh
    n = kernel[0] * kernel[1] * kernel[2] * cin
    bound = 2 * n * U * A * np.abs(sc) + U * np.abs(post)          # test_sparse_conv_gpu.check_conv's 'bn_relu' bound
    got = z.features.cpu().numpy()
    ratio = np.abs(got - np.maximum(post, 0)) / bound
    print(geo, 'bn + relu: max err / bound', float(ratio.max()))
    assert (got >= 0).all() and (ratio <= 1.0).all()


def test_inverse_conv_refuses_a_missing_key_a_subm_rulebook_and_the_grad_path(dev, arena):
    idx, x0, y, inv = build(dev, arena, 'k3s2p011', 16, 16, seed=3)
    with torch.no_grad():
        other = spconv.SparseInverseConv3d(16, 16, 3, indice_key='absent').to(dev).eval()
        with pytest.raises(KeyError, match='absent'):
            other(y)
        subm = spconv.SubMConv3d(16, 16, 3, padding=1, bias=False, indice_key='subm').to(dev).eval()
        t = subm(y)
        wrong = spconv.SparseInverseConv3d(16, 16, 3, indice_key='subm').to(dev).eval()
        with pytest.raises(AssertionError, match='submanifold'):
            wrong(t)
        thin = spconv.SparseInverseConv3d(16, 16, (3, 1, 1), indice_key='down').to(dev).eval()
        with pytest.raises(AssertionError, match='kernel'):
            thin(y)
    with pytest.raises(NotImplementedError):
        inv.train()(y)

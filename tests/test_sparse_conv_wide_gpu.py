"""The sparse convolution up to 256 channels on the device (pdm_sparse_conv_wide, pdm_sparse_conv_wide_split,
pdm_sparse_conv_wide_wgrad) and the 2-D layer over it (spconv.SubMConv2d, SparseConv2d), on the depth-1 geometries of
tests/pillarnet_reference.py.  Operator inputs and outputs are carved from a poisoned Arena, 4 bytes off a 16-byte boundary:
features between NaN red zones, tables between in-range values.

Exact: the wide entries against the narrow ones where both serve (same sizes; the column halves of Cout = 256; Cin = 256 with a zero
upper half); two runs of everything; a graph replay; the strided 2-D layer's sites; dense().
Bounded: test_sparse_conv_gpu.check_conv's bound restated, |err| <= 2 n 2^-24 A with n = kvol Cin and A the float64 convolution of
|x| with |w| (plus the epilogue's roundings); test_sparse_conv_grad_gpu's |dx err| <= 2 kvol Cout 2^-24 A_dx and per offset
|dW err| <= 2 max(n_k, 1) 2^-24 A_dW.
"""
import numpy as np
import pytest
import torch

import pillarnet_reference as pnr
from arena import Arena
from pdm_ssd_amd import _native, sparse_conv_ops, spconv

pytestmark = pytest.mark.gpu
U = 2.0 ** -24
GEOS = list(pnr.GEOMETRIES_2D)


@pytest.fixture(scope="module")
def arena(dev):
    return Arena(dev)


@pytest.fixture(scope="module")
def books():
    """the numpy rulebooks of the full site list, one per geometry, computed once"""
    idx = pnr.p2_indices()
    return idx, {name: pnr.book(idx, name) for name in GEOS}


def put(arena, src, misalign_bytes=0, poison=None):
    src = torch.as_tensor(src)
    return arena.put(src, misalign_bytes, poison) if src.numel() else src.to(arena.buf.device)


def carve(arena, shape, dtype, misalign_bytes=0):
    return arena.carve(shape, dtype, misalign_bytes) if int(np.prod(shape)) else torch.empty(shape, dtype=dtype, device=arena.buf.device)


# ---- forward ------------------------------------------------------------------------------------------------------------------
def run_conv(arena, x, nbr, w, scale=None, shift=None, res=None, relu=False, split=False, wide=True):
    """one launch on arena views; w (Cout, kz, ky, kx, Cin) numpy -> (P_out, Cout) numpy"""
    arena.reset()
    dev = arena.buf.device
    cout, cin = w.shape[0], w.shape[-1]
    xv = put(arena, x, misalign_bytes=4, poison=float('nan'))
    nv = put(arena, nbr, misalign_bytes=4, poison=0)
    out = carve(arena, (len(nbr), cout), torch.float32, 4)
    if out.numel():
        out.fill_(float('nan'))
    wpack = sparse_conv_ops.pack_weight(torch.from_numpy(np.ascontiguousarray(w)).to(dev), wide=wide)
    opt = [None if t is None else put(arena, t, misalign_bytes=4, poison=float('nan')) for t in (scale, shift, res)]
    sparse_conv_ops.sparse_conv(xv, nv, wpack, cin, cout, opt[0], opt[1], opt[2], relu, out=out, split=split, wide=wide)
    torch.cuda.synchronize()
    arena.check()
    return out.cpu().numpy()


def check_conv(arena, case, split=False):
    """The four epilogues of test_sparse_conv_gpu.check_conv through the wide entry: |err| <= 2 n 2^-24 A (times |scale| when
    folded); a shift adds the rounding of the epilogue's fma, 2^-24 |y scale + shift|, a residual that of its addition,
    2^-24 |out|; ReLU is 1-Lipschitz.  The first form runs twice, bit for bit."""
    y, A, n = case['y'], case['A'], case['n']
    sc, sh, res = case['scale'].astype(np.float64), case['shift'].astype(np.float64), case['res'].astype(np.float64)
    a = (arena, case['x'], case['nbr'], case['w'])
    worst = {}
    got = run_conv(*a, split=split)
    assert np.array_equal(got, run_conv(*a, split=split)), 'two runs differ'
    worst['none'] = np.abs(got - y) / np.maximum(2 * n * U * A, 1e-300)
    got = run_conv(*a, case['scale'], np.zeros_like(case['shift']), split=split)
    worst['scale'] = np.abs(got - y * sc) / np.maximum(2 * n * U * A * np.abs(sc), 1e-300)
    bn = y * sc + sh
    got = run_conv(*a, case['scale'], case['shift'], relu=True, split=split)
    worst['bn_relu'] = np.abs(got - np.maximum(bn, 0)) / (2 * n * U * A * np.abs(sc) + U * np.abs(bn))
    got = run_conv(*a, case['scale'], case['shift'], case['res'], relu=True, split=split)
    worst['bn_res_relu'] = np.abs(got - np.maximum(bn + res, 0)) / (2 * n * U * A * np.abs(sc) + U * np.abs(bn) + U * np.abs(bn + res))
    for k, v in worst.items():
        print(f'  {k}: max err / bound {float(v.max()) if v.size else 0.0:.3f}')
        assert np.isfinite(v).all() and (v <= 1.0).all(), k


@pytest.mark.parametrize("cin, cout", [(128, 256), (256, 256), (256, 64), (5, 256)])
@pytest.mark.parametrize("name", GEOS)
def test_wide_conv_matches_the_dense_convolution_in_float64(arena, books, name, cin, cout):
    idx, bk = books
    case = pnr.conv_case(idx, bk[name], name, cin, cout, seed=cin * 1000 + cout)
    print(name, cin, cout, 'sites', len(case['nbr']))
    assert len(case['nbr']) > 64 and np.abs(case['y']).max() > 0.1
    check_conv(arena, case)


@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("cin, cout", [(32, 64), (128, 128)])
@pytest.mark.parametrize("name", GEOS)
def test_wide_entry_gives_the_narrow_entrys_bits_where_both_serve(arena, books, name, cin, cout, split):
    idx, bk = books
    case = pnr.conv_case(idx, bk[name], name, cin, cout, seed=7 + cin)
    a = (arena, case['x'], case['nbr'], case['w'], case['scale'], case['shift'], case['res'])
    wide, narrow = run_conv(*a, relu=True, split=split, wide=True), run_conv(*a, relu=True, split=split, wide=False)
    assert np.isfinite(wide).all() and wide.any() and np.array_equal(wide, narrow)


@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("name", GEOS)
def test_the_halves_of_256_output_columns_are_two_narrow_runs(arena, books, name, split):
    """an output element's chain does not depend on how the output columns are blocked: columns [0, 128) and [128, 256) of the
    128 -> 256 run are, bit for bit, the narrow entry's 128 -> 128 runs on the two halves of the weight"""
    idx, bk = books
    case = pnr.conv_case(idx, bk[name], name, 128, 256, seed=11)
    wide = run_conv(arena, case['x'], case['nbr'], case['w'], case['scale'], case['shift'], case['res'], relu=True, split=split)
    assert np.isfinite(wide).all()
    for lo in (0, 128):
        half = slice(lo, lo + 128)
        narrow = run_conv(arena, case['x'], case['nbr'], case['w'][half], case['scale'][half], case['shift'][half],
                          np.ascontiguousarray(case['res'][:, half]), relu=True, split=split, wide=False)
        assert narrow.any() and np.array_equal(wide[:, half], narrow), lo


@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("name", GEOS)
def test_256_input_channels_with_a_zero_upper_half_are_the_narrow_run_on_the_lower(arena, books, name, split):
    """W[..., 128:] = 0: blocks kb = 8..15 of every offset add +-0 to the chain, which leaves its value; the inputs are finite,
    so no 0 * inf arises.  Equal under np.array_equal to the narrow 128 -> 128 run on x[:, :128]."""
    idx, bk = books
    case = pnr.conv_case(idx, bk[name], name, 256, 128, seed=13)
    w = case['w'].copy()
    w[..., 128:] = 0.0
    assert np.isfinite(case['x']).all()
    wide = run_conv(arena, case['x'], case['nbr'], w, split=split)
    narrow = run_conv(arena, np.ascontiguousarray(case['x'][:, :128]), case['nbr'], np.ascontiguousarray(w[..., :128]), split=split, wide=False)
    assert narrow.any() and np.array_equal(wide, narrow)


@pytest.mark.parametrize("P", [0, 1, 63, 64, 65])
def test_wide_conv_at_the_row_tile_boundaries(arena, P):
    idx = pnr.p2_indices(P)
    case = pnr.conv_case(idx, pnr.book(idx, 'subm133'), 'subm133', 256, 256, seed=P)
    check_conv(arena, case)
    if P == 65:
        check_conv(arena, case, split=True)


def test_wide_entries_refuse_other_widths_and_a_misaligned_pack(dev):
    x = torch.zeros((8, 256), device=dev)
    nbr = torch.zeros((8, 9), dtype=torch.int32, device=dev)
    pack = torch.zeros(9 * 16 * 16 * 256 + 4, device=dev)
    out = torch.empty((8, 256), device=dev)
    err = _native.NativeLibraryError
    for entry in ("pdm_sparse_conv_wide", "pdm_sparse_conv_wide_split"):
        def call(cin, cout, wp):
            _native.call(entry, _native.stream(dev), 8, 8, 9, cin, cout, x.data_ptr(), nbr.data_ptr(), wp, None, None, None, 0, out.data_ptr())
        with pytest.raises(err, match='192 output channels'):
            call(256, 192, pack.data_ptr())
        with pytest.raises(err, match='12 input channels'):
            call(12, 256, pack.data_ptr())
        with pytest.raises(err, match='16-byte aligned'):
            call(256, 256, pack.data_ptr() + 4)
        call(256, 256, pack.data_ptr())
    torch.cuda.synchronize()
    with pytest.raises(ValueError, match='channels'):
        sparse_conv_ops.pack_weight(torch.zeros((192, 1, 3, 3, 16), device=dev), wide=True)


# ---- data gradient ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cin, cout", [(128, 256), (256, 256), (256, 128)])
@pytest.mark.parametrize("name", GEOS)
def test_wide_data_gradient_within_the_summation_bound(arena, books, name, cin, cout):
    """the wide split kernel with the channels swapped, over the layer's own table (submanifold, offsets reversed in the pack) or the
    transposed one: |err| <= 2 n 2^-24 A_dx, n = kvol Cout; twice, bit for bit"""
    idx, bk = books
    kernel, _, _, subm = pnr.GEOMETRIES_2D[name]
    case = pnr.grad_case(len(idx), bk[name][1], kernel, cin, cout, seed=cin * 1000 + cout)

    def run():
        arena.reset()
        dev = arena.buf.device
        dy = put(arena, case['dy'], misalign_bytes=4, poison=float('nan'))
        nbr = put(arena, case['nbr'], misalign_bytes=4, poison=0)
        w = torch.from_numpy(case['w']).to(dev)
        if subm:
            table, pack = nbr, sparse_conv_ops.pack_weight_transposed(w, flip=True, wide=True)
        else:
            table, pack = sparse_conv_ops.rulebook_transpose(nbr, len(case['x'])), sparse_conv_ops.pack_weight_transposed(w, wide=True)
        out = carve(arena, (len(case['x']), cin), torch.float32, 4)
        out.fill_(float('nan'))
        sparse_conv_ops.sparse_conv(dy, table, pack, cout, cin, out=out, split=True, wide=True)
        torch.cuda.synchronize()
        arena.check()
        return out.cpu().numpy()
    got = run()
    n = kernel[0] * kernel[1] * kernel[2] * cout
    ratio = np.abs(got - case['dx64']) / np.maximum(2 * n * U * case['A_dx'], 1e-300)
    print(name, cin, cout, 'max err / bound %.3f' % float(ratio.max()))
    assert np.isfinite(ratio).all() and (ratio <= 1.0).all() and np.abs(case['dx64']).max() > 0.1
    assert np.array_equal(got, run()), 'two runs differ'
    w = torch.from_numpy(case['w']).to(arena.buf.device)
    wrapped = sparse_conv_ops.sparse_conv_dgrad(torch.from_numpy(case['dy']).to(w.device), torch.from_numpy(case['nbr']).to(w.device) if subm else
                                                sparse_conv_ops.rulebook_transpose(torch.from_numpy(case['nbr']).to(w.device), len(case['x'])),
                                                sparse_conv_ops.pack_weight_transposed(w, flip=subm, wide=True), cin, cout, wide=True)
    assert np.array_equal(wrapped.cpu().numpy(), got)


# ---- weight gradient ----------------------------------------------------------------------------------------------------------
def run_wgrad(arena, case, wide=True):
    arena.reset()
    x = put(arena, case['x'], misalign_bytes=4, poison=float('nan'))
    dy = put(arena, case['dy'], misalign_bytes=4, poison=float('nan'))
    nbr = put(arena, case['nbr'], misalign_bytes=4, poison=0)
    out = carve(arena, (case['cout'], *case['kernel'], case['cin']), torch.float32, 4)
    out.fill_(float('nan'))                 # every element is written
    sparse_conv_ops.sparse_conv_wgrad(dy, x, nbr, case['kernel'], out=out, wide=wide)
    torch.cuda.synchronize()
    arena.check()
    return out.cpu().numpy().reshape(case['cout'], -1, case['cin'])


def check_wgrad(arena, case, tag=''):
    got = run_wgrad(arena, case)
    bound = 2 * np.maximum(case['n_k'], 1)[None, :, None] * U * case['A_dW']
    err = np.abs(got - case['dW64'])
    ratio = err / np.maximum(bound, 1e-300)
    print(tag, 'rows', len(case['nbr']), 'max err / bound %.3f' % (float(ratio.max()) if ratio.size else 0.0))
    assert np.isfinite(got).all() and (err <= bound).all()
    assert np.array_equal(got, run_wgrad(arena, case)), 'two runs differ'
    return got


@pytest.mark.parametrize("name, cin, cout", [(name, ci, co) for name in GEOS for ci, co in ((128, 256), (256, 256), (256, 128))] +
                         [('subm133', 5, 256), ('k133s122p011', 256, 16), ('subm133', 64, 256)])
def test_wide_weight_gradient_within_the_summation_bound(arena, books, name, cin, cout):
    """every sub-block layout: both sides split (256, 256), one side split beside a full, a padded (Cin = 5) and a small block"""
    idx, bk = books
    case = pnr.grad_case(len(idx), bk[name][1], pnr.GEOMETRIES_2D[name][0], cin, cout, seed=cin * 1000 + cout + 1)
    got = check_wgrad(arena, case, f'{name} {cin}->{cout}')
    assert np.abs(got).max() > 0.1


@pytest.mark.parametrize("P", [0, 1, 63, 65, 'rows + 1'])
def test_wide_weight_gradient_sizes_and_two_chunks(arena, P):
    """256 -> 256 over the nine offsets on the (1, 48, 40) grid: no row (zeros), tile edges, and one row more than a chunk, so that
    phase two adds two partials"""
    rows = sparse_conv_ops.wgrad_chunk_rows(1025, 9, 256, 256, wide=True)
    assert rows == 1024 and sparse_conv_ops.wgrad_chunk_rows(1025, 9, 256, 256) == 0
    P = rows + 1 if P == 'rows + 1' else P
    idx = pnr.chunk_indices(P)
    nbr = pnr.book(idx, 'subm133', 1, pnr.CHUNK_SHAPE)[1]
    case = pnr.grad_case(P, nbr, (1, 3, 3), 256, 256, seed=P)
    got = check_wgrad(arena, case, f'P={P}')
    if P == 0:
        assert not got.any(), 'no row: zeros'
    else:
        assert got.any()


@pytest.mark.parametrize("name", GEOS)
def test_wide_weight_gradient_at_128_x_128_gives_the_narrow_entrys_bits(arena, books, name):
    """the chunk rule is the narrow one and the launch the narrow one"""
    idx, bk = books
    case = pnr.grad_case(len(idx), bk[name][1], pnr.GEOMETRIES_2D[name][0], 128, 128, seed=3)
    assert sparse_conv_ops.wgrad_chunk_rows(5000, 9, 128, 128, wide=True) == sparse_conv_ops.wgrad_chunk_rows(5000, 9, 128, 128)
    wide, narrow = run_wgrad(arena, case, wide=True), run_wgrad(arena, case, wide=False)
    assert wide.any() and np.array_equal(wide, narrow)


# ---- the 2-D layer --------------------------------------------------------------------------------------------------------------
def tensor2d(idx4, feats, dev):
    idx3 = torch.from_numpy(np.ascontiguousarray(idx4[:, [0, 2, 3]])).to(dev)
    return spconv.SparseConvTensor(torch.as_tensor(feats).to(dev), idx3, pnr.P2_SHAPE[1:], pnr.P2_B)


@pytest.mark.parametrize("cls, cin, cout", [('SubMConv2d', 32, 256), ('SparseConv2d', 128, 256), ('SparseConv2d', 256, 64), ('SubMConv2d', 256, 256)])
def test_2d_layer_matches_conv2d_in_float64(dev, books, cls, cin, cout):
    """SubMConv2d / SparseConv2d (stride 2, padding 1) with a bias against F.conv2d in float64 on the densified input at the
    layer's sites, within the forward bound plus the bias fma's rounding; the strided layer's indices (P, 3) equal the numpy
    rulebook's entry for entry; dense() is (B, C, H', W') and equals a torch scatter exactly."""
    idx, bk = books
    rng = np.random.default_rng(cin + cout)
    subm = cls == 'SubMConv2d'
    layer = getattr(spconv, cls)(cin, cout, 3, stride=1 if subm else 2, padding=1, bias=True, indice_key='k').to(dev).eval()
    assert tuple(layer.weight.shape) == (cout, 3, 3, cin) and set(layer.state_dict()) == {'weight', 'bias'}
    x = rng.uniform(-1, 1, (len(idx), cin)).astype(np.float32)
    with torch.no_grad():
        out = layer(tensor2d(idx, x, dev))
    want_idx = bk['subm133' if subm else 'k133s122p011'][0][:, [0, 2, 3]]
    assert out.indices.dtype == torch.int32 and np.array_equal(out.indices.cpu().numpy(), want_idx)
    hw = pnr.P2_SHAPE[1:] if subm else (12, 10)
    assert list(out.spatial_shape) == list(hw)
    w, b = layer.weight.detach().cpu().numpy(), layer.bias.detach().cpu().numpy().astype(np.float64)
    y, A = pnr.conv2d_reference(x, idx[:, [0, 2, 3]], pnr.P2_B, pnr.P2_SHAPE[1:], w, 1 if subm else 2, 1, want_idx)
    err = np.abs(out.features.cpu().numpy() - (y + b))
    bound = 2 * 9 * cin * U * A + U * np.abs(y + b)
    print(cls, cin, cout, 'sites', len(want_idx), 'max err / bound %.3f' % float((err / np.maximum(bound, 1e-300)).max()))
    assert (err <= bound).all() and np.abs(y).max() > 0.05
    dense = out.dense()
    want = torch.zeros((pnr.P2_B, *hw, cout), device=dev)
    i = out.indices.long()
    want[i[:, 0], i[:, 1], i[:, 2]] = out.features
    assert tuple(dense.shape) == (pnr.P2_B, cout, *hw) and torch.equal(dense, want.permute(0, 3, 1, 2))


def test_2d_dense_gradient_is_the_gather(dev, books):
    idx, _ = books
    rng = np.random.default_rng(9)
    f = torch.from_numpy(rng.uniform(-1, 1, (len(idx), 16)).astype(np.float32)).to(dev).requires_grad_()
    t = tensor2d(idx, f.detach(), dev).replace_feature(f)
    dense = t.dense()
    g = torch.from_numpy(rng.uniform(-1, 1, tuple(dense.shape)).astype(np.float32)).to(dev)
    dense.backward(g)
    i = t.indices.long()
    assert torch.equal(f.grad, g[i[:, 0], :, i[:, 1], i[:, 2]])


def test_2d_layers_that_share_an_indice_key_build_one_rulebook(dev, books):
    idx, _ = books
    x = tensor2d(idx, np.random.default_rng(1).uniform(-1, 1, (len(idx), 32)).astype(np.float32), dev)
    down = spconv.SparseConv2d(32, 64, 3, stride=2, padding=1, bias=False, indice_key='spconv2').to(dev).eval()
    a = spconv.SubMConv2d(64, 64, 3, padding=1, bias=False, indice_key='subm2').to(dev).eval()
    b = spconv.SubMConv2d(64, 256, 3, padding=1, bias=False, indice_key='subm2').to(dev).eval()
    before = sparse_conv_ops.HOST_READS
    with torch.no_grad():
        h = down(x)
        assert sparse_conv_ops.HOST_READS == before + 1
        h = a(h)
        book = h.indice_dict['subm2']
        out = b(h)
    assert sparse_conv_ops.HOST_READS == before + 1 and out.indice_dict['subm2'] is book
    assert set(k for k in out.indice_dict if not isinstance(k, tuple)) == {'spconv2', 'subm2'} and out.features.shape[1] == 256


def test_2d_training_layer_backward_within_the_operator_bounds(dev, books):
    """SparseConv2d 128 -> 256 in training mode, the input requiring grad: dx, dW (in the parameter's (Cout, kh, kw, Cin) shape)
    and dbias within the operator bounds of the float64 restatement"""
    idx, bk = books
    out_idx, nbr, _ = bk['k133s122p011']
    case = pnr.grad_case(len(idx), nbr, (1, 3, 3), 128, 256, seed=21)
    layer = spconv.SparseConv2d(128, 256, 3, stride=2, padding=1, bias=True, indice_key='d').to(dev).train()
    with torch.no_grad():
        layer.weight.copy_(torch.from_numpy(case['w']).reshape(256, 3, 3, 128))
    f = torch.from_numpy(case['x']).to(dev).requires_grad_()
    out = layer(tensor2d(idx, f.detach(), dev).replace_feature(f))
    assert np.array_equal(out.indices.cpu().numpy(), out_idx[:, [0, 2, 3]])
    out.features.backward(torch.from_numpy(case['dy']).to(dev))
    assert (np.abs(f.grad.cpu().numpy() - case['dx64']) <= 2 * 9 * 256 * U * case['A_dx']).all()
    bound = 2 * np.maximum(case['n_k'], 1)[None, :, None] * U * case['A_dW']
    assert tuple(layer.weight.grad.shape) == (256, 3, 3, 128)
    assert (np.abs(layer.weight.grad.cpu().numpy().reshape(256, 9, 128) - case['dW64']) <= bound).all()
    dy64 = case['dy'].astype(np.float64)
    assert (np.abs(layer.bias.grad.cpu().numpy() - dy64.sum(0)) <= 2 * len(dy64) * U * np.abs(dy64).sum(0)).all()


def test_three_chained_2d_layers_replay_from_a_graph_bit_for_bit(dev, books):
    """SubMConv2d 32 -> 128 -> 256 -> 256, each with BatchNorm1d and ReLU folded into its launch, over one shared rulebook built
    before the capture"""
    idx, _ = books
    torch.manual_seed(3)
    rng = np.random.default_rng(3)
    dims = [(32, 128), (128, 256), (256, 256)]
    mods = []
    for ci, co in dims:
        bn = torch.nn.BatchNorm1d(co, eps=1e-3)
        with torch.no_grad():
            bn.running_var.uniform_(0.5, 1.5)
            bn.running_mean.uniform_(-0.2, 0.2)
            bn.bias.uniform_(0.0, 0.4)
        mods += [spconv.SubMConv2d(ci, co, 3, padding=1, bias=False, indice_key='subm'), bn, torch.nn.ReLU()]
    net = spconv.SparseSequential(*mods).to(dev).eval()
    x = tensor2d(idx, rng.uniform(-1, 1, (len(idx), 32)).astype(np.float32), dev)
    with torch.no_grad():
        eager = net(x).features.clone()         # builds the rulebook, the packs and the folds
        assert float(eager.abs().max()) > 0 and eager.shape[1] == 256
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = net(x).features
        out.fill_(float('nan'))
        graph.replay()
        torch.cuda.synchronize()
    assert torch.equal(out, eager)

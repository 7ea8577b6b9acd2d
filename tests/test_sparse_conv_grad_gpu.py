"""The sparse convolution's gradients on the device (csrc/sparse_conv_wgrad.hip, pdm_sparse_rulebook_transpose, the data gradient
as pdm_sparse_conv_split over the transposed rulebook, sparse_conv_ops.SparseConvFunction and the training path of spconv/) against
the float64 restatement of tests/sparse_conv_grad_reference.py, and a training step of the voxel backbones and detectors.
Inputs and outputs of the operators are carved from a poisoned Arena, 4 bytes off a 16-byte boundary: features between NaN red
zones, tables between in-range values.

Exact: the transposed table; two runs of everything; a graph replay; a hand-derived known answer.
Bounded: |dx err| <= 2 n 2^-24 A_dx with n = kvol Cout, and per offset |dW err| <= 2 max(n_k, 1) 2^-24 A_dW: twice the first-order
worst case of any fp32 summation order of n (n_k) products, A the same sums of absolute values.
"""
import copy
import json
import os

import numpy as np
import pytest
import torch

import sparse_conv_grad_reference as sgr
import sparse_conv_reference as scr
from arena import Arena
from pdm_ssd_amd import sparse_conv_ops

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
U = 2.0 ** -24
WIDTHS = [(4, 16), (16, 32), (64, 64), (32, 128)]
STRIDED = ['k3s2p1', 'k3s2p011', 'k311s211p0']


@pytest.fixture(scope="module")
def ref():
    z = np.load(os.path.join(GOLDEN, "ref_sparse_conv.npz"))
    return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def manifest():
    with open(os.path.join(GOLDEN, "ref_sparse_conv_manifest.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def arena(dev):
    return Arena(dev)


@pytest.fixture(scope="module")
def r1_books():
    """the numpy rulebooks of the full R1 site list, one per geometry, computed once"""
    idx = scr.r1_indices()
    return idx, {name: scr.rulebook(idx, scr.R1_B, scr.R1_SHAPE, *geo) for name, geo in scr.GEOMETRIES.items()}


@pytest.fixture(scope="module")
def chunk_sites():
    """seeded random distinct sites of a (41, 64, 64) grid, B = 2, and their submanifold rulebook at the largest size asked for
    (a prefix of the site list is NOT a prefix of the rulebook: each size builds its own)"""
    rng = np.random.default_rng(41)
    D, H, W = 41, 64, 64
    cells = rng.choice(2 * D * H * W, size=2 * 1024 + 1, replace=False)
    idx = np.stack([cells // (D * H * W), cells % D, (cells // D) % H, (cells // (D * H)) % W], 1).astype(np.int32)
    return idx, (D, H, W)


def put(arena, src, misalign_bytes=0, poison=None):
    src = torch.as_tensor(src)
    return arena.put(src, misalign_bytes, poison) if src.numel() else src.to(arena.buf.device)


def carve(arena, shape, dtype, misalign_bytes=0):
    return arena.carve(shape, dtype, misalign_bytes) if int(np.prod(shape)) else torch.empty(shape, dtype=dtype, device=arena.buf.device)


def grad_case(num_in, nbr, kernel, cin, cout, seed):
    rng = np.random.default_rng(seed)
    n = kernel[0] * kernel[1] * kernel[2] * cin
    c = dict(x=rng.uniform(-1, 1, (num_in, cin)).astype(np.float32), w=(rng.uniform(-1, 1, (cout, *kernel, cin)) / np.sqrt(n)).astype(np.float32),
             dy=rng.uniform(-1, 1, (len(nbr), cout)).astype(np.float32), nbr=np.ascontiguousarray(nbr), kernel=kernel, cin=cin, cout=cout)
    c.update(sgr.grads(c['x'], c['w'], c['dy'], nbr))
    return c


# ---- the transposed rulebook ------------------------------------------------------------------------------------------------
def run_transpose(arena, nbr_np, num_in):
    arena.reset()
    nbr = put(arena, nbr_np, misalign_bytes=4, poison=0)
    kvol = nbr_np.shape[1]
    out = carve(arena, (num_in, kvol), torch.int32, 4)
    from pdm_ssd_amd import _native
    _native.call("pdm_sparse_rulebook_transpose", _native.stream(arena.buf), len(nbr_np), num_in, kvol, nbr.data_ptr() if len(nbr_np) else None,
                 out.data_ptr() if num_in else None)
    torch.cuda.synchronize()
    arena.check()
    return out.cpu().numpy()


@pytest.mark.parametrize("P", [0, 1, 63, 64, 65, None])
@pytest.mark.parametrize("name", list(scr.GEOMETRIES))
def test_transpose_equals_the_restatement_entry_for_entry(arena, r1_books, name, P):
    idx = scr.r1_indices(P)
    nbr = r1_books[1][name][1] if P is None else scr.rulebook(idx, scr.R1_B, scr.R1_SHAPE, *scr.GEOMETRIES[name])[1]
    got = run_transpose(arena, nbr, len(idx))
    assert got.shape == (len(idx), nbr.shape[1]) and np.array_equal(got, sgr.transpose(nbr, len(idx)))
    if name == 'subm3':
        assert np.array_equal(got, nbr[:, ::-1])
    if P is None:
        hurt = nbr.copy()
        hurt[::3, 0], hurt[1::3, -1] = len(idx), -7          # out of range counts as -1
        assert np.array_equal(run_transpose(arena, hurt, len(idx)), sgr.transpose(hurt, len(idx)))
        wrapped = sparse_conv_ops.rulebook_transpose(torch.from_numpy(nbr).to(arena.buf.device), len(idx))
        assert np.array_equal(wrapped.cpu().numpy(), got)


# ---- the data gradient ------------------------------------------------------------------------------------------------------
def run_dgrad(arena, case, subm):
    arena.reset()
    dev = arena.buf.device
    cin, cout = case['cin'], case['cout']
    dy = put(arena, case['dy'], misalign_bytes=4, poison=float('nan'))
    nbr = put(arena, case['nbr'], misalign_bytes=4, poison=0)
    w = torch.from_numpy(case['w']).to(dev)
    if subm:
        table, pack = nbr, sparse_conv_ops.pack_weight_transposed(w, flip=True)
    else:
        table, pack = sparse_conv_ops.rulebook_transpose(nbr, len(case['x'])), sparse_conv_ops.pack_weight_transposed(w)
    out = carve(arena, (len(case['x']), max(cin, 16)), torch.float32, 4)
    sparse_conv_ops.sparse_conv(dy, table, pack, cout, max(cin, 16), out=out, split=True)
    torch.cuda.synchronize()
    arena.check()
    got = out.cpu().numpy()
    assert not got[:, cin:].any(), 'the padded columns of the data gradient are zero'
    return got[:, :cin]


@pytest.mark.parametrize("cin, cout", WIDTHS)
@pytest.mark.parametrize("name", list(scr.GEOMETRIES))
def test_data_gradient_within_the_summation_bound(arena, r1_books, name, cin, cout):
    """|err| <= 2 n 2^-24 A_dx, n = kvol Cout (the forward test's bound on the transposed convolution); Cin = 4 runs the padded
    pack; (4, 16) and (64, 64) twice, bit for bit"""
    idx, books = r1_books
    kernel, _, _, subm = scr.GEOMETRIES[name]
    case = grad_case(len(idx), books[name][1], kernel, cin, cout, seed=cin * 1000 + cout)
    got = run_dgrad(arena, case, subm)
    n = kernel[0] * kernel[1] * kernel[2] * cout
    ratio = np.abs(got - case['dx64']) / np.maximum(2 * n * U * case['A_dx'], 1e-300)
    print(name, cin, cout, 'max err / bound %.3f' % float(ratio.max()))
    assert np.isfinite(ratio).all() and (ratio <= 1.0).all() and np.abs(case['dx64']).max() > 0.1
    if (cin, cout) in ((4, 16), (64, 64)):
        assert np.array_equal(got, run_dgrad(arena, case, subm)), 'two runs differ'


# ---- the weight gradient ----------------------------------------------------------------------------------------------------
def run_wgrad(arena, case, nbr=None):
    arena.reset()
    x = put(arena, case['x'], misalign_bytes=4, poison=float('nan'))
    dy = put(arena, case['dy'], misalign_bytes=4, poison=float('nan'))
    nbr = put(arena, case['nbr'] if nbr is None else nbr, misalign_bytes=4, poison=0)
    out = carve(arena, (case['cout'], *case['kernel'], case['cin']), torch.float32, 4)
    sparse_conv_ops.sparse_conv_wgrad(dy, x, nbr, case['kernel'], out=out)
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


@pytest.mark.parametrize("name, cin, cout", [(name, ci, co) for name in scr.GEOMETRIES for ci, co in WIDTHS] + [('subm3', 128, 128)])
def test_weight_gradient_within_the_summation_bound(arena, r1_books, name, cin, cout):
    idx, books = r1_books
    case = grad_case(len(idx), books[name][1], scr.GEOMETRIES[name][0], cin, cout, seed=cin * 1000 + cout + 1)
    got = check_wgrad(arena, case, f'{name} {cin}->{cout}')
    assert np.abs(got).max() > 0.1


@pytest.mark.parametrize("P", [0, 1, 63, 64, 65])
def test_weight_gradient_at_the_row_tile_boundaries(arena, P):
    idx = scr.r1_indices(P)
    geo = scr.GEOMETRIES['subm3']
    case = grad_case(len(idx), scr.rulebook(idx, scr.R1_B, scr.R1_SHAPE, *geo)[1], geo[0], 16, 32, seed=P)
    got = check_wgrad(arena, case, f'P={P}')
    if P == 0:
        assert not got.any(), 'no row: zeros'


@pytest.mark.parametrize("where", ['rows - 1', 'rows', 'rows + 1', '2 rows + 1'])
def test_weight_gradient_at_the_chunk_edges(arena, chunk_sites, where):
    """(16, 32) over 27 offsets: P_out one short of a chunk, a whole chunk, one row into the second, one row into the third"""
    idx, shape = chunk_sites
    rows = sparse_conv_ops.wgrad_chunk_rows(2 * 1024 + 1, 27, 16, 32)
    P = {'rows - 1': rows - 1, 'rows': rows, 'rows + 1': rows + 1, '2 rows + 1': 2 * rows + 1}[where]
    assert rows == 1024 and sparse_conv_ops.wgrad_chunk_rows(P, 27, 16, 32) == rows and P <= len(idx)
    geo = scr.GEOMETRIES['subm3']
    case = grad_case(P, scr.rulebook(idx[:P], 2, shape, *geo)[1], geo[0], 16, 32, seed=P)
    check_wgrad(arena, case, where)


def test_weight_gradient_counts_out_of_range_entries_as_missing(arena, r1_books):
    idx, books = r1_books
    nbr = books['k3s2p1'][1]
    rng = np.random.default_rng(2)
    hit = (rng.uniform(size=nbr.shape) < 0.3) & (nbr >= 0)
    minus = np.where(hit, -1, nbr).astype(np.int32)
    wild = np.where(hit, rng.choice([len(idx), len(idx) + 7, -5, 2 ** 30, -2 ** 31], size=nbr.shape), nbr).astype(np.int32)
    case = grad_case(len(idx), minus, (3, 3, 3), 16, 32, seed=8)
    got = check_wgrad(arena, case, 'with -1')
    assert np.array_equal(run_wgrad(arena, case, wild), got)


def test_weight_gradient_replays_from_a_graph_bit_for_bit(dev, r1_books):
    idx, books = r1_books
    case = grad_case(len(idx), books['subm3'][1], (3, 3, 3), 32, 64, seed=4)
    x, dy, nbr = (torch.from_numpy(case[k]).to(dev) for k in ('x', 'dy', 'nbr'))
    out = torch.empty((64, 3, 3, 3, 32), device=dev)
    eager = sparse_conv_ops.sparse_conv_wgrad(dy, x, nbr, 3, out=out).clone()
    assert float(eager.abs().max()) > 0
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        sparse_conv_ops.sparse_conv_wgrad(dy, x, nbr, 3, out=out)
    out.fill_(float('nan'))
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)


# ---- known answer, and the autograd node ------------------------------------------------------------------------------------
def test_known_answer_one_voxel_and_a_pair(dev):
    """The forward's known-answer case: submanifold 3 x 3 x 3, Cin = 4, Cout = 16, W[c][k][0] = 1 where c == k mod 16 and 0 elsewhere;
    x column 0 holds the values, columns 1-3 hold 100.
    One voxel, value 3, dy = 2 at channel 13: its only pair is (itself, k = 13), so dW[13][13] = 2 x = (6, 200, 200, 200), zeros
    elsewhere; dx = W[13][13]^T 2 = (2, 0, 0, 0).
    The pair A = (z 5, y 5, x 5) value 3 and B = (z 6, y 5, x 5) value 5, dy[A] = 2 at channel 6, dy[B] = 7 at channel 13.  A's pairs: (A,
    k = 13), (B, k = 22); B's pairs: (B, k = 13), (A, k = 4).  dW[6][13] = 2 x[A] = (6, 200, 200, 200), dW[6][22] = 2 x[B] = (10, 200, 200,
    200), dW[13][13] = 7 x[B] = (35, 700, 700, 700), dW[13][4] = 7 x[A] = (21, 700, 700, 700), zeros elsewhere.  dx[A] = W[6][13]^T 2 +
    W[13][4]^T 7 = 0 (13 mod 16 != 6, 4 != 13); dx[B] = W[6][22]^T 2 + W[13][13]^T 7 = (9, 0, 0, 0) (22 mod 16 == 6)."""
    w = torch.zeros((16, 27, 4), device=dev)
    for k in range(27):
        w[k % 16, k, 0] = 1.0
    w = w.reshape(16, 3, 3, 3, 4).requires_grad_()

    def run(sites, values, dy_at):
        idx = torch.tensor(sites, dtype=torch.int32, device=dev)
        x = torch.full((len(sites), 4), 100.0, device=dev)
        x[:, 0] = torch.tensor(values, device=dev)
        x.requires_grad_()
        rb = sparse_conv_ops.rulebook(idx, 1, (41, 16, 21), 3, 1, 1, subm=True)
        dy = torch.zeros((len(sites), 16), device=dev)
        for row, (ch, v) in enumerate(dy_at):
            dy[row, ch] = v
        w.grad = None
        out = sparse_conv_ops.SparseConvFunction.apply(x, w, None, rb.nbr, True, 4, 16)
        out.backward(dy)
        by_table = sparse_conv_ops.sparse_conv_dgrad(dy, sparse_conv_ops.rulebook_transpose(rb.nbr, len(sites)),
                                                     sparse_conv_ops.pack_weight_transposed(w), 4, 16)
        assert torch.equal(by_table, x.grad), 'the transposed table and the reversed-offset identity give the same data gradient'
        return w.grad.reshape(16, 27, 4).cpu().numpy(), x.grad.cpu().numpy()

    dw, dx = run([(0, 5, 5, 5)], [3.0], [(13, 2.0)])
    want = np.zeros((16, 27, 4), dtype=np.float32)
    want[13, 13] = [6, 200, 200, 200]
    assert np.array_equal(dw, want) and np.array_equal(dx, np.array([[2, 0, 0, 0]], dtype=np.float32))
    dw, dx = run([(0, 5, 5, 5), (0, 6, 5, 5)], [3.0, 5.0], [(6, 2.0), (13, 7.0)])
    want = np.zeros((16, 27, 4), dtype=np.float32)
    want[6, 13], want[6, 22], want[13, 13], want[13, 4] = [6, 200, 200, 200], [10, 200, 200, 200], [35, 700, 700, 700], [21, 700, 700, 700]
    assert np.array_equal(dw, want) and np.array_equal(dx, np.array([[0, 0, 0, 0], [9, 0, 0, 0]], dtype=np.float32))


@pytest.mark.parametrize("name, cin, cout", [('k3s2p1', 16, 32), ('subm3', 5, 16), ('k311s211p0', 64, 128)])
def test_autograd_node_backward_within_the_operator_bounds(dev, r1_books, name, cin, cout):
    """SparseConvFunction through .backward(), bias included, the input requiring grad (a strided layer among the cases): dx and dW
    within the two operator bounds; dbias = dy.sum(0) within 2 P 2^-24 sum |dy|; the forward within the forward's bound plus the
    rounding of the bias addition.  No finite differences: fp32 is too coarse for them."""
    idx, books = r1_books
    kernel, _, _, subm = scr.GEOMETRIES[name]
    out_idx, nbr_np, _ = books[name]
    case = grad_case(len(idx), nbr_np, kernel, cin, cout, seed=77)
    bias_np = np.random.default_rng(5).uniform(-0.5, 0.5, cout).astype(np.float32)
    x = torch.from_numpy(case['x']).to(dev).requires_grad_()
    w = torch.from_numpy(case['w']).to(dev).requires_grad_()
    b = torch.from_numpy(bias_np).to(dev).requires_grad_()
    nbr = torch.from_numpy(nbr_np).to(dev)
    nbr_t = True if subm else sparse_conv_ops.rulebook_transpose(nbr, len(idx))
    before = sparse_conv_ops.HOST_READS
    out = sparse_conv_ops.SparseConvFunction.apply(x, w, b, nbr, nbr_t, cin, cout)
    out.backward(torch.from_numpy(case['dy']).to(dev))
    assert sparse_conv_ops.HOST_READS == before
    kvol = nbr_np.shape[1]
    y64 = np.zeros((len(nbr_np), cout))
    A = np.zeros_like(y64)
    w64 = case['w'].astype(np.float64).reshape(cout, kvol, cin)
    for k in range(kvol):
        i = np.nonzero(nbr_np[:, k] >= 0)[0]
        y64[i] += case['x'][nbr_np[i, k]].astype(np.float64) @ w64[:, k].T
        A[i] += np.abs(case['x'][nbr_np[i, k]]).astype(np.float64) @ np.abs(w64[:, k]).T
    y64b = y64 + bias_np
    assert (np.abs(out.detach().cpu().numpy() - y64b) <= 2 * kvol * cin * U * A + U * np.abs(y64b) + 1e-300).all()
    assert (np.abs(x.grad.cpu().numpy() - case['dx64']) <= 2 * kvol * cout * U * case['A_dx']).all()
    bound = 2 * np.maximum(case['n_k'], 1)[None, :, None] * U * case['A_dW']
    assert (np.abs(w.grad.cpu().numpy().reshape(cout, kvol, cin) - case['dW64']) <= bound).all()
    dy64 = case['dy'].astype(np.float64)
    assert (np.abs(b.grad.cpu().numpy() - dy64.sum(0)) <= 2 * len(dy64) * U * np.abs(dy64).sum(0)).all()
    # an input that takes no gradient: no data gradient is computed, the others are the same bits
    w2, b2 = w.detach().clone().requires_grad_(), b.detach().clone().requires_grad_()
    sparse_conv_ops.SparseConvFunction.apply(x.detach(), w2, b2, nbr, None, cin, cout).backward(torch.from_numpy(case['dy']).to(dev))
    assert torch.equal(w2.grad, w.grad) and torch.equal(b2.grad, b.grad)


def test_to_dense_is_differentiable_in_the_features(dev):
    idx_np = scr.r1_indices(65)
    rng = np.random.default_rng(9)
    f = torch.from_numpy(rng.uniform(-1, 1, (65, 16)).astype(np.float32)).to(dev).requires_grad_()
    idx = torch.from_numpy(idx_np).to(dev)
    dense = sparse_conv_ops.to_dense(f, idx, scr.R1_B, scr.R1_SHAPE)
    assert torch.equal(dense, sparse_conv_ops.to_dense(f.detach(), idx, scr.R1_B, scr.R1_SHAPE))
    g = torch.from_numpy(rng.uniform(-1, 1, tuple(dense.shape)).astype(np.float32)).to(dev)
    dense.backward(g)
    i = idx.long()
    assert torch.equal(f.grad, g[i[:, 0], :, i[:, 1], i[:, 2], i[:, 3]])


# ---- the backbones ------------------------------------------------------------------------------------------------------------
def built_backbone(name, manifest, dev):
    from pdm_ssd_amd import backbones_3d
    net = backbones_3d.__all__[name](model_cfg={}, input_channels=4, grid_size=scr.B1_GRID)
    fill = manifest[f'{name}.fill']
    assert abs(scr.fill_backbone(net, fill['seed'], fill['gain']) - fill['checksum']) <= 1e-9 * fill['checksum'], 'not the generator\'s parameters'
    return net.to(dev)


def device_books(enc):
    """the rulebooks a forward left in the tensors' shared indice_dict, on the CPU, for sgr.backbone_step"""
    books = {k: (rb.out_indices.cpu(), rb.nbr.cpu()) for k, rb in enc.indice_dict.items() if isinstance(rb, sparse_conv_ops.Rulebook)}
    books['out_shape'] = tuple(enc.spatial_shape)
    return books


@pytest.mark.parametrize("name", ['VoxelBackBone8x', 'VoxelResBackBone8x'])
def test_backbone_training_step_equals_the_torch_formulation(ref, manifest, dev, name):
    """A training step on the b1 fixture (410 / 574 / 258 / 60 / 24 rows per level: every BatchNorm sees at least 24 rows), loss =
    (spatial_features * proj).sum() / numel: every parameter's gradient, every running statistic and spatial_features against the
    torch formulation over the same device rulebooks in float64 (per offset index_select -> mm -> index_add_, BatchNorm1d, ReLU).
    The tolerance is measured: the same formulation runs on the CPU in float32 as well, e = max |f32 - f64| / max |f64| per tensor,
    and the bound is 4 e max |f64|: ours is another fp32 order of the same sums; the factor covers the different order and
    BatchNorm's amplification.  4 host reads in the forward (the strided rulebooks), none in backward; every gradient finite and
    nonzero.
    The convolution biases of the residual blocks sit in front of a training BatchNorm: their gradient is zero in exact arithmetic,
    both sides hold rounding noise there, e is of the order 1e8 and the check says nothing about them.

    Measured on an MI355X (e, ours and ours / e are the largest over the tensors of a kind, all relative to max |f64| of the tensor):
      VoxelBackBone8x     spatial_features e 9.8e-07 ours 8.8e-07 (0.89 e)    running_mean 8.3e-08 / 7.1e-08 (1.06 e)  running_var 8.5e-08 / 8.5e-08 (1.0 e)
                          grad weight      e 9.8e-07 ours 1.2e-06 (1.63 e)    grad bias    e 1.0e-06 ours 9.9e-07 (1.96 e)
      VoxelResBackBone8x  spatial_features e 7.7e-07 ours 9.7e-07 (1.26 e)    running_mean 8.2e-08 / 8.2e-08 (1.58 e)  running_var 8.2e-08 / 8.3e-08 (1.18 e)
                          grad weight      e 1.2e-06 ours 1.7e-06 (1.99 e)    (the noise biases: 2.76 e)
    This is with the training path on pdm_sparse_conv_split (one accumulator per offset, added to a running sum).  On the plain
    pdm_sparse_conv, which adds all 27 x Cin products of an output into one fp32 accumulator in sequence, the same step gave
    spatial_features 3.15 e / 2.77 e and 3 of 37 / 5 of 64 gradients over 4 e (up to 5.8 e / 6.0 e), while the torch formulation in
    float32 on the GPU landed at the CPU's e: the excess was that one long chain's rounding."""
    from pdm_ssd_amd.backbones_2d.map_to_bev import HeightCompression
    net = built_backbone(name, manifest, dev).train()
    start = copy.deepcopy(net)
    hc = HeightCompression({'NUM_BEV_FEATURES': 256})
    feats, coords = ref['b1.features'], ref['b1.coords']
    before = sparse_conv_ops.HOST_READS
    bd = hc(net({'voxel_features': torch.from_numpy(feats).to(dev), 'voxel_coords': torch.from_numpy(coords).to(dev), 'batch_size': scr.B1_B}))
    assert sparse_conv_ops.HOST_READS - before == 4
    sf = bd['spatial_features']
    rows = [len(bd['multi_scale_3d_features'][k].indices) for k in ('x_conv1', 'x_conv2', 'x_conv3', 'x_conv4')] + [len(bd['encoded_spconv_tensor'].indices)]
    assert rows == [410, 574, 258, 60, 24]
    proj = np.random.default_rng(13).uniform(-1, 1, tuple(sf.shape)).astype(np.float32)
    before = sparse_conv_ops.HOST_READS
    ((sf * torch.from_numpy(proj).to(dev)).sum() / sf.numel()).backward()
    assert sparse_conv_ops.HOST_READS == before
    ours = {'spatial_features': sf.detach().cpu().numpy()}
    for n, p in net.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all() and bool(p.grad.any()), n
        ours['grad.' + n] = p.grad.cpu().numpy()
    for n, b in net.named_buffers():
        if n.endswith('running_mean') or n.endswith('running_var'):
            ours['stat.' + n] = b.cpu().numpy()
    books = device_books(bd['encoded_spconv_tensor'])
    r64 = sgr.backbone_step(start, feats, coords, scr.B1_B, books, proj, torch.float64)
    r32 = sgr.backbone_step(start, feats, coords, scr.B1_B, books, proj, torch.float32)
    assert set(ours) | {'loss'} == set(r64)
    worst = {}
    failed = []
    for key, got in ours.items():
        scale = np.abs(r64[key]).max()
        e = np.abs(r32[key] - r64[key]).max() / scale
        mine = np.abs(got - r64[key]).max() / scale
        kind = key.split('.')[0] + ('.' + key.split('.')[-1] if '.' in key else '')
        w = worst.setdefault(kind, [0.0, 0.0, 0.0])
        w[0], w[1], w[2] = max(w[0], e), max(w[1], mine), max(w[2], mine / e if e > 0 else np.inf if mine > 0 else 0.0)
        if not mine <= 4 * e:
            failed.append((key, e, mine))
    for kind, (e, mine, ratio) in sorted(worst.items()):
        print(f'{name} {kind}: largest e {e:.3g}, largest ours {mine:.3g}, largest ours / e {ratio:.3g}')
    assert not failed, failed


def test_frozen_backbone_passes_the_gradient_to_its_input(ref, manifest, dev):
    """The backbone in eval mode with voxel_features requiring grad takes the autograd path with BatchNorm's running statistics.
    Its levels equal the no-grad eval forward's (the folded one-launch path) within 1e-4 absolute, the parity contract for fp32
    features that the backbone's forward test holds both to (four times the 2.5e-5 the fixture's generator found between float32
    and float64): the two are fp32 orders of the same sums, a conv bound per layer compounded over twelve layers.  The gradient
    reaches the input through the padded data gradient of the first layer (Cin = 4)."""
    net = built_backbone('VoxelBackBone8x', manifest, dev).eval()
    feats = torch.from_numpy(ref['b1.features']).to(dev)
    coords = torch.from_numpy(ref['b1.coords']).to(dev)
    with torch.no_grad():
        want = net({'voxel_features': feats, 'voxel_coords': coords, 'batch_size': scr.B1_B})
    x = feats.clone().requires_grad_()
    got = net({'voxel_features': x, 'voxel_coords': coords, 'batch_size': scr.B1_B})
    for lv in ('x_conv1', 'x_conv2', 'x_conv3', 'x_conv4'):
        a, b = got['multi_scale_3d_features'][lv], want['multi_scale_3d_features'][lv]
        assert torch.equal(a.indices, b.indices) and float((a.features - b.features).abs().max()) <= 1e-4, lv
    a, b = got['encoded_spconv_tensor'], want['encoded_spconv_tensor']
    assert a.features.requires_grad and float((a.features - b.features).abs().max()) <= 1e-4
    a.dense().square().sum().backward()
    assert x.grad is not None and x.grad.shape == feats.shape and torch.isfinite(x.grad).all() and bool(x.grad.any())
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in net.parameters())


# ---- the detectors ------------------------------------------------------------------------------------------------------------
def d1_points(dev):
    """the recipe of the eval test's cloud"""
    rng = np.random.default_rng(21)
    n = 3000
    centres = rng.uniform([1, -3, -2.5], [15, 3, 0.5], (12, 3))
    p = centres[rng.integers(0, 12, n)] + rng.normal(0, 0.6, (n, 3))
    pts = np.concatenate([rng.integers(0, 2, (n, 1)), p, rng.uniform(0, 1, (n, 1))], 1).astype(np.float32)
    return torch.from_numpy(pts).to(dev)


@pytest.mark.parametrize("builder", ['build_second', 'build_center_voxel'])
def test_detector_takes_a_training_step(dev, builder):
    """An eval forward, then .train(), forward, loss.backward(): the loss is finite, every parameter has a finite gradient, the
    first convolution's is nonzero, and the training forward reads the host as often as the eval forward up to the BEV map (the
    VFE's one read and the four strided rulebooks': at most 5)."""
    from pdm_ssd_amd import detector_config as dc
    torch.manual_seed(5)
    g = scr.D1
    cfg = copy.deepcopy(dc.SECOND_CFG if builder == 'build_second' else dc.CENTER_VOXEL_CFG)
    if builder == 'build_center_voxel':     # the BEV map of this shape has 2 x 4 cells: the head's top-K cannot exceed them
        cfg['DENSE_HEAD']['POST_PROCESSING']['MAX_OBJ_PER_SAMPLE'] = 8
    model = getattr(dc, builder)(cfg, dataset=dc.voxel_dataset(4, g['range'], g['voxel'], g['grid'])).to(dev)
    gt = np.zeros((g['B'], 3, 8), dtype=np.float32)
    gt[0, 0] = [6.0, 1.0, -1.0, 3.9, 1.6, 1.5, 0.3, 1]
    gt[0, 1] = [12.0, -3.0, -0.8, 0.8, 0.6, 1.7, -1.2, 2]
    gt[1, 0] = [14.0, -2.2, -0.9, 1.7, 0.6, 1.7, 2.1, 3]
    batch = {'batch_size': g['B'], 'points': d1_points(dev), 'gt_boxes': torch.from_numpy(gt).to(dev)}
    seen = {}
    model.map_to_bev_module.register_forward_hook(lambda m, a, out: seen.update(reads=sparse_conv_ops.HOST_READS))
    model.eval()
    before = sparse_conv_ops.HOST_READS
    with torch.no_grad():
        pred, _ = model(dict(batch))
    eval_reads = seen['reads'] - before
    assert len(pred) == g['B'] and 1 <= eval_reads <= 5
    model.train()
    before = sparse_conv_ops.HOST_READS
    ret, tb, _ = model(dict(batch))
    assert seen['reads'] - before == eval_reads
    before = sparse_conv_ops.HOST_READS
    ret['loss'].backward()
    assert sparse_conv_ops.HOST_READS == before
    assert torch.isfinite(ret['loss'])
    for n, p in model.named_parameters():
        if p.requires_grad:
            assert p.grad is not None and torch.isfinite(p.grad).all(), n
    assert bool(model.backbone_3d.conv_input[0].weight.grad.any())

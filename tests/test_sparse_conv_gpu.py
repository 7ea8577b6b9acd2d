"""The voxel path's device operators (csrc/sparse_conv.hip, csrc/sparse_conv_mfma.hip) against the numpy restatement of
tests/sparse_conv_reference.py row for row, against F.conv3d in float64 at the active sites, and against the reference's own
DynamicMeanVFE / VoxelBackBone8x / VoxelResBackBone8x / HeightCompression run over a dense-convolution stub of spconv
(tests/golden/ref_sparse_conv.npz, gen_sparse_conv_fixtures.py: parity unpinned by spconv itself).  Shapes V1, V2, R1, B1, D1
are described in sparse_conv_reference.py.  Inputs and outputs are carved from a poisoned Arena: features sit 4 bytes off a
16-byte boundary between NaN red zones, index inputs between in-range values.

Exact: kept_idx, unq_inv, voxel_coords, voxel_count; the set and order of output sites and every nbr entry; the dense canvas;
two runs of everything; a graph replay; a hand-derived known answer.
Bounded: each test's docstring derives its bound.
"""
import copy
import json
import os

import numpy as np
import pytest
import torch

import sparse_conv_reference as scr
from arena import Arena
from pdm_ssd_amd import _native, sparse_conv_ops

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CHANNELS = [(4, 16), (5, 16), (16, 16), (16, 32), (32, 32), (64, 64), (64, 128), (128, 128)]


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


def put(arena, src, misalign_bytes=0, poison=None):
    """arena.put, or a plain empty tensor: an Arena hands out no view of zero elements"""
    src = torch.as_tensor(src)
    return arena.put(src, misalign_bytes, poison) if src.numel() else src.to(arena.buf.device)


def carve(arena, shape, dtype, misalign_bytes=0):
    return arena.carve(shape, dtype, misalign_bytes) if int(np.prod(shape)) else torch.empty(shape, dtype=dtype, device=arena.buf.device)


# ---- a. voxel assign ------------------------------------------------------------------------------------------------------
def raw_voxel_assign(arena, points_np, geo):
    """pdm_voxel_assign on arena views -> dict of the sliced outputs"""
    arena.reset()
    nx, ny, nz = geo['grid']
    N, C1 = points_np.shape
    cap = min(N, geo['B'] * nx * ny * nz)
    pts = arena.put(points_np, misalign_bytes=4, poison=float('nan'))
    i32 = torch.int32
    o = {'kept_idx': arena.carve(N, i32, 4), 'unq_inv': arena.carve(N, i32, 8), 'voxel_coords': arena.carve((cap, 4), i32, 12),
         'voxel_count': arena.carve(cap, i32, 4), 'voxel_mean': arena.carve((cap, C1 - 1), torch.float32, 4), 'record': arena.carve(2, i32, 8)}
    nbytes = _native.lib().pdm_voxel_assign_workspace_bytes(N, C1, geo['B'], nx, ny, nz)
    ws = arena.carve(max(nbytes, 8), torch.uint8, 8)
    _native.call("pdm_voxel_assign", _native.stream(pts), N, C1, pts.data_ptr(), geo['B'], nx, ny, nz, *geo['range'][:3], *geo['voxel'],
                 o['kept_idx'].data_ptr(), o['unq_inv'].data_ptr(), o['voxel_coords'].data_ptr(), o['voxel_count'].data_ptr(),
                 o['voxel_mean'].data_ptr(), o['record'].data_ptr(), ws.data_ptr(), nbytes)
    torch.cuda.synchronize()
    arena.check()
    n_kept, P = o['record'].cpu().tolist()
    return {'kept_idx': o['kept_idx'][:n_kept].cpu().numpy(), 'unq_inv': o['unq_inv'][:n_kept].cpu().numpy(),
            'voxel_coords': o['voxel_coords'][:P].cpu().numpy(), 'voxel_count': o['voxel_count'][:P].cpu().numpy(),
            'voxel_mean': o['voxel_mean'][:P].cpu().numpy()}


@pytest.mark.parametrize("tag, C", [('v1', 4), ('v1', 5), ('v2', 4), ('v2', 5)])
def test_voxel_assign_matches_the_reference_exactly_and_its_means_within_the_fixed_point_bound(ref, arena, tag, C):
    """Exact: kept_idx, unq_inv, voxel_coords, voxel_count against the fixture (the reference's own DynamicMeanVFE) and two runs
    bit for bit.  Means against a float64 mean: |err| <= n 2^-23 max|v in the voxel| + 2^-20 with n the voxel's count: twice the
    first-order worst case of any fp32 summation order (the device sums exactly, in fixed point), plus the fixed-point step."""
    geo = scr.V1 if tag == 'v1' else scr.V2
    pts = np.ascontiguousarray(ref[f'{tag}.points'][:, :1 + C])
    got = raw_voxel_assign(arena, pts, geo)
    for k in ('kept_idx', 'unq_inv', 'voxel_coords', 'voxel_count'):
        assert np.array_equal(got[k], ref[f'{tag}.{k}']), k
    mean64 = ref[f'{tag}.mean64'][:, :C]
    vmax = np.zeros(mean64.shape)
    np.maximum.at(vmax, got['unq_inv'], np.abs(pts[got['kept_idx'], 1:]).astype(np.float64))
    bound = got['voxel_count'][:, None] * 2.0 ** -23 * vmax.max(1, keepdims=True) + 2.0 ** -20
    err = np.abs(got['voxel_mean'] - mean64)
    print(tag, C, 'voxels', len(mean64), 'max err / bound', float((err / bound).max()))
    assert (err <= bound).all()
    again = raw_voxel_assign(arena, pts, geo)
    for k, v in got.items():
        assert np.array_equal(v, again[k], equal_nan=True), k


def test_voxel_assign_of_no_point_and_of_an_all_empty_batch(dev):
    geo = scr.V1
    for pts in (torch.zeros((0, 5), device=dev), torch.full((7, 5), 100.0, device=dev)):
        before = sparse_conv_ops.HOST_READS
        v = sparse_conv_ops.voxel_assign(pts, geo['B'], geo['range'], geo['voxel'], geo['grid'])
        assert v.num_kept == 0 and v.num_voxels == 0 and v.voxel_coords.shape == (0, 4) and v.voxel_mean.shape == (0, 4)
        assert sparse_conv_ops.HOST_READS - before == 1


# ---- b. rulebook ------------------------------------------------------------------------------------------------------------
def raw_rulebook(arena, idx_np, geo):
    arena.reset()
    dev = arena.buf.device
    kernel, stride, padding, subm = geo
    D, H, W = scr.R1_SHAPE
    P = len(idx_np)
    idx = put(arena, idx_np.reshape(-1, 4), misalign_bytes=4, poison=[0, 1, 1, 1])
    g = (scr.R1_B, D, H, W, *kernel, *((1, 1, 1) if subm else stride), *padding, int(subm))
    nbytes = _native.lib().pdm_sparse_rulebook_workspace_bytes(P, *g)
    assert nbytes > 0
    ws = carve(arena, nbytes, torch.uint8, 8)
    record = carve(arena, 1, torch.int32, 4)
    _native.call("pdm_sparse_sites", _native.stream(dev), P, idx.data_ptr(), *g, record.data_ptr(), ws.data_ptr(), nbytes)
    P_out = P if subm else int(record.cpu())
    out_idx = carve(arena, (P_out, 4), torch.int32, 12)
    nbr = carve(arena, (P_out, 27 if kernel == (3, 3, 3) else 3), torch.int32, 4)
    _native.call("pdm_sparse_rulebook", _native.stream(dev), P, idx.data_ptr(), P_out, *g, None if subm else out_idx.data_ptr(), nbr.data_ptr(),
                 ws.data_ptr(), nbytes)
    torch.cuda.synchronize()
    arena.check()
    return (idx_np if subm else out_idx.cpu().numpy()), nbr.cpu().numpy()


@pytest.mark.parametrize("P", [0, 1, 63, 64, 65, None])
@pytest.mark.parametrize("name", list(scr.GEOMETRIES))
def test_rulebook_matches_the_numpy_restatement_entry_for_entry(arena, r1_books, name, P):
    """The set and order of output sites and every nbr entry, exactly, and two runs bit for bit.  The site list holds a voxel at
    x = W - 1 beside x = 0 of the next grid row and of the next sample: the restatement looks coordinates up in a dictionary, so
    it cannot wrap, and the device must agree."""
    idx = scr.r1_indices(P)
    want = r1_books[1][name] if P is None else scr.rulebook(idx, scr.R1_B, scr.R1_SHAPE, *scr.GEOMETRIES[name])
    out_idx, nbr = raw_rulebook(arena, idx, scr.GEOMETRIES[name])
    assert np.array_equal(out_idx.reshape(-1, 4), want[0].reshape(-1, 4))
    assert np.array_equal(nbr, want[1])
    again = raw_rulebook(arena, idx, scr.GEOMETRIES[name])
    assert np.array_equal(again[0], out_idx) and np.array_equal(again[1], nbr)
    if P is None and name == 'subm3':       # the wrap candidates are really there, and are no neighbours
        where = {tuple(c): i for i, c in enumerate(idx.tolist())}
        W = scr.R1_SHAPE[2]
        a, b = where[(0, 22, 6, W - 1)], where[(0, 22, 7, 0)]
        assert a not in nbr[b] and b not in nbr[a]
        c, d = where[(0, scr.R1_SHAPE[0] - 1, scr.R1_SHAPE[1] - 1, W - 1)], where[(2, 0, 0, 0)]
        assert c not in nbr[d] and d not in nbr[c]


def test_rulebook_host_reads(dev):
    idx = torch.from_numpy(scr.r1_indices()).to(dev)
    before = sparse_conv_ops.HOST_READS
    sparse_conv_ops.rulebook(idx, scr.R1_B, scr.R1_SHAPE, 3, 1, 1, subm=True)
    assert sparse_conv_ops.HOST_READS == before
    sparse_conv_ops.rulebook(idx, scr.R1_B, scr.R1_SHAPE, 3, 2, 1)
    assert sparse_conv_ops.HOST_READS == before + 1


# ---- c. convolution ---------------------------------------------------------------------------------------------------------
def conv_case(idx, book, geo, cin, cout, seed):
    """fp32 inputs of one convolution and its float64 references: y = F.conv3d, A = the same convolution of |x| with |w|"""
    rng = np.random.default_rng(seed)
    kernel, stride, padding, subm = geo
    out_idx, nbr, _ = book
    n = kernel[0] * kernel[1] * kernel[2] * cin
    x = rng.uniform(-1, 1, (len(idx), cin)).astype(np.float32)
    w = (rng.uniform(-1, 1, (cout, *kernel, cin)) / np.sqrt(n)).astype(np.float32)
    y = scr.conv_reference(x, idx, scr.R1_B, scr.R1_SHAPE, w, kernel, stride, padding, subm, out_idx)
    A = scr.conv_reference(np.abs(x), idx, scr.R1_B, scr.R1_SHAPE, np.abs(w), kernel, stride, padding, subm, out_idx)
    return dict(x=x, w=w, y=y, A=A, n=n, nbr=nbr,
                scale=rng.uniform(0.5, 1.5, cout).astype(np.float32) * rng.choice([-1, 1], cout).astype(np.float32),
                shift=rng.uniform(-0.5, 0.5, cout).astype(np.float32), res=rng.uniform(-1, 1, (len(out_idx), cout)).astype(np.float32))


def run_conv(arena, case, cin, cout, scale=None, shift=None, res=None, relu=False):
    arena.reset()
    dev = arena.buf.device
    x = put(arena, case['x'], misalign_bytes=4, poison=float('nan'))
    nbr = put(arena, case['nbr'], misalign_bytes=4, poison=0)
    out = carve(arena, (len(case['nbr']), cout), torch.float32, 4)
    wpack = sparse_conv_ops.pack_weight(torch.from_numpy(case['w']).to(dev))
    opt = [None if t is None else put(arena, t, misalign_bytes=4, poison=float('nan')) for t in (scale, shift, res)]
    sparse_conv_ops.sparse_conv(x, nbr, wpack, cin, cout, opt[0], opt[1], opt[2], relu, out=out)
    torch.cuda.synchronize()
    arena.check()
    return out.cpu().numpy()


def check_conv(arena, case, cin, cout):
    """The four epilogues.  |err| <= 2 n 2^-24 A with n = kvol Cin and A the float64 convolution of |x| with |w| (times |scale|
    when folded): twice the first-order worst case of any fp32 summation order of n products.  A shift adds the one rounding of
    the epilogue's fma, 2^-24 |y scale + shift|, and a residual the rounding of its addition, 2^-24 |out|: neither is part of A.
    ReLU is 1-Lipschitz and keeps the bound."""
    u, y, A, n = 2.0 ** -24, case['y'], case['A'], case['n']
    sc, sh, res = case['scale'].astype(np.float64), case['shift'].astype(np.float64), case['res'].astype(np.float64)
    worst = {}
    got = run_conv(arena, case, cin, cout)
    assert np.array_equal(got, run_conv(arena, case, cin, cout)), 'two runs differ'
    worst['none'] = np.abs(got - y) / np.maximum(2 * n * u * A, 1e-300)
    got = run_conv(arena, case, cin, cout, case['scale'], np.zeros_like(case['shift']))
    worst['scale'] = np.abs(got - y * sc) / np.maximum(2 * n * u * A * np.abs(sc), 1e-300)
    bn = y * sc + sh
    got = run_conv(arena, case, cin, cout, case['scale'], case['shift'], relu=True)
    worst['bn_relu'] = np.abs(got - np.maximum(bn, 0)) / (2 * n * u * A * np.abs(sc) + u * np.abs(bn))
    got = run_conv(arena, case, cin, cout, case['scale'], case['shift'], case['res'], relu=True)
    worst['bn_res_relu'] = np.abs(got - np.maximum(bn + res, 0)) / (2 * n * u * A * np.abs(sc) + u * np.abs(bn) + u * np.abs(bn + res))
    for k, v in worst.items():
        zero_ok = np.isfinite(v).all()
        print(f'  {k}: max err / bound {float(v.max()) if v.size else 0.0:.3f}')
        assert zero_ok and (v <= 1.0).all(), k


@pytest.mark.parametrize("cin, cout", CHANNELS)
@pytest.mark.parametrize("name", list(scr.GEOMETRIES))
def test_conv_matches_the_dense_convolution_in_float64(arena, r1_books, name, cin, cout):
    idx, books = r1_books
    case = conv_case(idx, books[name], scr.GEOMETRIES[name], cin, cout, seed=cin * 1000 + cout)
    print(name, cin, cout, 'sites', len(case['nbr']))
    check_conv(arena, case, cin, cout)


@pytest.mark.parametrize("P", [0, 1, 63, 64, 65])
def test_conv_at_the_row_tile_boundaries(arena, P):
    idx = scr.r1_indices(P)
    geo = scr.GEOMETRIES['subm3']
    case = conv_case(idx, scr.rulebook(idx, scr.R1_B, scr.R1_SHAPE, *geo), geo, 16, 32, seed=P)
    check_conv(arena, case, 16, 32)


def test_conv_known_answer_one_voxel_and_a_pair(dev):
    """Submanifold 3 x 3 x 3, Cin = 4, Cout = 16, W[c][k][0] = 1 where c == k mod 16 and 0 elsewhere: output channel c is the sum
    of input column 0 of the neighbours at the offsets k = c and k = c + 16 (columns 1-3 hold 100 and must not show).
    One voxel, value 3: its only neighbour is itself at the centre offset k = 13, so row = 3 at channel 13, zeros elsewhere.
    A pair A = (z 5, y 5, x 5) value 3 and B = (z 6, y 5, x 5) value 5: from A, B lies at (kz, ky, kx) = (2, 1, 1), k = 22 -> channel 6,
    so row A = 3 at channel 13 and 5 at channel 6; from B, A lies at (0, 1, 1), k = 4, so row B = 5 at channel 13 and 3 at channel 4."""
    w = torch.zeros((16, 27, 4), device=dev)
    for k in range(27):
        w[k % 16, k, 0] = 1.0
    wpack = sparse_conv_ops.pack_weight(w.reshape(16, 3, 3, 3, 4))

    def run(sites, values):
        idx = torch.tensor(sites, dtype=torch.int32, device=dev)
        x = torch.full((len(sites), 4), 100.0, device=dev)
        x[:, 0] = torch.tensor(values, device=dev)
        rb = sparse_conv_ops.rulebook(idx, 1, (41, 16, 21), 3, 1, 1, subm=True)
        return sparse_conv_ops.sparse_conv(x, rb.nbr, wpack, 4, 16).cpu().numpy()

    one = np.zeros((1, 16), dtype=np.float32)
    one[0, 13] = 3.0
    assert np.array_equal(run([(0, 5, 5, 5)], [3.0]), one)
    pair = np.zeros((2, 16), dtype=np.float32)
    pair[0, 13], pair[0, 6], pair[1, 13], pair[1, 4] = 3.0, 5.0, 5.0, 3.0
    assert np.array_equal(run([(0, 5, 5, 5), (0, 6, 5, 5)], [3.0, 5.0]), pair)


def test_three_chained_submanifold_layers_replay_from_a_graph_bit_for_bit(dev, r1_books):
    idx, books = r1_books
    rng = np.random.default_rng(3)
    nbr = torch.from_numpy(books['subm3'][1]).to(dev)
    x = torch.from_numpy(rng.uniform(-1, 1, (len(idx), 16)).astype(np.float32)).to(dev)
    dims = [(16, 32), (32, 32), (32, 64)]
    packs = [sparse_conv_ops.pack_weight(torch.from_numpy((rng.uniform(-1, 1, (co, 3, 3, 3, ci)) / np.sqrt(27 * ci)).astype(np.float32)).to(dev))
             for ci, co in dims]
    scales = [torch.from_numpy(rng.uniform(0.5, 1.5, co).astype(np.float32)).to(dev) for _, co in dims]
    shifts = [torch.from_numpy(rng.uniform(-0.2, 0.2, co).astype(np.float32)).to(dev) for _, co in dims]
    bufs = [torch.empty((len(idx), co), device=dev) for _, co in dims]

    def chain():
        h = x
        for (ci, co), wp, sc, sh, o in zip(dims, packs, scales, shifts, bufs):
            h = sparse_conv_ops.sparse_conv(h, nbr, wp, ci, co, sc, sh, relu=True, out=o)
        return h
    eager = chain().clone()
    assert float(eager.abs().max()) > 0
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        chain()
    for o in bufs:
        o.fill_(float('nan'))
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(bufs[-1], eager)


# ---- d. dense ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P, C", [(0, 16), (1, 3), (65, 128), (None, 16)])
def test_to_dense_equals_a_torch_scatter_exactly(arena, P, C):
    arena.reset()
    dev = arena.buf.device
    idx_np = scr.r1_indices(P)
    rng = np.random.default_rng(9)
    f = put(arena, rng.uniform(-1, 1, (len(idx_np), C)).astype(np.float32), misalign_bytes=4, poison=float('nan'))
    idx = put(arena, idx_np.reshape(-1, 4), misalign_bytes=4, poison=[0, 1, 1, 1])
    D, H, W = scr.R1_SHAPE
    out = carve(arena, (scr.R1_B, C, D, H, W), torch.float32, 4)
    sparse_conv_ops.to_dense(f, idx, scr.R1_B, scr.R1_SHAPE, out=out)
    torch.cuda.synchronize()
    arena.check()
    want = torch.zeros((scr.R1_B, D, H, W, C), device=dev)
    i = idx.long()
    want[i[:, 0], i[:, 1], i[:, 2], i[:, 3]] = f
    assert torch.equal(out, want.permute(0, 4, 1, 2, 3))


# ---- the backbones ------------------------------------------------------------------------------------------------------------
def built_backbone(name, manifest, dev):
    from pdm_ssd_amd import backbones_3d
    net = backbones_3d.__all__[name](model_cfg={}, input_channels=4, grid_size=scr.B1_GRID)
    fill = manifest[f'{name}.fill']
    assert abs(scr.fill_backbone(net, fill['seed'], fill['gain']) - fill['checksum']) <= 1e-9 * fill['checksum'], 'not the generator\'s parameters'
    return net.to(dev).eval()


@pytest.mark.parametrize("name", ['VoxelBackBone8x', 'VoxelResBackBone8x'])
def test_backbone_matches_the_reference_over_the_dense_convolution_stub(ref, manifest, dev, name):
    """Every level's sites, exactly and in the fixture's order (ascending key, which this build defines as well), and every
    level's features and spatial_features within 1e-4 absolute, the project's parity contract for fp32 features: the generator
    ran the reference in float32 and in float64 and found them within 2.5e-5 of each other, a quarter of the bound.  At most four
    host reads (one per strided convolution); a second forward gives the same bits."""
    from pdm_ssd_amd.backbones_2d.map_to_bev import HeightCompression
    net = built_backbone(name, manifest, dev)
    hc = HeightCompression({'NUM_BEV_FEATURES': 256})

    def forward():
        bd = {'voxel_features': torch.from_numpy(ref['b1.features']).to(dev), 'voxel_coords': torch.from_numpy(ref['b1.coords']).to(dev),
              'batch_size': scr.B1_B}
        with torch.no_grad():
            return hc(net(bd))
    before = sparse_conv_ops.HOST_READS
    bd = forward()
    assert sparse_conv_ops.HOST_READS - before == 4
    levels = dict(bd['multi_scale_3d_features'], out=bd['encoded_spconv_tensor'])
    for lv, t in levels.items():
        assert list(t.spatial_shape) == ref[f'{name}.{lv}.shape'].tolist(), lv
        assert np.array_equal(t.indices.cpu().numpy(), ref[f'{name}.{lv}.indices']), lv
        err = float(np.abs(t.features.cpu().numpy() - ref[f'{name}.{lv}.features']).max())
        print(name, lv, 'sites', len(t.indices), 'max err', err)
        assert err <= 1e-4, lv
    assert bd['encoded_spconv_tensor_stride'] == 8 and bd['multi_scale_3d_strides'] == {'x_conv1': 1, 'x_conv2': 2, 'x_conv3': 4, 'x_conv4': 8}
    sf = bd['spatial_features'].cpu().numpy()
    assert sf.shape == ref[f'{name}.spatial_features'].shape
    assert float(np.abs(sf - ref[f'{name}.spatial_features']).max()) <= 1e-4
    again = forward()
    assert torch.equal(again['spatial_features'], bd['spatial_features'])
    for lv in ('x_conv1', 'x_conv2', 'x_conv3', 'x_conv4'):
        assert torch.equal(again['multi_scale_3d_features'][lv].features, bd['multi_scale_3d_features'][lv].features), lv


def test_backbone_of_no_voxel(manifest, dev):
    net = built_backbone('VoxelBackBone8x', manifest, dev)
    bd = {'voxel_features': torch.zeros((0, 4), device=dev), 'voxel_coords': torch.zeros((0, 4), dtype=torch.int32, device=dev), 'batch_size': 2}
    with torch.no_grad():
        bd = net(bd)
    assert bd['encoded_spconv_tensor'].features.shape == (0, 128)
    dense = bd['encoded_spconv_tensor'].dense()
    assert dense.shape == (2, 128, 2, 2, 3) and float(dense.abs().max()) == 0.0


# ---- the detectors ------------------------------------------------------------------------------------------------------------
def d1_points(dev):
    rng = np.random.default_rng(21)
    n = 3000
    centres = rng.uniform([1, -3, -2.5], [15, 3, 0.5], (12, 3))
    p = centres[rng.integers(0, 12, n)] + rng.normal(0, 0.6, (n, 3))
    pts = np.concatenate([rng.integers(0, 2, (n, 1)), p, rng.uniform(0, 1, (n, 1))], 1).astype(np.float32)
    return torch.from_numpy(pts).to(dev)


@pytest.mark.parametrize("builder", ['build_second', 'build_center_voxel'])
def test_detector_eval_forward(dev, builder):
    """pred_dicts of the right length with finite boxes; spatial_features equal, bit for bit, to the separately tested pieces
    composed by hand (voxel_assign -> the backbone -> a torch scatter of the encoded tensor); at most 5 host reads from the points
    to the BEV map."""
    from pdm_ssd_amd import detector_config as dc
    torch.manual_seed(5)
    g = scr.D1
    cfg = copy.deepcopy(dc.SECOND_CFG if builder == 'build_second' else dc.CENTER_VOXEL_CFG)
    if builder == 'build_center_voxel':     # the BEV map of this shape has 2 x 4 cells: the head's top-K cannot exceed them
        cfg['DENSE_HEAD']['POST_PROCESSING']['MAX_OBJ_PER_SAMPLE'] = 8
    model = getattr(dc, builder)(cfg, dataset=dc.voxel_dataset(4, g['range'], g['voxel'], g['grid'])).to(dev).eval()
    want = ['DynamicMeanVFE', 'VoxelBackBone8x' if builder == 'build_second' else 'VoxelResBackBone8x', 'HeightCompression', 'BaseBEVBackbone',
            'AnchorHeadSingle' if builder == 'build_second' else 'CenterHead']
    assert [type(m).__name__ for m in model.module_list] == want
    pts = d1_points(dev)
    seen = {}
    model.map_to_bev_module.register_forward_hook(lambda m, a, out: seen.update(sf=out['spatial_features'], reads=sparse_conv_ops.HOST_READS))
    before = sparse_conv_ops.HOST_READS
    with torch.no_grad():
        pred, _ = model({'batch_size': g['B'], 'points': pts})
    assert 1 <= seen['reads'] - before <= 5
    assert len(pred) == g['B']
    for p in pred:
        assert p['pred_boxes'].shape[1] == 7 and torch.isfinite(p['pred_boxes']).all() and torch.isfinite(p['pred_scores']).all()
    assert seen['sf'].shape == (g['B'], 256, 2, 4)
    with torch.no_grad():
        vox = sparse_conv_ops.voxel_assign(pts, g['B'], g['range'], g['voxel'], g['grid'])
        enc = model.backbone_3d({'voxel_features': vox.voxel_mean, 'voxel_coords': vox.voxel_coords, 'batch_size': g['B']})['encoded_spconv_tensor']
    assert vox.num_voxels > 100 and enc.features.shape[0] > 0 and float(enc.features.abs().max()) > 0
    D, H, W = enc.spatial_shape
    dense = torch.zeros((g['B'], D, H, W, 128), device=dev)
    i = enc.indices.long()
    dense[i[:, 0], i[:, 1], i[:, 2], i[:, 3]] = enc.features
    assert torch.equal(seen['sf'], dense.permute(0, 4, 1, 2, 3).reshape(g['B'], 128 * D, H, W))

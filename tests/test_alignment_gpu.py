"""Every operator's unaligned and odd-size path, on tensors carved out of a poisoned arena (tests/arena.py).

The kernels pick their code path from `pointer & 15` and from whether a size divides by 4 or 8 ("Alignment and
divisibility contract").  Tensors from torch's allocator are 256-byte aligned and followed by slack, so the rest of the suite
runs one side of most of those branches and would not see a kernel that reads or writes a few elements past a buffer.  Here
  * class (a) pairs (handled: a scalar or narrower path) run with one pointer at a time off a 16-byte boundary, and with all
    of them, and are compared with the oracle / the fp64 torch expression of the operator's own test (same tolerance) and,
    where the fallback performs the same operations in the same order, bit for bit with the aligned call;
  * class (b) pairs (rejected) raise before anything is launched and leave the output untouched;
  * the other side of every size condition runs on aligned pointers.
Inputs sit between red zones whose content would change the result if it were used; Arena.check() after every call asserts
that no red zone of any tensor of the call was written.  Outputs are pre-filled, so an element the kernel skips is seen."""
import ctypes

import numpy as np
import pytest
import torch

from arena import Arena
from pdm_ssd_amd import _native
from pdm_ssd_amd.pointnet2_batch import pointnet2_batch_hip as ext
from pdm_ssd_amd.pointnet2_stack import pointnet2_stack_hip as sext

pytestmark = pytest.mark.gpu

NAN = float("nan")
_cache = {}


def cached(key, fn):
    """references and aligned results are computed once and shared by the cases that compare with them"""
    if key not in _cache:
        _cache[key] = fn()
    return _cache[key]


def sweep(*names):
    """all aligned, one pointer at a time 4 bytes off, all of them off (by 4, 8, 12, ...)"""
    out = [pytest.param({}, id="aligned")]
    out += [pytest.param({n: 4}, id=n + "+4") for n in names]
    out.append(pytest.param({n: (4, 8, 12)[k % 3] for k, n in enumerate(names)}, id="all"))
    return out


def done(arena):
    torch.cuda.synchronize()
    arena.check()


def lib():
    return _native.lib()


# ------------------------------------------------------------------ ball query

def bq_clouds(n, m, seed):
    """~8 points per unit volume, z in [10, 12]: a ball of radius 0.45 holds a handful of points (rows with padding) and a
    stale or zero coordinate is far from every centre.  Centre j is point n - 1 - j: the LAST point of the cloud is a centre,
    so it must come out of the last staged element.  One centre is far away (an empty ball)."""
    rng = np.random.default_rng(seed)
    side = float(np.sqrt(n / 15.6))
    xyz = np.stack([rng.uniform(0, side, (2, n)), rng.uniform(0, side, (2, n)), rng.uniform(10, 12, (2, n))], -1).astype(np.float32)
    new = np.ascontiguousarray(xyz[:, (n - 1 - np.arange(m)) % n])
    new[:, m // 2] += 100.0
    return xyz, new


def run_ball_query(dev, xyz, new, radius, ns, mis):
    B, n, _ = xyz.shape
    m = new.shape[1]
    a = Arena(dev)
    first = new[-1, 0]          # behind the last cloud: a "point" at distance 0 from its first centre, index >= n
    x = a.put(xyz, mis.get("xyz", 0), poison=first)
    c = a.put(new, mis.get("new_xyz", 0), poison=first)
    idx = a.carve((B, m, ns), torch.int32, mis.get("idx", 0))
    idx.fill_(-7)
    ext.ball_query_wrapper(B, n, m, radius, ns, c, x, idx)
    done(a)
    return idx.cpu().numpy()


SCAN_CASES = [(1001, 77, 16, {}), (70, 70, 8, {}), (70, 9, 8, {}), (70, 16500, 8, {}), (1000, 77, 16, {}),
              (1000, 77, 16, {"xyz": 4}), (1000, 77, 16, {"new_xyz": 4}), (1000, 77, 16, {"idx": 4}),
              (1000, 77, 16, {"xyz": 4, "new_xyz": 8, "idx": 12}), (1001, 77, 16, {"xyz": 12, "new_xyz": 4, "idx": 8})]


@pytest.mark.parametrize("n,m,ns,mis", SCAN_CASES, ids=lambda v: "-".join(f"{k}+{o}" for k, o in v.items()) or "aligned" if isinstance(v, dict) else str(v))
@pytest.mark.parametrize("radius", [0.45, 2.5])
def test_scan_ball_query_scalar_staging(oracle, dev, monkeypatch, n, m, ns, mis, radius):
    """ball_query.hip:55: the tile is staged 16 bytes at a time only when n % 4 == 0 and xyz is aligned.  n = 1001 and 70
    (and any n at xyz + 4) take the scalar loop; m = 9 / 70 / 16500 select the three instantiations of the kernel."""
    monkeypatch.setattr(ext, "GRID_MIN_N", 1 << 30)
    xyz, new = cached(("bq", n, m), lambda: bq_clouds(n, m, n + m))
    want = cached(("bq_ref", n, m, ns, radius), lambda: oracle.ball_query(radius, ns, xyz, new))
    if radius == 0.45:
        assert (want[:, 0] == n - 1).any(axis=-1).all(), "the last point must be among its own ball's first hits"
    got = run_ball_query(dev, xyz, new, radius, ns, mis)
    np.testing.assert_array_equal(got, want)


@pytest.mark.parametrize("form", [1, 2], ids=["quad", "lane"])
@pytest.mark.parametrize("ns,mis", [(6, {}), (16, {}), (16, {"idx": 4}), (16, {"xyz": 4, "new_xyz": 8, "idx": 12}), (6, {"idx": 8})],
                         ids=["ns6", "ns16", "ns16-idx+4", "ns16-all", "ns6-idx+8"])
def test_grid_ball_query_row_stores(oracle, dev, monkeypatch, form, ns, mis):
    """ball_query_grid.hip:572: the lane form writes a row with 16-byte stores only when nsample % 4 == 0 and idx is aligned."""
    monkeypatch.setattr(ext, "GRID_MIN_N", 1)
    xyz, new = cached(("bq", 1000, 77), lambda: bq_clouds(1000, 77, 1077))
    old = lib().pdm_tune_bq_quad(form)
    try:
        for radius in (0.45, 2.5):
            want = cached(("bq_ref", 1000, 77, ns, radius), lambda: oracle.ball_query(radius, ns, xyz, new))
            np.testing.assert_array_equal(run_ball_query(dev, xyz, new, radius, ns, mis), want)
    finally:
        lib().pdm_tune_bq_quad(old)


# ------------------------------------------------------------------ group_points

def gp_inputs(B, C, n, L0, L1, seed):
    rng = np.random.default_rng(seed)
    feat = rng.standard_normal((B, C, n)).astype(np.float32)
    idx = rng.integers(0, n, (B, L0, L1)).astype(np.int32)
    idx[:, 0, 0] = n - 1                 # the last element of every staged row is gathered
    idx[:, -1, -1] = n - 1
    return feat, idx


def run_group_points(dev, feat, idx, mis, tune=0, nbytes=32 << 20):
    B, C, n = feat.shape
    _, L0, L1 = idx.shape
    a = Arena(dev, nbytes)
    f = a.put(feat, mis.get("points", 0), poison=NAN)
    i = a.put(idx, mis.get("idx", 0), poison=0)
    out = a.carve((B, C, L0, L1), torch.float32, mis.get("out", 0))
    out.fill_(NAN)
    old = lib().pdm_tune_group_rows(tune)
    try:
        ext.group_points_wrapper(B, C, n, L0, L1, f, i, out)
    finally:
        lib().pdm_tune_group_rows(old)
    done(a)
    return out.cpu().numpy()


def gp_tune(variant, rpw=0, lsplit=0, threads=0, uq=0):
    return variant | rpw << 4 | lsplit << 8 | threads << 16 | uq << 20


@pytest.mark.parametrize("tune", [0, gp_tune(1, 1), gp_tune(2), gp_tune(3, 1)], ids=["heuristic", "rows", "lds", "rows-plain"])
@pytest.mark.parametrize("shape,mis", [((7, 301, 33, 5), {}), ((8, 300, 64, 16), {}), ((8, 300, 64, 16), {"points": 4}),
                                       ((8, 300, 64, 16), {"idx": 4}), ((8, 300, 64, 16), {"out": 4}),
                                       ((8, 300, 64, 16), {"points": 4, "idx": 8, "out": 12})],
                         ids=["C7-n301-L165", "C8-n300-L1024", "points+4", "idx+4", "out+4", "all"])
def test_group_points_small_shapes_every_variant(oracle, dev, shape, mis, tune):
    """group_points.hip:356: 16-byte index loads and stores need L % 4 == 0 and aligned idx / out.  At these shapes (two
    clouds, L < 4 n) every setting of pdm_tune_group_rows ends in the direct kernels: the dispatcher has no other choice."""
    C, n, L0, L1 = shape
    feat, idx = cached(("gp", shape), lambda: gp_inputs(2, C, n, L0, L1, C * n))
    want = cached(("gp_ref", shape), lambda: oracle.grouping_operation(feat, idx))
    np.testing.assert_array_equal(run_group_points(dev, feat, idx, mis, tune), want)


LDS_SHAPE = (64, 61, 63)      # 64 clouds x 61 rows of 63 floats: 512 workgroups of 8 rows, the last of 5; rows never 16-byte multiples
LDS_CASES = [
    ("rows-256x4", 64, 4, gp_tune(1, 1), {}), ("rows-uq1", 64, 4, gp_tune(1, 1, uq=1), {}), ("rows-uq2", 64, 4, gp_tune(1, 2, uq=2), {}),
    ("rows-512-split2", 64, 4, gp_tune(1, 3, lsplit=2, threads=2), {}), ("rows-1024", 64, 4, gp_tune(1, 1, threads=4), {}),
    ("rows-plain", 64, 4, gp_tune(3, 1), {}), ("lds-vector-gather", 64, 4, gp_tune(2), {}), ("heuristic-rows8", 64, 4, 0, {}),
    ("lds-scalar-gather-L255", 85, 3, 0, {}), ("lds-scalar-gather-L255-forced", 85, 3, gp_tune(2), {}),
    ("rows-asked-points+4", 64, 4, gp_tune(1, 1), {"points": 4}), ("lds-idx+4", 64, 4, gp_tune(2), {"idx": 4}),
    ("lds-out+4", 64, 4, gp_tune(2), {"out": 4}), ("lds-all", 64, 4, gp_tune(2), {"points": 12, "idx": 4, "out": 8}),
]


@pytest.mark.parametrize("name,L0,L1,tune,mis", LDS_CASES, ids=[c[0] for c in LDS_CASES])
def test_group_points_lds_forms(oracle, dev, name, L0, L1, tune, mis):
    """group_points.hip:147/156/238/328: the LDS-staged kernels stage a workgroup's rows 16 bytes at a time only when their
    size and address allow it (63-float rows: most workgroups take the scalar loop, those of every fourth cloud the vector
    one; the last workgroup of a cloud has 5 rows, an odd float count) and gather with 16-byte index loads / stores only
    for L % 4 == 0 and aligned idx / out.  The rows kernel is only chosen on aligned pointers with L % 4 == 0; every variant
    and decomposition pdm_tune_group_rows can ask for at this shape is run."""
    B, C, n = LDS_SHAPE
    feat, idx = cached(("gpl", L0, L1), lambda: gp_inputs(B, C, n, L0, L1, L0))
    want = cached(("gpl_ref", L0, L1), lambda: oracle.grouping_operation(feat, idx))
    np.testing.assert_array_equal(run_group_points(dev, feat, idx, mis, tune, 48 << 20), want)


@pytest.mark.parametrize("ns", [6, 16])
@pytest.mark.parametrize("mis", sweep("xyz", "new_xyz", "features", "idx", "out"))
def test_group_concat_direct_kernels(oracle, dev, ns, mis):
    """group_points.hip:420: query_group_v4_kernel needs nsample % 4 == 0 and aligned idx / out, else the element kernel."""
    B, n, m, C = 2, 1000, 77, 5
    xyz, new = cached(("bq", n, m), lambda: bq_clouds(n, m, n + m))
    feat = cached(("gc_feat", C, n), lambda: np.random.default_rng(3).standard_normal((B, C, n)).astype(np.float32))
    want, widx = cached(("gc_ref", ns), lambda: oracle.query_and_group(0.6, ns, xyz, new, feat))
    a = Arena(dev)
    x = a.put(xyz, mis.get("xyz", 0), poison=NAN)
    c = a.put(new, mis.get("new_xyz", 0), poison=NAN)
    f = a.put(feat, mis.get("features", 0), poison=NAN)
    i = a.put(widx, mis.get("idx", 0), poison=0)
    out = a.carve((B, 3 + C, m, ns), torch.float32, mis.get("out", 0))
    out.fill_(NAN)
    _native.call("pdm_group_concat", _native.stream(dev), B, n, m, C, ns, x.data_ptr(), c.data_ptr(), f.data_ptr(), i.data_ptr(), out.data_ptr())
    done(a)
    np.testing.assert_array_equal(out.cpu().numpy(), want)


@pytest.mark.parametrize("C,ld,out_bf16,feat_bf16,mis", [
    (5, 8, 1, 0, {}), (5, 8, 1, 0, {"out": 2}), (5, 8, 1, 0, {"out": 8}), (5, 8, 1, 1, {}), (5, 8, 1, 1, {"feat": 2}),
    (8, 11, 1, 0, {}), (8, 16, 1, 0, {"xyz": 4, "new_xyz": 8, "feat": 12, "idx": 4, "out": 14}), (8, 11, 0, 0, {}), (8, 11, 0, 0, {"out": 4}),
], ids=["cl8", "cl8-out+2", "cl8-out+8", "cl8-bf16feat", "cl8-bf16feat+2", "ld11-bf16", "ld16-all", "ld11-fp32", "ld11-fp32-out+4"])
def test_group_concat_channels_last_rows(oracle, dev, C, ld, out_bf16, feat_bf16, mis):
    """group_points.hip:544: eight bf16 channels per 16-byte store need ld % 8 == 0 and an aligned out; ld = 11 and an out at
    + 2 / + 8 bytes take the element kernel.  Bit-exact: the oracle's fp32 value rounded to nearest even, zeros in the padding."""
    B, n, m, ns = 2, 1000, 77, 16
    xyz, new = cached(("bq", n, m), lambda: bq_clouds(n, m, n + m))
    feat = cached(("gcl_feat", C), lambda: np.random.default_rng(C).standard_normal((B, C, n)).astype(np.float32))
    if feat_bf16:
        feat = torch.from_numpy(feat).bfloat16().float().numpy()
    want, widx = cached(("gcl_ref", C, feat_bf16), lambda: oracle.query_and_group(0.6, ns, xyz, new, feat))
    rows = torch.from_numpy(np.ascontiguousarray(feat.transpose(0, 2, 1)))
    a = Arena(dev)
    x = a.put(xyz, mis.get("xyz", 0), poison=NAN)
    c = a.put(new, mis.get("new_xyz", 0), poison=NAN)
    f = a.put(rows.bfloat16() if feat_bf16 else rows, mis.get("feat", 0), poison=NAN)
    i = a.put(widx, mis.get("idx", 0), poison=0)
    out = a.carve((B, m, ns, ld), torch.bfloat16 if out_bf16 else torch.float32, mis.get("out", 0))
    out.fill_(NAN)
    _native.call("pdm_group_concat_cl_ld_f", _native.stream(dev), B, n, m, C, ns, x.data_ptr(), c.data_ptr(), f.data_ptr(), feat_bf16,
                 i.data_ptr(), out.data_ptr(), out_bf16, ld)
    done(a)
    w = torch.from_numpy(want).permute(0, 2, 3, 1)
    got = out.cpu()
    assert torch.equal(got[..., :3 + C].float(), (w.bfloat16().float() if out_bf16 else w))
    assert ld == 3 + C or float(got[..., 3 + C:].float().abs().max()) == 0.0


@pytest.mark.parametrize("C,ld,bf16,mis", [(5, 8, 1, {}), (5, 8, 1, {"grad": 2}), (5, 8, 1, {"grad": 8}), (5, 8, 1, {"grad": 14, "idx": 4, "out": 12}),
                                          (8, 11, 1, {}), (8, 11, 1, {"grad": 2}), (5, 8, 0, {}), (5, 8, 0, {"grad": 4}), (5, 8, 0, {"out": 8})],
                         ids=["bf16x4", "bf16x4-grad+2", "bf16x4-grad+8", "bf16x4-all", "ld11-bf16", "ld11-bf16-grad+2", "fp32", "fp32-grad+4", "fp32-out+8"])
def test_group_concat_channels_last_grad(oracle, dev, C, ld, bf16, mis):
    """pdm_group_concat_cl_grad_ld (group_points.hip): a bf16 gradient is read as 8-byte words only when ld % 8 == 0 and grad is 16-byte aligned; ld = 11,
    a grad at + 2 / + 8 / + 14 bytes and an fp32 grad take gcl_grad_kernel.  Bound of tests/test_modules_gpu.py (1e-4 of the
    oracle's scatter-add: the CSR lists are filled through an LDS atomic cursor, the fp32 order is not fixed)."""
    B, n, m, ns = 2, 1000, 77, 16
    xyz, new = cached(("bq", n, m), lambda: bq_clouds(n, m, n + m))
    idx = cached(("bq_ref", n, m, ns, 0.6), lambda: oracle.ball_query(0.6, ns, xyz, new))
    go = torch.randn(B, m, ns, ld, generator=torch.Generator().manual_seed(ld + C))
    if bf16:
        go = go.bfloat16()
    want = cached(("gclg_ref", C, ld, bf16), lambda: oracle.grouping_operation_grad(
        np.ascontiguousarray(go[..., 3:3 + C].float().permute(0, 3, 1, 2).numpy()), idx, n).transpose(0, 2, 1))
    a = Arena(dev)
    g = a.put(go, mis.get("grad", 0), poison=NAN)
    i = a.put(idx, mis.get("idx", 0), poison=0)
    out = a.carve((B, n, C), torch.float32, mis.get("out", 0)); out.fill_(NAN)
    nbytes = lib().pdm_group_concat_cl_grad_ws_bytes(B, n, m, ns)
    ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=dev)
    _native.call("pdm_group_concat_cl_grad_ld", _native.stream(dev), B, n, m, C, ns, g.data_ptr(), bf16, ld, i.data_ptr(), out.data_ptr(),
                 ws.data_ptr(), nbytes)
    done(a)
    np.testing.assert_allclose(out.cpu().numpy(), want, rtol=1e-4, atol=1e-4)


# ------------------------------------------------------------------ the other batch operators (element kernels: every offset is the same path)

def nn_case():
    rng = np.random.default_rng(21)
    unknown = rng.uniform(0, 3, (2, 77, 3)).astype(np.float32)
    known = rng.uniform(0, 3, (2, 33, 3)).astype(np.float32)
    known[:, 5] = known[:, 6]
    return unknown, known


@pytest.mark.parametrize("mis", sweep("unknown", "known", "dist2", "idx"))
def test_three_nn(oracle, dev, mis):
    unknown, known = cached("nn", nn_case)
    wd, wi = cached("nn_ref", lambda: oracle.three_nn_dist2(unknown, known))
    a = Arena(dev)
    first = unknown[-1, 0]      # behind the last known set: a "point" at distance 0 from the first query, index >= m
    u = a.put(unknown, mis.get("unknown", 0), poison=first)
    k = a.put(known, mis.get("known", 0), poison=first)
    d = a.carve((2, 77, 3), torch.float32, mis.get("dist2", 0)); d.fill_(NAN)
    i = a.carve((2, 77, 3), torch.int32, mis.get("idx", 0)); i.fill_(-7)
    ext.three_nn_wrapper(2, 77, 33, u, k, d, i)
    done(a)
    np.testing.assert_array_equal(i.cpu().numpy(), wi)
    np.testing.assert_array_equal(d.cpu().numpy(), wd)


def interp_case():
    rng = np.random.default_rng(22)
    feat = rng.standard_normal((2, 5, 33)).astype(np.float32)
    idx = rng.integers(0, 33, (2, 77, 3)).astype(np.int32)
    idx[:, -1] = 32
    w = rng.uniform(0, 1, (2, 77, 3)).astype(np.float32)
    w /= w.sum(-1, keepdims=True)
    go = rng.standard_normal((2, 5, 77)).astype(np.float32)
    return feat, idx, w, go


@pytest.mark.parametrize("mis", sweep("points", "idx", "weight", "out"))
def test_three_interpolate_and_grad(oracle, dev, mis):
    feat, idx, w, go = cached("ti", interp_case)
    want = cached("ti_ref", lambda: oracle.three_interpolate(feat, idx, w))
    wantg = cached("ti_gref", lambda: oracle.three_interpolate_grad(go, idx, w, 33))
    a = Arena(dev)
    f = a.put(feat, mis.get("points", 0), poison=NAN)
    i = a.put(idx, mis.get("idx", 0), poison=0)
    ww = a.put(w, mis.get("weight", 0), poison=NAN)
    out = a.carve((2, 5, 77), torch.float32, mis.get("out", 0)); out.fill_(NAN)
    ext.three_interpolate_wrapper(2, 5, 33, 77, f, i, ww, out)
    done(a)
    np.testing.assert_array_equal(out.cpu().numpy(), want)
    g = a.put(go, mis.get("out", 0), poison=NAN)
    gp = a.carve((2, 5, 33), torch.float32, mis.get("points", 0)); gp.zero_()
    ext.three_interpolate_grad_wrapper(2, 5, 77, 33, g, i, ww, gp)
    done(a)
    np.testing.assert_allclose(gp.cpu().numpy(), wantg, rtol=1e-4, atol=1e-4)       # tests/test_ops_gpu.py's bound


@pytest.mark.parametrize("mis", sweep("points", "idx", "out"))
def test_gather_points_and_grads(oracle, dev, mis):
    rng = np.random.default_rng(23)
    feat = rng.standard_normal((2, 5, 77)).astype(np.float32)
    idx = rng.integers(0, 77, (2, 33)).astype(np.int32)
    idx[:, -1] = 76
    go = rng.standard_normal((2, 5, 33)).astype(np.float32)
    a = Arena(dev)
    f = a.put(feat, mis.get("points", 0), poison=NAN)
    i = a.put(idx, mis.get("idx", 0), poison=0)
    out = a.carve((2, 5, 33), torch.float32, mis.get("out", 0)); out.fill_(NAN)
    ext.gather_points_wrapper(2, 5, 77, 33, f, i, out)
    done(a)
    np.testing.assert_array_equal(out.cpu().numpy(), oracle.gather_operation(feat, idx))
    g = a.put(go, mis.get("out", 0), poison=NAN)
    gp = a.carve((2, 5, 77), torch.float32, mis.get("points", 0)); gp.zero_()
    ext.gather_points_grad_wrapper(2, 5, 77, 33, g, i, gp)
    done(a)
    np.testing.assert_allclose(gp.cpu().numpy(), oracle.gather_operation_grad(go, idx, 77), rtol=1e-5, atol=1e-5)
    # group_points_grad: (B, C, M, ns) -> (B, C, N), the CSR form and (without a workspace) the LDS / atomic forms
    gidx = rng.integers(0, 77, (2, 11, 3)).astype(np.int32)
    ggo = rng.standard_normal((2, 5, 11, 3)).astype(np.float32)
    gi = a.put(gidx, mis.get("idx", 0), poison=0)
    gg = a.put(ggo, mis.get("out", 0), poison=NAN)
    want = oracle.grouping_operation_grad(ggo, gidx, 77)
    for entry in ("wrapper", "pdm_group_points_grad"):
        gp.zero_()
        if entry == "wrapper":
            ext.group_points_grad_wrapper(2, 5, 77, 11, 3, gg, gi, gp)
        else:
            _native.call(entry, _native.stream(dev), 2, 5, 77, 11, 3, gg.data_ptr(), gi.data_ptr(), gp.data_ptr())
        done(a)
        np.testing.assert_allclose(gp.cpu().numpy(), want, rtol=1e-4, atol=1e-4)


# ------------------------------------------------------------------ stack operators (element kernels)

def stack_case():
    rng = np.random.default_rng(31)
    counts, mcounts = [150, 0, 77], [20, 0, 13]
    xyz = np.concatenate([np.stack([rng.uniform(0, 3, c), rng.uniform(0, 3, c), rng.uniform(10, 12, c)], -1) for c in counts]).astype(np.float32)
    starts = np.concatenate([[0], np.cumsum(counts)])
    new = np.concatenate([xyz[starts[b + 1] - m:starts[b + 1]][::-1] for b, m in enumerate(mcounts)]).astype(np.float32)
    new[3] += 100.0
    feats = rng.standard_normal((xyz.shape[0], 5)).astype(np.float32)
    return counts, mcounts, xyz, np.ascontiguousarray(new), feats


@pytest.mark.parametrize("mis", sweep("xyz", "new_xyz", "cnt", "idx", "features", "out"))
def test_stack_ball_query_and_group(oracle, dev, mis):
    counts, mcounts, xyz, new, feats = cached("stack", stack_case)
    ns, M, N = 7, new.shape[0], xyz.shape[0]
    ridx, rmask = cached("stack_bq", lambda: oracle.stack_ball_query(0.7, ns, xyz, counts, new, mcounts))
    a = Arena(dev)
    x = a.put(xyz, mis.get("xyz", 0), poison=new[-1])
    c = a.put(new, mis.get("new_xyz", 0), poison=new[-1])
    xc = a.put(np.array(counts, np.int32), mis.get("cnt", 0), poison=0)
    nc = a.put(np.array(mcounts, np.int32), mis.get("cnt", 0), poison=0)
    idx = a.carve((M, ns), torch.int32, mis.get("idx", 0)); idx.zero_()
    sext.ball_query_wrapper(3, M, 0.7, ns, c, nc, x, xc, idx)
    done(a)
    got = idx.cpu().numpy()
    empty = got[:, 0] == -1
    got[empty] = 0
    np.testing.assert_array_equal(got, ridx)
    np.testing.assert_array_equal(empty, rmask)
    assert rmask[3] and not rmask.all()
    f = a.put(feats, mis.get("features", 0), poison=NAN)
    i = a.put(ridx, mis.get("idx", 0), poison=0)
    out = a.carve((M, 5, ns), torch.float32, mis.get("out", 0)); out.fill_(NAN)
    sext.group_points_wrapper(3, M, 5, ns, f, xc, i, nc, out)
    done(a)
    np.testing.assert_array_equal(out.cpu().numpy(), oracle.stack_grouping_operation(feats, counts, ridx, mcounts))
    go = np.random.default_rng(32).standard_normal((M, 5, ns)).astype(np.float32)
    g = a.put(go, mis.get("out", 0), poison=NAN)
    gf = a.carve((N, 5), torch.float32, mis.get("features", 0)); gf.zero_()
    sext.group_points_grad_wrapper(3, M, 5, N, ns, g, i, nc, xc, gf)
    done(a)
    np.testing.assert_allclose(gf.cpu().numpy(), oracle.stack_grouping_operation_grad(go, ridx, mcounts, counts, N), rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize("mis", sweep("unknown", "known", "cnt", "dist2", "idx", "features", "weight", "out"))
def test_stack_three_nn_and_interpolate(oracle, dev, mis):
    counts, mcounts, xyz, new, feats = cached("stack", stack_case)
    ucounts, kcounts = counts, [20, 0, 2]                    # the last sample has only two known points: +inf and a repeated index
    known = np.ascontiguousarray(np.concatenate([new[:20], new[20:22]]))
    rd, ri = cached("stack_nn", lambda: oracle.stack_three_nn(xyz, ucounts, known, kcounts))
    N = xyz.shape[0]
    a = Arena(dev)
    u = a.put(xyz, mis.get("unknown", 0), poison=xyz[-1])
    k = a.put(known, mis.get("known", 0), poison=xyz[-1])
    uc = a.put(np.array(ucounts, np.int32), mis.get("cnt", 0), poison=0)
    kc = a.put(np.array(kcounts, np.int32), mis.get("cnt", 0), poison=0)
    d = a.carve((N, 3), torch.float32, mis.get("dist2", 0)); d.fill_(NAN)
    i = a.carve((N, 3), torch.int32, mis.get("idx", 0)); i.fill_(-7)
    sext.three_nn_wrapper(u, uc, k, kc, d, i)
    done(a)
    np.testing.assert_array_equal(i.cpu().numpy(), ri)
    np.testing.assert_array_equal(torch.sqrt(d).cpu().numpy(), rd)
    rng = np.random.default_rng(33)
    kf = rng.standard_normal((known.shape[0], 9)).astype(np.float32)
    w = rng.uniform(0, 1, ri.shape).astype(np.float32)
    w /= w.sum(1, keepdims=True)
    f = a.put(kf, mis.get("features", 0), poison=NAN)
    ww = a.put(w, mis.get("weight", 0), poison=NAN)
    ii = a.put(ri, mis.get("idx", 0), poison=0)
    out = a.carve((N, 9), torch.float32, mis.get("out", 0)); out.fill_(NAN)
    sext.three_interpolate_wrapper(f, ii, ww, out)
    done(a)
    np.testing.assert_allclose(out.cpu().numpy(), oracle.stack_three_interpolate(kf, ri, w), rtol=1e-6, atol=1e-6)   # tests/test_stack_gpu.py's bounds
    go = rng.standard_normal((N, 9)).astype(np.float32)
    g = a.put(go, mis.get("out", 0), poison=NAN)
    gf = a.carve((known.shape[0], 9), torch.float32, mis.get("features", 0)); gf.zero_()
    sext.three_interpolate_grad_wrapper(g, ii, ww, gf)
    done(a)
    np.testing.assert_allclose(gf.cpu().numpy(), oracle.stack_three_interpolate_grad(go, ri, w, known.shape[0]), rtol=1e-4, atol=1e-5)


# ------------------------------------------------------------------ interp_concat_rows (the bf16 rows of the FP modules)

def icr_case(c2, c1, kb, sb, ld):
    B, n, m = 2, 150, 40
    rng = np.random.default_rng(c2 + c1)
    unknown = rng.uniform(0, 3, (B, n, 3)).astype(np.float32)
    known = np.ascontiguousarray(unknown[:, :m]) + np.float32(0.05)
    g = torch.Generator().manual_seed(c2 * 100 + c1)
    kf = torch.randn(B, m, c2, generator=g)
    sf = torch.randn(B, n, c1, generator=g) if c1 else None
    if kb:
        kf = kf.bfloat16().float()
    if sb and c1:
        sf = sf.bfloat16().float()
    dx = torch.randn(B, n, ld, generator=g).bfloat16()
    return unknown, known, kf, sf, dx


ICR = [(12, 5, 0, 1, 24, {}), (12, 5, 0, 1, 24, {"known": 8, "skip": 2, "idx": 4, "weight": 12, "out": 2}),
       (16, 0, 0, 0, 16, {}), (16, 0, 0, 0, 16, {"known": 8}), (16, 0, 0, 0, 16, {"out": 2}), (16, 0, 0, 0, 16, {"out": 8}),
       (16, 0, 1, 0, 16, {}), (16, 0, 1, 0, 16, {"known": 2}), (16, 0, 1, 0, 16, {"known": 8}), (16, 0, 1, 0, 16, {"known": 2, "out": 8, "idx": 4, "weight": 8}),
       (16, 1, 0, 0, 17, {}), (16, 1, 0, 0, 17, {"known": 8}), (16, 1, 0, 0, 17, {"out": 2}), (16, 1, 1, 1, 17, {}), (16, 1, 1, 1, 17, {"known": 2, "skip": 2, "out": 8}),
       (16, 1, 0, 0, 20, {}), (16, 1, 0, 0, 20, {"out": 8}), (16, 1, 1, 0, 20, {"known": 2})]


@pytest.mark.parametrize("c2,c1,kb,sb,ld,mis", ICR, ids=[f"c2={c[0]}-c1={c[1]}-ld={c[4]}-{'bf16' if c[2] else 'fp32'}-" + ("-".join(f"{k}+{o}" for k, o in c[5].items()) or "aligned") for c in ICR])
def test_interp_concat_rows_and_grad(oracle, dev, c2, c1, kb, sb, ld, mis):
    """pdm_interp_concat_rows (interpolate.hip): eight channels per thread need c2 % 8 == 0, ld % 8 == 0 and aligned known / out; c2 = 12 and a
    known / out at + 2 or + 8 bytes take the element kernel.  Forward bit-exact against the oracle's pinned fma order rounded to
    bf16; ld = 17 and 20 (c2 = 16, c1 = 1: rows that start at 2-byte granularity) are the other side of ld % 8.  The
    backward's eight-channel form has the same conditions on c2, ld, dx and dknown, decided on the host.  Its CSR lists are filled through an LDS atomic cursor, so the order of a known point's terms — and with
    it the last bits of the fp32 sums — changes from launch to launch even on the same pointers: no bit comparison with
    the aligned call is possible, the bound is tests/test_modules_gpu.py's 1e-4 of the oracle (2e-2 for a bf16 result)."""
    B, n, m = 2, 150, 40
    unknown, known, kf, sf, dx = cached(("icr", c2, c1, kb, sb, ld), lambda: icr_case(c2, c1, kb, sb, ld))
    dist, idx = cached(("icr_nn", c2, c1), lambda: oracle.three_nn(unknown, known))
    w = 1.0 / (dist + 1e-8)
    w = (w / w.sum(2, keepdims=True)).astype(np.float32)
    a = Arena(dev)
    k = a.put(kf.bfloat16() if kb else kf, mis.get("known", 0), poison=NAN)
    s = None if sf is None else a.put(sf.bfloat16() if sb else sf, mis.get("skip", 0), poison=NAN)
    i = a.put(idx, mis.get("idx", 0), poison=0)
    ww = a.put(w, mis.get("weight", 0), poison=NAN)
    out = a.carve((B, n, ld), torch.bfloat16, mis.get("out", 0)); out.fill_(NAN)
    _native.call("pdm_interp_concat_rows", _native.stream(dev), B, n, m, c2, c1, ld, k.data_ptr(), kb, 0 if s is None else s.data_ptr(), sb,
                 i.data_ptr(), ww.data_ptr(), out.data_ptr())
    done(a)
    interp = torch.from_numpy(oracle.three_interpolate(np.ascontiguousarray(kf.numpy().transpose(0, 2, 1)), idx, w)).permute(0, 2, 1)
    want = interp if sf is None else torch.cat([interp, sf], 2)
    got = out.cpu().float()
    assert torch.equal(got[..., :c2 + c1], want.bfloat16().float())
    assert ld == c2 + c1 or float(got[..., c2 + c1:].abs().max()) == 0.0
    # backward: dx (B, n, ld) bf16 -> dknown (B, m, c2), fp32 and bf16 results
    nbytes = lib().pdm_three_interpolate_grad_ws_bytes(B, n, m)
    ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=dev)
    g = a.put(dx, mis.get("out", 0), poison=NAN)
    ref = oracle.three_interpolate_grad(np.ascontiguousarray(dx[..., :c2].float().numpy().transpose(0, 2, 1)), idx, w, m).transpose(0, 2, 1)
    for ob, dt in ((0, torch.float32), (1, torch.bfloat16)):
        def grad(moff, goff):
            dk = a.carve((B, m, c2), dt, moff); dk.fill_(NAN)
            _native.call("pdm_interp_concat_rows_grad_out", _native.stream(dev), B, n, m, c2, ld, goff.data_ptr(), i.data_ptr(), ww.data_ptr(),
                         dk.data_ptr(), ob, ws.data_ptr(), nbytes)
            done(a)
            return dk.cpu()
        koff = mis.get("known", 0)
        got = grad(koff if koff % (2 if ob else 4) == 0 else 8, g)
        assert not bool(torch.isnan(got.float()).any())          # every row of dknown is written
        tol = 2e-2 if ob else 1e-4           # tests/test_modules_gpu.py: a bf16 gradient is the fp32 one rounded
        np.testing.assert_allclose(got.float().numpy(), ref, rtol=tol, atol=tol)


# ------------------------------------------------------------------ MLP kernels

def mlp_case(rows, cin, widths, relu_last):
    from pdm_ssd_amd import fused
    torch.manual_seed(rows + cin)
    chans = [cin] + widths
    seq = torch.nn.Sequential(*[mod for i in range(len(widths)) for mod in
                                (torch.nn.Conv1d(chans[i], chans[i + 1], 1, bias=False), torch.nn.BatchNorm1d(chans[i + 1]), torch.nn.ReLU())]).eval()
    g = torch.Generator().manual_seed(2)
    for mod in seq.modules():
        if isinstance(mod, torch.nn.BatchNorm1d):
            with torch.no_grad():
                mod.weight.copy_(torch.rand(mod.weight.shape, generator=g) + 0.5); mod.bias.copy_(torch.randn(mod.bias.shape, generator=g) * 0.1)
                mod.running_mean.copy_(torch.randn(mod.bias.shape, generator=g) * 0.1); mod.running_var.copy_(torch.rand(mod.bias.shape, generator=g) + 0.5)
    x = torch.randn(rows, cin)
    with torch.no_grad():
        y = x.double().t().unsqueeze(0)
        mods = list(seq.double())
        for i, mod in enumerate(mods):
            if i == len(mods) - 1 and not relu_last:
                break
            y = mod(y)
        ref = y[0].t().float()
    seq.float()
    return x, ref, fused.split_shared_mlp(seq)


def run_rows_mlp(dev, case, relu_last, mis, nbytes=32 << 20):
    from pdm_ssd_amd import fused
    x, ref, layers = case
    pk = cached(("pk", id(case)), lambda: fused.PackedMLP(layers, dev))
    a = Arena(dev, nbytes)
    xin = a.put(x, mis.get("in", 0), poison=NAN)
    out = a.carve((x.shape[0], pk.dims[-1] + 4), torch.float32, mis.get("out", 0)); out.fill_(7.0)
    try:
        fused.rows_forward(pk, xin, out, relu_last=relu_last)
    except _native.NativeLibraryError:
        done(a)
        assert bool((out == 7.0).all()), "a rejected call must leave the output as it was"
        raise
    done(a)
    return out.cpu()


@pytest.mark.parametrize("rows,cin,widths,mis,handled", [
    (37, 8, [16], {}, True), (37, 8, [16], {"in": 4}, False), (37, 8, [16], {"out": 4}, False), (37, 7, [16], {"in": 4}, True),
    (37, 7, [16], {"in": 12}, True), (32768, 32, [64], {}, True), (32768, 32, [64], {"in": 4}, True), (32768, 32, [64], {"in": 8}, True),
    (32768, 32, [64], {"out": 4}, False), (32768, 30, [64], {"in": 4}, True)],
    ids=["37x8", "37x8-in+4", "37x8-out+4", "37x7-in+4", "37x7-in+12", "gemm", "gemm-in+4", "gemm-in+8", "gemm-out+4", "gemm-cin30-in+4"])
def test_rows_mlp_fused(dev, rows, cin, widths, mis, handled):
    """fused_mlp.hip:1450 / rows_gemm.hip:77.  The general kernel reads a row 16 bytes at a time when cin % 4 == 0 and then
    REJECTS an unaligned `in` (rows = 37, cin = 8 at + 4: class (b)); cin = 7 reads by elements at any offset.  The LDS-tiled
    GEMM (one layer, >= 256 tiles: 32768 rows) chooses in the kernel and handles `in` at + 4 / + 8 with element loads of the
    same values: bit-equal to the aligned call.  `out` must be aligned everywhere.  1e-4 of torch in fp64
    (tests/test_fused_gpu.py's bound)."""
    case = cached(("mlp", rows, cin), lambda: mlp_case(rows, cin, widths, False))
    big = 64 << 20 if rows > 1000 else 32 << 20
    if not handled:
        with pytest.raises(_native.NativeLibraryError, match="rows_mlp_fused: buffers must be 16-byte aligned"):
            run_rows_mlp(dev, case, False, mis, big)
        return
    out = run_rows_mlp(dev, case, False, mis, big)
    torch.testing.assert_close(out[:, :widths[-1]], case[1], rtol=1e-4, atol=1e-4)
    assert bool((out[:, widths[-1]:] == 7.0).all())
    assert torch.equal(out, cached(("mlp_aligned", rows, cin), lambda: run_rows_mlp(dev, case, False, {}, big)))


# ------------------------------------------------------------------ PDM neck

BEV = (2, 22, 25)       # B, H, W


def bev_case(C):
    g = torch.Generator().manual_seed(C)
    B, H, W = BEV
    x = torch.randn(B, H, W, C, generator=g)
    w = torch.randn(B, H, W, 1, generator=g)
    w[torch.rand(w.shape, generator=g) < 0.3] = 0.0
    dy = torch.randn(B, H, W, C, generator=g)
    x1, w1 = x.double().requires_grad_(True), w.double().requires_grad_(True)
    on = w1.abs() > 1e-6
    ref = torch.where(on, x1 / torch.where(on, w1, torch.ones_like(w1)), x1)
    ref.backward(dy.double())
    return x, w, dy, ref.detach().float(), x1.grad.float(), w1.grad.float()


@pytest.mark.parametrize("C", [8, 5])
@pytest.mark.parametrize("mis", sweep("grid", "wsum", "y", "dy", "dx", "dwsum"))
def test_bev_normalize_and_grad(dev, C, mis):
    """pdm_scatter.hip:434 / :522: the float4 kernels need C * D % 4 == 0 (C = 5: never) and aligned grid / y / dy / dx.
    Values: x *= 1 / w in every form (bit-equal); dx = dy * (1 / w) likewise; dwsum is a wave reduction in another order in
    the float4 form, so it keeps the bound of tests/test_pdm_gpu.py (1e-4)."""
    B, H, W = BEV
    x, w, dy, ref, rdx, rdw = cached(("bev", C), lambda: bev_case(C))

    def run(mis):
        a = Arena(dev)
        grid = a.put(x, mis.get("grid", 0))                  # in place: input and output, the red zones are an output's
        ws = a.put(w, mis.get("wsum", 0), poison=0.0)        # a stray weight of 0 leaves a cell unnormalised
        _native.call("pdm_bev_normalize", _native.stream(dev), B, C, W, H, 1, 1, 1e-6, grid.data_ptr(), ws.data_ptr())
        done(a)
        y = a.put(grid, mis.get("y", 0), poison=NAN)
        g = a.put(dy, mis.get("dy", 0), poison=NAN)
        dx = a.carve((B, H, W, C), torch.float32, mis.get("dx", 0)); dx.fill_(NAN)
        dw = a.carve((B, H, W, 1), torch.float32, mis.get("dwsum", 0)); dw.fill_(NAN)
        _native.call("pdm_bev_normalize_grad", _native.stream(dev), B, C, W, H, 1, 1e-6, y.data_ptr(), ws.data_ptr(), g.data_ptr(),
                     dx.data_ptr(), dw.data_ptr())
        done(a)
        dw2 = a.carve((B, H, W, 1), torch.float32, mis.get("dwsum", 0)); dw2.fill_(NAN)
        _native.call("pdm_bev_normalize_grad", _native.stream(dev), B, C, W, H, 1, 1e-6, y.data_ptr(), ws.data_ptr(), g.data_ptr(), 0, dw2.data_ptr())
        done(a)
        return grid.cpu(), dx.cpu(), dw.cpu(), dw2.cpu()

    y, dx, dw, dw2 = run(mis)
    ay, adx, adw, _ = cached(("bev_aligned", C), lambda: run({}))
    assert torch.equal(y, ay) and torch.equal(dx, adx)
    torch.testing.assert_close(y, ref, rtol=1e-6, atol=1e-6)
    torch.testing.assert_close(dx, rdx, rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(dw, rdw, rtol=1e-4, atol=1e-4)
    torch.testing.assert_close(dw2, rdw, rtol=1e-4, atol=1e-4)      # dx = NULL (dwsum only) counts as aligned


PDM_RANGE = (0.0, -40.0, -3.0, 70.4, 40.0, 1.0)


def pdm_case(C):
    rng = np.random.default_rng(C)
    B, P, degree = 2, 150, 2
    xyz = np.stack([rng.uniform(0, 70.4, (B, P)), rng.uniform(-40, 40, (B, P)), rng.uniform(-3, 1, (B, P))], -1).astype(np.float32)
    xyz[:, 0] = [-0.3, -39.9, 0.9]
    xyz[:, 3] = [70.39, 39.99, 0.99]
    xyz[:, 4] = xyz[:, 5]
    feat = rng.standard_normal((B, P, C)).astype(np.float32)
    sh = (rng.standard_normal((B, P, 9)) * 0.5).astype(np.float32)
    sh[..., 0] += 3.0
    sigma = rng.uniform(0.3, 1.5, (B, P)).astype(np.float32)
    return xyz, feat, sh, (0.5 / (sigma * sigma)).astype(np.float32)


@pytest.mark.parametrize("C", [8, 6])
@pytest.mark.parametrize("mis", sweep("xyz", "feat", "sh", "inv2s2", "grid", "wsum"))
def test_pdm_gather_bev(oracle, dev, C, mis):
    """pdm_gather.hip:306: a point's C features are staged 16 bytes at a time when C % 4 == 0 and feat is aligned.  A pure copy into LDS: bit-equal to the aligned call; 1e-4 of the oracle's scale
    (tests/test_pdm_gpu.py)."""
    from pdm_ssd_amd import pdm_ops
    cell, kernel, degree = (3.2, 3.2, 4.0), (3, 3, 1), 2
    g = pdm_ops.BevGrid(PDM_RANGE, cell)
    xyz, feat, sh, inv = cached(("pdm", C), lambda: pdm_case(C))
    origin, cellf, inv_cell, dims = oracle.pdm_grid_params(PDM_RANGE, cell)
    rg, rw = cached(("pdm_ref", C), lambda: oracle.pdm_scatter(xyz, feat, sh, inv, origin, cellf, inv_cell, dims, kernel, degree, 1))
    B, P = xyz.shape[:2]

    def run(mis):
        a = Arena(dev)
        t = [a.put(v, mis.get(k, 0), poison=NAN) for k, v in (("xyz", xyz), ("feat", feat), ("sh", sh), ("inv2s2", inv))]
        grid = a.carve((B, g.H, g.W, C), torch.float32, mis.get("grid", 0)); grid.fill_(NAN)
        wsum = a.carve((B, g.H, g.W, 1), torch.float32, mis.get("wsum", 0)); wsum.fill_(NAN)
        nbytes = lib().pdm_gather_bev_workspace_bytes(B, P, g.W, g.H, kernel[0], kernel[1])
        ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=dev)
        _native.call("pdm_gather_bev", _native.stream(dev), B, P, C, degree, *[v.data_ptr() for v in t], *g.floats(), g.W, g.H, g.D, *kernel,
                     0, 1e-6, grid.data_ptr(), wsum.data_ptr(), ws.data_ptr(), nbytes)
        done(a)
        return grid.cpu(), wsum.cpu()

    grid, wsum = run(mis)
    ag, aw = cached(("pdm_gather_aligned", C), lambda: run({}))
    assert torch.equal(grid, ag) and torch.equal(wsum, aw)
    np.testing.assert_allclose(grid.numpy(), rg, rtol=1e-4, atol=1e-4 * np.abs(rg).max())
    np.testing.assert_allclose(wsum.numpy(), rw, rtol=1e-4, atol=1e-4 * np.abs(rw).max())


@pytest.mark.parametrize("C", [8, 7])
@pytest.mark.parametrize("mis", sweep("feat", "dgrid", "dfeat", "dsh"))
def test_pdm_scatter_bev_grad(oracle, dev, C, mis):
    """pdm_scatter.hip:283: with one height bin and an even C a lane owns a channel PAIR (8-byte loads of feat / dgrid, 8-byte
    stores of dfeat) only when the three are 8-byte aligned; at + 4 the element form runs.
    Bound of tests/test_pdm_gpu.py::test_scatter_grad_matches_oracle."""
    from pdm_ssd_amd import pdm_ops
    cell, kernel, degree = (3.2, 3.2, 4.0), (3, 3, 1), 2
    g = pdm_ops.BevGrid(PDM_RANGE, cell)
    xyz, feat, sh, inv = cached(("pdm", C), lambda: pdm_case(C))
    origin, cellf, inv_cell, dims = oracle.pdm_grid_params(PDM_RANGE, cell)
    B, P = xyz.shape[:2]
    rng = np.random.default_rng(1)
    dgrid = rng.standard_normal((B, g.H, g.W, C)).astype(np.float32)
    dwsum = rng.standard_normal((B, g.H, g.W, 1)).astype(np.float32)
    refs = cached(("pdm_gref", C), lambda: oracle.pdm_scatter_grad(xyz, feat, sh, inv, origin, cellf, inv_cell, dims, kernel, degree, dgrid, dwsum, 1))
    a = Arena(dev)
    x = a.put(xyz, 0, poison=NAN)
    f = a.put(feat, mis.get("feat", 0), poison=NAN)
    s = a.put(sh, 0, poison=NAN)
    i2 = a.put(inv, 0, poison=NAN)
    dg = a.put(dgrid, mis.get("dgrid", 0), poison=NAN)
    dw = a.put(dwsum, 0, poison=NAN)
    df = a.carve((B, P, C), torch.float32, mis.get("dfeat", 0)); df.fill_(NAN)
    ds = a.carve((B, P, 9), torch.float32, mis.get("dsh", 0)); ds.fill_(NAN)
    di = a.carve((B, P), torch.float32, 0); di.fill_(NAN)
    _native.call("pdm_scatter_bev_grad", _native.stream(dev), B, P, C, degree, x.data_ptr(), f.data_ptr(), s.data_ptr(), i2.data_ptr(),
                 *g.floats(), g.W, g.H, g.D, *kernel, 1, dg.data_ptr(), dw.data_ptr(), df.data_ptr(), ds.data_ptr(), di.data_ptr())
    done(a)
    for got, ref in zip((df, ds, di), refs):
        np.testing.assert_allclose(got.cpu().numpy(), ref, rtol=1e-3, atol=1e-4 * max(1.0, np.abs(ref).max()))


# ------------------------------------------------------------------ helpers: pdm_copy_many

@pytest.mark.parametrize("variant", [-1, 7])
@pytest.mark.parametrize("soff", [0, 1, 4, 15])
@pytest.mark.parametrize("doff", [0, 1, 4, 15])
def test_copy_many_offsets_and_tails(dev, soff, doff, variant):
    """api.hip:95: 16-byte pieces only when source AND destination are aligned, then a byte tail; bytes otherwise.  1 byte
    (tail only), 4099 (256 pieces + 3 bytes: no whole tile) and 65537 (four / two whole tiles + 1 byte) in one launch."""
    a = Arena(dev)
    g = torch.Generator().manual_seed(soff * 16 + doff)
    pairs = []
    for n in (1, 4099, 65537):
        data = torch.randint(0, 256, (n,), dtype=torch.uint8, generator=g)
        src = a.put(data, soff, poison=0x5A)
        dst = a.carve((n,), torch.uint8, doff)
        dst.copy_(data ^ 0xFF)                      # every byte differs from what must arrive
        pairs.append((data, src, dst))
    old = lib().pdm_tune_copy_variant(variant)
    try:
        _native.copy_many([p[2] for p in pairs], [p[1] for p in pairs])
    finally:
        lib().pdm_tune_copy_variant(old)
    done(a)
    for data, src, dst in pairs:
        assert torch.equal(dst.cpu(), data) and torch.equal(src.cpu(), data)


# ------------------------------------------------------------------ class (b): rejected on the host, nothing launched

def _dims(*v):
    return _native.host_array(ctypes.c_int, v)


def rej_tg_gemm_nt(a, which):
    off = {"X": (2, 0, 0), "W": (0, 8, 0), "Y": (0, 0, 4)}[which]
    X = a.carve((8, 8), torch.bfloat16, off[0], poison=NAN); W = a.carve((8, 8), torch.bfloat16, off[1], poison=NAN)
    Y = a.carve((8, 8), torch.bfloat16, off[2])
    return "tg_gemm_nt", (8, 8, 8, X.data_ptr(), 8, W.data_ptr(), 8, Y.data_ptr(), 8, 0, 0, 0), [Y]


def rej_tg_wgrad(a, which):
    off = {"dY": (2, 0, 0, 0), "X": (0, 8, 0, 0), "workspace": (0, 0, 8, 0), "x_bn_coef": (0, 0, 0, 4)}[which]
    dY = a.carve((8, 8), torch.bfloat16, off[0], poison=NAN); X = a.carve((8, 8), torch.bfloat16, off[1], poison=NAN)
    dW = a.carve((8, 8), torch.float32, 0)
    nbytes = lib().pdm_tg_wgrad_ws_bytes(8, 8, 8)
    ws = a.carve((nbytes,), torch.uint8, off[2])
    coef = a.carve((4, 8), torch.float32, off[3], poison=NAN)
    return "tg_wgrad", (8, 8, 8, dY.data_ptr(), 8, X.data_ptr(), 8, dW.data_ptr(), 0, ws.data_ptr(), nbytes, coef.data_ptr()), [dW, ws]


def rej_bn_relu_forward(a, which):
    off = {"x": (4, 0, 0, 0), "y": (0, 8, 0, 0), "coef": (0, 0, 4, 0), "partial": (0, 0, 0, 4)}[which]
    x = a.carve((4, 8), torch.float32, off[0], poison=NAN); y = a.carve((4, 8), torch.float32, off[1])
    coef = a.carve((4, 8), torch.float32, off[2])
    partial = a.carve((lib().pdm_bn_parts(0, 4, 8, 1), 8, 2), torch.float32, off[3])
    return "bn_relu_forward", (0, 0, 4, 8, 1, x.data_ptr(), y.data_ptr(), 0, 0, 1e-5, 0.1, 0, 0, coef.data_ptr(), partial.data_ptr(), 1), [y, coef, partial]


def rej_bn_relu_backward(a, which):
    off = {"dy": (4, 0, 0), "dx": (0, 12, 0), "grads": (0, 0, 8)}[which]
    x = a.carve((4, 8), torch.float32, 0, poison=NAN); dy = a.carve((4, 8), torch.float32, off[0], poison=NAN)
    dx = a.carve((4, 8), torch.float32, off[1]); coef = a.carve((4, 8), torch.float32, 0, poison=NAN)
    grads = a.carve((4, 8), torch.float32, off[2])
    partial = a.carve((lib().pdm_bn_parts(0, 4, 8, 1), 8, 2), torch.float32, 0)
    return "bn_relu_backward", (0, 0, 4, 8, 1, x.data_ptr(), dy.data_ptr(), dx.data_ptr(), coef.data_ptr(), grads.data_ptr(), partial.data_ptr(), 1), [dx, grads, partial]


def rej_bn_finalize_stats(a, which):
    coef = a.carve((4, 8), torch.float32, 0)
    partial = a.carve((1, 8, 2), torch.float32, 4, poison=NAN)
    return "bn_finalize_stats", (4, 8, 0, 0, 1e-5, 0.1, 0, 0, coef.data_ptr(), partial.data_ptr(), 1), [coef]


def rej_bev_depthwise3x3(a, which):
    off = {"in": (4, 0, 0, 0), "w": (0, 4, 0, 0), "shift": (0, 0, 8, 0), "out": (0, 0, 0, 12)}[which]
    x = a.carve((1, 2, 2, 4), torch.float32, off[0], poison=NAN); w = a.carve((9, 4), torch.float32, off[1], poison=NAN)
    s = a.carve((4,), torch.float32, off[2], poison=NAN); out = a.carve((1, 2, 2, 4), torch.float32, off[3])
    return "bev_depthwise3x3", (1, 2, 2, 4, x.data_ptr(), w.data_ptr(), s.data_ptr(), out.data_ptr(), 1), [out]


def rej_bev_depthwise3x3_wgrad(a, which):
    x = a.carve((1, 2, 2, 4), torch.float32, 0, poison=NAN); g = a.carve((1, 2, 2, 4), torch.float32, 4, poison=NAN)
    gw = a.carve((9, 4), torch.float32, 0)
    return "bev_depthwise3x3_wgrad", (1, 2, 2, 4, x.data_ptr(), g.data_ptr(), gw.data_ptr()), [gw]


def rej_point_head_decode(a, which):
    cls = a.carve((2, 3), torch.float32, 0, poison=NAN); code = a.carve((2, 8), torch.float32, 4, poison=NAN)
    pts = a.carve((2, 3), torch.float32, 0, poison=NAN); mean = a.carve((3, 3), torch.float32, 0, poison=NAN)
    boxes = a.carve((2, 7), torch.float32, 0); scores = a.carve((2,), torch.float32, 0)
    return "point_head_decode", (2, 3, cls.data_ptr(), 3, code.data_ptr(), 8, pts.data_ptr(), 3, mean.data_ptr(), boxes.data_ptr(), scores.data_ptr()), [boxes, scores]


def rej_rows_mlp_x3(a, which):
    dims = _dims(128, 256, 256, 16)
    nbytes = lib().pdm_rows_mlp_x3_stream_bytes(3, dims)
    x = a.carve((1, 128), torch.float32, 4, poison=NAN); ws = a.carve((nbytes,), torch.uint8, 0, poison=0)
    bias = a.carve((528,), torch.float32, 0, poison=NAN); out = a.carve((1, 16), torch.float32, 0)
    return "rows_mlp_x3", (1, 128, x.data_ptr(), 3, dims, ws.data_ptr(), nbytes, bias.data_ptr(), 0, out.data_ptr(), 16, 16), [out]


def rej_bev_head_fused(a, which):
    dims = _dims(128, 64, 64, 16)
    m = a.carve((1, 1, 1, 128), torch.float32, 4, poison=NAN); w = a.carve((9, 128), torch.float32, 0, poison=NAN)
    s = a.carve((128,), torch.float32, 0, poison=NAN); wp = a.carve((128 * 64 + 64 * 64 + 64 * 16,), torch.float32, 0, poison=NAN)
    b = a.carve((144,), torch.float32, 0, poison=NAN); out = a.carve((1, 16), torch.float32, 0)
    return "bev_head_fused", (1, 1, 1, 128, m.data_ptr(), w.data_ptr(), s.data_ptr(), 3, dims, wp.data_ptr(), b.data_ptr(), 0, out.data_ptr(), 16, 16), [out]


def rej_fp_head_fused(a, which):
    dims, hdims = _dims(16, 128, 128), _dims(128, 256, 256, 16)
    z = a.carve((1, 128), torch.float32, 4, poison=NAN); idx = a.carve((1, 3), torch.int32, 0, poison=0); w = a.carve((1, 3), torch.float32, 0, poison=NAN)
    wp = a.carve((16 * 128 + 128 * 128,), torch.float32, 0, poison=NAN); b = a.carve((256,), torch.float32, 0, poison=NAN)
    hw = [a.carve((128 * 256 + 256 * 256 + 256 * 16,), torch.float32, 0, poison=NAN) for _ in range(2)]
    hb = [a.carve((528,), torch.float32, 0, poison=NAN) for _ in range(2)]
    out = a.carve((1, 128), torch.float32, 0); oa = a.carve((1, 16), torch.float32, 0); ob = a.carve((1, 16), torch.float32, 0)
    return "fp_head_fused", (1, 1, 1, 0, z.data_ptr(), 128, 0, idx.data_ptr(), w.data_ptr(), dims, wp.data_ptr(), b.data_ptr(), out.data_ptr(), 128, 128,
                             hdims, hw[0].data_ptr(), hb[0].data_ptr(), hw[1].data_ptr(), hb[1].data_ptr(), 0, oa.data_ptr(), 16, 16, ob.data_ptr(), 16, 16), [out, oa, ob]


def rej_sa_pack(a, which):
    off = {"idx": (4, 0, 0), "pack": (0, 4, 0), "workspace": (0, 0, 4)}[which]
    idx = a.carve((1, 2, 16), torch.int32, off[0], poison=0)
    nbytes = lib().pdm_sa_pack_workspace_bytes(1, 2)
    ws = a.carve((max(nbytes, 16),), torch.uint8, off[2])
    pack = a.carve((lib().pdm_sa_pack_rows(1, 2, 16), 2), torch.int32, off[1]); meta = a.carve((8,), torch.int32, 0)
    return "sa_pack", (1, 4, 2, 16, idx.data_ptr(), ws.data_ptr(), nbytes, pack.data_ptr(), meta.data_ptr()), [pack, meta, ws]


def rej_kitti_data_fov_count(a, which):
    raw = a.carve((2, 4), torch.float32, 4 if which == "raw" else 0, poison=NAN); counts = a.carve((1,), torch.int32, 0, poison=0)
    cal = [a.carve(s, torch.float32, 0, poison=NAN) for s in ((1, 3, 4), (1, 3, 3), (1, 3, 4))]
    shape = a.carve((1, 2), torch.int32, 0, poison=0); oc = a.carve((1,), torch.int32, 0); ov = a.carve((1,), torch.int32, 0)
    nbytes = lib().pdm_kitti_data_fov_workspace_bytes(1)
    ws = a.carve((nbytes,), torch.uint8, 4 if which == "workspace" else 0)
    return "kitti_data_fov_count", (1, 4, 2, raw.data_ptr(), counts.data_ptr(), *[c.data_ptr() for c in cal], shape.data_ptr(), 2, oc.data_ptr(),
                                    ov.data_ptr(), 0, ws.data_ptr(), nbytes), [oc, ov, ws]


def rej_sa_mlp_fused(a, which):
    dims = _dims(16, 16)
    xyz = a.carve((1, 4, 3), torch.float32, 0, poison=NAN); new = a.carve((1, 1, 3), torch.float32, 0, poison=NAN)
    feat = a.carve((1, 4, 4), torch.float32, 4 if which == "feat_pm" else 0, poison=NAN)      # cin = 4: rows read 16 bytes at a time
    idx = a.carve((1, 1, 16), torch.int32, 0, poison=0); wp = a.carve((256,), torch.float32, 0, poison=NAN); b = a.carve((16,), torch.float32, 0, poison=NAN)
    out = a.carve((1, 1, 16), torch.float32, 4 if which == "out" else 0)
    return "sa_mlp_fused", (1, 4, 1, 4, 16, xyz.data_ptr(), new.data_ptr(), feat.data_ptr(), idx.data_ptr(), 1, dims, wp.data_ptr(), b.data_ptr(), out.data_ptr(), 16, 0, 16), [out]


def rej_sa_mlp_packed(a, which):
    dims = _dims(16, 16)
    xyz = a.carve((1, 4, 3), torch.float32, 0, poison=NAN); new = a.carve((1, 1, 3), torch.float32, 0, poison=NAN)
    pack = a.carve((lib().pdm_sa_pack_rows(1, 1, 16), 2), torch.int32, 4, poison=0); meta = a.carve((8,), torch.int32, 0, poison=0)
    wp = a.carve((256,), torch.float32, 0, poison=NAN); b = a.carve((16,), torch.float32, 0, poison=NAN); out = a.carve((1, 1, 16), torch.float32, 0)
    return "sa_mlp_packed", (1, 4, 1, 0, 16, xyz.data_ptr(), new.data_ptr(), 0, 0, 0, 0, pack.data_ptr(), meta.data_ptr(), 1, dims, wp.data_ptr(), b.data_ptr(),
                             out.data_ptr(), 16, 0, 16), [out]


def rej_fp_mlp_fused(a, which):
    dims = _dims(16, 16)
    off = {"known": (4, 0, 0), "out": (0, 8, 0), "skip_pm": (0, 0, 12)}[which]
    known = a.carve((1, 2, 4), torch.float32, off[0], poison=NAN); idx = a.carve((1, 1, 3), torch.int32, 0, poison=0)
    skip = a.carve((1, 1, 4), torch.float32, off[2], poison=NAN)                                  # c_skip = 4: read 16 bytes at a time
    w = a.carve((1, 1, 3), torch.float32, 0, poison=NAN); wp = a.carve((256,), torch.float32, 0, poison=NAN); b = a.carve((16,), torch.float32, 0, poison=NAN)
    out = a.carve((1, 1, 16), torch.float32, off[1])
    return "fp_mlp_fused", (1, 1, 2, 4, 4, known.data_ptr(), skip.data_ptr(), idx.data_ptr(), w.data_ptr(), 1, dims, wp.data_ptr(), b.data_ptr(), out.data_ptr(), 16, 16), [out]


def rej_heatmap_focal_loss(a, which):
    logits = a.carve((1, 1, 2, 2), torch.float32, 0, poison=NAN); hm = a.carve((1, 1, 2, 2), torch.float32, 0, poison=NAN)
    dl = a.carve((1, 1, 2, 2), torch.float32, 0); out = a.carve((3,), torch.float32, 0)
    nbytes = lib().pdm_heatmap_focal_loss_workspace_bytes(4)
    ws = a.carve((nbytes,), torch.uint8, 4)
    return "heatmap_focal_loss", (1, 1, 2, 2, logits.data_ptr(), 0, 4, 4, 2, 1, hm.data_ptr(), 1.0, dl.data_ptr(), out.data_ptr(), ws.data_ptr(), nbytes), [dl, out, ws]


def rej_center_reg_loss(a, which):
    ch = a.carve((1, 1, 1), torch.float32, 0, poison=NAN)
    inds = a.carve((1, 1), torch.int64, 0, poison=0); mask = a.carve((1, 1), torch.int64, 0, poison=0); target = a.carve((1, 1, 1), torch.float32, 0, poison=NAN)
    lpc = a.carve((1,), torch.float32, 0); out = a.carve((3,), torch.float32, 0); grad = a.carve((1, 1, 1, 1), torch.float32, 0)
    nbytes = lib().pdm_center_reg_loss_workspace_bytes(1, 1)
    ws = a.carve((nbytes,), torch.uint8, 4)
    return "center_reg_loss", (1, 1, 1, 1, 1, _native.host_array(ctypes.c_void_p, [ch.data_ptr()]), _dims(0), _native.host_array(ctypes.c_longlong, [1, 1, 1]),
                               inds.data_ptr(), mask.data_ptr(), target.data_ptr(), _native.host_array(ctypes.c_float, [1.0]), 1.0, lpc.data_ptr(), out.data_ptr(),
                               grad.data_ptr(), ws.data_ptr(), nbytes), [lpc, out, grad, ws]


def rej_tg_gemm_nt_pool(a, which):
    X = a.carve((8, 8), torch.bfloat16, 0, poison=NAN); W = a.carve((8, 8), torch.bfloat16, 0, poison=NAN); Y = a.carve((8, 8), torch.bfloat16, 0)
    xmax = a.carve((2, 8), torch.bfloat16, 0); xmin = a.carve((2, 8), torch.bfloat16, 0)
    imax = a.carve((2, 8), torch.uint8, 4 if which == "imax" else 0); imin = a.carve((2, 8), torch.uint8, 4 if which == "imin" else 0)
    return "tg_gemm_nt_pool", (8, 8, 8, X.data_ptr(), 8, W.data_ptr(), 8, Y.data_ptr(), 8, 0, 0, 0, 4, xmax.data_ptr(), xmin.data_ptr(), imax.data_ptr(),
                               imin.data_ptr()), [Y, xmax, xmin, imax, imin]


def rej_tg_gemm_nt_dy(a, which):
    off = {"dZ": (2, 0, 0), "dYout": (0, 8, 0), "coef": (0, 0, 4)}[which]
    dZ = a.carve((8, 8), torch.bfloat16, off[0], poison=NAN); Yp = a.carve((8, 8), torch.bfloat16, 0, poison=NAN); W = a.carve((8, 8), torch.bfloat16, 0, poison=NAN)
    dX = a.carve((8, 8), torch.bfloat16, 0); dYo = a.carve((8, 8), torch.bfloat16, off[1])
    coef = a.carve((4, 8), torch.float32, off[2], poison=NAN); grads = a.carve((4, 8), torch.float32, 0, poison=NAN)
    return "tg_gemm_nt_dy", (8, 8, 8, dZ.data_ptr(), 8, Yp.data_ptr(), 8, W.data_ptr(), 8, dX.data_ptr(), 8, dYo.data_ptr(), 8, coef.data_ptr(), grads.data_ptr()), [dX, dYo]


def rej_tg_colsum(a, which):
    Y = a.carve((8, 8), torch.bfloat16, 2, poison=NAN); out = a.carve((8,), torch.float32, 0)
    scratch = a.carve((lib().pdm_tg_colsum_ws_floats(8, 8),), torch.float32, 0)
    return "tg_colsum", (8, 8, Y.data_ptr(), 8, out.data_ptr(), scratch.data_ptr()), [out, scratch]


def _kitti_frames(a):
    raw = a.carve((2, 4), torch.float32, 0, poison=NAN); counts = a.carve((1,), torch.int32, 0, poison=0)
    cal = [a.carve(s, torch.float32, 0, poison=NAN) for s in ((1, 3, 4), (1, 3, 3), (1, 3, 4))]
    shape = a.carve((1, 2), torch.int32, 0, poison=0)
    return (1, 4, 2, raw.data_ptr(), counts.data_ptr(), *[c.data_ptr() for c in cal], shape.data_ptr())


def rej_kitti_data_fov_fill(a, which):
    frames = _kitti_frames(a)
    oc = a.carve((1,), torch.int32, 0); ov = a.carve((1,), torch.int32, 0); rows = a.carve((2, 4), torch.float32, 4)
    nbytes = lib().pdm_kitti_data_fov_workspace_bytes(1)
    ws = a.carve((nbytes,), torch.uint8, 0)
    return "kitti_data_fov_fill", (*frames, 2, oc.data_ptr(), ov.data_ptr(), rows.data_ptr(), ws.data_ptr(), nbytes), [oc, ov, rows, ws]


def rej_kitti_data_boxes_fill(a, which):
    frames = _kitti_frames(a)
    boxes = a.carve((1, 1, 7), torch.float32, 0, poison=NAN); bc = a.carve((1,), torch.int32, 0, poison=0); centres = a.carve((1, 1, 3), torch.float64, 0, poison=NAN)
    npg = a.carve((1, 1), torch.int32, 0); dbc = a.carve((1, 1), torch.int32, 0); totals = a.carve((2,), torch.int64, 0)
    pts = a.carve((2, 4), torch.float32, 4); offs = a.carve((2,), torch.int64, 0); ob = a.carve((1, 7), torch.float32, 0)
    nbytes = lib().pdm_kitti_data_boxes_workspace_bytes(1, 1)
    ws = a.carve((nbytes,), torch.uint8, 0)
    return "kitti_data_boxes_fill", (*frames, 1, boxes.data_ptr(), bc.data_ptr(), centres.data_ptr(), npg.data_ptr(), dbc.data_ptr(), totals.data_ptr(), 2, 1,
                                     pts.data_ptr(), offs.data_ptr(), ob.data_ptr(), ws.data_ptr(), nbytes), [npg, dbc, totals, pts, offs, ob, ws]


def rej_nms(a, which):
    boxes = a.carve((2, 7), torch.float32, 0, poison=NAN); keep = a.carve((2,), torch.int64, 0); num = a.carve((1,), torch.int32, 0)
    nbytes = lib().pdm_nms_workspace_bytes(2)
    ws = a.carve((nbytes,), torch.uint8, 4)
    return "nms", (2, boxes.data_ptr(), 0.5, 0, ws.data_ptr(), nbytes, keep.data_ptr(), num.data_ptr()), [keep, num, ws]


def rej_furthest_point_sampling_jobs(a, which):
    n = 16385
    pts = a.carve((1, n, 3), torch.float32, 0, poison=NAN); temp = a.carve((1, n), torch.float32, 0); idx = a.carve((1, 2), torch.int32, 0)
    nbytes = lib().pdm_furthest_point_sampling_ws_bytes(1, n)
    ws = a.carve((nbytes,), torch.uint8, 4)
    P = lambda t: _native.host_array(ctypes.c_void_p, [t.data_ptr()])
    return "fps_jobs", (1, 1, n, 2, P(pts), P(temp), P(idx), _dims(1), _dims(2), P(ws), nbytes), [temp, idx, ws]


def rej_group_concat_cl_ld_f(a, which):
    xyz = a.carve((1, 4, 3), torch.float32, 0, poison=NAN); new = a.carve((1, 1, 3), torch.float32, 0, poison=NAN)
    feat = a.carve((1, 4, 5), torch.bfloat16, 0, poison=NAN); idx = a.carve((1, 1, 4), torch.int32, 0, poison=0)
    out = a.carve((1, 1, 4, 8), torch.bfloat16, 2)
    return "group_concat_cl", (1, 4, 1, 5, 4, xyz.data_ptr(), new.data_ptr(), feat.data_ptr(), 1, idx.data_ptr(), out.data_ptr(), 1, 8), [out]


def rej_furthest_point_sampling_ws(a, which):
    n = 16385
    pts = a.carve((1, n, 3), torch.float32, 0, poison=NAN); temp = a.carve((1, n), torch.float32, 0); idx = a.carve((1, 1), torch.int32, 0)
    nbytes = lib().pdm_furthest_point_sampling_ws_bytes(1, n)
    ws = a.carve((nbytes,), torch.uint8, 4)
    return "fps_ws", (1, n, 1, pts.data_ptr(), temp.data_ptr(), idx.data_ptr(), ws.data_ptr(), nbytes), [temp, idx, ws]


REJECTED = [("pdm_tg_gemm_nt", rej_tg_gemm_nt, w) for w in ("X", "W", "Y")] + [("pdm_tg_wgrad", rej_tg_wgrad, w) for w in ("dY", "X", "workspace", "x_bn_coef")] + \
           [("pdm_tg_gemm_nt_pool", rej_tg_gemm_nt_pool, w) for w in ("imax", "imin")] + [("pdm_tg_gemm_nt_dy", rej_tg_gemm_nt_dy, w) for w in ("dZ", "dYout", "coef")] + \
           [("pdm_tg_colsum", rej_tg_colsum, "Y"), ("pdm_heatmap_focal_loss", rej_heatmap_focal_loss, "workspace"), ("pdm_center_reg_loss", rej_center_reg_loss, "workspace"),
            ("pdm_sa_mlp_packed", rej_sa_mlp_packed, "pack"), ("pdm_sa_mlp_fused", rej_sa_mlp_fused, "feat_pm"), ("pdm_fp_mlp_fused", rej_fp_mlp_fused, "skip_pm"),
            ("pdm_kitti_data_fov_fill", rej_kitti_data_fov_fill, "out_rows"), ("pdm_kitti_data_boxes_fill", rej_kitti_data_boxes_fill, "out_points"),
            ("pdm_kitti_data_fov_count", rej_kitti_data_fov_count, "workspace"), ("pdm_sa_pack", rej_sa_pack, "workspace"), ("pdm_nms", rej_nms, "workspace"),
            ("pdm_furthest_point_sampling_jobs", rej_furthest_point_sampling_jobs, "workspace")] + \
           [("pdm_bn_relu_forward", rej_bn_relu_forward, w) for w in ("x", "y", "coef", "partial")] + \
           [("pdm_bn_relu_backward", rej_bn_relu_backward, w) for w in ("dy", "dx", "grads")] + \
           [("pdm_bn_finalize_stats", rej_bn_finalize_stats, "partial")] + \
           [("pdm_bev_depthwise3x3", rej_bev_depthwise3x3, w) for w in ("in", "w", "shift", "out")] + \
           [("pdm_bev_depthwise3x3_wgrad", rej_bev_depthwise3x3_wgrad, "gout"), ("pdm_point_head_decode", rej_point_head_decode, "code"),
            ("pdm_rows_mlp_x3", rej_rows_mlp_x3, "in"), ("pdm_bev_head_fused", rej_bev_head_fused, "map"), ("pdm_fp_head_fused", rej_fp_head_fused, "z"),
            ("pdm_sa_pack", rej_sa_pack, "idx"), ("pdm_sa_pack", rej_sa_pack, "pack"), ("pdm_kitti_data_fov_count", rej_kitti_data_fov_count, "raw"),
            ("pdm_sa_mlp_fused", rej_sa_mlp_fused, "out"), ("pdm_fp_mlp_fused", rej_fp_mlp_fused, "known"), ("pdm_fp_mlp_fused", rej_fp_mlp_fused, "out"),
            ("pdm_group_concat_cl_ld_f", rej_group_concat_cl_ld_f, "out"), ("pdm_furthest_point_sampling_ws", rej_furthest_point_sampling_ws, "workspace")]


@pytest.mark.parametrize("entry,build,which", REJECTED, ids=[f"{e[0]}-{e[2]}" for e in REJECTED])
def test_rejecting_operators_refuse_an_unaligned_buffer_on_the_host(dev, entry, build, which):
    """Class (b): PDM_REQUIRE returns PDM_E_BADARG before any launch.  The message names the operator, the outputs keep what
    they held and no red zone changes.  Tiny shapes: nothing runs on the device."""
    a = Arena(dev)
    who, args, outputs = build(a, which)
    before = []
    for k, o in enumerate(outputs):
        o.view(torch.uint8).fill_(0x30 + k)
        before.append(o.clone())
    torch.cuda.synchronize()
    with pytest.raises(_native.NativeLibraryError, match=f"{entry} failed with code -1: {who}: ") as err:
        _native.call(entry, _native.stream(dev), *args)
    assert "align" in str(err.value).lower()
    done(a)
    for o, b in zip(outputs, before):
        assert torch.equal(o.view(torch.uint8), b.view(torch.uint8))

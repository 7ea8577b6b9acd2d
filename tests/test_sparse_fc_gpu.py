"""pdm_sparse_fc (csrc/sparse_fc.hip): SparseConvTensor.dense() + the head's first shared FC without the dense tensor, against the
dense formulation in float64: to_dense of cat(xa, xb) as (R, C, cells), then W @ v with the Conv1d weight's column c cells + cell.

Bound per output element: (n_r + 8) 2^-24 T with n_r = C (active rows of that box) the number of products and T the sum of
their absolute values: the first-order bound of an fp32 sum of n_r rounded products in ANY order (the operator adds them in
MFMA chains over the channels, cell after cell, then over its fixed partials; no fixed point, so no quantisation term).
S = 3 (27 cells); the row patterns: 'mixed' (box 0 holds all 27 cells, every fifth box from 2 has no row, the others a random
30 %), 'one_cell' (every box holds cell 13 and nothing else).
"""
import numpy as np
import pytest
import torch

from arena import Arena
from pdm_ssd_amd import sparse_conv_ops

pytestmark = pytest.mark.gpu
S, CELLS = (3, 3, 3), 27
U = 2.0 ** -24


@pytest.fixture(scope="module")
def arena(dev):
    return Arena(dev)


def make_case(R, ca, cb, cout, pattern, seed):
    rng = np.random.default_rng(seed)
    rows = []
    for r in range(R):
        if pattern == 'one_cell':
            cells = [13]
        elif r == 0:
            cells = list(range(CELLS))
        elif r % 5 == 2:
            cells = []
        else:
            cells = np.nonzero(rng.random(CELLS) < 0.3)[0].tolist()
        rows += [(r, c // 9, (c // 3) % 3, c % 3) for c in cells]
    coords = np.array(rows, dtype=np.int32).reshape(-1, 4)
    Q, C = len(coords), ca + cb
    xa = rng.uniform(-1, 1, (Q, ca)).astype(np.float32)
    xb = rng.uniform(-1, 1, (Q, cb)).astype(np.float32)
    w = (rng.uniform(-1, 1, (cout, C * CELLS, 1)) / np.sqrt(C * CELLS)).astype(np.float32)
    x = np.concatenate([xa, xb], 1).astype(np.float64)
    cell = (coords[:, 1] * 3 + coords[:, 2]) * 3 + coords[:, 3]
    dense = np.zeros((R, C, CELLS))
    dense[coords[:, 0], :, cell] = x
    w64 = w[:, :, 0].astype(np.float64)
    want = dense.reshape(R, -1) @ w64.T
    T = np.abs(dense).reshape(R, -1) @ np.abs(w64).T
    n_r = C * np.bincount(coords[:, 0], minlength=R)
    # the same rows under the WRONG column order cell C + c: what a mis-packed weight computes
    wrong = dense.transpose(0, 2, 1).reshape(R, -1) @ w64.T
    return dict(coords=coords, xa=xa, xb=xb, w=w, want=want, bound=(n_r[:, None] + 8) * U * T, wrong=wrong, rows=n_r // C)


def run(arena, case, R, cout, scale=None, shift=None, relu=False):
    dev = arena.buf.device
    arena.reset()
    Q = len(case['coords'])
    put = lambda a, mis, poison: arena.put(a, mis, poison) if a.size else torch.from_numpy(a).to(dev)      # noqa: E731
    coords = put(case['coords'], 4, 0)
    xa = put(case['xa'], 0, float('nan'))
    xb = put(case['xb'], 0, float('nan')) if case['xb'].shape[1] else None
    out = arena.carve((R, cout), torch.float32, 4)
    wpack = sparse_conv_ops.pack_fc_weight(torch.from_numpy(case['w']).to(dev), CELLS)
    opt = [None if t is None else arena.put(t, 4, float('nan')) for t in (scale, shift)]
    sparse_conv_ops.sparse_fc(coords, xa, xb, R, S, wpack, cout, opt[0], opt[1], relu, out=out)
    torch.cuda.synchronize()
    arena.check()
    assert Q == coords.shape[0]
    return out.clone()


@pytest.mark.parametrize("pattern", ['mixed', 'one_cell'])
@pytest.mark.parametrize("R", [1, 37])
@pytest.mark.parametrize("cout", [16, 256])
@pytest.mark.parametrize("ca, cb", [(64, 64), (16, 0)])
def test_sparse_fc_matches_the_dense_formulation_in_float64(dev, arena, ca, cb, cout, R, pattern):
    case = make_case(R, ca, cb, cout, pattern, seed=ca + cout + R)
    if pattern == 'mixed':
        assert case['rows'][0] == CELLS and (R == 1 or (case['rows'] == 0).any())
    else:
        assert (case['rows'] == 1).all()
    raw = run(arena, case, R, cout)
    assert torch.equal(raw, run(arena, case, R, cout)), 'two runs differ'
    got = raw.cpu().numpy().astype(np.float64)
    ratio = np.abs(got - case['want']) / np.maximum(case['bound'], 1e-300)
    print(pattern, 'R', R, 'C', ca + cb, 'Cout', cout, 'rows', len(case['coords']), 'chunks', sparse_conv_ops.sparse_fc_chunks(R, CELLS, cout),
          'max err / bound', float(ratio.max()))
    assert np.isfinite(got).all() and (ratio <= 1.0).all()
    assert (got[case['rows'] == 0] == 0).all(), 'a box without rows is epilogue(0) = 0'
    # the wrong column order (cell C + c) is far outside the bound: this test tells the two apart
    if len(case['coords']) > 1 or ca + cb > 1:
        assert (np.abs(got - case['wrong']) > case['bound']).any()
    # the epilogue, from the operator's own raw output: one multiply and one add, or one fma
    rng = np.random.default_rng(cout)
    scale = (rng.uniform(0.5, 1.5, cout) * rng.choice([-1, 1], cout)).astype(np.float32)
    shift = rng.uniform(-0.5, 0.5, cout).astype(np.float32)
    ep = run(arena, case, R, cout, scale, shift, relu=True)
    sc, sh = torch.from_numpy(scale).to(dev), torch.from_numpy(shift).to(dev)
    want = torch.relu(raw * sc + sh)
    tol = 2.0 ** -23 * ((raw * sc).abs() + sh.abs())
    assert ((ep - want).abs() <= tol).all() and (ep >= 0).all()
    assert torch.equal(ep[torch.from_numpy(case['rows'] == 0).to(dev)], torch.relu(sh).expand(int((case['rows'] == 0).sum()), cout))


def test_sparse_fc_without_rows_is_the_epilogue_of_zero(dev):
    R, cout = 5, 16
    w = torch.randn(cout, 16 * CELLS, 1, device=dev)
    shift = torch.linspace(-1, 1, cout, device=dev)
    out = sparse_conv_ops.sparse_fc(torch.empty((0, 4), dtype=torch.int32, device=dev), torch.empty((0, 16), device=dev), None, R, S,
                                    sparse_conv_ops.pack_fc_weight(w, CELLS), cout, torch.ones(cout, device=dev), shift, relu=True)
    assert torch.equal(out, torch.relu(shift).expand(R, cout))

"""The sparse convolution's gradients without a GPU: the numpy restatement of tests/sparse_conv_grad_reference.py against torch
autograd of F.conv3d in float64 on the densified input, the two facts the data gradient rests on (the reversed-offset identity
of a submanifold rulebook, one writer per entry of a transposed table), the transposed pack's layout, and the argument checks
of the new entry points (they come before any launch)."""
import ctypes as C

import numpy as np
import pytest
import torch

import sparse_conv_grad_reference as sgr
import sparse_conv_reference as scr


@pytest.fixture(scope="module")
def r1_books():
    idx = scr.r1_indices()
    return idx, {name: scr.rulebook(idx, scr.R1_B, scr.R1_SHAPE, *geo) for name, geo in scr.GEOMETRIES.items()}


@pytest.mark.parametrize("name", list(scr.GEOMETRIES))
def test_restatement_equals_autograd_of_the_dense_convolution_in_float64(r1_books, name):
    """dx and dW of loss = sum(y * dy) with y = F.conv3d(dense input) read at the output sites: 1e-12 of the largest entry"""
    idx, books = r1_books
    kernel, stride, padding, subm = scr.GEOMETRIES[name]
    out_idx, nbr, oshape = books[name]
    cin, cout = 3, 5
    rng = np.random.default_rng(17)
    x = rng.uniform(-1, 1, (len(idx), cin))
    w = rng.uniform(-1, 1, (cout, *kernel, cin))
    dy = rng.uniform(-1, 1, (len(out_idx), cout))
    got = sgr.grads(x, w, dy, nbr)
    assert got['n_k'].sum() == (nbr >= 0).sum() and got['n_k'].min() > 0

    xt, wt = torch.from_numpy(x).requires_grad_(), torch.from_numpy(w).requires_grad_()
    D, H, W = scr.R1_SHAPE
    i, o = torch.from_numpy(idx).long(), torch.from_numpy(out_idx).long()
    dense = torch.zeros((scr.R1_B, D, H, W, cin), dtype=torch.float64).index_put((i[:, 0], i[:, 1], i[:, 2], i[:, 3]), xt)
    pad = tuple(k // 2 for k in kernel) if subm else padding
    y = torch.nn.functional.conv3d(dense.permute(0, 4, 1, 2, 3), wt.permute(0, 4, 1, 2, 3), stride=(1, 1, 1) if subm else stride, padding=pad)
    assert tuple(y.shape[2:]) == tuple(oshape)
    (y[o[:, 0], :, o[:, 1], o[:, 2], o[:, 3]] * torch.from_numpy(dy)).sum().backward()
    for ours, want in ((got['dx64'], xt.grad.numpy()), (got['dW64'], wt.grad.numpy().reshape(cout, -1, cin))):
        assert np.abs(want).max() > 0.1
        assert np.abs(ours - want).max() <= 1e-12 * np.abs(want).max()
    assert (got['A_dx'] >= np.abs(got['dx64']) - 1e-12).all() and (got['A_dW'] >= np.abs(got['dW64']) - 1e-12).all()


@pytest.mark.parametrize("P", [1, 65, None])
def test_submanifold_transpose_is_the_reversed_offset_order(P):
    idx = scr.r1_indices(P)
    _, nbr, _ = scr.rulebook(idx, scr.R1_B, scr.R1_SHAPE, *scr.GEOMETRIES['subm3'])
    assert np.array_equal(sgr.transpose(nbr, len(idx)), nbr[:, ::-1])


@pytest.mark.parametrize("name", ['k3s2p1', 'k3s2p011', 'k311s211p0'])
def test_a_transposed_entry_has_at_most_one_writer(r1_books, name):
    idx, books = r1_books
    nbr = books[name][1]
    cnt = sgr.writers(nbr, len(idx))
    assert cnt.max() == 1 and cnt.sum() == (nbr >= 0).sum()
    t = sgr.transpose(nbr, len(idx))
    j, k = np.nonzero(t >= 0)
    assert np.array_equal(nbr[t[j, k], k], j)
    hurt = nbr.copy()
    hurt[0, :] = len(idx)           # out of range counts as -1
    assert (sgr.transpose(hurt, len(idx)) != 0).all()


def test_pack_weight_transposed_layout_and_refusals():
    """[k][kb][nb][lane][j] = W[cout = 16 kb + 4 (lane >> 4) + j][k or kvol - 1 - k][cin = 16 nb + (lane & 15)], zero past Cin: the
    convolution Cout -> Cin (padded) in pack_weight's own fragment order"""
    from pdm_ssd_amd import sparse_conv_ops
    for cin, cout in ((5, 32), (32, 16), (16, 64)):
        w = torch.arange(cout * 27 * cin, dtype=torch.float32).reshape(cout, 3, 3, 3, cin)
        flat = w.reshape(cout, 27, cin)
        cin_p = max(cin, 16)
        for flip in (False, True):
            p = sparse_conv_ops.pack_weight_transposed(w, flip=flip)
            assert p.numel() == 27 * (cout // 16) * (cin_p // 16) * 256
            p = p.reshape(27, cout // 16, cin_p // 16, 64, 4)
            for k, kb, nb, lane, j in ((0, 0, 0, 0, 0), (26, cout // 16 - 1, cin_p // 16 - 1, 17, 0), (13, 0, 0, 15, 3), (5, 0, 0, 4, 2),
                                       (5, 0, 0, 5, 1), (22, cout // 16 - 1, 0, 63, 3)):
                co, ci = 16 * kb + 4 * (lane >> 4) + j, 16 * nb + (lane & 15)
                want = float(flat[co, 26 - k if flip else k, ci]) if ci < cin else 0.0
                assert float(p[k, kb, nb, lane, j]) == want, (cin, cout, flip, k, kb, nb, lane, j)
    w = torch.rand(16, 3, 1, 1, 16)
    assert torch.equal(sparse_conv_ops.pack_weight_transposed(w, flip=True), sparse_conv_ops.pack_weight_transposed(w.flip(1)))
    for shape in ((16, 3, 3, 3, 2), (16, 3, 3, 3, 9), (24, 3, 3, 3, 16), (256, 3, 3, 3, 16)):
        with pytest.raises(ValueError, match='channels'):
            sparse_conv_ops.pack_weight_transposed(torch.zeros(shape))


def test_new_entry_points_validate_their_arguments_before_any_launch():
    """null pointers, a workspace that is too small or misaligned, unsupported widths, more than 27 offsets, over-int32 sizes, a
    misaligned transposed pack: an error code and a message, no launch (no GPU is touched: the checks come first)"""
    from pdm_ssd_amd import _native, sparse_conv_ops
    lib = _native.lib()
    buf = (C.c_float * 4096)()
    ptr = C.cast(buf, C.c_void_p)
    err = _native.NativeLibraryError

    with pytest.raises(err, match='null pointer'):
        _native.call("pdm_sparse_rulebook_transpose", 0, 100, 50, 27, None, ptr)
    with pytest.raises(err, match='null pointer'):
        _native.call("pdm_sparse_rulebook_transpose", 0, 100, 50, 27, ptr, None)
    with pytest.raises(err, match='at most 27'):
        _native.call("pdm_sparse_rulebook_transpose", 0, 100, 50, 28, ptr, ptr)
    with pytest.raises(err, match='bad size'):
        _native.call("pdm_sparse_rulebook_transpose", 0, -1, 50, 27, ptr, ptr)
    with pytest.raises(err, match='exceed int32'):
        _native.call("pdm_sparse_rulebook_transpose", 0, 100, 1 << 27, 27, ptr, ptr)

    need = lib.pdm_sparse_conv_wgrad_workspace_bytes(100, 27, 16, 32)
    assert need >= 27 * 32 * 16 * 4 and lib.pdm_sparse_conv_wgrad_workspace_bytes(100, 27, 5, 32) == need      # Cin 5 is padded to 16
    ok = (100, 100, 27, 16, 32, ptr, ptr, ptr, ptr, ptr, need)
    for at in (5, 7, 8, 9):
        with pytest.raises(err, match='null pointer'):
            _native.call("pdm_sparse_conv_wgrad", 0, *ok[:at], None, *ok[at + 1:])
    with pytest.raises(err, match='null pointer'):
        _native.call("pdm_sparse_conv_wgrad", 0, *ok[:6], None, *ok[7:])
    with pytest.raises(err, match='workspace too small'):
        _native.call("pdm_sparse_conv_wgrad", 0, *ok[:10], need - 256)
    with pytest.raises(err, match='8-byte aligned'):
        _native.call("pdm_sparse_conv_wgrad", 0, *ok[:9], C.c_void_p(ptr.value + 4), need)
    for cin, cout, text in ((2, 16, 'input channels'), (12, 16, 'input channels'), (256, 16, 'input channels'), (16, 8, 'output channels'),
                            (16, 48, 'output channels'), (16, 256, 'output channels')):
        with pytest.raises(err, match=text):
            _native.call("pdm_sparse_conv_wgrad", 0, 100, 100, 27, cin, cout, *ok[5:])
        assert lib.pdm_sparse_conv_wgrad_workspace_bytes(100, 27, cin, cout) == 0 and lib.pdm_sparse_conv_wgrad_chunk_rows(100, 27, cin, cout) == 0
    with pytest.raises(err, match='offsets'):
        _native.call("pdm_sparse_conv_wgrad", 0, 100, 100, 28, *ok[3:])
    assert lib.pdm_sparse_conv_wgrad_workspace_bytes(100, 28, 16, 32) == 0 and lib.pdm_sparse_conv_wgrad_chunk_rows(100, 0, 16, 32) == 0
    with pytest.raises(err, match='exceed int32'):
        _native.call("pdm_sparse_conv_wgrad", 0, 1 << 27, *ok[1:10], 1 << 40)
    with pytest.raises(err, match='bad size'):
        _native.call("pdm_sparse_conv_wgrad", 0, -1, *ok[1:])

    # the data gradient is pdm_sparse_conv_split over a transposed pack: the forward's checks, a pack off a 16-byte boundary among them
    pack = sparse_conv_ops.pack_weight_transposed(torch.zeros(32, 3, 3, 3, 16))
    assert pack.numel() == lib.pdm_sparse_conv_packed_floats(27, 32, 16)
    conv = (100, 100, 27, 32, 16, ptr, ptr, ptr, None, None, None, 0, ptr)
    with pytest.raises(err, match='16-byte aligned'):
        _native.call("pdm_sparse_conv_split", 0, *conv[:7], C.c_void_p(ptr.value + 4), *conv[8:])
    with pytest.raises(err, match='null pointer'):
        _native.call("pdm_sparse_conv_split", 0, *conv[:6], None, *conv[7:])
    with pytest.raises(err, match='input channels'):
        _native.call("pdm_sparse_conv_split", 0, 100, 100, 27, 12, 16, *conv[5:])
    with pytest.raises(err, match='offsets'):
        _native.call("pdm_sparse_conv_split", 0, 100, 100, 28, *conv[3:])
    with pytest.raises(err, match='come together'):
        _native.call("pdm_sparse_conv_split", 0, *conv[:8], ptr, None, None, 0, ptr)


def test_chunk_rows_is_a_pure_function_of_its_arguments():
    """the same answer however often and in whatever order it is asked; a multiple of 64, at least 1024 rows; the partials of all
    chunks stay within the 64 MiB cap (or one chunk's), and at most 1024 chunks"""
    from pdm_ssd_amd import _native, sparse_conv_ops
    lib = _native.lib()
    cases = [(P, kvol, cin, cout) for P in (0, 1, 1023, 1024, 1025, 100000, 4800000, 70000000) for kvol in (1, 3, 27)
             for cin, cout in ((4, 16), (16, 16), (16, 32), (64, 64), (128, 128))]
    first = [lib.pdm_sparse_conv_wgrad_chunk_rows(*c) for c in cases]
    assert [lib.pdm_sparse_conv_wgrad_chunk_rows(*c) for c in reversed(cases)] == first[::-1]
    for (P, kvol, cin, cout), rows in zip(cases, first):
        assert rows >= 1024 and rows % 64 == 0 and rows == sparse_conv_ops.wgrad_chunk_rows(P, kvol, cin, cout)
        nchunks = -(-P // rows)
        partial = 4 * kvol * cout * max(cin, 16)
        assert nchunks <= 1024 and (nchunks * partial <= 64 << 20 or nchunks == 1)
        assert lib.pdm_sparse_conv_wgrad_workspace_bytes(P, kvol, cin, cout) >= max(nchunks, 1) * partial
    assert lib.pdm_sparse_conv_wgrad_chunk_rows(2049, 27, 16, 32) == 1024
    assert lib.pdm_sparse_conv_wgrad_chunk_rows(4800000, 27, 16, 16) == 4736          # 1024 chunks at most
    assert lib.pdm_sparse_conv_wgrad_chunk_rows(4800000, 27, 128, 128) == 129792       # 37 chunks of 1.77 MB under 64 MiB: ceil(4.8e6 / 37) = 129730, up to 64

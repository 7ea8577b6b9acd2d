"""The one A-fragment permutation (_native.mfma_a_fragments, the layout of csrc/mfma_f32.h) element by element, and the four
weight packers built on it against the reshape / permute each of them carried before, bit for bit.  No GPU."""
import numpy as np
import torch

from pdm_ssd_amd import _native, bev_roi_ops, fused, sparse_conv_ops


def _arange(*shape):
    return torch.arange(int(np.prod(shape)), dtype=torch.float32).reshape(*shape)      # every element distinct


def test_a_fragments_follow_the_layout_formula():
    """[nb][kb][lane][j] = w[16 nb + (lane & 15)][16 kb + 4 (lane >> 4) + j] at Cout = 32, K = 48: two blocks one way and three
    the other, so swapped block or lane axes cannot pass; then the same under a leading batch axis"""
    w = _arange(32, 48)
    p = _native.mfma_a_fragments(w)
    assert p.shape == (2, 3, 64, 4) and p.dtype == w.dtype
    for nb in range(2):
        for kb in range(3):
            for lane in range(64):
                for j in range(4):
                    assert p[nb, kb, lane, j] == w[16 * nb + (lane & 15), 16 * kb + 4 * (lane >> 4) + j], (nb, kb, lane, j)
    wb = torch.stack([w, -w, w + 0.5])
    pb = _native.mfma_a_fragments(wb)
    assert pb.shape == (3, 2, 3, 64, 4)
    for b in range(3):
        assert torch.equal(pb[b], _native.mfma_a_fragments(wb[b]))
    assert torch.equal(pb[0], p)


def test_pack_weight_keeps_its_bits():
    for shape in [(32, 1, 1, 2, 32), (32, 1, 1, 2, 5)]:      # two blocks on both axes and two offsets; a padded Cin
        weight = _arange(*shape)
        cout, cin = shape[0], shape[-1]
        w = weight.reshape(cout, -1, cin)
        kvol, nkb, nb = w.shape[1], (cin + 15) // 16, cout // 16
        w = torch.nn.functional.pad(w, (0, 16 * nkb - cin))
        want = w.reshape(nb, 16, kvol, nkb, 4, 4).permute(2, 3, 0, 4, 1, 5).contiguous().reshape(-1)      # (kvol, nkb, nb, g, i, j)
        assert torch.equal(sparse_conv_ops.pack_weight(weight), want)


def test_pack_fc_weight_keeps_its_bits():
    cout, C, cells = 32, 32, 2
    weight = _arange(cout, C * cells, 1)
    w = weight.reshape(cout, -1)
    want = w.reshape(cout // 16, 16, C // 16, 4, 4, cells).permute(5, 2, 0, 3, 1, 4).contiguous().reshape(-1)  # (cell, kb, nb, g, i, j)
    assert torch.equal(sparse_conv_ops.pack_fc_weight(weight, cells), want)


def test_pack_crop_fc_weight_keeps_its_bits():
    cout, C, G = 32, 16, 2
    weight = _arange(cout, C * G * G, 1)
    w = weight.reshape(cout, -1)
    want = w.reshape(cout // 16, 16, C * G * G // 16, 4, 4).permute(2, 0, 3, 1, 4).contiguous().reshape(-1)    # (kb, nb, g, i, j)
    assert torch.equal(bev_roi_ops.pack_crop_fc_weight(weight, C, G), want)


def test_pack_layer_keeps_its_bits():
    cout, cin = 20, 18      # both padded to 32: two blocks each way
    w = _arange(cout, cin).numpy()
    shift = np.arange(cout, dtype=np.float32)
    wp = np.zeros((32, 32), dtype=np.float32)
    wp[:cout, :cin] = w
    want = np.ascontiguousarray(wp.reshape(2, 16, 2, 4, 4).transpose(0, 2, 3, 1, 4)).reshape(-1)     # [mb][kb][g][oc][s]
    pw, pb, kp, cp = fused.pack_layer(w, shift)
    assert isinstance(pw, np.ndarray) and isinstance(pb, np.ndarray) and pw.dtype == np.float32 and pw.flags['C_CONTIGUOUS']
    assert (kp, cp) == (32, 32) and np.array_equal(pw, want)
    assert np.array_equal(pb[:cout], shift) and not pb[cout:].any()

"""The two forms of pdm_bev_head_fused (pdm_tune_bev_head_form): 0 = every wave runs the depthwise prologue and the chain
(rows_chain_kernel<8,4,4,1,true>), 1 = depthwise producer waves beside MFMA consumer waves (csrc/bev_head_roles.hip).
Form 1 must give the bits of form 0 and of the two-kernel path (depthwise kernel, then the row MLP) on every map shape
that reaches another path of its tile walk, leave everything around its output alone, and hand tiles over without a race."""
import pytest
import torch

from pdm_ssd_amd.detector_config import build_pdm_ssd

# (B, H, W, grid cap in workgroups per CU, fill); B * H * W >= 8192 is the entry point's own floor
CASES = [
    (3, 64, 48, 1, "sparse"),      # 144 tiles: fewer than workgroups, every workgroup has one tile
    (2, 47, 97, 1, "sparse"),      # ragged in both directions
    (1, 93, 90, 2, "sparse"),      # ragged in both directions
    (8, 129, 9, 1, "sparse"),      # map narrower than a patch
    (4, 3, 700, 1, "sparse"),      # map lower than a patch
    (2, 188, 188, 1, "sparse"),    # 4-5 tiles per workgroup, unequal counts: the double buffer wraps
    (2, 188, 188, 12, "sparse"),   # many workgroups per CU
    (1, 200, 176, 2, "sparse"),    # the bench map
    (3, 64, 48, 1, "zero+dense"),  # one image all zero (shift and bias only), one fully dense (every tap live)
]


def _head(dev, seed):
    torch.manual_seed(seed)
    head = build_pdm_ssd().dense_head.to(dev).eval()
    for m in head.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            m.running_mean.normal_(0, 0.1); m.running_var.uniform_(0.5, 1.5); m.weight.data.uniform_(0.5, 1.5); m.bias.data.normal_(0, 0.1)
    return head


def _map(dev, B, H, W, fill):
    x = torch.randn(B, H, W, 128, device=dev) * (torch.rand(B, H, W, 1, device=dev) < 0.4)
    if fill == "zero+dense":
        x[0] = 0.0
        x[1] = torch.randn(H, W, 128, device=dev)
    return x


def _logits(head, sf, form, one_kernel, cap):
    from pdm_ssd_amd import _native
    l = _native.lib()
    oldform, oldcap = l.pdm_tune_bev_head_form(form), l.pdm_tune_rows_chain_dw_wg_per_cu(cap)
    head.use_one_kernel = one_kernel
    try:
        with torch.no_grad():
            head({'spatial_features': sf})
        return head.forward_ret_dict['hm_logits'].clone()
    finally:
        head.use_one_kernel = True
        l.pdm_tune_bev_head_form(oldform)
        l.pdm_tune_rows_chain_dw_wg_per_cu(oldcap)


@pytest.mark.gpu
@pytest.mark.parametrize("B,H,W,cap,fill", CASES)
def test_role_split_form_equals_both_references(dev, B, H, W, cap, fill):
    head = _head(dev, B * 1000 + H + W)
    sf = _map(dev, B, H, W, fill).permute(0, 3, 1, 2)
    two = _logits(head, sf, 0, False, cap)      # depthwise kernel, then the row MLP
    one = _logits(head, sf, 0, True, cap)       # the one-role kernel
    new = _logits(head, sf, 1, True, cap)
    assert tuple(new.shape) == (B, 3, H, W) and torch.isfinite(new).all()
    assert torch.equal(new, two)
    assert torch.equal(new, one)


@pytest.mark.gpu
def test_role_split_form_repeats_its_bits_launch_after_launch(dev):
    """A race in the hand-over (a consumer reading a tile the producers are still writing, or the reverse) shows as bits that
    change from launch to launch: 4-5 tiles per workgroup, eight launches on one input."""
    head = _head(dev, 7)
    sf = _map(dev, 2, 188, 188, "sparse").permute(0, 3, 1, 2)
    first = _logits(head, sf, 1, True, 1)
    for _ in range(7):
        assert torch.equal(_logits(head, sf, 1, True, 1), first)
    assert torch.equal(first, _logits(head, sf, 0, True, 1))


@pytest.mark.gpu
@pytest.mark.parametrize("B,H,W", [(2, 47, 97), (8, 129, 9)])
def test_role_split_form_writes_nothing_around_its_output(dev, B, H, W):
    """pdm_bev_head_fused into the middle of a patterned buffer: the rows in front of and behind `out` and the padding
    channel of every row (cout = 3 of out_stride = 4) keep the pattern; the three logits are those of form 0."""
    from pdm_ssd_amd import _native, fused
    head = _head(dev, 11)
    x = _map(dev, B, H, W, "sparse")
    with torch.no_grad():
        head({'spatial_features': x.permute(0, 3, 1, 2)})          # fills the head's caches: folded taps, packed layers
    _, w, shift = head._pdm_fused_cache['dw']
    mods = list(head.shared_conv)
    pk = fused.cached_layers(head, 'pw', head, lambda: [(mods[3], mods[4]), (head.hm[0], None), (head.hm[2], None)], dev)
    assert pk.dims == [128, 64, 64, 16]
    rows, pad, pattern = B * H * W, 4096, -12345.5
    l = _native.lib()
    outs = []
    for form in (0, 1):
        big = torch.full((pad + rows * 4 + pad,), pattern, device=dev)
        out = big[pad:pad + rows * 4]
        old = l.pdm_tune_bev_head_form(form)
        try:
            _native.call("pdm_bev_head_fused", _native.stream(dev), B, H, W, 128, x.data_ptr(), w.data_ptr(), shift.data_ptr(), pk.nlayers,
                         pk.dims_c, pk.wpack.data_ptr(), pk.bias.data_ptr(), 0, out.data_ptr(), 4, 3)
            torch.cuda.synchronize()
        finally:
            l.pdm_tune_bev_head_form(old)
        outs.append(big)
    ref, got = outs
    assert bool((got[:pad] == pattern).all()) and bool((got[pad + rows * 4:] == pattern).all())
    body = got[pad:pad + rows * 4].view(rows, 4)
    assert bool((body[:, 3] == pattern).all())
    assert bool((body[:, :3] != pattern).all())
    assert torch.equal(got, ref)

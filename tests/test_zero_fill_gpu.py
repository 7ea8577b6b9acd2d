"""The library's one zero fill (pdm::zero_fill, csrc/api.hip) through the entry points that clear with it: cleared again on
every replay of a captured graph, and exact at the edges of a range that is neither 16-byte aligned nor a multiple of 16 bytes.

pdm_nms' count and pdm_query_and_group's index buffer are caller-provided only at the C ABI (the Python wrappers allocate
them), so those two cases go through _native.call."""
import numpy as np
import pytest
import torch

from pdm_ssd_amd import _native, heatmap_loss, train_gemm
from pdm_ssd_amd.pointnet2_batch import pointnet2_batch_hip as ext

pytestmark = pytest.mark.gpu


def test_heatmap_targets_clears_the_map_on_every_replay(dev):
    B, C, H, W, M = 2, 3, 16, 16, 4
    gt = np.zeros((B, M, 8), dtype=np.float32)
    rng = np.random.default_rng(3)
    for b in range(B):
        for r in range(M - 1):                      # the last row of each sample stays padding (class 0)
            gt[b, r] = [rng.uniform(1, 7), rng.uniform(1, 7), -1.0, 3.9, 1.6, 1.5, rng.uniform(-3, 3), 1 + (b + r) % C]
    gt = torch.from_numpy(gt).to(dev)
    run = lambda: heatmap_loss.heatmap_targets(gt, C, H, W, 0.0, 0.0, 0.5, 0.5, 1, 0.1, 2, 8)
    want = run()                                    # eager; also the warm-up
    assert int((want == 1).sum()) > 0 and int((want == 0).sum()) > 0
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        hm = run()
    for _ in range(2):
        hm.fill_(7.0)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(hm, want)


def test_nms_of_zero_boxes_writes_a_zero_count_eagerly_and_on_replay(dev):
    boxes = torch.empty((0, 7), dtype=torch.float32, device=dev)
    keep = torch.empty((1,), dtype=torch.int64, device=dev)
    ws = torch.empty((8,), dtype=torch.uint8, device=dev)
    num = torch.full((1,), 7, dtype=torch.int32, device=dev)
    run = lambda: _native.call("pdm_nms", _native.stream(num), 0, boxes.data_ptr(), 0.5, 0, ws.data_ptr(), 0, keep.data_ptr(), num.data_ptr())
    run()
    assert int(num.item()) == 0
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        run()
    num.fill_(7)
    g.replay()
    assert int(num.item()) == 0


def test_query_and_group_clears_an_unaligned_index_range_and_nothing_else(dev):
    """15 ints (60 bytes) one element past a 16-byte boundary; a centre with an empty ball keeps the zeros of the fill"""
    b, n, m, c, ns, radius = 1, 32, 3, 2, 5, 0.5
    rng = np.random.default_rng(5)
    xyz = torch.from_numpy(rng.uniform(0, 1, (b, n, 3)).astype(np.float32)).to(dev)
    feat = torch.from_numpy(rng.standard_normal((b, c, n)).astype(np.float32)).to(dev)
    new_xyz = torch.stack([xyz[0, 0], xyz[0, 1], xyz.new_full((3,), 50.0)])[None].contiguous()
    want_idx = torch.full((b, m, ns), 7, dtype=torch.int32, device=dev)
    want_out = torch.empty((b, 3 + c, m, ns), dtype=torch.float32, device=dev)
    ext.query_and_group_wrapper(b, n, m, c, radius, ns, xyz, new_xyz, feat, want_idx, want_out)
    assert int(want_idx[0, 2].abs().sum()) == 0 and int(want_idx[0, :2].sum()) > 0
    base = torch.full((24,), 7, dtype=torch.int32, device=dev)
    idx = base[1:1 + m * ns]
    assert base.data_ptr() % 16 == 0 and idx.data_ptr() % 16 == 4 and (idx.numel() * 4) % 16 != 0
    out = torch.empty_like(want_out)
    _native.call("pdm_query_and_group", _native.stream(xyz), b, n, m, c, radius, ns, xyz.data_ptr(), new_xyz.data_ptr(), feat.data_ptr(),
                 idx.data_ptr(), out.data_ptr())
    assert torch.equal(idx.view(b, m, ns), want_idx) and torch.equal(out, want_out)
    assert int(base[0]) == 7 and bool((base[1 + m * ns:] == 7).all())


@pytest.mark.parametrize("floats", [1, 1025, 16385])
@pytest.mark.parametrize("offset", [0, 4, 8, 12])
def test_colsum_of_zero_rows_clears_exactly_its_range_at_every_float_offset(dev, floats, offset):
    """pdm_tg_colsum with R = 0 hands its `out` (N floats, any N) to the zero fill: 4, 4100 and 65540 bytes — the lengths next
    to 1, 4099 and 65537 that a float pointer can have — at every offset a float pointer can have: a range shorter than its
    head, one with a 16-byte middle of one workgroup and one of several, each with head and tail; red zones on both sides."""
    from arena import Arena
    a = Arena(dev)
    out = a.carve((floats,), torch.float32, offset)
    out.fill_(7.0)
    _native.call("pdm_tg_colsum", _native.stream(dev), 0, floats, 0, 8, out.data_ptr(), 0)
    torch.cuda.synchronize()
    a.check()
    assert bool((out == 0).all())


def test_wgrad_of_zero_rows_clears_an_unaligned_range_with_head_and_tail(dev):
    """21 floats (84 bytes) one element past a 16-byte boundary: 12 bytes of head, four 16-byte stores, 8 bytes of tail"""
    N, K = 3, 7
    base = torch.full((32,), 7.0, dtype=torch.float32, device=dev)
    dw = base[1:1 + N * K].view(N, K)
    assert base.data_ptr() % 16 == 0 and dw.is_contiguous()
    dy = torch.empty((0, N), dtype=torch.bfloat16, device=dev)
    x = torch.empty((0, K), dtype=torch.bfloat16, device=dev)
    assert train_gemm.wgrad(dy, x, out=dw) is dw
    assert bool((dw == 0).all()) and float(base[0]) == 7.0 and bool((base[1 + N * K:] == 7.0).all())

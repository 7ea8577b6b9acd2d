"""SECOND-IoU's RoI pooling (csrc/bev_roi_crop.hip): the rotated G x G crop of the 2-D backbone's map under every RoI
of the batch in one launch, and the same crop followed by the head's first shared FC without the (R, C G^2) tensor.

Neither operator has a gradient and none is written: SECONDHead detaches both the map and the rois in front of this step, so the
crop is a constant of the training graph and gradients reach the FC stacks behind it only.

For tensors on the GPU there is no torch fallback: a missing kernel is an error.  For CPU tensors `bev_roi_crop` is
`bev_roi_crop_torch`, the same arithmetic in the same fp32 order written with torch's own operators: the CPU path of the head and
the on-device checker of the kernels.
"""
import torch

from . import _native


def _cells(voxel_size, downsample_ratio):
    """VOXEL_SIZE * DOWNSAMPLE_RATIO as the python double products the reference divides by (rounded once to fp32 where used)"""
    return float(voxel_size[0] * downsample_ratio), float(voxel_size[1] * downsample_ratio)


def bev_roi_crop_torch(rois, spatial_features_2d, point_cloud_range, voxel_size, downsample_ratio, grid_size):
    """The crop with torch's operators, on any device: rois (B, n, 7 + ..), map (B, C, H, W) -> (B n, C, G, G).  Position of cell
    (i, j) of a RoI, in pixels: px = hx cos(a) u - hx sin(a) v + cx, py = hy sin(a) u + hy cos(a) v + cy with cx = (x - x0) / cell_x,
    hx = (dx / 2) / cell_x, u = (2 j - (G - 1)) / (G - 1), v = (2 i - (G - 1)) / (G - 1) (the reference's theta, affine_grid and
    un-normalisation multiplied out); the value is the bilinear blend of the four pixels around it, a pixel outside the map
    counting as 0."""
    B, n = rois.shape[0], rois.shape[1]
    _, C, H, W = spatial_features_2d.shape
    G = int(grid_size)
    cell_x, cell_y = _cells(voxel_size, downsample_ratio)
    r = rois.detach().reshape(B * n, -1).float()
    feat = spatial_features_2d.detach().float()
    cx, hx = (r[:, 0] - float(point_cloud_range[0])) / cell_x, (r[:, 3] * 0.5) / cell_x
    cy, hy = (r[:, 1] - float(point_cloud_range[1])) / cell_y, (r[:, 4] * 0.5) / cell_y
    sin, cos = torch.sin(r[:, 6]), torch.cos(r[:, 6])
    lattice = (2 * torch.arange(G, device=r.device) - (G - 1)).float() / float(G - 1)
    u, v = lattice.view(1, 1, G), lattice.view(1, G, 1)
    col = lambda t: t.view(-1, 1, 1)      # noqa: E731
    px = ((col(hx * cos) * u) - (col(hx * sin) * v)) + col(cx)          # (R, G, G)
    py = ((col(hy * sin) * u) + (col(hy * cos) * v)) + col(cy)
    inside = (px > -1) & (px < W) & (py > -1) & (py < H)
    px, py = torch.where(inside, px, torch.full_like(px, -4.0)), torch.where(inside, py, torch.full_like(py, -4.0))
    fl_x, fl_y = torch.floor(px), torch.floor(py)
    fx, fy = px - fl_x, py - fl_y
    ix, iy = fl_x.long(), fl_y.long()
    sample = torch.arange(B, device=r.device).repeat_interleave(n).view(-1, 1, 1)
    chan = torch.arange(C, device=r.device).view(1, C, 1)
    planes = feat.reshape(B, C, H * W)

    def corner(dx, dy):
        x, y = (ix + dx).view(B * n, 1, G * G), (iy + dy).view(B * n, 1, G * G)
        on_map = (x >= 0) & (x < W) & (y >= 0) & (y < H)
        value = planes[sample, chan, (y.clamp(0, H - 1) * W + x.clamp(0, W - 1))]          # (R, C, G G)
        return torch.where(on_map, value, torch.zeros_like(value))
    wx0, wy0 = (1 - fx).view(-1, 1, G * G), (1 - fy).view(-1, 1, G * G)
    wx1, wy1 = fx.view(-1, 1, G * G), fy.view(-1, 1, G * G)
    out = ((corner(0, 0) * (wx0 * wy0) + corner(1, 0) * (wx1 * wy0)) + corner(0, 1) * (wx0 * wy1)) + corner(1, 1) * (wx1 * wy1)
    return out.view(B * n, C, G, G)


def _check(rois, spatial_features_2d, grid_size):
    assert rois.dtype == torch.float32 and rois.dim() == 3 and rois.shape[2] >= 7, 'rois: fp32 (B, n, 7 + C)'
    assert spatial_features_2d.dtype == torch.float32 and spatial_features_2d.dim() == 4, 'spatial_features_2d: fp32 (B, C, H, W)'
    assert spatial_features_2d.shape[0] == rois.shape[0], 'rois and the map: one batch'
    assert spatial_features_2d.device == rois.device, 'rois and the map: one device'
    if not 2 <= int(grid_size) <= 8:
        raise ValueError(f'bev_roi_crop: grid size {grid_size} (2 to 8)')


@torch.no_grad()
def bev_roi_crop(rois, spatial_features_2d, point_cloud_range, voxel_size, downsample_ratio, grid_size, out=None):
    """rois (B, n, 7 + C) fp32, spatial_features_2d (B, C, H, W) fp32 as BaseBEVBackbone leaves it (read in place) ->
    pooled (B n, C, G, G): what SECONDHead.roi_grid_pool's per-sample affine_grid + grid_sample(align_corners=True) compute, in one
    launch (pdm_bev_roi_crop).  `out`: a (B n, ld >= C G^2) fp32 tensor with unit column stride to write the rows into (it is
    returned as it is).  No gradient: the head detaches both inputs here (module docstring)."""
    _check(rois, spatial_features_2d, grid_size)
    B, n = rois.shape[0], rois.shape[1]
    _, C, H, W = spatial_features_2d.shape
    G = int(grid_size)
    if not rois.is_cuda:
        pooled = bev_roi_crop_torch(rois, spatial_features_2d, point_cloud_range, voxel_size, downsample_ratio, G)
        if out is None:
            return pooled
        out[:, :C * G * G] = pooled.view(B * n, -1)
        return out
    rois, feat = rois.detach().contiguous(), spatial_features_2d.detach().contiguous()
    if out is None:
        dest = pooled = torch.empty((B * n, C, G, G), dtype=torch.float32, device=rois.device)
        ld = C * G * G
    else:
        assert out.is_cuda and out.dtype == torch.float32 and out.dim() == 2 and out.shape[0] == B * n and out.shape[1] >= C * G * G \
            and (out.stride(1) == 1 or out.shape[1] == 1), 'out: fp32 (B n, ld >= C G^2) rows'
        dest, pooled, ld = out, out, (out.stride(0) if B * n > 1 else out.shape[1])
    cell_x, cell_y = _cells(voxel_size, downsample_ratio)
    _native.call("pdm_bev_roi_crop", _native.stream(rois), B, n, rois.shape[2], rois.data_ptr(), C, H, W, feat.data_ptr(),
                 float(point_cloud_range[0]), float(point_cloud_range[1]), cell_x, cell_y, G, dest.data_ptr(), ld)
    return pooled


def pack_crop_fc_weight(weight, channels, grid_size):
    """weight (Cout, C G^2[, 1]) of the Conv1d behind the crop (column c G^2 + i G + j) -> the flat fp32 tensor pdm_bev_roi_crop_fc
    reads: [kb][nb][lane][j] = W[16 nb + (lane & 15)][16 kb + 4 (lane >> 4) + j], the A fragments of mfma_f32_16x16x4f32 in the
    column order the weight already has.  Device arithmetic only."""
    w = weight.detach().float().reshape(weight.shape[0], -1)
    cout, K = w.shape
    C, G = int(channels), int(grid_size)
    if K != C * G * G or C % 16 or cout % 16:
        raise ValueError(f'bev_roi_crop_fc: weight {tuple(weight.shape)} for C = {C}, G = {G}; C and Cout must be multiples of 16')
    out = _native.mfma_a_fragments(w).transpose(0, 1).reshape(-1)      # (kb, nb, lane, j)
    assert not out.is_cuda or out.numel() == _native.lib().pdm_bev_roi_crop_fc_packed_floats(C, G, cout)
    return out


def bev_roi_crop_fc_chunks(num_rois, channels, grid_size, cout):
    """partials pdm_bev_roi_crop_fc adds per output, each over a run of ascending contraction indices: a function of these four
    numbers alone"""
    return _native.lib().pdm_bev_roi_crop_fc_chunks(int(num_rois), int(channels), int(grid_size), int(cout))


@torch.no_grad()
def bev_roi_crop_fc(rois, spatial_features_2d, point_cloud_range, voxel_size, downsample_ratio, grid_size, wpack, cout, scale=None,
                    shift=None, relu=False, out=None):
    """out (B n, cout) = epilogue(bev_roi_crop(...).view(B n, -1) @ W.T) without the (B n, C G^2) tensor (pdm_bev_roi_crop_fc):
    wpack = pack_crop_fc_weight(W, C, G); epilogue = * scale + shift (both or neither; a folded eval BatchNorm), ReLU.  The crop has
    bev_roi_crop's bits; fixed-order partials, no atomics: two runs give the same bits.  GPU tensors only; no host read; no
    gradient."""
    _check(rois, spatial_features_2d, grid_size)
    assert rois.is_cuda, 'bev_roi_crop_fc: GPU tensors (the CPU path is bev_roi_crop and the Conv1d)'
    B, n = rois.shape[0], rois.shape[1]
    _, C, H, W = spatial_features_2d.shape
    G, cout, R, dev = int(grid_size), int(cout), B * n, rois.device
    rois, feat = rois.detach().contiguous(), spatial_features_2d.detach().contiguous()
    assert wpack.is_cuda and wpack.dtype == torch.float32 and wpack.is_contiguous() and wpack.numel() == C * G * G * cout, \
        (wpack.numel(), C, G, cout)
    if out is None:
        out = torch.empty((R, cout), dtype=torch.float32, device=dev)
    assert out.shape == (R, cout) and out.is_contiguous() and out.dtype == torch.float32 and out.is_cuda
    opt = [None if t is None else t.detach().float().contiguous() for t in (scale, shift)]
    nbytes = _native.lib().pdm_bev_roi_crop_fc_workspace_bytes(R, C, G, cout)
    ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=dev)
    cell_x, cell_y = _cells(voxel_size, downsample_ratio)
    _native.call("pdm_bev_roi_crop_fc", _native.stream(dev), B, n, rois.shape[2], rois.data_ptr(), C, H, W, feat.data_ptr(),
                 float(point_cloud_range[0]), float(point_cloud_range[1]), cell_x, cell_y, G, cout, wpack.data_ptr(),
                 *(None if t is None else t.data_ptr() for t in opt), 1 if relu else 0, out.data_ptr(), ws.data_ptr(), nbytes)
    return out


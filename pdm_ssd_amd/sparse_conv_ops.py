"""The voxel path's device operators (csrc/sparse_conv.hip, csrc/sparse_conv_mfma.hip): points -> dynamic voxels with
means (voxel_assign), the rulebook of a sparse 3-D convolution (rulebook), the convolution itself on the exact f32 MFMA
(sparse_conv) with its gradients (rulebook_transpose, pack_weight_transposed, sparse_conv_dgrad, sparse_conv_wgrad of
csrc/sparse_conv_wgrad.hip, and the autograd node SparseConvFunction over them), the dense canvas of a sparse tensor (to_dense,
differentiable in the features), the site index of a level as an object of its own (site_index) and Voxel R-CNN's RoI-grid
pooling over it (roi_grid_pool, csrc/roi_grid_pool.hip) with its training form (roi_grid_query, RoIGridPoolFunction over
roi_grid_pool_train and roi_grid_pool_grad, csrc/roi_grid_train.hip).  An occupancy bitmap with scanned popcounts numbers
voxels and output sites in ascending key order: no host loop, no sort, no hash, no float atomics, so every result is a
function of the input alone and two runs give the same bits, the gradients' included.  voxel_assign and the site index
have no gradient.

Host reads: voxel_assign() copies the two ints {N', P} to the host, and a STRIDED rulebook() copies the one int P_out;
a submanifold rulebook, sparse_conv(), to_dense(), site_index(), roi_grid_pool(), roi_grid_query() and the gradients read nothing.  HOST_READS counts the copies.

Part-A2's head: pack_fc_weight / sparse_fc (csrc/sparse_fc.hip) apply the Conv1d behind SparseConvTensor.dense() to
the sparse rows of the RoI grids without the dense tensor, no host read; roiaware_pool3d_utils.roiaware_pool_sparse, which
produces those rows, counts its one host read in HOST_READS as well.

The torch formulations these stand for (torch.unique + scatter_mean, and per offset index_select -> mm -> index_add_) are
what the tests and tools/sparse_conv_rate.py compare with.
"""
from collections import namedtuple

import torch

from . import _native

HOST_READS = 0              # device-to-host copies this module has made
CIN_SUPPORTED = (3, 4, 5, 6, 7, 8, 16, 32, 64, 128)
COUT_SUPPORTED = (16, 32, 64, 128)
# wide=True (pdm_sparse_conv_wide*): the 2-D pillar backbones' 256-wide layers; the defaults keep refusing 256
CIN_WIDE = CIN_SUPPORTED + (256,)
COUT_WIDE = COUT_SUPPORTED + (256,)

Voxels = namedtuple('Voxels', ['kept_idx', 'unq_inv', 'voxel_coords', 'voxel_count', 'voxel_mean', 'num_kept', 'num_voxels'])
# in_indices / in_shape: the input rows and grid the table was built over, where an inverse convolution finds them
Rulebook = namedtuple('Rulebook', ['out_indices', 'nbr', 'out_shape', 'kernel_size', 'subm', 'in_indices', 'in_shape'],
                      defaults=(None, None))
SiteIndex = namedtuple('SiteIndex', ['workspace', 'nbytes', 'num_rows', 'batch_size', 'spatial_shape'])


def _triple(v):
    return (int(v),) * 3 if isinstance(v, int) else tuple(int(x) for x in v)


@torch.no_grad()
def voxel_assign(points, batch_size, point_cloud_range, voxel_size, grid_size):
    """points (N, 1 + C) fp32 rows (batch_idx, x, y, z, ...) in any row order -> Voxels (pdm_voxel_assign):
      kept_idx (N') int32       the rows whose cell is inside the grid on x, y and z, in input order: the reference's points[mask]
      unq_inv (N') int32        the voxel of each kept row
      voxel_coords (P, 4)       int32 (b, cz, cy, cx); voxels ascend in ((b nx + cx) ny + cy) nz + cz (torch.unique's order)
      voxel_count (P) int32, voxel_mean (P, C) = float(double(sum of llrint(v 2^20)) 2^-20 / count) of every column
    cell = floor((v - v0) / size) in fp32 with an IEEE division.  The outputs are allocated at capacity and sliced after ONE
    device-to-host copy of {N', P}."""
    global HOST_READS
    assert points.is_cuda and points.dtype == torch.float32 and points.dim() == 2 and points.shape[1] >= 4, \
        'points: fp32 (N, 1 + C) rows (batch_idx, x, y, z, ...) on the GPU'
    points = points if points.is_contiguous() else points.contiguous()
    nx, ny, nz = (int(v) for v in grid_size)
    N, C1, B, dev = points.shape[0], points.shape[1], int(batch_size), points.device
    nbytes = _native.lib().pdm_voxel_assign_workspace_bytes(N, C1, B, nx, ny, nz)
    cap = min(N, B * nx * ny * nz) if nbytes else 0     # (0: the call below rejects the sizes; nothing is allocated for it)
    i32 = dict(dtype=torch.int32, device=dev)
    kept_idx, unq_inv = (torch.empty(N, **i32) for _ in range(2))
    voxel_coords = torch.empty((cap, 4), **i32)
    voxel_count = torch.empty(cap, **i32)
    voxel_mean = torch.empty((cap, C1 - 1), dtype=torch.float32, device=dev)
    record = torch.empty(2, **i32)
    ws = torch.empty(max(nbytes, 8), dtype=torch.uint8, device=dev)
    _native.call("pdm_voxel_assign", _native.stream(dev), N, C1, points.data_ptr(), B, nx, ny, nz, *(float(v) for v in point_cloud_range[:3]),
                 *(float(v) for v in voxel_size[:3]), kept_idx.data_ptr(), unq_inv.data_ptr(), voxel_coords.data_ptr(), voxel_count.data_ptr(),
                 voxel_mean.data_ptr(), record.data_ptr(), ws.data_ptr(), nbytes)
    HOST_READS += 1
    n_kept, P = (int(v) for v in record.cpu().tolist())
    return Voxels(kept_idx[:n_kept], unq_inv[:n_kept], voxel_coords[:P], voxel_count[:P], voxel_mean[:P], n_kept, P)


def conv_out_shape(spatial_shape, kernel_size, stride=1, padding=0, subm=False):
    """(D, H, W) of the output grid: the input's for a submanifold convolution, else (in + 2 p - k) // s + 1 per axis"""
    k, s, p = _triple(kernel_size), _triple(stride), _triple(padding)
    if subm:
        return tuple(int(v) for v in spatial_shape)
    return tuple((int(n) + 2 * p[d] - k[d]) // s[d] + 1 for d, n in enumerate(spatial_shape))


@torch.no_grad()
def rulebook(indices, batch_size, spatial_shape, kernel_size, stride=1, padding=0, subm=False):
    """indices (P, 4) int32 (b, z, y, x), distinct sites in any row order on the grid spatial_shape = (D, H, W) -> Rulebook
    (pdm_sparse_sites, pdm_sparse_rulebook):
      out_indices (P_out, 4)   subm: `indices` itself (the output sites are the input rows, in input row order); strided: the
                               sites o for which some offset k has an input at o s - p + k, ascending in the key
                               ((b W' + x) H' + y) D' + z of the output grid (spconv's own order comes from a hash)
      nbr (P_out, kvol) int32  the input row under every offset, (kz, ky, kx) ascending with kx fastest, or -1; subm: the row
                               at coord + k - K // 2 (stride 1, padding unused, as spconv)
    Neighbours never cross a sample and never wrap from the end of a grid row into the next.  ONE host read (P_out) for a
    strided convolution, none for a submanifold one."""
    global HOST_READS
    assert indices.is_cuda and indices.dtype == torch.int32 and indices.dim() == 2 and indices.shape[1] == 4, \
        'indices: int32 (P, 4) rows (b, z, y, x) on the GPU'
    indices = indices if indices.is_contiguous() else indices.contiguous()
    k, s, p = _triple(kernel_size), _triple(stride), _triple(padding)
    if subm:
        s = (1, 1, 1)
    D, H, W = (int(v) for v in spatial_shape)
    P, B, dev = indices.shape[0], int(batch_size), indices.device
    geom = (B, D, H, W, *k, *s, *p, 1 if subm else 0)
    nbytes = _native.lib().pdm_sparse_rulebook_workspace_bytes(P, *geom)
    ws = torch.empty(max(nbytes, 8), dtype=torch.uint8, device=dev)
    record = torch.empty(1, dtype=torch.int32, device=dev)
    _native.call("pdm_sparse_sites", _native.stream(dev), P, indices.data_ptr(), *geom, record.data_ptr(), ws.data_ptr(), nbytes)
    kvol = k[0] * k[1] * k[2]
    if subm:
        P_out, out_indices = P, indices
    else:
        HOST_READS += 1
        P_out = int(record.cpu())
        out_indices = torch.empty((P_out, 4), dtype=torch.int32, device=dev)
    nbr = torch.empty((P_out, kvol), dtype=torch.int32, device=dev)
    _native.call("pdm_sparse_rulebook", _native.stream(dev), P, indices.data_ptr(), P_out, *geom,
                 None if subm else out_indices.data_ptr(), nbr.data_ptr(), ws.data_ptr(), nbytes)
    return Rulebook(out_indices, nbr, conv_out_shape((D, H, W), k, s, p, subm), k, bool(subm), indices, (D, H, W))


@torch.no_grad()
def site_index(indices, batch_size, spatial_shape):
    """indices (P, 4) int32 (b, z, y, x), distinct sites in any row order on the grid spatial_shape = (D, H, W) -> SiteIndex
    (pdm_sparse_index): the level's occupancy bitmap, group prefixes and row_of_rank in one workspace tensor, with the geometry
    it was built for.  roi_grid_pool() looks rows up in it: row_of_rank[rank(key)] is the row at a cell.  1 bit a cell plus 4
    bytes a row, against the 4 bytes a cell of a dense (B, D, H, W) table.  No host read; can be captured in a graph."""
    assert indices.is_cuda and indices.dtype == torch.int32 and indices.dim() == 2 and indices.shape[1] == 4, \
        'indices: int32 (P, 4) rows (b, z, y, x) on the GPU'
    indices = indices if indices.is_contiguous() else indices.contiguous()
    D, H, W = (int(v) for v in spatial_shape)
    P, B, dev = indices.shape[0], int(batch_size), indices.device
    nbytes = _native.lib().pdm_sparse_index_workspace_bytes(P, B, D, H, W)
    ws = torch.empty(max(nbytes, 8), dtype=torch.uint8, device=dev)
    _native.call("pdm_sparse_index", _native.stream(dev), P, indices.data_ptr(), B, D, H, W, ws.data_ptr(), nbytes)
    return SiteIndex(ws, nbytes, P, B, (D, H, W))


@torch.no_grad()
def roi_grid_pool(rois, grid_size, index, stride, voxel_size, point_cloud_range, features_in, wp, scale_p, shift_p, query_range, radius,
                  nsample, wout_pack, scale_o, shift_o, c_out, out=None, out_offset=0):
    """Voxel R-CNN's RoI-grid pooling over one level, one launch (pdm_roi_grid_pool): rois (B, n, 7 + ...) fp32,
    index = site_index() of the level's rows, features_in (P, C1) the level's features after mlps_in, wp (C1, 3), scale_p,
    shift_p the folded mlps_pos, query_range (rz, ry, rx), wout_pack = pack_weight of the folded mlps_out weight as
    (C2, 1, 1, 1, C1), scale_o, shift_o (C2) -> columns [out_offset, out_offset + c_out) of out (B n G^3, row stride), rows
    r G^3 + g.  No host read, no atomics: two runs and a graph replay give the same bits."""
    assert rois.is_cuda and rois.dtype == torch.float32 and rois.dim() == 3 and rois.shape[2] >= 7, 'rois: fp32 (B, n, 7 + C) on the GPU'
    rois = rois if rois.is_contiguous() else rois.contiguous()
    B, n, G = rois.shape[0], rois.shape[1], int(grid_size)
    assert B == index.batch_size, (B, index.batch_size)
    P, C1 = features_in.shape
    assert features_in.is_cuda and features_in.dtype == torch.float32 and features_in.is_contiguous() and P == index.num_rows
    M = B * n * G ** 3
    if out is None:
        out = torch.empty((M, out_offset + c_out), dtype=torch.float32, device=rois.device)
    assert out.dim() == 2 and out.shape[0] == M and out.dtype == torch.float32 and out.stride(1) == 1, tuple(out.shape)
    small = [t.detach().float().contiguous() for t in (wp, scale_p, shift_p, scale_o, shift_o)]
    rz, ry, rx = (int(v) for v in query_range)
    D, H, W = index.spatial_shape
    _native.call("pdm_roi_grid_pool", _native.stream(rois), B, n, rois.shape[2], rois.data_ptr(), G, D, H, W, int(stride),
                 *(float(v) for v in voxel_size[:3]), *(float(v) for v in point_cloud_range[:3]), P, index.workspace.data_ptr(), index.nbytes,
                 C1, features_in.data_ptr(), small[0].data_ptr(), small[1].data_ptr(), small[2].data_ptr(), rz, ry, rx, float(radius),
                 int(nsample), int(c_out), wout_pack.data_ptr(), small[3].data_ptr(), small[4].data_ptr(), out.data_ptr(),
                 out.stride(0) if M else max(out_offset + c_out, 1), int(out_offset))
    return out


RoIGroups = namedtuple('RoIGroups', ['rows', 'offsets', 'moments', 'num_rows'])


@torch.no_grad()
def roi_grid_query(rois, grid_size, index, stride, voxel_size, point_cloud_range, query_range, radius, nsample):
    """The query of the RoI-grid pooling's training form (pdm_roi_grid_query): rois (B, n, 7 + ...) fp32, index =
    site_index() of the level's rows -> RoIGroups: rows (M, nsample) int32, the group of every grid point in window order with -1
    in unused slots; offsets (M, nsample, 3) fp32, voxel centre - grid point, the bits roi_grid_pool forms; moments (9) float64,
    the sums [x, y, z, xx, xy, xz, yy, yz, zz] of the offsets over the M nsample slots of the reference's padded tensor (slot 0
    repeated into the unused slots, zeros for an empty group).  M = B n G^3 <= 2^22.  No host read; two runs give the same bits."""
    assert rois.is_cuda and rois.dtype == torch.float32 and rois.dim() == 3 and rois.shape[2] >= 7, 'rois: fp32 (B, n, 7 + C) on the GPU'
    rois = rois.detach()
    rois = rois if rois.is_contiguous() else rois.contiguous()
    B, n, G, S, dev = rois.shape[0], rois.shape[1], int(grid_size), int(nsample), rois.device
    assert B == index.batch_size, (B, index.batch_size)
    M = B * n * G ** 3
    rz, ry, rx = (int(v) for v in query_range)
    D, H, W = index.spatial_shape
    nbytes = _native.lib().pdm_roi_grid_query_workspace_bytes(M)
    ws = torch.empty(max(nbytes, 8), dtype=torch.uint8, device=dev)
    grp_row = torch.empty((M, S), dtype=torch.int32, device=dev)
    grp_off = torch.empty((M, S, 3), dtype=torch.float32, device=dev)
    moments = torch.empty(9, dtype=torch.float64, device=dev)
    _native.call("pdm_roi_grid_query", _native.stream(dev), B, n, rois.shape[2], rois.data_ptr(), G, D, H, W, int(stride),
                 *(float(v) for v in voxel_size[:3]), *(float(v) for v in point_cloud_range[:3]), index.num_rows, index.workspace.data_ptr(),
                 index.nbytes, rz, ry, rx, float(radius), S, grp_row.data_ptr(), grp_off.data_ptr(), moments.data_ptr(), ws.data_ptr(), nbytes)
    return RoIGroups(grp_row, grp_off, moments, index.num_rows)


def roi_grid_grad_chunk_points(num_grid_points, c1):
    """grid points of one partial of roi_grid_pool_grad's parameter sums: a function of these two numbers alone"""
    return _native.lib().pdm_roi_grid_pool_grad_chunk_points(int(num_grid_points), int(c1))


@torch.no_grad()
def roi_grid_pool_train(features_in, wp, scale_p, shift_p, grp_row, grp_off):
    """-> pooled (M, C1) fp32 and arg (M, C1) uint8, the winning slot or 0xFF (pdm_roi_grid_pool_train)"""
    assert features_in.is_cuda and features_in.dtype == torch.float32 and features_in.dim() == 2 and features_in.is_contiguous()
    assert grp_row.dtype == torch.int32 and grp_row.dim() == 2 and grp_row.is_contiguous() and grp_off.is_contiguous()
    assert grp_off.dtype == torch.float32 and tuple(grp_off.shape) == (*grp_row.shape, 3), tuple(grp_off.shape)
    (P, C1), (M, S), dev = features_in.shape, grp_row.shape, features_in.device
    small = [t.detach().float().contiguous() for t in (wp, scale_p, shift_p)]
    assert tuple(small[0].shape) == (C1, 3) and small[1].numel() == C1 and small[2].numel() == C1
    pooled = torch.empty((M, C1), dtype=torch.float32, device=dev)
    arg = torch.empty((M, C1), dtype=torch.uint8, device=dev)
    _native.call("pdm_roi_grid_pool_train", _native.stream(dev), M, S, P, C1, grp_row.data_ptr(), grp_off.data_ptr(), features_in.data_ptr(),
                 small[0].data_ptr(), small[1].data_ptr(), small[2].data_ptr(), pooled.data_ptr(), arg.data_ptr())
    return pooled, arg


@torch.no_grad()
def roi_grid_pool_grad(gpool, arg, grp_row, grp_off, wp, scale_p, num_rows):
    """-> dfeatures_in (P, C1), dwp (C1, 3), dscale_p (C1), dshift_p (C1) (pdm_roi_grid_pool_grad): the features' gradient in
    64-bit fixed point under integer atomics, the parameter sums through partials in a fixed order.  No host read."""
    assert gpool.is_cuda and gpool.dtype == torch.float32 and gpool.dim() == 2 and tuple(arg.shape) == tuple(gpool.shape) and arg.dtype == torch.uint8
    gpool, arg = gpool.contiguous(), arg.contiguous()
    (M, C1), S, P, dev = gpool.shape, grp_row.shape[1], int(num_rows), gpool.device
    assert tuple(grp_row.shape) == (M, S) and grp_row.is_contiguous() and grp_off.is_contiguous()
    small = [t.detach().float().contiguous() for t in (wp, scale_p)]
    nbytes = _native.lib().pdm_roi_grid_pool_grad_workspace_bytes(M, P, C1)
    ws = torch.empty(max(nbytes, 8), dtype=torch.uint8, device=dev)
    f32 = dict(dtype=torch.float32, device=dev)
    dfeat, dwp, dscale, dshift = torch.empty((P, C1), **f32), torch.empty((C1, 3), **f32), torch.empty(C1, **f32), torch.empty(C1, **f32)
    _native.call("pdm_roi_grid_pool_grad", _native.stream(dev), M, S, P, C1, gpool.data_ptr(), arg.data_ptr(), grp_row.data_ptr(), grp_off.data_ptr(),
                 small[0].data_ptr(), small[1].data_ptr(), dfeat.data_ptr(), dwp.data_ptr(), dscale.data_ptr(), dshift.data_ptr(), ws.data_ptr(),
                 nbytes)
    return dfeat, dwp, dscale, dshift


class RoIGridPoolFunction(torch.autograd.Function):
    """pooled (M, C1) = the RoI-grid pooling over kept groups (roi_grid_query), with its gradients in features_in (P, C1), wp
    (C1, 3), scale_p and shift_p (C1): forward pdm_roi_grid_pool_train, backward pdm_roi_grid_pool_grad.  Returns (pooled,
    arg); arg and the groups take no gradient."""

    @staticmethod
    def forward(ctx, features_in, wp, scale_p, shift_p, grp_row, grp_off):
        features_in = features_in.detach().float().contiguous()
        wp, scale_p, shift_p = (t.detach().float().contiguous() for t in (wp, scale_p, shift_p))
        pooled, arg = roi_grid_pool_train(features_in, wp.reshape(-1, 3), scale_p, shift_p, grp_row, grp_off)
        ctx.save_for_backward(arg, grp_row, grp_off, wp, scale_p)
        ctx.num_rows = features_in.shape[0]
        ctx.mark_non_differentiable(arg)
        return pooled, arg

    @staticmethod
    def backward(ctx, gpool, _garg=None):
        arg, grp_row, grp_off, wp, scale_p = ctx.saved_tensors
        dfeat, dwp, dscale, dshift = roi_grid_pool_grad(gpool.float(), arg, grp_row, grp_off, wp.reshape(-1, 3), scale_p, ctx.num_rows)
        return dfeat, dwp.reshape(wp.shape), dscale, dshift, None, None


def _check_widths(cin, cout, wide):
    cins, couts = (CIN_WIDE, COUT_WIDE) if wide else (CIN_SUPPORTED, COUT_SUPPORTED)
    if cin not in cins or cout not in couts:
        raise ValueError(f'sparse_conv: {cin} -> {cout} channels; Cin in {cins}, Cout in {couts}' + ('' if wide else ' (wide=True: up to 256)'))


def pack_weight(weight, wide=False):
    """weight (Cout, kz, ky, kx, Cin) (spconv 2.x's layout) -> the kernel's packed form, a flat fp32 tensor
    [k][kb][nb][lane][j] = W[cout = 16 nb + (lane & 15)][k][cin = 16 kb + 4 (lane >> 4) + j], zero past Cin: the A fragments
    of mfma_f32_16x16x4f32 in the order the kernel reads them.  Device arithmetic only.  wide: CIN_WIDE / COUT_WIDE, for the
    wide entries (the same layout, nb and kb up to 16)."""
    cout, cin = weight.shape[0], weight.shape[-1]
    _check_widths(cin, cout, wide)
    w = weight.detach().float().reshape(cout, -1, cin)
    kvol = w.shape[1]
    w = torch.nn.functional.pad(w, (0, -cin % 16))                              # (cout, kvol, 16 nkb)
    out = _native.mfma_a_fragments(w.transpose(0, 1)).transpose(1, 2).reshape(-1)      # (kvol, nkb, nb, lane, j)
    assert out.numel() == _native.lib().pdm_sparse_conv_packed_floats(kvol, cin, cout)
    return out


@torch.no_grad()
def sparse_conv(features, nbr, wpack, cin, cout, scale=None, shift=None, residual=None, relu=False, out=None, split=False, wide=False):
    """out[i, :] = epilogue(sum over k ascending of W[k] features[nbr[i, k], :]) (pdm_sparse_conv): features (P_in, cin) fp32,
    nbr (P_out, kvol) int32, wpack = pack_weight(weight); epilogue = * scale + shift (the folded BatchNorm, both or neither),
    + residual (P_out, cout), ReLU.  Output-stationary on the exact f32 MFMA, no atomics: two runs and a graph replay give
    the same bits.  No host read.  split: pdm_sparse_conv_split, which adds every offset's products in an accumulator of their own
    and that to a running sum (about a third of the rounding error of the one long chain; other bits): the training path's form.
    wide: pdm_sparse_conv_wide / pdm_sparse_conv_wide_split, which also take 256 channels and give the narrow entries' bits below."""
    assert features.is_cuda and features.dtype == torch.float32 and features.dim() == 2 and features.shape[1] == cin, tuple(features.shape)
    assert nbr.dtype == torch.int32 and nbr.dim() == 2
    features, nbr = features.contiguous(), nbr.contiguous()
    P_out, kvol = nbr.shape
    if out is None:
        out = torch.empty((P_out, cout), dtype=torch.float32, device=features.device)
    assert out.shape == (P_out, cout) and out.is_contiguous() and out.dtype == torch.float32
    if residual is not None:
        assert residual.shape == (P_out, cout) and residual.dtype == torch.float32
        residual = residual.contiguous()
    opt = [None if t is None else t.detach().float().contiguous() for t in (scale, shift)]
    entry = ("pdm_sparse_conv_wide_split" if split else "pdm_sparse_conv_wide") if wide else ("pdm_sparse_conv_split" if split else "pdm_sparse_conv")
    _native.call(entry, _native.stream(features), P_out, features.shape[0], kvol, cin, cout, features.data_ptr(), nbr.data_ptr(),
                 wpack.data_ptr(), *(None if t is None else t.data_ptr() for t in opt), None if residual is None else residual.data_ptr(),
                 1 if relu else 0, out.data_ptr())
    return out


def pack_weight_transposed(weight, flip=False, wide=False):
    """weight (Cout, kz, ky, kx, Cin) -> pack_weight of W^T, the convolution Cout -> Cin (padded to 16 when Cin < 16) that the
    data gradient runs: [k][kb][nb][lane][j] = W[cout = 16 kb + 4 (lane >> 4) + j][k' ][cin = 16 nb + (lane & 15)], zero past Cin,
    with k' = k, or k' = kvol - 1 - k when `flip` (the offset order reversed: a submanifold layer's data gradient walks the
    forward's own nbr, since nbr_t[j][k] == nbr[j][kvol - 1 - k]).  Device arithmetic only."""
    cout, cin = weight.shape[0], weight.shape[-1]
    _check_widths(cin, cout, wide)
    w = weight.detach().float().reshape(cout, -1, cin)
    if flip:
        w = w.flip(1)
    w = torch.nn.functional.pad(w.permute(2, 1, 0), (0, 0, 0, 0, 0, max(16 - cin, 0)))      # (cin padded, kvol, cout)
    return pack_weight(w.reshape(w.shape[0], *weight.shape[1:4], cout), wide=wide)


@torch.no_grad()
def rulebook_transpose(nbr, num_in_rows):
    """nbr (P_out, kvol) int32 -> nbr_t (num_in_rows, kvol) int32: nbr_t[nbr[i, k], k] = i, -1 elsewhere
    (pdm_sparse_rulebook_transpose).  At most one output site reads an input row at a given offset, so every entry has one
    writer: a fill and one launch of plain stores.  No host read."""
    assert nbr.is_cuda and nbr.dtype == torch.int32 and nbr.dim() == 2
    nbr = nbr.contiguous()
    P_out, kvol = nbr.shape
    nbr_t = torch.empty((int(num_in_rows), kvol), dtype=torch.int32, device=nbr.device)
    _native.call("pdm_sparse_rulebook_transpose", _native.stream(nbr), P_out, int(num_in_rows), kvol, nbr.data_ptr(), nbr_t.data_ptr())
    return nbr_t


def wgrad_chunk_rows(num_out_rows, kvol, cin, cout, wide=False):
    """rows of one chunk of sparse_conv_wgrad's first phase: a function of these four numbers alone"""
    query = _native.lib().pdm_sparse_conv_wide_wgrad_chunk_rows if wide else _native.lib().pdm_sparse_conv_wgrad_chunk_rows
    return query(int(num_out_rows), int(kvol), int(cin), int(cout))


@torch.no_grad()
def sparse_conv_wgrad(dy, features, nbr, kernel_size, out=None, wide=False):
    """dW (Cout, kz, ky, kx, Cin)[co, k, ci] = sum over i of dy[i, co] features[nbr[i, k], ci] (pdm_sparse_conv_wgrad): dy (P_out,
    Cout), features (P_in, Cin) fp32, nbr (P_out, kvol) int32.  Rows are the contraction of the exact f32 MFMA; partial blocks
    per (row chunk, offset) in a workspace, then one launch adds the chunks in ascending order.  No atomics, chunk boundaries a
    function of the sizes alone: two runs and a graph replay give the same bits.  No host read.  wide: pdm_sparse_conv_wide_wgrad,
    a 256-wide side as two 128-wide sub-blocks."""
    assert dy.is_cuda and dy.dtype == torch.float32 and dy.dim() == 2 and features.dtype == torch.float32 and features.dim() == 2
    assert nbr.dtype == torch.int32 and nbr.dim() == 2 and nbr.shape[0] == dy.shape[0], (tuple(nbr.shape), tuple(dy.shape))
    dy, features, nbr = dy.contiguous(), features.contiguous(), nbr.contiguous()
    k = _triple(kernel_size)
    (P_out, kvol), cin, cout = nbr.shape, features.shape[1], dy.shape[1]
    assert kvol == k[0] * k[1] * k[2], (kvol, k)
    if out is None:
        out = torch.empty((cout, *k, cin), dtype=torch.float32, device=dy.device)
    assert out.shape == (cout, *k, cin) and out.is_contiguous() and out.dtype == torch.float32
    entry = "pdm_sparse_conv_wide_wgrad" if wide else "pdm_sparse_conv_wgrad"
    nbytes = getattr(_native.lib(), entry + "_workspace_bytes")(P_out, kvol, cin, cout)
    ws = torch.empty(max(nbytes, 8), dtype=torch.uint8, device=dy.device)
    _native.call(entry, _native.stream(dy), P_out, features.shape[0], kvol, cin, cout, dy.data_ptr(), features.data_ptr(),
                 nbr.data_ptr(), out.data_ptr(), ws.data_ptr(), nbytes)
    return out


def sparse_conv_dgrad(dy, table, wpack_t, cin, cout, wide=False):
    """dx (P_in, cin) = sum over k of W[k]^T dy[table[:, k]]: the forward kernel (its split form) over `table` (P_in, kvol), which is
    rulebook_transpose(nbr, P_in) with wpack_t = pack_weight_transposed(weight), or a submanifold layer's own nbr with
    wpack_t = pack_weight_transposed(weight, flip=True).  Sliced to cin when the pack padded it to 16."""
    cin_p = max(cin, 16)
    dx = sparse_conv(dy, table, wpack_t, cout, cin_p, split=True, wide=wide)
    return dx if cin_p == cin else dx[:, :cin].contiguous()


class SparseConvFunction(torch.autograd.Function):
    """out = pdm_sparse_conv_split(features, nbr, W) + bias, with its gradients: dW by sparse_conv_wgrad, dbias = dy.sum(0), and, when
    the input requires grad, dx by sparse_conv_dgrad.  nbr_t: rulebook_transpose(nbr, P_in), or True for a submanifold layer
    (odd kernels), whose data gradient walks nbr itself; None when the input takes no gradient.  wpack / wpack_t: the packed
    weights when the caller keeps them (pack_weight, pack_weight_transposed with flip = nbr_t is True), else packed here.
    wide: every launch through the wide entries (up to 256 channels)."""

    @staticmethod
    def forward(ctx, features, weight, bias, nbr, nbr_t, cin, cout, wpack=None, wpack_t=None, wide=False):
        assert weight.shape[0] == cout and weight.shape[-1] == cin and weight.dim() == 5, (tuple(weight.shape), cin, cout)
        features = features.contiguous()
        if wpack is None:
            wpack = pack_weight(weight, wide=wide)
        shift = None if bias is None else bias.detach()
        out = sparse_conv(features.detach(), nbr, wpack, cin, cout, None if shift is None else torch.ones_like(shift), shift, split=True,
                          wide=wide)
        ctx.save_for_backward(features, weight, nbr, nbr_t if torch.is_tensor(nbr_t) else None, wpack_t)
        ctx.subm_identity, ctx.has_bias, ctx.dims, ctx.wide = nbr_t is True, bias is not None, (cin, cout), bool(wide)
        return out

    @staticmethod
    def backward(ctx, dy):
        features, weight, nbr, nbr_t, wpack_t = ctx.saved_tensors
        cin, cout = ctx.dims
        dy = dy.contiguous()
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            table = nbr if ctx.subm_identity else nbr_t
            if table is None:
                raise RuntimeError('SparseConvFunction: the input requires grad but no transposed rulebook was given')
            if wpack_t is None:
                wpack_t = pack_weight_transposed(weight, flip=ctx.subm_identity, wide=ctx.wide)
            dx = sparse_conv_dgrad(dy, table, wpack_t, cin, cout, wide=ctx.wide)
        if ctx.needs_input_grad[1]:
            dw = sparse_conv_wgrad(dy, features, nbr, weight.shape[1:4], wide=ctx.wide)
        if ctx.has_bias and ctx.needs_input_grad[2]:
            db = dy.sum(0)
        return dx, dw, db, None, None, None, None, None, None, None


class ToDenseFunction(torch.autograd.Function):
    """to_dense with the gradient of `features`: the canvas gradient gathered at `indices` (rows outside the grid, which the
    forward skips, take zero).  Torch indexing: no host read, no kernel of its own."""

    @staticmethod
    def forward(ctx, features, indices, batch_size, spatial_shape):
        ctx.save_for_backward(indices)
        ctx.grid = (int(batch_size), *(int(v) for v in spatial_shape))
        return to_dense(features.detach(), indices, batch_size, spatial_shape)

    @staticmethod
    def backward(ctx, grad):
        (indices,) = ctx.saved_tensors
        i = indices.long()
        hi = torch.tensor(ctx.grid, dtype=torch.long, device=i.device)
        inside = ((i >= 0) & (i < hi)).all(1)
        i = torch.minimum(i.clamp_min(0), hi - 1)
        g = grad[i[:, 0], :, i[:, 1], i[:, 2], i[:, 3]]
        return g * inside[:, None].to(g.dtype), None, None, None


def to_dense(features, indices, batch_size, spatial_shape, out=None):
    """features (P, C) fp32, indices (P, 4) int32 (b, z, y, x) -> (B, C, D, H, W): SparseConvTensor.dense().  One launch
    writes every element, zeros included, behind a small cell table (pdm_sparse_to_dense).  No host read.  Differentiable in
    `features` (ToDenseFunction) when they require grad and no `out` is given."""
    if out is None and features.requires_grad and torch.is_grad_enabled():
        return ToDenseFunction.apply(features, indices, batch_size, spatial_shape)
    return _to_dense(features, indices, batch_size, spatial_shape, out)


@torch.no_grad()
def _to_dense(features, indices, batch_size, spatial_shape, out=None):
    assert features.is_cuda and features.dtype == torch.float32 and features.dim() == 2 and features.shape[0] == indices.shape[0]
    assert indices.dtype == torch.int32 and indices.dim() == 2 and indices.shape[1] == 4
    features, indices = features.contiguous(), indices.contiguous()
    D, H, W = (int(v) for v in spatial_shape)
    B, (P, C), dev = int(batch_size), features.shape, features.device
    if out is None:
        out = torch.empty((B, C, D, H, W), dtype=torch.float32, device=dev)
    assert out.shape == (B, C, D, H, W) and out.is_contiguous() and out.dtype == torch.float32
    nbytes = _native.lib().pdm_sparse_to_dense_workspace_bytes(B, D, H, W)
    ws = torch.empty(max(nbytes, 8), dtype=torch.uint8, device=dev)
    _native.call("pdm_sparse_to_dense", _native.stream(dev), P, C, features.data_ptr(), indices.data_ptr(), B, D, H, W, out.data_ptr(),
                 ws.data_ptr(), nbytes)
    return out


def pack_fc_weight(weight, cells):
    """weight (Cout, C cells[, 1]), the Conv1d behind SparseConvTensor.dense() (column c cells + cell: dense() is channels-first) ->
    the flat fp32 tensor pdm_sparse_fc reads, cell-major: [cell][kb][nb][lane][j] = W[16 nb + (lane & 15)][(16 kb + 4 (lane >> 4) + j)
    cells + cell], the A fragments of mfma_f32_16x16x4f32.  Device arithmetic only."""
    w = weight.detach().float().reshape(weight.shape[0], -1)
    cout, cells = w.shape[0], int(cells)
    C = w.shape[1] // cells
    if w.shape[1] != C * cells or C % 16 or cout % 16:
        raise ValueError(f'sparse_fc: weight {tuple(weight.shape)} over {cells} cells; C and Cout must be multiples of 16')
    out = _native.mfma_a_fragments(w.reshape(cout, C, cells).permute(2, 0, 1)).transpose(1, 2).reshape(-1)     # (cell, kb, nb, lane, j)
    assert out.numel() == _native.lib().pdm_sparse_fc_packed_floats(cells, C, cout)
    return out


def sparse_fc_chunks(num_rois, cells, cout):
    """partials pdm_sparse_fc adds per output, each over a run of ascending cells: a function of these three numbers alone"""
    return _native.lib().pdm_sparse_fc_chunks(int(num_rois), int(cells), int(cout))


@torch.no_grad()
def sparse_fc(coords, feats_a, feats_b, num_rois, spatial_shape, wpack, cout, scale=None, shift=None, relu=False, out=None):
    """out (R, cout)[r] = epilogue(sum over the rows q of box r of W[:, :, cell(q)] x[q]) (pdm_sparse_fc, csrc/sparse_fc.hip):
    SparseConvTensor(cat(feats_a, feats_b), coords, spatial_shape, R).dense().view(R, -1) @ W.T without the dense tensor or the
    cat.  coords (Q, 4) int32 rows (box, x, y, z) ascending in ((box Sx + x) Sy + y) Sz + z, distinct; feats_a (Q, C_a), feats_b
    (Q, C_b) or None; wpack = pack_fc_weight(weight, Sx Sy Sz); epilogue = * scale + shift (both or neither), ReLU; boxes without
    rows get epilogue(0).  Fixed-order partials, no atomics: two runs give the same bits.  No host read."""
    assert coords.is_cuda and coords.dtype == torch.int32 and coords.dim() == 2 and coords.shape[1] == 4, 'coords: int32 (Q, 4) on the GPU'
    sx, sy, sz = (int(v) for v in spatial_shape)
    Q, R, dev = coords.shape[0], int(num_rois), coords.device
    coords, feats_a = coords.contiguous(), feats_a.contiguous()
    assert feats_a.dtype == torch.float32 and feats_a.dim() == 2 and feats_a.shape[0] == Q, tuple(feats_a.shape)
    ca, cb = feats_a.shape[1], 0
    if feats_b is not None:
        feats_b = feats_b.contiguous()
        assert feats_b.dtype == torch.float32 and feats_b.dim() == 2 and feats_b.shape[0] == Q, tuple(feats_b.shape)
        cb = feats_b.shape[1]
    assert wpack.numel() == sx * sy * sz * (ca + cb) * cout, (wpack.numel(), sx * sy * sz, ca + cb, cout)
    if out is None:
        out = torch.empty((R, cout), dtype=torch.float32, device=dev)
    assert out.shape == (R, cout) and out.is_contiguous() and out.dtype == torch.float32
    opt = [None if t is None else t.detach().float().contiguous() for t in (scale, shift)]
    nbytes = _native.lib().pdm_sparse_fc_workspace_bytes(Q, R, sx * sy * sz, cout)
    ws = torch.empty(max(nbytes, 8), dtype=torch.uint8, device=dev)
    _native.call("pdm_sparse_fc", _native.stream(dev), Q, R, sx, sy, sz, ca, cb, cout, coords.data_ptr(), feats_a.data_ptr(),
                 None if feats_b is None else feats_b.data_ptr(), wpack.data_ptr(), *(None if t is None else t.data_ptr() for t in opt),
                 1 if relu else 0, out.data_ptr(), ws.data_ptr(), nbytes)
    return out

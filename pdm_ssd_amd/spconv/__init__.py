"""A small stand-in for spconv 2.x's `spconv.pytorch` names on the device operators of sparse_conv_ops, so that the voxel
backbones read like the reference's: SparseConvTensor, SubMConv3d, SparseConv3d, SparseSequential, SparseModule.  Weights
keep spconv 2.x's layout (Cout, kz, ky, kx, Cin) and its state_dict keys (weight, bias).

Eval mode without grad: a convolution followed by BatchNorm1d and ReLU inside a SparseSequential is ONE pdm_sparse_conv
launch (the BatchNorm folded into the epilogue on the device).  A module or its norm in training mode, or an input that
requires grad, takes the autograd path on CUDA tensors: sparse_conv_ops.SparseConvFunction (forward and data gradient by
pdm_sparse_conv_split, the forward kernel with one accumulator per offset, the latter over the transposed rulebook; weight
gradient by pdm_sparse_conv_wgrad), then the BatchNorm1d module itself on the
(P, C) features (batch statistics over the active rows), + residual, ReLU, all in torch.  CPU tensors there raise
NotImplementedError.

SparseInverseConv3d(indice_key) is the forward kernel over the TRANSPOSED table of the strided convolution that built the
rulebook under that key, with the layer's own weights (not transposed, offsets not flipped): out[i] = sum over the pairs
nbr[j, k] = i of W[:, k, :] x[j].  Its rows are that convolution's input rows, in their order, on its input grid.  The table is
the one the data gradient walks (one (indice_key, 'nbr_t') slot for both).  Eval mode only: its gradients are not built.

A rulebook is built once per indice_key per forward and shared by the layers that name the key (the tensors of one forward
share one indice_dict), as spconv shares them.  Row orders: a submanifold convolution keeps its input's rows; a strided one
numbers its output sites in ascending key order of the output grid, which is build-defined (spconv's comes from a hash).

2-D: a SparseConvTensor with indices (P, 3) = (b, y, x) and spatial_shape (H, W); SubMConv2d and SparseConv2d,
weight (Cout, kh, kw, Cin).  They are the 3-D layers on a depth-1 grid (kd = 1, sd = 1, pd = 0) with everything above shared,
and they run the WIDE entries (pdm_sparse_conv_wide, _wide_split, _wide_wgrad), so they take up to 256 channels; the 3-D
classes keep the narrow entries and their 128.  dense() is (B, C, H, W).  SparseInverseConv2d is not built.
"""
import math

import torch
import torch.nn as nn

from .. import sparse_conv_ops

NEXT_STEP = ("the voxel path runs in eval mode only: the sparse convolution's data and weight gradients and BatchNorm over "
             "active rows are the next step")


class SparseConvTensor:
    def __init__(self, features, indices, spatial_shape, batch_size, indice_dict=None, indices4=None):
        """features (P, C) fp32, indices (P, 4) int32 (b, z, y, x), spatial_shape (D, H, W); or 2-D: indices (P, 3) int32
        (b, y, x), spatial_shape (H, W) (indices4: the same rows as (b, 0, y, x) when the caller holds them)"""
        self.features = features
        self.indices = indices
        self.spatial_shape = [int(v) for v in spatial_shape]
        self.batch_size = int(batch_size)
        self.indice_dict = {} if indice_dict is None else indice_dict      # indice_key -> sparse_conv_ops.Rulebook
        self._indices4 = indices4

    @property
    def ndim(self):
        return len(self.spatial_shape)

    def indices4(self):
        """the rows as the 3-D operators take them: `indices`, or (b, 0, y, x) of a 2-D tensor (made once, device arithmetic)"""
        if self.ndim == 3:
            return self.indices
        if self._indices4 is None:
            i = self.indices
            self._indices4 = torch.stack([i[:, 0], torch.zeros_like(i[:, 0]), i[:, 1], i[:, 2]], 1).contiguous()
        return self._indices4

    def shape3(self):
        return self.spatial_shape if self.ndim == 3 else [1] + self.spatial_shape

    def replace_feature(self, feature):
        return SparseConvTensor(feature, self.indices, self.spatial_shape, self.batch_size, self.indice_dict, self._indices4)

    def dense(self):
        """(B, C, D, H, W), or (B, C, H, W) of a 2-D tensor, zeros where no site is active: one launch writes every element;
        differentiable in the features"""
        out = sparse_conv_ops.to_dense(self.features, self.indices4(), self.batch_size, self.shape3())
        return out if self.ndim == 3 else out.squeeze(2)


def replace_feature(out, new_features):
    return out.replace_feature(new_features)


class SparseModule(nn.Module):
    """marks a module that takes and returns a SparseConvTensor"""


def fold_norm(norm, bias, cout, like):
    """(scale, shift) of `conv bias -> eval BatchNorm1d` as one multiply-add per channel, device arithmetic only:
    scale = gamma rsqrt(var + eps), shift = beta - mean scale + bias scale; without a norm (1, bias); (None, None) for neither"""
    if norm is None:
        return (None, None) if bias is None else (torch.ones_like(bias), bias)
    gamma = norm.weight if norm.weight is not None else torch.ones(cout, dtype=like.dtype, device=like.device)
    scale = gamma * torch.rsqrt(norm.running_var + norm.eps)
    shift = (norm.bias if norm.bias is not None else 0) - norm.running_mean * scale
    if bias is not None:
        shift = shift + bias * scale
    return scale, shift


def _depth1(v, first):
    """a 2-D layer's (h, w) setting as the depth-1 triple (first, h, w)"""
    return (first, int(v), int(v)) if isinstance(v, int) else (first, *(int(x) for x in v))


class SparseConvolution(SparseModule):
    ndim = 3            # 2 in the 2-D classes: the weight is (Cout, kh, kw, Cin), the tensors (b, y, x) on (H, W)
    wide = False        # True in the 2-D classes: the wide entries, up to 256 channels

    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, bias=True, indice_key=None, subm=False):
        super().__init__()
        self.in_channels, self.out_channels = in_channels, out_channels
        if self.ndim == 2:
            kernel_size, stride, padding = _depth1(kernel_size, 1), _depth1(stride, 1), _depth1(padding, 0)
        self.kernel_size = sparse_conv_ops._triple(kernel_size)
        self.stride = sparse_conv_ops._triple(stride)
        self.padding = sparse_conv_ops._triple(padding)
        self.indice_key = indice_key
        self.subm = subm
        self.weight = nn.Parameter(torch.empty(out_channels, *self.kernel_size[3 - self.ndim:], in_channels))
        self.bias = nn.Parameter(torch.empty(out_channels)) if bias else None
        self._cache = {}        # 'pack' / 'fold' -> (parameter versions, tensors)
        self.reset_parameters()

    def reset_parameters(self):
        nn.init.kaiming_uniform_(self.weight.view(self.out_channels, -1), a=math.sqrt(5))
        if self.bias is not None:
            bound = 1 / math.sqrt(self.in_channels * self.kernel_size[0] * self.kernel_size[1] * self.kernel_size[2])
            nn.init.uniform_(self.bias, -bound, bound)

    def _cached(self, slot, sources, make):
        """make() once per version of the source tensors (in-place updates, load_state_dict and .to() all change the key),
        as train_gemm.py caches its packed pairs"""
        key = tuple((t.data_ptr(), t._version) for t in sources if t is not None)
        hit = self._cache.get(slot)
        if hit is None or hit[0] != key:
            with torch.no_grad():
                hit = (key, make())
            self._cache[slot] = hit
        return hit[1]

    def get_rulebook(self, x):
        rb = x.indice_dict.get(self.indice_key) if self.indice_key is not None else None
        if rb is not None:
            assert rb.subm == self.subm and rb.kernel_size == self.kernel_size and (not self.subm or rb.nbr.shape[0] == x.indices.shape[0]), \
                f'indice_key {self.indice_key}: another convolution geometry built this rulebook'
            return rb
        rb = sparse_conv_ops.rulebook(x.indices4(), x.batch_size, x.shape3(), self.kernel_size, self.stride, self.padding, self.subm)
        if self.indice_key is not None:
            x.indice_dict[self.indice_key] = rb
        return rb

    def weight5(self):
        """the weight as the operators take it, (Cout, kz, ky, kx, Cin): the parameter itself, or a view of a 2-D layer's"""
        return self.weight if self.ndim == 3 else self.weight.view(self.out_channels, *self.kernel_size, self.in_channels)

    def out_tensor(self, x, features, rb):
        """the layer's output on the rulebook's output sites and grid, in the input's dimensionality"""
        if self.ndim == 3:
            return SparseConvTensor(features, rb.out_indices, rb.out_shape, x.batch_size, x.indice_dict)
        if self.subm:
            return SparseConvTensor(features, x.indices, x.spatial_shape, x.batch_size, x.indice_dict, x.indices4())
        return SparseConvTensor(features, rb.out_indices[:, [0, 2, 3]].contiguous(), rb.out_shape[1:], x.batch_size, x.indice_dict, rb.out_indices)

    def get_transpose(self, x, rb, num_in_rows=None):
        """the transposed table of a strided rulebook, built once per forward beside the rulebook it belongs to (under the
        key (indice_key, 'nbr_t') of the tensors' shared indice_dict).  num_in_rows: the rows of the rulebook's input when x
        is not that input (the inverse convolution's x is its output)"""
        key = (self.indice_key, 'nbr_t')
        nbr_t = x.indice_dict.get(key) if self.indice_key is not None else None
        if nbr_t is None:
            nbr_t = sparse_conv_ops.rulebook_transpose(rb.nbr, x.features.shape[0] if num_in_rows is None else num_in_rows)
            if self.indice_key is not None:
                x.indice_dict[key] = nbr_t
        return nbr_t

    def forward(self, x, norm=None, relu=False, residual=None):
        """x -> SparseConvTensor of epilogue(conv(x)).  norm: a BatchNorm1d; residual: (P_out, Cout) added behind it; relu
        last.  Eval mode without grad: one launch, the norm folded into the epilogue.  Training mode (the module's or the
        norm's) or an input that requires grad: the autograd path, norm, residual and ReLU in torch."""
        grad_path = self.training or (norm is not None and norm.training) or x.features.requires_grad
        if grad_path and not x.features.is_cuda:
            raise NotImplementedError(NEXT_STEP)
        assert x.features.shape[1] == self.in_channels, (tuple(x.features.shape), self.in_channels)
        assert x.ndim == self.ndim, f'a {self.ndim}-D layer on a {x.ndim}-D SparseConvTensor'
        rb = self.get_rulebook(x)
        weight, wide = self.weight5(), self.wide
        wpack = self._cached('pack', [self.weight], lambda: sparse_conv_ops.pack_weight(weight, wide=wide))
        if grad_path:
            nbr_t = wpack_t = None
            if x.features.requires_grad and torch.is_grad_enabled():
                identity = self.subm and all(k % 2 == 1 for k in self.kernel_size)      # nbr_t[j][k] == nbr[j][kvol - 1 - k]
                nbr_t = True if identity else self.get_transpose(x, rb)
                wpack_t = self._cached('pack_t', [self.weight], lambda: sparse_conv_ops.pack_weight_transposed(weight, flip=identity, wide=wide))
            out = sparse_conv_ops.SparseConvFunction.apply(x.features, weight, self.bias, rb.nbr, nbr_t, self.in_channels,
                                                           self.out_channels, wpack, wpack_t, wide)
            if norm is not None:
                out = norm(out)
            if residual is not None:
                out = out + residual
            if relu:
                out = torch.relu(out)
            return self.out_tensor(x, out, rb)
        sources = [self.bias] + ([norm.weight, norm.bias, norm.running_mean, norm.running_var] if norm is not None else [])
        scale, shift = self._cached('fold', sources, lambda: fold_norm(norm, self.bias, self.out_channels, self.weight))
        out = sparse_conv_ops.sparse_conv(x.features, rb.nbr, wpack, self.in_channels, self.out_channels, scale, shift, residual, relu,
                                          wide=wide)
        return self.out_tensor(x, out, rb)


class SubMConv3d(SparseConvolution):
    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, dilation=1, groups=1, bias=True, indice_key=None, **kwargs):
        assert dilation == 1 and groups == 1, 'dilation and groups are not built'
        super().__init__(in_channels, out_channels, kernel_size, 1, padding, bias, indice_key, subm=True)


class SparseConv3d(SparseConvolution):
    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, dilation=1, groups=1, bias=True, indice_key=None, **kwargs):
        assert dilation == 1 and groups == 1, 'dilation and groups are not built'
        super().__init__(in_channels, out_channels, kernel_size, stride, padding, bias, indice_key, subm=False)


class SubMConv2d(SparseConvolution):
    """spconv 2.x's SubMConv2d on the depth-1 grid: weight (Cout, kh, kw, Cin), up to 256 channels"""
    ndim, wide = 2, True

    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, dilation=1, groups=1, bias=True, indice_key=None, **kwargs):
        assert dilation == 1 and groups == 1, 'dilation and groups are not built'
        super().__init__(in_channels, out_channels, kernel_size, 1, padding, bias, indice_key, subm=True)


class SparseConv2d(SparseConvolution):
    """spconv 2.x's SparseConv2d on the depth-1 grid; the output sites ascend in (b W' + x) H' + y of the output grid"""
    ndim, wide = 2, True

    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, dilation=1, groups=1, bias=True, indice_key=None, **kwargs):
        assert dilation == 1 and groups == 1, 'dilation and groups are not built'
        super().__init__(in_channels, out_channels, kernel_size, stride, padding, bias, indice_key, subm=False)


class SparseInverseConv3d(SparseConvolution):
    """spconv 2.x's SparseInverseConv3d(in_channels, out_channels, kernel_size, indice_key, bias=True): undoes the site set of
    the SparseConv3d that shares its indice_key (not its values)"""

    def __init__(self, in_channels, out_channels, kernel_size, indice_key=None, bias=True, **kwargs):
        assert indice_key is not None, 'SparseInverseConv3d needs the indice_key of the convolution it inverts'
        super().__init__(in_channels, out_channels, kernel_size, 1, 0, bias, indice_key, subm=False)

    def forward(self, x, norm=None, relu=False, residual=None):
        """x: a tensor whose rows are the paired convolution's output rows -> SparseConvTensor on that convolution's input
        rows and grid.  One pdm_sparse_conv launch over the transposed table, norm and ReLU folded as SparseConvolution does."""
        if self.training or (norm is not None and norm.training) or x.features.requires_grad:
            raise NotImplementedError('SparseInverseConv3d runs in eval mode without grad: its data and weight gradients are not built')
        assert x.features.shape[1] == self.in_channels, (tuple(x.features.shape), self.in_channels)
        rb = x.indice_dict.get(self.indice_key)
        if rb is None:
            raise KeyError(f'SparseInverseConv3d: no convolution has stored a rulebook under indice_key {self.indice_key!r} in this '
                           f'tensor\'s indice_dict (keys: {[k for k in x.indice_dict if not isinstance(k, tuple)]})')
        assert not rb.subm and rb.in_indices is not None, \
            f'indice_key {self.indice_key}: a submanifold rulebook; an inverse convolution pairs with a strided SparseConv3d'
        assert rb.kernel_size == self.kernel_size, f'indice_key {self.indice_key}: kernel {rb.kernel_size}, this layer {self.kernel_size}'
        assert rb.nbr.shape[0] == x.features.shape[0], \
            f'indice_key {self.indice_key}: {x.features.shape[0]} rows, the paired convolution wrote {rb.nbr.shape[0]}'
        nbr_t = self.get_transpose(x, rb, rb.in_indices.shape[0])
        wpack = self._cached('pack', [self.weight], lambda: sparse_conv_ops.pack_weight(self.weight))
        sources = [self.bias] + ([norm.weight, norm.bias, norm.running_mean, norm.running_var] if norm is not None else [])
        scale, shift = self._cached('fold', sources, lambda: fold_norm(norm, self.bias, self.out_channels, self.weight))
        out = sparse_conv_ops.sparse_conv(x.features, nbr_t, wpack, self.in_channels, self.out_channels, scale, shift, residual, relu)
        return SparseConvTensor(out, rb.in_indices, rb.in_shape, x.batch_size, x.indice_dict)


class SparseSequential(SparseModule, nn.Sequential):
    """nn.Sequential over SparseConvTensors: sparse modules take the tensor, plain nn modules its features.  A convolution
    takes the BatchNorm1d and the ReLU behind it: into its own launch in eval mode without grad, behind its autograd node
    otherwise."""

    def forward(self, x):
        mods = list(self)
        i = 0
        while i < len(mods):
            m = mods[i]
            if isinstance(m, SparseConvolution):
                norm = mods[i + 1] if i + 1 < len(mods) and isinstance(mods[i + 1], nn.BatchNorm1d) else None
                j = i + 1 + (norm is not None)
                relu = j < len(mods) and isinstance(mods[j], nn.ReLU)
                x = m(x, norm=norm, relu=relu)
                i = j + relu
                continue
            if isinstance(m, SparseModule):
                x = m(x)
            elif isinstance(x, SparseConvTensor):
                if (self.training or x.features.requires_grad) and not x.features.is_cuda:
                    raise NotImplementedError(NEXT_STEP)
                x = x.replace_feature(m(x.features))
            else:
                x = m(x)
            i += 1
        return x


__all__ = ['SparseConvTensor', 'SparseModule', 'SparseSequential', 'SubMConv3d', 'SparseConv3d', 'SparseInverseConv3d', 'SubMConv2d',
           'SparseConv2d', 'replace_feature']

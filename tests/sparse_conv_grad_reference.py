"""What the tests of the sparse convolution's gradients share (a helper module like sparse_conv_reference.py: no tests, no
fixtures, nothing from pdm_ssd_amd's device code):

  * a numpy restatement in float64 over a rulebook's nbr (P_out, kvol): the transposed table, the data gradient dx64, the
    weight gradient dW64, their absolute-value companions A_dx and A_dW (the same sums of |dy| |w| and |dy| |x|, which bound
    the rounding error of any fp32 summation order) and n_k, the number of valid pairs per offset;
  * the torch formulation of a voxel backbone's training step over given rulebooks (per offset index_select -> mm ->
    index_add_, nn.BatchNorm1d, ReLU), in any dtype on the CPU: what the device's training step is held to.
"""
import copy

import numpy as np
import torch


def transpose(nbr, num_in_rows):
    """nbr_t (P_in, kvol): nbr_t[nbr[i, k], k] = i, -1 elsewhere; entries outside [0, P_in) count as -1"""
    nbr = np.asarray(nbr)
    out = np.full((int(num_in_rows), nbr.shape[1]), -1, dtype=np.int32)
    for k in range(nbr.shape[1]):
        col = nbr[:, k]
        ok = np.nonzero((col >= 0) & (col < num_in_rows))[0]
        out[col[ok], k] = ok
    return out


def writers(nbr, num_in_rows):
    """how many (i, k) pairs write each entry of the transposed table"""
    nbr = np.asarray(nbr)
    cnt = np.zeros((int(num_in_rows), nbr.shape[1]), dtype=np.int64)
    for k in range(nbr.shape[1]):
        col = nbr[:, k]
        np.add.at(cnt[:, k], col[(col >= 0) & (col < num_in_rows)], 1)
    return cnt


def grads(x, weight, dy, nbr):
    """x (P_in, Cin), weight (Cout, kz, ky, kx, Cin), dy (P_out, Cout), nbr (P_out, kvol) -> dict of float64 arrays:
    dx64, A_dx (P_in, Cin); dW64, A_dW (Cout, kvol, Cin); n_k (kvol)"""
    x, dy, nbr = np.asarray(x, dtype=np.float64), np.asarray(dy, dtype=np.float64), np.asarray(nbr)
    cout, cin = weight.shape[0], weight.shape[-1]
    w = np.asarray(weight, dtype=np.float64).reshape(cout, -1, cin)
    kvol, P_in = w.shape[1], len(x)
    o = dict(dx64=np.zeros((P_in, cin)), A_dx=np.zeros((P_in, cin)), dW64=np.zeros((cout, kvol, cin)), A_dW=np.zeros((cout, kvol, cin)),
             n_k=np.zeros(kvol, dtype=np.int64))
    for k in range(kvol):
        col = nbr[:, k]
        i = np.nonzero((col >= 0) & (col < P_in))[0]
        j = col[i]
        o['n_k'][k] = len(i)
        o['dW64'][:, k, :] = dy[i].T @ x[j]
        o['A_dW'][:, k, :] = np.abs(dy[i]).T @ np.abs(x[j])
        np.add.at(o['dx64'], j, dy[i] @ w[:, k, :])
        np.add.at(o['A_dx'], j, np.abs(dy[i]) @ np.abs(w[:, k, :]))
    return o


# ---- the torch formulation of a backbone's training step -----------------------------------------------------------------
def torch_conv(x, weight, bias, nbr):
    """per offset index_select -> mm -> index_add_, differentiable in x, weight and bias"""
    cout, cin = weight.shape[0], weight.shape[-1]
    w = weight.reshape(cout, -1, cin)
    out = torch.zeros((nbr.shape[0], cout), dtype=x.dtype, device=x.device)
    for k in range(w.shape[1]):
        i = torch.nonzero(nbr[:, k] >= 0).reshape(-1)
        if len(i):
            out = out.index_add(0, i, x.index_select(0, nbr[i, k].long()) @ w[:, k, :].t())
    return out if bias is None else out + bias


def _is(m, name):
    return any(c.__name__ == name for c in type(m).__mro__)


def _run(m, x, books):
    """x = (features, indices); the package's module tree, read by class name, over the rulebooks books[indice_key] =
    (out_indices, nbr)"""
    f, idx = x
    if _is(m, 'SparseConvolution'):
        out_idx, nbr = books[m.indice_key]
        return torch_conv(f, m.weight, m.bias, nbr), (idx if m.subm else out_idx)
    if _is(m, 'SparseBasicBlock'):
        assert m.downsample is None
        h = torch.relu(m.bn1(_run(m.conv1, x, books)[0]))
        return torch.relu(m.bn2(_run(m.conv2, (h, idx), books)[0]) + f), idx
    if _is(m, 'SparseSequential'):
        for child in m:
            x = _run(child, x, books)
        return x
    return m(f), idx            # BatchNorm1d, ReLU


def backbone_step(net, features, coords, batch_size, books, proj, dtype):
    """A copy of `net` in `dtype` on the CPU in training mode over the rulebooks `books` (CPU tensors): forward, the dense
    canvas by torch indexing, loss = (spatial_features * proj).sum() / numel, backward.  -> dict: 'spatial_features', 'loss',
    'grad.<parameter>', 'stat.<running statistic>' as float64 numpy arrays."""
    ref = copy.deepcopy(net).cpu().to(dtype).train()
    for p in ref.parameters():
        p.grad = None
    x = (torch.as_tensor(features).to(dtype), torch.as_tensor(coords))
    for name in ('conv_input', 'conv1', 'conv2', 'conv3', 'conv4', 'conv_out'):
        x = _run(getattr(ref, name), x, books)
    f, idx = x
    D, H, W = books['out_shape']
    dense = torch.zeros((batch_size, D, H, W, f.shape[1]), dtype=dtype)
    i = idx.long()
    dense = dense.index_put((i[:, 0], i[:, 1], i[:, 2], i[:, 3]), f)
    sf = dense.permute(0, 4, 1, 2, 3).reshape(batch_size, -1, H, W)
    loss = (sf * torch.as_tensor(proj).to(dtype)).sum() / sf.numel()
    loss.backward()
    out = {'spatial_features': sf.detach().double().numpy(), 'loss': loss.detach().double().numpy()}
    for n, p in ref.named_parameters():
        out['grad.' + n] = p.grad.double().numpy()
    for n, b in ref.named_buffers():
        if n.endswith('running_mean') or n.endswith('running_var'):
            out['stat.' + n] = b.double().numpy()
    return out

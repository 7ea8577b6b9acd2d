"""DSVT, the Dynamic Sparse Voxel Transformer backbone of the reference's pcdet/models/backbones_3d/dsvt.py, restated on this
package's operators: the same constructor signatures, config keys and state_dict keys (self_attn stays an
nn.MultiheadAttention, so the reference's checkpoints load), and the same block wiring, including the reference's use of
set_voxel_inds_list[block_id % 2][i] with pos_embed_list[i] inside a block.

Where the work runs.  In eval mode on the GPU with use_fused (the default):
  * DSVTInputLayer computes the window and set partition of every stage with dsvt_ops.set_partition (an occupancy bitmap and
    two tiled scans, one host read a stage) instead of the reference's torch.unique / torch.sort chain and its ingroup_inds
    extension; the partition is a pure function of voxel_coords and equals the reference's exactly.
  * SetAttention projects q, k (from x + pos) and v (from x) PER VOXEL with slices of self_attn.in_proj_weight, runs
    dsvt_ops.set_attention on the set indices (gather, masked softmax, both products, scatter-back in one launch) and applies
    out_proj per voxel.  A row-wise linear commutes with selecting rows, so this is the reference's result without its
    (S, ss, C) gathers and its per-layer torch.unique.
The pooling between stages and the three reduction types (linear, maxpool, attention) stay in torch.

On the CPU, with use_fused = False, and ALWAYS in training mode the torch formulations (dsvt_ops.set_partition_torch,
dsvt_ops.set_attention_torch) run: they are differentiable and apply the attention dropout.  The fused operators have no
backward yet.
"""
from math import ceil

import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import dsvt_ops
from ..config import cfg_get as _get
from ..utils.dsvt_utils import PositionEmbeddingLearned


def _prod(v):
    out = 1
    for x in v:
        out *= int(x)
    return out


class DSVT(nn.Module):
    """model_cfg: INPUT_LAYER (DSVTInputLayer's config), block_name, set_info [[set_size, blocks] a stage], d_model, nhead,
    dim_feedforward (a value a stage), dropout, activation, reduction_type ('attention' | 'maxpool' | 'linear'), output_shape,
    conv_out_channel.  forward: voxel_features (N, d_model[0]), voxel_coords (N, 4) (b, z, y, x) -> pillar_features =
    voxel_features (N_last, d_model[-1]) and the last stage's voxel_coords."""

    def __init__(self, model_cfg, **kwargs):
        super().__init__()
        self.model_cfg = model_cfg
        input_cfg = _get(model_cfg, 'INPUT_LAYER')
        self.input_layer = DSVTInputLayer(input_cfg)
        block_name, set_info = _get(model_cfg, 'block_name'), _get(model_cfg, 'set_info')
        d_model, nhead, dim_feedforward = _get(model_cfg, 'd_model'), _get(model_cfg, 'nhead'), _get(model_cfg, 'dim_feedforward')
        dropout, activation = _get(model_cfg, 'dropout'), _get(model_cfg, 'activation')
        self.reduction_type = _get(model_cfg, 'reduction_type', 'attention')
        self.use_torch_ckpt = _get(model_cfg, 'USE_CHECKPOINT', False)
        self.use_fused = True                       # False: the torch formulations on any device

        stage_num = len(block_name)
        for s in range(stage_num):
            block = _get_block_module(block_name[s])
            blocks = [block(d_model[s], nhead[s], dim_feedforward[s], dropout, activation, batch_first=True) for _ in range(set_info[s][-1])]
            self.__setattr__(f'stage_{s}', nn.ModuleList(blocks))
            self.__setattr__(f'residual_norm_stage_{s}', nn.ModuleList([nn.LayerNorm(d_model[s]) for _ in blocks]))
            if s < stage_num - 1:                   # a reduction after every stage but the last
                pool_volume = _prod(_get(input_cfg, 'downsample_stride')[s])
                if self.reduction_type == 'linear':
                    reduction = Stage_Reduction_Block(d_model[s] * pool_volume, d_model[s + 1])
                elif self.reduction_type == 'maxpool':
                    reduction = nn.MaxPool1d(pool_volume)
                elif self.reduction_type == 'attention':
                    reduction = Stage_ReductionAtt_Block(d_model[s], pool_volume)
                else:
                    raise NotImplementedError(self.reduction_type)
                self.__setattr__(f'stage_{s}_reduction', reduction)

        self.num_shifts = [2] * stage_num
        self.output_shape = _get(model_cfg, 'output_shape')
        self.stage_num = stage_num
        self.set_info = set_info
        self.num_point_features = _get(model_cfg, 'conv_out_channel')
        self._reset_parameters()

    def _fused(self, x):
        return self.use_fused and not self.training and x.is_cuda and x.dtype == torch.float32

    def forward(self, batch_dict):
        fused = self._fused(batch_dict['voxel_features'])
        self.input_layer.use_fused = fused
        info = self.input_layer(batch_dict)
        output = info['voxel_feats_stage0']
        block_id = 0
        for s in range(self.stage_num):
            inds = [info[f'set_voxel_inds_stage{s}_shift{i}'] for i in range(self.num_shifts[s])]
            masks = [info[f'set_voxel_mask_stage{s}_shift{i}'] for i in range(self.num_shifts[s])]
            blocks, norms = self.__getattr__(f'stage_{s}'), self.__getattr__(f'residual_norm_stage_{s}')
            for b, block in enumerate(blocks):
                pos = [info[f'pos_embed_stage{s}_block{b}_shift{i}'] for i in range(self.num_shifts[s])]
                residual = output
                if self.use_torch_ckpt and self.training:
                    from torch.utils.checkpoint import checkpoint
                    output = checkpoint(block, output, inds, masks, pos, block_id)
                else:
                    output = block(output, inds, masks, pos, block_id=block_id, fused=fused)
                output = norms[b](output + residual)
                block_id += 1
            if s < self.stage_num - 1:
                holder = info[f'pooling_preholder_feats_stage{s + 1}'].type_as(output)
                P, volume = holder.shape[0], holder.shape[1]
                holder[info[f'pooling_mapping_index_stage{s + 1}'], info[f'pooling_index_in_pool_stage{s + 1}']] = output
                reduction = self.__getattr__(f'stage_{s}_reduction')
                if self.reduction_type == 'linear':
                    output = reduction(holder.view(P, -1))
                elif self.reduction_type == 'maxpool':
                    output = reduction(holder.permute(0, 2, 1)).squeeze(-1)
                else:
                    output = reduction(holder.permute(0, 2, 1), torch.zeros((P, volume), dtype=torch.bool, device=holder.device))
        batch_dict['pillar_features'] = batch_dict['voxel_features'] = output
        batch_dict['voxel_coords'] = info[f'voxel_coors_stage{self.stage_num - 1}']
        return batch_dict

    def _reset_parameters(self):
        for name, p in self.named_parameters():
            if p.dim() > 1 and 'scaler' not in name:
                nn.init.xavier_uniform_(p)


class DSVTBlock(nn.Module):
    """two encoder layers: the y-axis sets, then the x-axis sets of the block's shift"""

    def __init__(self, d_model, nhead, dim_feedforward=2048, dropout=0.1, activation="relu", batch_first=True):
        super().__init__()
        self.encoder_list = nn.ModuleList([DSVT_EncoderLayer(d_model, nhead, dim_feedforward, dropout, activation, batch_first)
                                           for _ in range(2)])

    def forward(self, src, set_voxel_inds_list, set_voxel_masks_list, pos_embed_list, block_id, fused=False):
        shift = block_id % 2
        output = src
        for i, layer in enumerate(self.encoder_list):
            # the reference's wiring: axis i of shift (block_id % 2), with the position embedding of SHIFT i
            output = layer(output, set_voxel_inds_list[shift][i], set_voxel_masks_list[shift][i], pos_embed_list[i], fused=fused)
        return output


class DSVT_EncoderLayer(nn.Module):
    def __init__(self, d_model, nhead, dim_feedforward=2048, dropout=0.1, activation="relu", batch_first=True, mlp_dropout=0):
        super().__init__()
        self.win_attn = SetAttention(d_model, nhead, dropout, dim_feedforward, activation, batch_first, mlp_dropout)
        self.norm = nn.LayerNorm(d_model)
        self.d_model = d_model

    def forward(self, src, set_voxel_inds, set_voxel_masks, pos=None, fused=False):
        return self.norm(self.win_attn(src, pos, set_voxel_masks, set_voxel_inds, fused=fused) + src)


class SetAttention(nn.Module):
    def __init__(self, d_model, nhead, dropout, dim_feedforward=2048, activation="relu", batch_first=True, mlp_dropout=0):
        super().__init__()
        self.nhead = nhead
        self.self_attn = nn.MultiheadAttention(d_model, nhead, dropout=dropout, batch_first=batch_first)
        self.linear1 = nn.Linear(d_model, dim_feedforward)
        self.dropout = nn.Dropout(mlp_dropout)
        self.linear2 = nn.Linear(dim_feedforward, d_model)
        self.d_model = d_model
        self.norm1 = nn.LayerNorm(d_model)
        self.norm2 = nn.LayerNorm(d_model)
        self.dropout1 = nn.Identity()
        self.dropout2 = nn.Identity()
        self.activation = _get_activation_fn(activation)

    def forward(self, src, pos=None, key_padding_mask=None, voxel_inds=None, fused=False):
        """src (N, C) voxel features, pos (N, C) position embedding, voxel_inds (S, ss) the sets; key_padding_mask (S, ss) is
        what voxel_inds implies (a slot equal to its left neighbour) and is derived from the indices, not read."""
        C = self.d_model
        attn = self.self_attn
        w, b = attn.in_proj_weight, attn.in_proj_bias
        qk_in = src if pos is None else src + pos
        qk = F.linear(qk_in, w[:2 * C], None if b is None else b[:2 * C])          # per voxel: (N, 2C) = [q | k]
        v = F.linear(src, w[2 * C:], None if b is None else b[2 * C:])
        if fused and not (torch.is_grad_enabled() and (src.requires_grad or w.requires_grad)):
            att = dsvt_ops.set_attention(qk[:, :C], qk[:, C:], v, voxel_inds, self.nhead)
        else:
            att = dsvt_ops.set_attention_torch(qk[:, :C], qk[:, C:], v, voxel_inds, self.nhead, attn.dropout, self.training)
        src2 = attn.out_proj(att)
        src = self.norm1(src + self.dropout1(src2))
        src2 = self.linear2(self.dropout(self.activation(self.linear1(src))))
        return self.norm2(src + self.dropout2(src2))


class Stage_Reduction_Block(nn.Module):
    def __init__(self, input_channel, output_channel):
        super().__init__()
        self.linear1 = nn.Linear(input_channel, output_channel, bias=False)
        self.norm = nn.LayerNorm(output_channel)

    def forward(self, x):
        return self.norm(self.linear1(x))


class Stage_ReductionAtt_Block(nn.Module):
    """the pooled voxel's maximum over its pool queries the pool's members (plus a learned position of the member)"""

    def __init__(self, input_channel, pool_volume):
        super().__init__()
        self.pool_volume = pool_volume
        self.query_func = nn.MaxPool1d(pool_volume)
        self.norm = nn.LayerNorm(input_channel)
        self.self_attn = nn.MultiheadAttention(input_channel, 8, batch_first=True)
        self.pos_embedding = nn.Parameter(torch.randn(pool_volume, input_channel))
        nn.init.normal_(self.pos_embedding, std=.01)

    def forward(self, x, key_padding_mask):
        """x (P, C, pool_volume) -> (P, C)"""
        src = self.query_func(x).permute(0, 2, 1)
        value = x.permute(0, 2, 1)
        key = value + self.pos_embedding.unsqueeze(0)
        output = self.self_attn(src.clone(), key, value, key_padding_mask)[0]
        return self.norm(output + src).squeeze(1)


def _get_activation_fn(activation):
    if activation == "relu":
        return F.relu
    if activation == "gelu":
        return F.gelu
    if activation == "glu":
        return F.glu
    raise RuntimeError(f"activation should be relu/gelu, not {activation}.")


def _get_block_module(name):
    if name == "DSVTBlock":
        return DSVTBlock
    raise RuntimeError("This Block not exist.")


class DSVTInputLayer(nn.Module):
    """What the transformer needs of the VFE's output, per stage: the window partition for both shifts, the rotated set
    partition inside the windows, the pooling tables between stages and the position embeddings.

    model_cfg: sparse_shape (x, y, z), window_shape [(wx, wy, wz) a stage], downsample_stride [(x, y, z) between stages],
    d_model, set_info, hybrid_factor (the second shift's window is window_shape * hybrid_factor), shifts_list [[shift 0,
    shift 1] a stage], normalize_pos.  The returned dict has the reference's keys."""

    def __init__(self, model_cfg):
        super().__init__()
        self.model_cfg = model_cfg
        self.sparse_shape = _get(model_cfg, 'sparse_shape')
        self.downsample_stride = _get(model_cfg, 'downsample_stride')
        self.d_model = _get(model_cfg, 'd_model')
        self.set_info = _get(model_cfg, 'set_info')
        self.stage_num = len(self.d_model)
        self.hybrid_factor = _get(model_cfg, 'hybrid_factor')
        base = _get(model_cfg, 'window_shape')
        self.window_shape = [[list(base[s]), [base[s][c] * self.hybrid_factor[c] for c in range(3)]] for s in range(self.stage_num)]
        self.shift_list = _get(model_cfg, 'shifts_list')
        self.normalize_pos = _get(model_cfg, 'normalize_pos')
        self.num_shifts = [2] * self.stage_num
        self.use_fused = True
        self.sparse_shape_list = [tuple(self.sparse_shape)]
        for stride in self.downsample_stride:
            last = self.sparse_shape_list[-1]
            self.sparse_shape_list.append(tuple(ceil(last[c] / stride[c]) for c in range(3)))
        self.posembed_layers = nn.ModuleList()
        for s in range(self.stage_num):
            input_dim = 3 if self.sparse_shape_list[s][-1] > 1 else 2
            self.posembed_layers.append(nn.ModuleList([
                nn.ModuleList([PositionEmbeddingLearned(input_dim, self.d_model[s]) for _ in range(self.num_shifts[s])])
                for _ in range(self.set_info[s][1])]))

    def forward(self, batch_dict):
        feats, coors = batch_dict['voxel_features'], batch_dict['voxel_coords']
        batch_size = batch_dict.get('batch_size', None)
        if batch_size is None:
            batch_size = int(coors[:, 0].max()) + 1 if coors.shape[0] else 0
        info = {'voxel_feats_stage0': feats, 'voxel_coors_stage0': coors}
        for s in range(self.stage_num):
            self.partition(info, s, int(batch_size))
            for b in range(self.set_info[s][1]):
                for i in range(self.num_shifts[s]):
                    info[f'pos_embed_stage{s}_block{b}_shift{i}'] = self.get_pos_embed(info[f'coors_in_win_stage{s}_shift{i}'], s, b, i)
            if s < self.stage_num - 1:
                self.subm_pooling(info, s)
        return info

    @torch.no_grad()
    def partition(self, info, s, batch_size):
        coors = info[f'voxel_coors_stage{s}']
        args = (self.sparse_shape_list[s], self.window_shape[s], self.shift_list[s], self.set_info[s][0])
        if self.use_fused and coors.is_cuda:
            part = dsvt_ops.set_partition(coors.int(), batch_size, *args)
        else:
            part = dsvt_ops.set_partition_torch(coors, *args)
        for i in range(2):
            info[f'coors_in_win_stage{s}_shift{i}'] = part.coors_in_win[i]
            info[f'set_voxel_inds_stage{s}_shift{i}'] = part.set_voxel_inds[i]
            info[f'set_voxel_mask_stage{s}_shift{i}'] = part.set_voxel_mask[i]

    @torch.no_grad()
    def subm_pooling(self, info, s):
        stride = self.downsample_stride[s]
        win, _, index_in_win, win_coors = dsvt_ops.pooling_index(info[f'voxel_coors_stage{s}'], self.sparse_shape_list[s], stride)
        unique, inverse = torch.unique(win, return_inverse=True)
        info[f'pooling_mapping_index_stage{s + 1}'] = inverse
        info[f'pooling_index_in_pool_stage{s + 1}'] = index_in_win
        info[f'pooling_preholder_feats_stage{s + 1}'] = info['voxel_feats_stage0'].new_zeros((len(unique), _prod(stride), self.d_model[s]))
        # every member of a pool has the pool's coordinates: any of them serves
        pool_coors = win_coors.new_zeros((len(unique), 4))
        pool_coors[inverse] = win_coors
        info[f'voxel_coors_stage{s + 1}'] = pool_coors

    def get_pos_embed(self, coors_in_win, s, b, i):
        """coors_in_win (N, 3) (z, y, x) -> (N, d_model): the embedding of the position relative to the window's centre"""
        wx, wy, wz = self.window_shape[s][i]
        layer = self.posembed_layers[s][b][i]
        ndim = 2 if wz == 1 else 3
        c = coors_in_win.to(layer.position_embedding_head[0].weight.dtype)
        x, y = c[:, 2] - wx / 2, c[:, 1] - wy / 2
        if self.normalize_pos:
            x, y = x / wx * 2 * 3.1415, y / wy * 2 * 3.1415
        cols = [x, y]
        if ndim == 3:
            z = c[:, 0] - wz / 2
            cols.append(z / wz * 2 * 3.1415 if self.normalize_pos else z)
        return layer(torch.stack(cols, dim=-1))

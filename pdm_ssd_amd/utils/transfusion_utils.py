"""The transformer pieces of TransFusionHead (the reference's pcdet/models/model_utils/transfusion_utils.py):
PositionEmbeddingLearned and a decoder layer of self-attention, cross-attention and a feed-forward block, post-norm.

self_attn and multihead_attn are nn.MultiheadAttention modules, so the state-dict keys are the reference's; the CPU path,
training mode and use_fused = False run through them.  On the GPU in eval mode the layer applies slices of their
in_proj_weight / in_proj_bias itself (one GEMM gives [Q; K; V] of the self-attention and [K; V] of the cross-attention,
whose key and value are both key + key_pos_embed), calls attention_ops.mha_forward on the projected rows and then the
out-projection.  LayerNorm, the feed-forward block and the residuals stay torch.

fused_train = True (TransFusionHead's FUSED_ATTENTION_TRAIN) gives training mode the same structure under autograd:
attention_ops.mha_qkv / mha_kv on the packed projections, with the modules' attention dropout drawn from the layer's own
counter-based draws (set_attention_seed; one device step counter per attention, two non-persistent buffers, so the state
dict is unchanged and the counters are NOT checkpointed: a resumed run draws from step 0 unless the caller restores them).
"""
import torch
from torch import nn
import torch.nn.functional as F


def clip_sigmoid(x, eps=1e-4):
    return torch.clamp(x.sigmoid_(), min=eps, max=1 - eps)


class PositionEmbeddingLearned(nn.Module):
    """(B, N, input_channel) positions -> (B, num_pos_feats, N): two 1 x 1 convolutions with BatchNorm and ReLU between"""

    def __init__(self, input_channel, num_pos_feats=288):
        super().__init__()
        self.position_embedding_head = nn.Sequential(
            nn.Conv1d(input_channel, num_pos_feats, kernel_size=1), nn.BatchNorm1d(num_pos_feats), nn.ReLU(inplace=True),
            nn.Conv1d(num_pos_feats, num_pos_feats, kernel_size=1))

    def forward(self, xyz):
        return self.position_embedding_head(xyz.transpose(1, 2).contiguous())


_ACTIVATIONS = {'relu': F.relu, 'gelu': F.gelu, 'glu': F.glu}


class TransformerDecoderLayer(nn.Module):
    def __init__(self, d_model, nhead, dim_feedforward=2048, dropout=0.1, activation='relu', self_posembed=None, cross_posembed=None,
                 cross_only=False):
        super().__init__()
        self.cross_only = cross_only
        if not cross_only:
            self.self_attn = nn.MultiheadAttention(d_model, nhead, dropout=dropout)
        self.multihead_attn = nn.MultiheadAttention(d_model, nhead, dropout=dropout)
        self.linear1 = nn.Linear(d_model, dim_feedforward)
        self.dropout = nn.Dropout(dropout)
        self.linear2 = nn.Linear(dim_feedforward, d_model)
        self.norm1, self.norm2, self.norm3 = nn.LayerNorm(d_model), nn.LayerNorm(d_model), nn.LayerNorm(d_model)
        self.dropout1, self.dropout2, self.dropout3 = nn.Dropout(dropout), nn.Dropout(dropout), nn.Dropout(dropout)
        if activation not in _ACTIVATIONS:
            raise RuntimeError(f'activation should be relu/gelu/glu, not {activation}.')
        self.activation = _ACTIVATIONS[activation]
        self.self_posembed, self.cross_posembed = self_posembed, cross_posembed
        self.nhead = nhead
        self.use_fused = True            # False: nn.MultiheadAttention on any device
        self.fused_self = True           # which of the two attentions the fused path hands to mha_forward
        self.fused_cross = True
        self.keys_per_chunk = 0          # 0: the library's default
        self.fused_train = False         # True: training mode runs the fused attention under autograd
        self.attention_seed = 0
        self.register_buffer('attn_step_self', torch.zeros(1, dtype=torch.int32), persistent=False)
        self.register_buffer('attn_step_cross', torch.zeros(1, dtype=torch.int32), persistent=False)

    def set_attention_seed(self, seed):
        """the seed of the fused training path's attention dropout; data-parallel ranks must pass different seeds"""
        self.attention_seed = int(seed)

    def reset_attention_steps(self, value=0):
        self.attn_step_self.fill_(int(value))
        self.attn_step_cross.fill_(int(value))

    @staticmethod
    def with_pos_embed(tensor, pos_embed):
        return tensor if pos_embed is None else tensor + pos_embed

    def _fusable(self, query):
        d = query.shape[1] // self.nhead
        return (self.use_fused and (not self.training or self.fused_train) and query.is_cuda and query.dtype == torch.float32 and d in (16, 32)
                and query.shape[1] <= 256 and (self.fused_self or self.fused_cross))

    def forward(self, query, key, query_pos, key_pos, key_padding_mask=None, attn_mask=None):
        """query (B, C, P), key (B, C, N), query_pos (B, P, 2), key_pos (B | 1, N, 2) -> (B, C, P)"""
        if key_padding_mask is None and attn_mask is None and self._fusable(query):
            if self.training:
                return self._forward_fused_train(query, key, query_pos, key_pos)
            return self._forward_fused(query, key, query_pos, key_pos)
        # sequence first, as nn.MultiheadAttention takes it: (P, B, C), (N, B, C)
        query_pos_embed = self.self_posembed(query_pos).permute(2, 0, 1) if self.self_posembed is not None else None
        key_pos_embed = self.cross_posembed(key_pos).permute(2, 0, 1) if self.cross_posembed is not None else None
        query, key = query.permute(2, 0, 1), key.permute(2, 0, 1)
        if not self.cross_only:
            q = k = v = self.with_pos_embed(query, query_pos_embed)
            query = self.norm1(query + self.dropout1(self.self_attn(q, k, value=v)[0]))
        kv = self.with_pos_embed(key, key_pos_embed)
        query2 = self.multihead_attn(query=self.with_pos_embed(query, query_pos_embed), key=kv, value=kv,
                                     key_padding_mask=key_padding_mask, attn_mask=attn_mask)[0]
        query = self.norm2(query + self.dropout2(query2))
        query2 = self.linear2(self.dropout(self.activation(self.linear1(query))))
        query = self.norm3(query + self.dropout3(query2))
        return query.permute(1, 2, 0)

    def _attend(self, attn, fused, q_in, kv_in, same):
        """one attention of the eval path, batch first: q_in (B, P, C), kv_in (B, N, C) (key = value); same: q_in is kv_in"""
        from .. import attention_ops
        C = q_in.shape[-1]
        W, b = attn.in_proj_weight, attn.in_proj_bias
        if same:
            qkv = F.linear(q_in, W, b)                                # (B, P, 3C): [Q; K; V] in one GEMM
            q, k, v = qkv[..., :C], qkv[..., C:2 * C], qkv[..., 2 * C:]
        else:
            q = F.linear(q_in, W[:C], None if b is None else b[:C])
            kv = F.linear(kv_in, W[C:], None if b is None else b[C:])    # (B, N, 2C): [K; V] in one GEMM
            k, v = kv[..., :C], kv[..., C:]
        if fused:
            out = attention_ops.mha_forward(q, k, v, self.nhead, self.keys_per_chunk)
        else:
            out = attention_ops.mha_reference(q, k, v, self.nhead)
        return F.linear(out, attn.out_proj.weight, attn.out_proj.bias)

    @torch.no_grad()
    def _forward_fused(self, query, key, query_pos, key_pos):
        B = query.shape[0]
        x = query.transpose(1, 2)                                     # (B, P, C)
        qpe = self.self_posembed(query_pos).transpose(1, 2) if self.self_posembed is not None else None
        kpe = self.cross_posembed(key_pos).transpose(1, 2) if self.cross_posembed is not None else None    # (B | 1, N, C)
        if not self.cross_only:
            t = self.with_pos_embed(x, qpe)
            x = self.norm1(x + self._attend(self.self_attn, self.fused_self, t, t, True))
        kv_in = self.with_pos_embed(key.transpose(1, 2), kpe)
        if kv_in.shape[0] != B:
            kv_in = kv_in.expand(B, -1, -1)
        x = self.norm2(x + self._attend(self.multihead_attn, self.fused_cross, self.with_pos_embed(x, qpe), kv_in, False))
        x = self.norm3(x + self.linear2(self.activation(self.linear1(x))))
        return x.transpose(1, 2)

    def _attend_train(self, attn, fused, q_in, kv_in, same, draws):
        """_attend under autograd with the module's attention dropout: the packed projections go to mha_qkv / mha_kv"""
        from .. import attention_ops
        C = q_in.shape[-1]
        W, b = attn.in_proj_weight, attn.in_proj_bias
        p = float(attn.dropout)
        if same:
            qkv = F.linear(q_in, W, b)                                # (B, P, 3C)
            if fused:
                out = attention_ops.mha_qkv(qkv, self.nhead, p, draws, self.keys_per_chunk)
            else:
                out = self._attend_torch(qkv[..., :C], qkv[..., C:2 * C], qkv[..., 2 * C:], p)
        else:
            q = F.linear(q_in, W[:C], None if b is None else b[:C])
            kv = F.linear(kv_in, W[C:], None if b is None else b[C:])    # (B, N, 2C)
            if fused:
                out = attention_ops.mha_kv(q, kv, self.nhead, p, draws, self.keys_per_chunk)
            else:
                out = self._attend_torch(q, kv[..., :C], kv[..., C:], p)
        return F.linear(out, attn.out_proj.weight, attn.out_proj.bias)

    def _attend_torch(self, q, k, v, p):
        """an attention fused_self / fused_cross leaves to torch: the weights materialised, torch's own dropout on them"""
        B, P, C = q.shape
        d = C // self.nhead
        qh, kh, vh = (t.reshape(B, t.shape[1], self.nhead, d).transpose(1, 2) for t in (q, k, v))
        w = F.dropout(torch.softmax(qh @ kh.transpose(-1, -2) / d ** 0.5, dim=-1), p, True)
        return (w @ vh).transpose(1, 2).reshape(B, P, C)

    def _forward_fused_train(self, query, key, query_pos, key_pos):
        from .. import attention_ops
        B = query.shape[0]
        seed = (2 * self.attention_seed) & 0xFFFFFFFF                 # two streams of the seed: even self, odd cross
        x = query.transpose(1, 2)                                     # (B, P, C)
        qpe = self.self_posembed(query_pos).transpose(1, 2) if self.self_posembed is not None else None
        kpe = self.cross_posembed(key_pos).transpose(1, 2) if self.cross_posembed is not None else None    # (B | 1, N, C)
        if not self.cross_only:
            t = self.with_pos_embed(x, qpe)
            draws = attention_ops.AttentionDraws(seed, x.device, self.attn_step_self)
            x = self.norm1(x + self.dropout1(self._attend_train(self.self_attn, self.fused_self, t, t, True, draws)))
        kv_in = self.with_pos_embed(key.transpose(1, 2), kpe)
        if kv_in.shape[0] != B:
            kv_in = kv_in.expand(B, -1, -1)
        draws = attention_ops.AttentionDraws(seed | 1, x.device, self.attn_step_cross)
        x = self.norm2(x + self.dropout2(self._attend_train(self.multihead_attn, self.fused_cross, self.with_pos_embed(x, qpe), kv_in,
                                                            False, draws)))
        x = self.norm3(x + self.dropout3(self.linear2(self.dropout(self.activation(self.linear1(x))))))
        return x.transpose(1, 2)

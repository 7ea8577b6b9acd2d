"""The learned position embedding of DSVT (the reference's pcdet/models/model_utils/dsvt_utils.py keeps it with the window
arithmetic; that arithmetic lives in dsvt_ops.py here, next to the operator that replaces it)."""
import torch.nn as nn


class PositionEmbeddingLearned(nn.Module):
    """in-window coordinates (N, input_channel) -> (N, num_pos_feats): Linear, BatchNorm1d, ReLU, Linear
    (state_dict keys position_embedding_head.{0, 1, 3}.*)"""

    def __init__(self, input_channel, num_pos_feats):
        super().__init__()
        self.position_embedding_head = nn.Sequential(
            nn.Linear(input_channel, num_pos_feats), nn.BatchNorm1d(num_pos_feats), nn.ReLU(inplace=True),
            nn.Linear(num_pos_feats, num_pos_feats))

    def forward(self, xyz):
        return self.position_embedding_head(xyz)

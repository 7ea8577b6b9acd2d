"""Target assigners of the RoI heads (as /root/reference/pcdet/models/roi_heads/target_assigner/)."""
from .proposal_target_layer import ProposalTargetLayer

__all__ = ['ProposalTargetLayer']

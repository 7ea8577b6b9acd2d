"""Anchor generation and target assignment of the anchor heads (the reference's pcdet/models/dense_heads/target_assigner)."""
from .anchor_generator import AnchorGenerator
from .axis_aligned_target_assigner import AxisAlignedTargetAssigner

__all__ = ['AnchorGenerator', 'AxisAlignedTargetAssigner']

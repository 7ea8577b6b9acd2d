"""Anchor generation and target assignment of the anchor heads, and the Hungarian assigner of TransFusionHead (the reference's pcdet/models/dense_heads/target_assigner)."""
from .anchor_generator import AnchorGenerator
from .axis_aligned_target_assigner import AxisAlignedTargetAssigner
from .hungarian_assigner import HungarianAssigner3D

__all__ = ['AnchorGenerator', 'AxisAlignedTargetAssigner', 'HungarianAssigner3D']

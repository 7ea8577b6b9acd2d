"""Heads of the detector, registered by NAME as /root/reference/pcdet/models/dense_heads/__init__.py:11-21 does."""
from .anchor_head_single import AnchorHeadSingle
from .anchor_head_template import AnchorHeadTemplate
from .center_head import CenterHead
from .pdm_heatmap_head import PDMHeatmapHead
from .point_head_box import PointHeadBox
from .point_head_simple import PointHeadSimple
from .point_intra_part_head import PointIntraPartOffsetHead
from .point_head_template import PointHeadTemplate
from .transfusion_head import TransFusionHead

__all__ = {
    'PointHeadTemplate': PointHeadTemplate,
    'PointHeadBox': PointHeadBox,
    'PointHeadSimple': PointHeadSimple,
    'PointIntraPartOffsetHead': PointIntraPartOffsetHead,
    'PDMHeatmapHead': PDMHeatmapHead,
    'CenterHead': CenterHead,
    'AnchorHeadTemplate': AnchorHeadTemplate,
    'AnchorHeadSingle': AnchorHeadSingle,
    'TransFusionHead': TransFusionHead,
}

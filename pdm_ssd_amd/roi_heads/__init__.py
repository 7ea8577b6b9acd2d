"""RoI (second-stage) heads, registered by NAME as /root/reference/pcdet/models/roi_heads/__init__.py does."""
from .partA2_head import PartA2FCHead
from .pointrcnn_head import PointRCNNHead
from .pvrcnn_head import PVRCNNHead
from .roi_head_template import RoIHeadTemplate
from .second_head import SECONDHead
from .voxelrcnn_head import VoxelRCNNHead

__all__ = {
    'RoIHeadTemplate': RoIHeadTemplate,
    'PointRCNNHead': PointRCNNHead,
    'VoxelRCNNHead': VoxelRCNNHead,
    'PVRCNNHead': PVRCNNHead,
    'PartA2FCHead': PartA2FCHead,
    'SECONDHead': SECONDHead,
}

"""Pillars or an encoded sparse tensor -> BEV canvas, registered by NAME as the reference's
pcdet/models/backbones_2d/map_to_bev/__init__.py does."""
from .height_compression import HeightCompression
from .pointpillar_scatter import PointPillarScatter, PointPillarScatter3d

__all__ = {
    'PointPillarScatter': PointPillarScatter,
    'PointPillarScatter3d': PointPillarScatter3d,
    'HeightCompression': HeightCompression,
}

"""Voxel feature encoders, registered by NAME as the reference's pcdet/models/backbones_3d/vfe/__init__.py does.  Only the
dynamic pillar encoder exists here: the hard-voxel encoders (MeanVFE, PillarVFE) need spconv's voxel generator."""
from .dynamic_pillar_vfe import DynamicPillarVFE, PFNLayerV2
from .vfe_template import VFETemplate

__all__ = {
    'VFETemplate': VFETemplate,
    'DynamicPillarVFE': DynamicPillarVFE,
}

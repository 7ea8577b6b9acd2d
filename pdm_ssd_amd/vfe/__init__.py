"""Voxel feature encoders, registered by NAME as the reference's pcdet/models/backbones_3d/vfe/__init__.py does.  The two
dynamic encoders exist here, DynamicPillarVFE for the pillar path and DynamicMeanVFE for the voxel path; the hard-voxel
encoders (MeanVFE, PillarVFE) need spconv's voxel generator and stay refused."""
from .dynamic_mean_vfe import DynamicMeanVFE
from .dynamic_pillar_vfe import DynamicPillarVFE, PFNLayerV2
from .vfe_template import VFETemplate

__all__ = {
    'VFETemplate': VFETemplate,
    'DynamicPillarVFE': DynamicPillarVFE,
    'DynamicMeanVFE': DynamicMeanVFE,
}

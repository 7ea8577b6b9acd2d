"""Voxel feature encoders, registered by NAME as the reference's pcdet/models/backbones_3d/vfe/__init__.py does.  The two
dynamic encoders, DynamicPillarVFE for the pillar path and DynamicMeanVFE for the voxel path, keep every point of every
occupied cell; DynamicPillarVFESimple2D is the pillar encoder of the sparse 2-D backbones (PillarNet).  The hard-voxel encoders (at most MAX_POINTS_PER_VOXEL points a cell, at most MAX_NUMBER_OF_VOXELS cells a
sample: what the reference's published KITTI models were trained on) are the classes MeanVFE and PillarVFE, registered under
the names `HardMeanVFE` and `HardPillarVFE`: they voxelize on the device (hard_voxel_ops) and so carry the voxelizer's two
sizes in their own config, which the reference keeps in its dataset's; a config written for the reference does not have them
there.  The plain names `MeanVFE` / `PillarVFE` as a config NAME therefore stay refused, with the message that names spconv,
whose CPU voxel generator the reference's versions depend on."""
from .dynamic_mean_vfe import DynamicMeanVFE
from .dynamic_pillar_vfe import DynamicPillarVFE, PFNLayerV2
from .dynamic_pillar_vfe_simple2d import DynamicPillarVFESimple2D
from .mean_vfe import MeanVFE
from .pillar_vfe import PFNLayer, PillarVFE
from .vfe_template import VFETemplate

__all__ = {
    'VFETemplate': VFETemplate,
    'DynamicPillarVFE': DynamicPillarVFE,
    'DynamicPillarVFESimple2D': DynamicPillarVFESimple2D,
    'DynamicMeanVFE': DynamicMeanVFE,
    'HardMeanVFE': MeanVFE,
    'HardPillarVFE': PillarVFE,
}

"""Point feature encoders, registered by NAME as the reference's pcdet/models/backbones_3d/pfe/__init__.py does."""
from .voxel_set_abstraction import VoxelSetAbstraction
from .voxel_set_abstraction_spc import VoxelSetAbstractionSPC

__all__ = {
    'VoxelSetAbstraction': VoxelSetAbstraction,
    'VoxelSetAbstractionSPC': VoxelSetAbstractionSPC,
}

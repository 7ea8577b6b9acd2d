"""3-D backbones of the voxel family, the sparse 2-D backbones of the pillar family (PillarNet) and DSVT, registered by NAME as the
reference's pcdet/models/backbones_3d/__init__.py does."""
from . import pfe  # noqa: F401
from .dsvt import DSVT
from .spconv_backbone import SparseBasicBlock, VoxelBackBone8x, VoxelResBackBone8x, post_act_block
from .spconv_backbone_2d import PillarBackBone8x, PillarRes18BackBone8x
from .spconv_unet import UNetV2

__all__ = {
    'VoxelBackBone8x': VoxelBackBone8x,
    'VoxelResBackBone8x': VoxelResBackBone8x,
    'UNetV2': UNetV2,
    'PillarBackBone8x': PillarBackBone8x,
    'PillarRes18BackBone8x': PillarRes18BackBone8x,
    'DSVT': DSVT,
}

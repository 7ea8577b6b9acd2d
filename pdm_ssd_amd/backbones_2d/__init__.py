"""2-D backbones, registered by NAME as the reference's pcdet/models/backbones_2d/__init__.py does."""
from .base_bev_backbone import BaseBEVBackbone, BaseBEVBackboneV1, BaseBEVResBackbone

__all__ = {
    'BaseBEVBackbone': BaseBEVBackbone,
    'BaseBEVBackboneV1': BaseBEVBackboneV1,
    'BaseBEVResBackbone': BaseBEVResBackbone,
}

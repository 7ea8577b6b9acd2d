"""PillarNet: DynamicPillarVFESimple2D -> a sparse 2-D pillar backbone -> BaseBEVBackboneV1 -> CenterHead, the forward,
get_training_loss and post_processing of the reference's pcdet/models/detectors/pillarnet.py on this repository's template: they are
CenterPoint's (the head has decoded and suppressed its boxes; post_processing adds the recall record), and tb_dict holds detached
0-dim tensors instead of the reference's .item() (no host read in the training step)."""
from .centerpoint import CenterPoint


class PillarNet(CenterPoint):
    pass

"""AnchorGenerator: per anchor set a (1, ny, nx, #sizes, #rotations, 7) table of [x, y, z, dx, dy, dz, heading], the
reference's pcdet/models/dense_heads/target_assigner/anchor_generator.py.  The tables are built on the CPU (the reference
builds them on the GPU); whoever owns them moves them."""
import torch


def _get(cfg, key, default=None):
    return cfg.get(key, default) if isinstance(cfg, dict) else getattr(cfg, key, default)


class AnchorGenerator(object):
    def __init__(self, anchor_range, anchor_generator_config):
        super().__init__()
        self.anchor_generator_cfg = anchor_generator_config
        self.anchor_range = anchor_range
        self.anchor_sizes = [_get(config, 'anchor_sizes') for config in anchor_generator_config]
        self.anchor_rotations = [_get(config, 'anchor_rotations') for config in anchor_generator_config]
        self.anchor_heights = [_get(config, 'anchor_bottom_heights') for config in anchor_generator_config]
        self.align_center = [_get(config, 'align_center', False) for config in anchor_generator_config]
        assert len(self.anchor_sizes) == len(self.anchor_rotations) == len(self.anchor_heights)
        self.num_of_anchor_sets = len(self.anchor_sizes)

    def generate_anchors(self, grid_sizes):
        """grid_sizes: per set the map's [nx, ny] -> (list of (1, ny, nx, #sizes, #rotations, 7) fp32 tables, list of anchors per
        location).  Cell centres lie on [range_min, range_max] end points included (align_center: False) or in the middle
        of nx equal cells (True); z is the bottom height plus half the anchor's height."""
        assert len(grid_sizes) == self.num_of_anchor_sets
        all_anchors, num_anchors_per_location = [], []
        lo, hi = self.anchor_range[0:3], self.anchor_range[3:6]
        for grid_size, sizes, rotations, heights, align_center in zip(grid_sizes, self.anchor_sizes, self.anchor_rotations,
                                                                      self.anchor_heights, self.align_center):
            num_anchors_per_location.append(len(rotations) * len(sizes) * len(heights))
            if align_center:
                x_stride, y_stride = (hi[0] - lo[0]) / grid_size[0], (hi[1] - lo[1]) / grid_size[1]
                x_offset, y_offset = x_stride / 2, y_stride / 2
            else:
                x_stride, y_stride = (hi[0] - lo[0]) / (grid_size[0] - 1), (hi[1] - lo[1]) / (grid_size[1] - 1)
                x_offset, y_offset = 0, 0
            x_shifts = torch.arange(lo[0] + x_offset, hi[0] + 1e-5, step=x_stride, dtype=torch.float32)
            y_shifts = torch.arange(lo[1] + y_offset, hi[1] + 1e-5, step=y_stride, dtype=torch.float32)
            z_shifts = x_shifts.new_tensor(heights)
            nx, ny, nz, ns, nr = len(x_shifts), len(y_shifts), len(z_shifts), len(sizes), len(rotations)
            anchors = x_shifts.new_zeros((nz, ny, nx, ns, nr, 7))
            anchors[..., 0] = x_shifts.view(1, 1, nx, 1, 1)
            anchors[..., 1] = y_shifts.view(1, ny, 1, 1, 1)
            anchors[..., 2] = z_shifts.view(nz, 1, 1, 1, 1)
            anchors[..., 3:6] = x_shifts.new_tensor(sizes).view(1, 1, 1, ns, 1, 3)
            anchors[..., 6] = x_shifts.new_tensor(rotations).view(1, 1, 1, 1, nr)
            anchors[..., 2] += anchors[..., 5] / 2                  # bottom height -> box centre
            all_anchors.append(anchors)
        return all_anchors, num_anchors_per_location

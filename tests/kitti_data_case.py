"""Shared by the KITTI dataset front end's tests: the fixture of the reference's run (tests/golden/ref_kitti_data.*),
split per frame and per object, and the synthetic tree it was made on."""
import hashlib
import json
import os

import numpy as np

import kitti_tree

HERE = os.path.dirname(os.path.abspath(__file__))
NPZ = os.path.join(HERE, 'golden', 'ref_kitti_data.npz')
META = os.path.join(HERE, 'golden', 'ref_kitti_data.json')
CLASS_NAMES = ['Car', 'Pedestrian', 'Cyclist']
PER_GT = ('truncated', 'occluded', 'alpha', 'bbox', 'dimensions', 'location', 'rotation_y', 'score', 'difficulty', 'index',
          'num_points_in_gt')


def tree_digest(root):
    h = hashlib.sha256()
    for part in ('training', 'testing'):
        for sub in ('velodyne', 'calib', 'label_2'):
            d = os.path.join(str(root), part, sub)
            for name in sorted(os.listdir(d)) if os.path.isdir(d) else []:
                h.update(name.encode())
                with open(os.path.join(d, name), 'rb') as f:
                    h.update(f.read())
    return h.hexdigest()


class Case:
    """z: the arrays, meta: the json; frames(split) -> per-frame dicts of the reference's values"""

    def __init__(self):
        self.z = dict(np.load(NPZ))
        with open(META) as f:
            self.meta = json.load(f)

    def write_tree(self, root):
        split = kitti_tree.write_tree(root, seed=self.meta['tree']['seed'])
        assert split == self.meta['tree']['split']
        assert tree_digest(root) == self.meta['tree']['sha256'], \
            "the synthetic tree differs from the one the fixture was generated on"
        return split

    def frames(self, split):
        z, m = self.z, self.meta[split]
        out = []
        g0 = o0 = p0 = 0
        for k, idx in enumerate(m['frames']):
            f = {'idx': idx, 'image_shape': z[f'{split}_image_shape'][k],
                 'calib': {key: z[f'{split}_calib_{key}'][k] for key in ('P2', 'R0_rect', 'Tr_velo_to_cam')}}
            if split != 'test':
                ng, no, npts = int(z[f'{split}_num_gt'][k]), int(z[f'{split}_num_objects'][k]), int(z[f'{split}_point_counts'][k])
                f['annos'] = {key: z[f'{split}_{key}'][g0:g0 + ng] for key in PER_GT}
                f['annos']['name'] = np.array(m['names'][k])
                f['annos']['gt_boxes_lidar'] = z[f'{split}_gt_boxes_lidar'][o0:o0 + no]
                f['object_fragile'] = z[f'{split}_object_fragile'][o0:o0 + no]
                bits = np.unpackbits(z[f'{split}_fov_bits'])[p0:p0 + npts].astype(bool)
                frag = np.unpackbits(z[f'{split}_fov_fragile_bits'])[p0:p0 + npts].astype(bool)
                f['fov'], f['fov_fragile'], f['num_points'] = bits, frag, npts
                g0, o0, p0 = g0 + ng, o0 + no, p0 + npts
            out.append(f)
        return out

    def info_of(self, frame):
        """a reference-format info dict rebuilt from the fixture's numbers (for the device tests: the boxes are the
        reference's own, bit for bit)"""
        info = {'point_cloud': {'num_features': 4, 'lidar_idx': frame['idx']},
                'image': {'image_idx': frame['idx'], 'image_shape': frame['image_shape']}, 'calib': dict(frame['calib'])}
        if 'annos' in frame:
            info['annos'] = {k: v for k, v in frame['annos'].items()}
        return info

"""Point-anchored residual box coder of the point head.

Behaviour of /root/reference/pcdet/utils/box_coder_utils.py:144-222 (PointResidualCoder): a box is coded relative to
the POINT that votes for it — centre offset divided by the class's mean-size diagonal (xy) / height (z), log size
ratios, and the heading as (cos, sin).  The reference moves `mean_size` to the GPU in the constructor; here it
follows the device of the tensors it is used with.
"""
import numpy as np
import torch


class PointResidualCoder(object):
    def __init__(self, code_size=8, use_mean_size=True, **kwargs):
        super().__init__()
        self.code_size = code_size
        self.use_mean_size = use_mean_size
        if self.use_mean_size:
            self.mean_size = torch.from_numpy(np.array(kwargs['mean_size'])).float()
            assert self.mean_size.min() > 0

    def _anchor(self, classes, like, check=False):
        if self.mean_size.device != like.device:
            self.mean_size = self.mean_size.to(like.device)
        if check:   # (a host synchronisation: only where the classes come from data, i.e. target encoding)
            assert classes.max() <= self.mean_size.shape[0]
        size = self.mean_size[classes - 1]
        dxa, dya, dza = torch.split(size, 1, dim=-1)
        return dxa, dya, dza, torch.sqrt(dxa ** 2 + dya ** 2)

    def encode_torch(self, gt_boxes, points, gt_classes=None, check_classes=True):
        """gt_boxes (N, 7 + C), points (N, 3), gt_classes (N) in [1, num_classes] -> (N, 8 + C).
        As in the reference (:164) the sizes of `gt_boxes` are clamped IN PLACE to >= 1e-5.
        check_classes: the reference's range assert on the classes (:166), a device->host synchronisation; the point
        head's per-step target encoding passes False and checks the range on the device instead (class_range_ok)."""
        gt_boxes[:, 3:6] = torch.clamp_min(gt_boxes[:, 3:6], min=1e-5)
        xg, yg, zg, dxg, dyg, dzg, rg, *cgs = torch.split(gt_boxes, 1, dim=-1)
        xa, ya, za = torch.split(points, 1, dim=-1)
        if self.use_mean_size:
            dxa, dya, dza, diagonal = self._anchor(gt_classes, gt_boxes, check=check_classes)
            xt, yt, zt = (xg - xa) / diagonal, (yg - ya) / diagonal, (zg - za) / dza
            dxt, dyt, dzt = torch.log(dxg / dxa), torch.log(dyg / dya), torch.log(dzg / dza)
        else:
            xt, yt, zt = xg - xa, yg - ya, zg - za
            dxt, dyt, dzt = torch.log(dxg), torch.log(dyg), torch.log(dzg)
        return torch.cat([xt, yt, zt, dxt, dyt, dzt, torch.cos(rg), torch.sin(rg), *cgs], dim=-1)

    def class_range_ok(self, classes):
        """0-dim bool tensor on the device: every class id addresses a row of the mean-size table (no synchronisation)."""
        if not self.use_mean_size:
            return torch.ones((), dtype=torch.bool, device=classes.device)
        return classes.max() <= self.mean_size.shape[0]

    def decode_torch(self, box_encodings, points, pred_classes=None):
        """box_encodings (N, 8 + C) [x, y, z, dx, dy, dz, cos, sin, ...], points (N, 3) -> boxes (N, 7 + C).
        pred_classes in [1, num_classes] (an arg-max + 1 in the head: the reference's range assert, a device->host
        synchronisation per call, is kept for the encoder only, so decoding can be captured in a hipGraph)."""
        xt, yt, zt, dxt, dyt, dzt, cost, sint, *cts = torch.split(box_encodings, 1, dim=-1)
        xa, ya, za = torch.split(points, 1, dim=-1)
        if self.use_mean_size:
            dxa, dya, dza, diagonal = self._anchor(pred_classes, box_encodings)
            xg, yg, zg = xt * diagonal + xa, yt * diagonal + ya, zt * dza + za
            dxg, dyg, dzg = torch.exp(dxt) * dxa, torch.exp(dyt) * dya, torch.exp(dzt) * dza
        else:
            xg, yg, zg = xt + xa, yt + ya, zt + za
            dxg, dyg, dzg = torch.split(torch.exp(box_encodings[..., 3:6]), 1, dim=-1)
        rg = torch.atan2(sint, cost)
        return torch.cat([xg, yg, zg, dxg, dyg, dzg, rg, *cts], dim=-1)



class ResidualCoder(object):
    """Anchor-relative box code of the RoI heads; behaviour of /root/reference/pcdet/utils/box_coder_utils.py:5-77.

    code = [centre offset / (d, d, dz_a), log(size / size_a), heading - heading_a, extra columns - anchor's], d the
    anchor's BEV diagonal.  encode_angle_by_sincos codes the heading as the two differences (cos - cos_a, sin - sin_a)
    instead, which makes the code one column longer (code_size 8)."""

    def __init__(self, code_size=7, encode_angle_by_sincos=False, **kwargs):
        super().__init__()
        self.encode_angle_by_sincos = bool(encode_angle_by_sincos)
        self.code_size = code_size + (1 if self.encode_angle_by_sincos else 0)

    @staticmethod
    def _centre_scale(anchors):
        """(.., 3): what the three centre offsets are measured in"""
        diagonal = torch.sqrt(anchors[..., 3:4] ** 2 + anchors[..., 4:5] ** 2)
        return torch.cat([diagonal, diagonal, anchors[..., 5:6]], dim=-1)

    def encode_torch(self, boxes, anchors):
        """boxes (N, 7 + C), anchors (N, 7 + C) -> codes (N, code_size + C).  Like the reference (:22-23) this clamps the
        sizes of BOTH arguments to >= 1e-5 IN PLACE."""
        for t in (anchors, boxes):
            t[:, 3:6] = t[:, 3:6].clamp_min(1e-5)
        centre = (boxes[..., 0:3] - anchors[..., 0:3]) / self._centre_scale(anchors)
        size = torch.log(boxes[..., 3:6] / anchors[..., 3:6])
        rg, ra = boxes[..., 6:7], anchors[..., 6:7]
        if self.encode_angle_by_sincos:
            angle = torch.cat([torch.cos(rg) - torch.cos(ra), torch.sin(rg) - torch.sin(ra)], dim=-1)
        else:
            angle = rg - ra
        return torch.cat([centre, size, angle, boxes[..., 7:] - anchors[..., 7:]], dim=-1)

    def decode_torch(self, box_encodings, anchors):
        """codes (.., code_size + C), anchors (.., 7 + C) of the same leading shape -> boxes (.., 7 + C)."""
        centre = box_encodings[..., 0:3] * self._centre_scale(anchors) + anchors[..., 0:3]
        size = torch.exp(box_encodings[..., 3:6]) * anchors[..., 3:6]
        ra = anchors[..., 6:7]
        if self.encode_angle_by_sincos:
            heading = torch.atan2(box_encodings[..., 7:8] + torch.sin(ra), box_encodings[..., 6:7] + torch.cos(ra))
            extra = box_encodings[..., 8:]
        else:
            heading = box_encodings[..., 6:7] + ra
            extra = box_encodings[..., 7:]
        return torch.cat([centre, size, heading, extra + anchors[..., 7:]], dim=-1)

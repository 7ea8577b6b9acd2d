"""A seeded writer of a small synthetic KITTI directory (ImageSets, training/velodyne|calib|label_2|image_2, testing/...)
for the dataset front end's tests and fixtures.  Lidar-like clouds (a ground sheet, clutter, points on and around the
placed objects), a calibration perturbed per frame around KITTI's usual one, labels with DontCare / Van / truncated /
occluded rows, three image sizes, valid PNGs written with zlib only.

Deliberate cases (frame ids in CASES): an object without a single point, an object partly outside the image, two
overlapping boxes (their shared points belong to both), a frame with DontCare rows only and one with a Van only.

The tree must come out the same on every machine: the draws are numpy Generator uniforms / integers (a stable stream),
the arithmetic on them is + - * / only except one cos / sin per object, and every coordinate is then snapped to a
2^-10 m grid (exact in float32), which hides a last-bit difference of those two calls.
"""
import math
import os
import struct
import zlib

import numpy as np

CLASSES = ['Car', 'Pedestrian', 'Cyclist']
SIZES = {'Car': (3.9, 1.6, 1.56), 'Pedestrian': (0.8, 0.6, 1.73), 'Cyclist': (1.76, 0.6, 1.73), 'Van': (5.0, 2.0, 2.2)}   # l, w, h
IMAGE_SIZES = [(375, 1242), (370, 1224), (376, 1241)]
P2 = np.array([[721.5377, 0.0, 609.5593, 44.85728], [0.0, 721.5377, 172.854, 0.2163791], [0.0, 0.0, 1.0, 0.002745884]])
R0 = np.array([[0.9999239, 0.00983776, -0.007445048], [-0.009869795, 0.9999421, -0.004278459],
               [0.007402527, 0.004351614, 0.9999631]])
V2C = np.array([[0.007533745, -0.9999714, -0.000616602, -0.004069766], [0.01480249, 0.0007280733, -0.9998902, -0.07631618],
                [0.9998621, 0.00752379, 0.01480755, -0.2717806]])
CASES = {'zero_points': '000002', 'partly_outside': '000003', 'overlapping': '000004', 'dontcare_only': '000005',
         'van_only': '000006'}
GROUND_Z = -1.7


def write_png(path, height, width):
    """a valid 8-bit grey PNG of zeros: signature, IHDR, one IDAT, IEND"""
    def chunk(tag, data):
        return struct.pack('>I', len(data)) + tag + data + struct.pack('>I', zlib.crc32(tag + data) & 0xffffffff)
    raw = (b'\x00' + b'\x00' * width) * height
    with open(path, 'wb') as f:
        f.write(b'\x89PNG\r\n\x1a\n' + chunk(b'IHDR', struct.pack('>IIBBBBB', width, height, 8, 0, 0, 0, 0)) +
                chunk(b'IDAT', zlib.compress(raw, 9)) + chunk(b'IEND', b''))


def snap(a):
    return (np.round(np.asarray(a, dtype=np.float64) * 1024.0) / 1024.0).astype(np.float32)


def frame_calib(rng):
    p2, v2c = P2.copy(), V2C.copy()
    f = 1.0 + rng.uniform(-0.01, 0.01)
    p2[0, 0] *= f
    p2[1, 1] *= f
    p2[0, 2] += rng.uniform(-4, 4)
    p2[1, 2] += rng.uniform(-3, 3)
    v2c[:, 3] += rng.uniform(-0.01, 0.01, 3)
    return p2, R0.copy(), v2c


def write_calib(path, p2, r0, v2c):
    def line(name, m):
        return name + ': ' + ' '.join('%.12e' % v for v in m.reshape(-1)) + '\n'
    with open(path, 'w') as f:
        f.write(line('P0', p2) + line('P1', p2) + line('P2', p2) + line('P3', p2) + line('R0_rect', r0) +
                line('Tr_velo_to_cam', v2c) + line('Tr_imu_to_velo', v2c))


def project(p2, r0, v2c, pts):
    """lidar (n, 3) -> (rect (n, 3), image (n, 2)) in float64"""
    cam = pts @ v2c[:, :3].T + v2c[:, 3]
    rect = cam @ r0.T
    hom = rect @ p2[:, :3].T + p2[:, 3]
    return rect, hom[:, :2] / rect[:, 2:3]


def box_corners(x, y, z, l, w, h, heading):
    c, s = math.cos(heading), math.sin(heading)
    out = []
    for sx in (-0.5, 0.5):
        for sy in (-0.5, 0.5):
            for sz in (-0.5, 0.5):
                out.append([x + sx * l * c - sy * w * s, y + sx * l * s + sy * w * c, z + sz * h])
    return np.array(out)


def object_points(rng, n, x, y, z, l, w, h, heading):
    """n points within +-0.75 extents of the box (about a third of them inside it)"""
    c, s = math.cos(heading), math.sin(heading)
    u = rng.uniform(-0.75, 0.75, (n, 3))
    near = rng.uniform(size=n) < 0.3                   # a share drawn well inside, as returns from the object's faces
    u[near] *= 0.6
    lx, ly, lz = u[:, 0] * l, u[:, 1] * w, u[:, 2] * h
    return np.stack([x + lx * c - ly * s, y + lx * s + ly * c, z + lz, rng.uniform(0, 1, n)], 1)


def make_frame(rng, idx, n_points, calib, shape, labelled):
    """-> (points (N, 4) float32, label lines)"""
    p2, r0, v2c = calib
    H, W = shape
    n_ground = int(n_points * 0.7)
    ground = np.stack([rng.uniform(-12, 72, n_ground), rng.uniform(-32, 32, n_ground),
                       GROUND_Z + rng.uniform(-0.06, 0.06, n_ground), rng.uniform(0, 0.5, n_ground)], 1)
    n_clutter = n_points - n_ground
    clutter = np.stack([rng.uniform(0, 70, n_clutter), rng.uniform(-30, 30, n_clutter), rng.uniform(-1.6, 2.0, n_clutter),
                        rng.uniform(0, 1, n_clutter)], 1)
    parts = [ground, clutter]
    lines, care = [], []
    if not labelled:
        return snap(np.concatenate(parts)), lines
    # placed objects: (class, x, y, heading, points)
    objs = []
    if idx == CASES['dontcare_only']:
        pass
    elif idx == CASES['van_only']:
        objs.append(('Van', 22.0, 3.0, 0.3, 150))
    else:
        for k in range(int(rng.integers(3, 7))):
            name = ['Car', 'Car', 'Pedestrian', 'Cyclist', 'Van'][int(rng.integers(0, 5))]
            objs.append((name, 8.0 + 9.0 * k + rng.uniform(-2, 2), rng.uniform(-0.25, 0.25) * (8.0 + 9.0 * k),
                         rng.uniform(-3.1, 3.1), int(rng.integers(40, 220))))
        if idx == CASES['zero_points']:
            objs.append(('Car', 66.0, -4.0, 1.2, 0))
        if idx == CASES['partly_outside']:
            objs.append(('Car', 7.5, 6.4, 0.1, 200))
        if idx == CASES['overlapping']:
            objs.append(('Car', 30.0, 14.0, 0.4, 200))
            objs.append(('Pedestrian', 30.6, 14.5, 1.0, 120))
    for name, x, y, heading, n in objs:
        l, w, h = (v * rng.uniform(0.95, 1.05) for v in SIZES[name])
        z = GROUND_Z + h / 2
        if n:
            parts.append(object_points(rng, n, x, y, z, l, w, h, heading))
        else:                                                    # clear the ground around an object without points
            parts = [p[(p[:, 0] - x) ** 2 + (p[:, 1] - y) ** 2 > 16.0] for p in parts]
        corners = box_corners(x, y, z, l, w, h, heading)
        rect, img = project(p2, r0, v2c, corners)
        bottom, _ = project(p2, r0, v2c, np.array([[x, y, GROUND_Z]]))
        x1, y1 = max(img[:, 0].min(), 0.0), max(img[:, 1].min(), 0.0)
        x2, y2 = min(img[:, 0].max(), W - 1.0), min(img[:, 1].max(), H - 1.0)
        cut = 1.0 - max(x2 - x1, 0.0) * max(y2 - y1, 0.0) / max((np.ptp(img[:, 0]) * np.ptp(img[:, 1])), 1e-6)
        trunc = min(max(cut, 0.0), 1.0)
        occ = int(rng.integers(0, 4))
        ry = -heading - math.pi / 2
        ry = (ry + math.pi) % (2 * math.pi) - math.pi
        alpha = ry - math.atan2(bottom[0, 0], bottom[0, 2])
        lines.append('%s %.2f %d %.2f %.2f %.2f %.2f %.2f %.2f %.2f %.2f %.2f %.2f %.2f %.2f' % (
            name, trunc, occ, alpha, x1, y1, x2, y2, h, w, l, bottom[0, 0], bottom[0, 1], bottom[0, 2], ry))
    for _ in range(int(rng.integers(1, 3))):
        x1, y1 = rng.uniform(0, W - 120), rng.uniform(100, H - 60)
        care.append('DontCare -1 -1 -10 %.2f %.2f %.2f %.2f -1 -1 -1 -1000 -1000 -1000 -10' % (
            x1, y1, x1 + rng.uniform(20, 100), y1 + rng.uniform(10, 40)))
    pts = np.concatenate(parts)
    return snap(pts[rng.permutation(len(pts))]), lines + care


def write_tree(root, seed=0, n_train=8, n_val=8, n_test=3, n_points=3000):
    """-> {'train': [ids], 'val': [ids], 'test': [ids]}; ids '000000' ... as KITTI's, even ones train, odd ones val"""
    root = str(root)
    rng = np.random.default_rng(seed)
    ids = ['%06d' % k for k in range(n_train + n_val)]
    split = {'train': ids[0::2], 'val': ids[1::2], 'test': ['%06d' % k for k in range(n_test)]}
    os.makedirs(os.path.join(root, 'ImageSets'), exist_ok=True)
    for name, members in list(split.items()) + [('trainval', sorted(split['train'] + split['val']))]:
        with open(os.path.join(root, 'ImageSets', name + '.txt'), 'w') as f:
            f.write(''.join(i + '\n' for i in members))
    for part, members, labelled in (('training', ids, True), ('testing', split['test'], False)):
        for sub in ('velodyne', 'calib', 'label_2', 'image_2'):
            os.makedirs(os.path.join(root, part, sub), exist_ok=True)
        for k, idx in enumerate(members):
            shape = IMAGE_SIZES[k % len(IMAGE_SIZES)]
            calib = frame_calib(rng)
            n = int(n_points * rng.uniform(0.8, 1.2))
            pts, lines = make_frame(rng, idx, n, calib, shape, labelled)
            pts.tofile(os.path.join(root, part, 'velodyne', idx + '.bin'))
            write_calib(os.path.join(root, part, 'calib', idx + '.txt'), *calib)
            write_png(os.path.join(root, part, 'image_2', idx + '.png'), *shape)
            if labelled:
                with open(os.path.join(root, part, 'label_2', idx + '.txt'), 'w') as f:
                    f.write(''.join(line + '\n' for line in lines))
    return split

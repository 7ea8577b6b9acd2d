"""Numpy restatement of the device augmentor (pdm_ssd_amd/csrc/augment.hip): the draws
(scene keys, the keyed Feistel permutation, sample_with_fixed_number's pointer rule) and, per scene, gt_sampling's
collision select and point removal, the world transforms, limit_period and the range mask, in the fp32 operation
order the kernels pin.  Collisions use the CPU oracle's rotated-box overlap (oracle/iou3d_oracle.c, the arithmetic of
the reference's iou3d_cpu.cpp); everything else is numpy.
"""
import numpy as np

from oracle import cpu_oracle as o

OP_FLIP_X, OP_FLIP_Y, OP_ROT, OP_SCALE = 1, 2, 3, 4
F32 = np.float32
PI32, TWO_PI32 = F32(np.pi), F32(2 * np.pi)


def u32(x):
    return np.uint32(int(x) & 0xffffffff)


def fmix32(h):
    return int(o._fmix32(u32(h)))


def scene_key(seed, step, b, s):
    with np.errstate(over='ignore'):
        return fmix32(fmix32(int(seed) ^ (int(step) * 0x85EBCA6B & 0xffffffff)) ^ (b * 0x9E3779B1 & 0xffffffff) ^
                      (s * 0x7F4A7C15 & 0xffffffff))


def uniform(lo, hi, k):
    u = F32(k >> 8) * F32(2.0 ** -24)
    return F32(F32(lo) + F32(u * F32(F32(hi) - F32(lo))))


def perm_key(seed, group, epoch):
    return fmix32((fmix32(int(seed) ^ 0x5BD1E995 ^ (group * 0x9E3779B1 & 0xffffffff)) + (epoch * 0x85EBCA6B)) & 0xffffffff)


def perm(i, n, kp):
    """Position i of the keyed permutation of [0, n): 4-round balanced Feistel network, cycle-walked."""
    w = 1
    while (1 << (2 * w)) < n:
        w += 1
    mask = (1 << w) - 1
    x = i
    while True:
        L, R = x >> w, x & mask
        for r in range(4):
            f = fmix32(kp ^ ((R * 0x9E3779B1) & 0xffffffff) ^ (((r + 1) * 0x7F4A7C15) & 0xffffffff)) & mask
            L, R = R, L ^ f
        x = (L << w) | R
        if x < n:
            return x


def initial_state(group_len):
    return np.array([0] + sum([[-1, n] for n in group_len], []), dtype=np.int64)


def schedule(state, groups, gt_boxes, limit, seed):
    """groups: list of (class index, sample_num, entries, first database index).  -> (sampled (B, K) int32 database
    indices, -1 padded; the new state; the walk [(b, group, epoch, pointer, take)])."""
    state = np.array(state, dtype=np.int64).copy()
    B = gt_boxes.shape[0]
    K = sum(g[1] for g in groups)
    sampled = np.full((B, K), -1, dtype=np.int32)
    walk = []
    slot = 0
    for t, (cls, num0, n, first) in enumerate(groups):
        epoch, ptr = int(state[1 + 2 * t]), int(state[2 + 2 * t])
        for b in range(B):
            num = num0 - (int((gt_boxes[b, :, 7] == cls + 1).sum()) if limit else 0)
            if num <= 0:
                continue
            if ptr >= n:
                epoch, ptr = epoch + 1, 0
            take = min(num, n - ptr)
            kp = perm_key(seed, t, epoch)
            for j in range(take):
                sampled[b, slot + j] = first + perm(ptr + j, n, kp)
            walk.append((b, t, epoch, ptr, take))
            ptr += num
        state[1 + 2 * t], state[2 + 2 * t] = epoch, ptr
        slot += num0
    state[0] += 1
    return sampled, state, walk


def scene_params(seed, step, B, flip_axes, rot, scale):
    flip = np.zeros(B, np.int32)
    angle = np.zeros(B, np.float32)
    sc = np.ones(B, np.float32)
    for b in range(B):
        if flip_axes & 1:
            flip[b] |= scene_key(seed, step, b, 1) & 1
        if flip_axes & 2:
            flip[b] |= (scene_key(seed, step, b, 2) & 1) << 1
        if rot is not None:
            angle[b] = uniform(rot[0], rot[1], scene_key(seed, step, b, 3))
        if scale is not None:
            sc[b] = uniform(scale[0], scale[1], scene_key(seed, step, b, 4))
    return flip, angle, sc


def cos_sin(a):
    return F32(np.cos(np.float64(F32(a)))), F32(np.sin(np.float64(F32(a))))


def world(ops, flip, angle, scale, xyz, heading=None, dims=None):
    """xyz (n, 3) fp32 (and optionally heading (n,), dims (n, 3)) through the transform list, pinned fp32 order."""
    x, y, z = (np.array(xyz[:, k], dtype=F32) for k in range(3))
    h = None if heading is None else np.array(heading, dtype=F32)
    d = None if dims is None else np.array(dims, dtype=F32)
    c, s = cos_sin(angle)
    zero = F32(0.0)
    for op in ops:
        if op == OP_FLIP_X and flip & 1:
            y = -y
            if h is not None:
                h = -h
        elif op == OP_FLIP_Y and flip & 2:
            x = -x
            if h is not None:
                h = -(h + PI32)
        elif op == OP_ROT:
            nx = (x * c + y * (-s)) + z * zero
            ny = (x * s + y * c) + z * zero
            nz = (x * zero + y * zero) + z
            x, y, z = nx, ny, nz
            if h is not None:
                h = h + F32(angle)
        elif op == OP_SCALE:
            sc = F32(scale)
            x, y, z = x * sc, y * sc, z * sc
            if d is not None:
                d = d * sc
    return np.stack([x, y, z], 1).astype(F32), h, d


def limit_period(h):
    h = np.asarray(h, dtype=F32)
    return (h - np.floor(h / TWO_PI32 + F32(0.5)) * TWO_PI32).astype(F32)


def points_in_box_cpu(pts, box):
    """points_in_boxes_cpu's test (roiaware_pool3d.cpp:121-140): margin 1e-2, comparisons in double."""
    x, y, z = pts[:, 0].astype(F32), pts[:, 1].astype(F32), pts[:, 2].astype(F32)
    zin = ~(np.abs(z - F32(box[2])).astype(np.float64) > np.float64(F32(box[5])) / 2.0)
    c, s = cos_sin(-F32(box[6]))
    sx, sy = x - F32(box[0]), y - F32(box[1])
    lx = sx * c + sy * (-s)
    ly = sx * s + sy * c
    m = np.float64(F32(1e-2))
    return zin & (np.abs(lx).astype(np.float64) < np.float64(F32(box[3])) / 2.0 + m) & \
        (np.abs(ly).astype(np.float64) < np.float64(F32(box[4])) / 2.0 + m)


def apply_scene(points, gt, db, groups, sampled, flip, angle, scale, ops, pc_range, extra, remove_outside=True):
    """ONE scene.  points (N, C), gt (M, 8) with the class convention, db = dict(points, offsets, boxes) on the host,
    groups [(class index, sample_num, ...)], sampled (K,) database indices (-1 padded).
    -> (rows (R, C), boxes (n, 8), accepted (list of database indices))."""
    points = np.asarray(points, dtype=F32)
    present = gt[gt[:, 7] != 0]
    exist = [present[:, :7].astype(F32)]
    exist_cls = list(present[:, 7])
    accepted, acc_cls = [], []
    slot = 0
    for t, g in enumerate(groups):
        num = g[1]
        idx = [int(i) for i in sampled[slot:slot + num] if 0 <= i < len(db['boxes'])]
        slot += num
        if not idx:
            continue
        cand = db['boxes'][idx].astype(F32)
        ex = np.concatenate(exist, 0)
        valid = np.ones(len(idx), bool)
        if len(ex):
            valid &= ~(o.boxes_overlap_bev(cand, ex) != 0).any(1)
        ov = o.boxes_overlap_bev(cand, cand)
        np.fill_diagonal(ov, 0)
        valid &= ~(ov != 0).any(1)
        for k in np.nonzero(valid)[0]:
            accepted.append(idx[k])
            acc_cls.append(g[0] + 1)
        exist.append(cand[valid])
        exist_cls += [g[0] + 1] * int(valid.sum())
    # rows: object points shifted by their box centre, then the scene points outside every enlarged accepted box
    obj = []
    keep = np.ones(len(points), bool)
    for i in accepted:
        bx = db['boxes'][i].astype(F32)
        p = db['points'][db['offsets'][i]:db['offsets'][i + 1]].astype(F32).copy()
        p[:, :3] = p[:, :3] + bx[:3]
        obj.append(p)
        large = bx.copy()
        large[3:6] = large[3:6] + np.asarray(extra, F32)
        keep &= ~points_in_box_cpu(points, large)
    rows = np.concatenate(obj + [points[keep]], 0) if obj else points[keep]
    xyz, _, _ = world(ops, flip, angle, scale, rows[:, :3])
    rows = rows.copy()
    rows[:, :3] = xyz
    r = np.asarray(pc_range, F32)
    m = (rows[:, 0] >= r[0]) & (rows[:, 0] <= r[3]) & (rows[:, 1] >= r[1]) & (rows[:, 1] <= r[4])
    rows = rows[m]
    # boxes: targets then accepted
    ex = np.concatenate(exist, 0)
    cls = np.asarray(exist_cls, F32)
    tgt = cls > 0
    bx = ex[tgt].astype(F32).copy()
    xyz, h, d = world(ops, flip, angle, scale, bx[:, :3], bx[:, 6], bx[:, 3:6])
    bx[:, :3], bx[:, 3:6], bx[:, 6] = xyz, d, limit_period(h)
    if remove_outside:
        mb = ((bx[:, :3] >= r[:3]) & (bx[:, :3] <= r[3:])).all(1)
    else:
        mb = np.ones(len(bx), bool)
    boxes = np.concatenate([bx, cls[tgt][:, None]], 1)[mb].astype(F32)
    return rows.astype(F32), boxes, accepted

// Rotated-box geometry, one definition per function so that every operator evaluates it operation for operation:
//   box_overlap_bev / iou_bev / iou_normal   iou3d_nms.hip, post_process.hip (through nms.h), augment.hip
//   bev_radius / bev_circles_disjoint        the bounding-circle prefilter of those
//   box_cos_sin / box_reach2 / point_in_box_margin   the point-in-box test of augment.hip and kitti_data.hip
//   box_cos_sin_f / point_in_box3d / box_reach2_pool / roiaware_voxel   check_pt_in_box3d and the voxel of a point, shared by
//                                                      points_in_boxes (iou3d_nms.hip) and the RoI pooling of roi_pool.hip
// Boxes are 7 floats [x, y, z, dx, dy, dz, heading]; see iou3d_nms.hip for the geometry.
#pragma once
#include "common.h"

namespace pdm {

struct P2 { float x, y; };

__device__ __forceinline__ float cross2(P2 a, P2 b) { return a.x * b.y - a.y * b.x; }
__device__ __forceinline__ float cross3(P2 p1, P2 p2, P2 p0) { return (p1.x - p0.x) * (p2.y - p0.y) - (p2.x - p0.x) * (p1.y - p0.y); }
__device__ __forceinline__ float fmn(float a, float b) { return a > b ? b : a; }
__device__ __forceinline__ float fmx(float a, float b) { return a > b ? a : b; }

__device__ __forceinline__ bool rects_touch(P2 p1, P2 p2, P2 q1, P2 q2) {
    return fmn(p1.x, p2.x) <= fmx(q1.x, q2.x) && fmn(q1.x, q2.x) <= fmx(p1.x, p2.x) &&
           fmn(p1.y, p2.y) <= fmx(q1.y, q2.y) && fmn(q1.y, q2.y) <= fmx(p1.y, p2.y);
}

__device__ __forceinline__ bool inside_box(const float *box, P2 p) {
    const float margin = 1e-2f;
    const float c = cosf(-box[6]), s = sinf(-box[6]);
    const float rx = (p.x - box[0]) * c + (p.y - box[1]) * (-s);
    const float ry = (p.x - box[0]) * s + (p.y - box[1]) * c;
    return fabsf(rx) < box[3] / 2 + margin && fabsf(ry) < box[4] / 2 + margin;
}

__device__ __forceinline__ bool seg_intersection(P2 p1, P2 p0, P2 q1, P2 q0, P2 &ans) {
    if (!rects_touch(p0, p1, q0, q1)) return false;
    const float s1 = cross3(q0, p1, p0), s2 = cross3(p1, q1, p0), s3 = cross3(p0, q1, q0), s4 = cross3(q1, p1, q0);
    if (!(s1 * s2 > 0 && s3 * s4 > 0)) return false;
    const float s5 = cross3(q1, p1, p0);
    if (fabsf(s5 - s1) > 1e-8f) {
        ans.x = (s5 * q0.x - s1 * q1.x) / (s5 - s1);
        ans.y = (s5 * q0.y - s1 * q1.y) / (s5 - s1);
    } else {
        const float a0 = p0.y - p1.y, b0 = p1.x - p0.x, c0 = p0.x * p1.y - p1.x * p0.y;
        const float a1 = q0.y - q1.y, b1 = q1.x - q0.x, c1 = q0.x * q1.y - q1.x * q0.y;
        const float D = a0 * b1 - a1 * b0;
        ans.x = (b0 * c1 - b1 * c0) / D;
        ans.y = (a1 * c0 - a0 * c1) / D;
    }
    return true;
}

__device__ __forceinline__ void corners_of(const float *box, P2 *c) {
    const float hx = box[3] / 2, hy = box[4] / 2;
    const float x1 = box[0] - hx, y1 = box[1] - hy, x2 = box[0] + hx, y2 = box[1] + hy;
    const float ca = cosf(box[6]), sa = sinf(box[6]);
    const float rx[4] = {x1, x2, x2, x1}, ry[4] = {y1, y1, y2, y2};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float dx = rx[k] - box[0], dy = ry[k] - box[1];
        c[k].x = dx * ca + dy * (-sa) + box[0];
        c[k].y = dx * sa + dy * ca + box[1];
    }
    c[4] = c[0];
}

__device__ inline float box_overlap_bev(const float *a, const float *b) {
    P2 ca[5], cb[5], pts[24];
    corners_of(a, ca);
    corners_of(b, cb);
    int cnt = 0;
    P2 centre{0.f, 0.f};
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) {
            P2 x;
            if (seg_intersection(ca[i + 1], ca[i], cb[j + 1], cb[j], x)) {
                pts[cnt++] = x;
                centre.x += x.x; centre.y += x.y;
            }
        }
    for (int k = 0; k < 4; ++k) {
        if (inside_box(a, cb[k])) { centre.x += cb[k].x; centre.y += cb[k].y; pts[cnt++] = cb[k]; }
        if (inside_box(b, ca[k])) { centre.x += ca[k].x; centre.y += ca[k].y; pts[cnt++] = ca[k]; }
    }
    centre.x /= cnt; centre.y /= cnt;
    for (int j = 0; j < cnt - 1; ++j)
        for (int i = 0; i < cnt - j - 1; ++i)
            if (atan2f(pts[i].y - centre.y, pts[i].x - centre.x) > atan2f(pts[i + 1].y - centre.y, pts[i + 1].x - centre.x)) {
                const P2 t = pts[i]; pts[i] = pts[i + 1]; pts[i + 1] = t;
            }
    float area = 0;
    for (int k = 0; k < cnt - 1; ++k) {
        const P2 u{pts[k].x - pts[0].x, pts[k].y - pts[0].y}, v{pts[k + 1].x - pts[0].x, pts[k + 1].y - pts[0].y};
        area += cross2(u, v);
    }
    return fabsf(area) / 2.0f;
}

// radius of the BEV footprint's bounding circle
__device__ __forceinline__ float bev_radius(const float *box) { return 0.5f * sqrtf(box[3] * box[3] + box[4] * box[4]); }

// bounding-circle prefilter: true only if the two BEV footprints are certainly disjoint (then box_overlap_bev and
// iou_normal both return an overlap of exactly 0).  The margin covers inside_box's 1e-2 tolerance (a corner within
// 1e-2 of the other box lies within its circle radius + 0.0142) plus the rounding of corners and distances.
__device__ __forceinline__ bool bev_circles_disjoint(float ax, float ay, float ar, float bx, float by, float br) {
    const float dx = ax - bx, dy = ay - by;
    const float lim = ar + br + 0.05f + 1e-3f * (ar + br) + 2e-5f * (fabsf(ax) + fabsf(ay) + fabsf(bx) + fabsf(by));
    return dx * dx + dy * dy > lim * lim;   // NaN / inf anywhere: false, the pair is evaluated
}

__device__ __forceinline__ float iou_bev(const float *a, const float *b) {
    const float so = box_overlap_bev(a, b);
    return so / fmaxf(a[3] * a[4] + b[3] * b[4] - so, 1e-8f);
}

__device__ __forceinline__ float iou_normal(const float *a, const float *b) {
    const float left = fmaxf(a[0] - a[3] / 2, b[0] - b[3] / 2), right = fminf(a[0] + a[3] / 2, b[0] + b[3] / 2);
    const float top = fmaxf(a[1] - a[4] / 2, b[1] - b[4] / 2), bottom = fminf(a[1] + a[4] / 2, b[1] + b[4] / 2);
    const float w = fmaxf(right - left, 0.f), h = fmaxf(bottom - top, 0.f);
    const float inter = w * h;
    return inter / fmaxf(a[3] * a[4] + b[3] * b[4] - inter, 1e-8f);
}

// ---- point-in-box with points_in_boxes_cpu's margin (roiaware_pool3d.cpp:121-140), shared by the augmentation's point
// removal (augment.hip) and the ground-truth database builder (kitti_data.hip) so that both evaluate one and the same
// test.  c, s = box_cos_sin(-heading); dx, dy = fp32 (point - centre).  The local coordinates are fp32, one rounding at a
// time; the comparisons are in double.  The callers' translation units are built with -ffp-contract=off.
__device__ __forceinline__ void box_cos_sin(float a, float *c, float *s) {
    *c = (float)cos((double)a);
    *s = (float)sin((double)a);
}

// squared bounding-circle reject radius of the margin test: a point inside lies within
// sqrt((dx/2 + 0.01)^2 + (dy/2 + 0.01)^2) <= r + 0.0142 of the centre; the rest of the slack covers the rounding of the
// local coordinates and of this bound (NaN: never rejected)
__device__ __forceinline__ float box_reach2(const float *bx) {
    const float r = bev_radius(bx);
    const float lim = r * 1.001f + 0.02f + 4e-5f * (fabsf(bx[0]) + fabsf(bx[1]) + r + 1.f);
    return lim * lim;
}

__device__ __forceinline__ bool point_in_box_margin(float dx, float dy, float pz, const float *bx, float c, float s) {
    if ((double)fabsf(pz - bx[2]) > (double)bx[5] / 2.0) return false;
    const float lx = __fadd_rn(__fmul_rn(dx, c), __fmul_rn(dy, -s));
    const float ly = __fadd_rn(__fmul_rn(dx, s), __fmul_rn(dy, c));
    return (double)fabsf(lx) < (double)bx[3] / 2.0 + (double)1e-2f && (double)fabsf(ly) < (double)bx[4] / 2.0 + (double)1e-2f;
}

// ---- check_pt_in_box3d (roipoint_pool3d_kernel.cu:22-35, roiaware_pool3d_kernel.cu:23-36), one definition for
// points_in_boxes (iou3d_nms.hip) and the RoI point / RoI-aware pooling (roi_pool.hip): |z - cz| > dz / 2 rejects (compared
// in double), the local coordinates are fp32 from cosf(-rz) / sinf(-rz), one rounding per operation, then
// |local| < d / 2 + 1e-5 compared in double.  lx, ly are written only when the height test passes.
__device__ __forceinline__ void box_cos_sin_f(float rz, float *c, float *s) {
    *c = cosf(-rz);
    *s = sinf(-rz);
}

__device__ __forceinline__ bool point_in_box3d_cs(float x, float y, float z, const float *bx, float c, float s, float *lx, float *ly) {
    if ((double)fabsf(z - bx[2]) > (double)bx[5] / 2.0) return false;
    const float sx = x - bx[0], sy = y - bx[1];
    *lx = sx * c + sy * (-s);
    *ly = sx * s + sy * c;
    return fabs((double)*lx) < (double)bx[3] / 2.0 + (double)1e-5f && fabs((double)*ly) < (double)bx[4] / 2.0 + (double)1e-5f;
}

__device__ __forceinline__ bool point_in_box3d(float x, float y, float z, const float *bx, float *lx, float *ly) {
    if ((double)fabsf(z - bx[2]) > (double)bx[5] / 2.0) return false;   // before the trigonometry, as the reference
    float c, s;
    box_cos_sin_f(bx[6], &c, &s);
    return point_in_box3d_cs(x, y, z, bx, c, s, lx, ly);
}

// squared bounding-circle reject radius of point_in_box3d, compared with sx * sx + sy * sy of the fp32 shifts sx = x - cx,
// sy = y - cy.  A point that passes lies within sqrt((dx/2 + 1e-5)^2 + (dy/2 + 1e-5)^2) <= r + 1.42e-5 of the centre in
// the ROUNDED local frame; the local coordinates differ from an exact rotation of (sx, sy) by at most ~4 * 2^-24 relative
// (two products, a sum, cosf / sinf a few ulp off the unit circle) and sx * sx + sy * sy by 3 * 2^-24 relative: r * 1.001
// covers both a thousand times over, 1e-4 covers the margin seven times, the last term is box_reach2's (NaN: never rejected).
__device__ __forceinline__ float box_reach2_pool(const float *bx) {
    const float r = bev_radius(bx);
    const float lim = r * 1.001f + 1e-4f + 4e-5f * (fabsf(bx[0]) + fabsf(bx[1]) + r + 1.f);
    return lim * lim;
}

// voxel of an in-box point (roiaware_pool3d_kernel.cu:57-73), all fp32: res = d / out, idx = int((local + d / 2) / res)
// truncated toward zero, then the reference's clamp, which runs on `unsigned`: a negative index and an index >= out both
// land in out - 1.  The quotient is first limited to [-1, 256] (out <= 256), which changes none of that and keeps the
// conversion in range for a box of zero size (result unspecified there, but always a voxel of the grid).
__device__ __forceinline__ unsigned roiaware_axis(float local, float d, int out) {
    const float res = d / out;
    const float q = fminf(fmaxf((local + d / 2) / res, -1.f), 256.f);
    const unsigned i = (unsigned)(int)q;
    return i < (unsigned)(out - 1) ? i : (unsigned)(out - 1);
}

__device__ __forceinline__ int roiaware_voxel(float lx, float ly, float z, const float *bx, int ox, int oy, int oz) {
    const unsigned xi = roiaware_axis(lx, bx[3], ox), yi = roiaware_axis(ly, bx[4], oy), zi = roiaware_axis(z - bx[2], bx[5], oz);
    return (int)((xi * oy + yi) * oz + zi);
}

}  // namespace pdm

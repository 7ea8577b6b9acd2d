// The gaussian of one ground-truth box on a BEV heat map, shared by pdm_heatmap_targets (heatmap_loss.hip) and
// pdm_center_targets (center_head.hip), so that both draw the same bits by construction; pdm_tf_assign (tf_assign.hip) shares
// the window (hm_draw_window) under TransFusionHead's own rule for cell and radius (hm_draw_box_unclamped).  hm_draw_box:
//   cell   = trunc(clamp((x - x0) / vx / stride, 0, W - 0.5)), likewise y
//   r      = max(int(gaussian_radius(dx cells, dy cells, overlap)), min_radius), sigma = (2 r + 1) / 6
//   value  = exp(-(ddx^2 + ddy^2) / (2 sigma^2)) inside the (2 r + 1)^2 window, values under fp32 eps dropped,
//            max-merged with integer atomic max (non-negative floats order like their bit patterns)
#pragma once
#include "common.h"

namespace pdm {

// centernet_utils.gaussian_radius in torch's fp32 evaluation order: the python scalars (1 - o, 1 + o, -2 o, o - 1, 4 (4 o)) are
// formed in double and enter the tensor arithmetic as fp32 factors
__device__ __forceinline__ float hm_gaussian_radius(float height, float width, double o) {
    const float k1m = (float)(1.0 - o), k1p = (float)(1.0 + o), kn2 = (float)(-2.0 * o), km1 = (float)(o - 1.0), k16 = (float)(4.0 * (4.0 * o));
    const float b1 = height + width;
    const float c1 = __fmul_rn(__fmul_rn(__fmul_rn(width, height), k1m), __fdiv_rn(1.0f, k1p));   // (tensor / python scalar = tensor * (1 / scalar) in torch's kernel)
    const float r1 = __fmul_rn(__fadd_rn(b1, __fsqrt_rn(__fsub_rn(__fmul_rn(b1, b1), __fmul_rn(4.0f, c1)))), 0.5f);
    const float b2 = __fmul_rn(2.0f, height + width);
    const float c2 = __fmul_rn(__fmul_rn(k1m, width), height);
    const float r2 = __fmul_rn(__fadd_rn(b2, __fsqrt_rn(__fsub_rn(__fmul_rn(b2, b2), __fmul_rn(16.0f, c2)))), 0.5f);
    const float b3 = __fmul_rn(kn2, height + width);
    const float c3 = __fmul_rn(__fmul_rn(km1, width), height);
    const float r3 = __fmul_rn(__fadd_rn(b3, __fsqrt_rn(__fsub_rn(__fmul_rn(b3, b3), __fmul_rn(k16, c3)))), 0.5f);
    return fminf(fminf(r1, r2), r3);
}

struct HmGrid {
    int C, H, W;
    float x0, y0, vx, vy, stride;   // point-cloud range minimum, voxel size, feature-map stride
    double min_overlap;
    int min_radius, max_radius;     // the window is clipped at max_radius cells, sigma keeps the true radius
};

// the box's centre in cells, clamped as the head clamps it (division of a tensor by a python scalar is a multiplication
// by the scalar's fp32 reciprocal in torch's kernel: the same here, so that the integer cell and radius come out the same)
__device__ __forceinline__ void hm_center_cells(const HmGrid &a, float x, float y, float *cx, float *cy) {
    const float ivx = __fdiv_rn(1.0f, a.vx), ivy = __fdiv_rn(1.0f, a.vy), is = __fdiv_rn(1.0f, a.stride);
    *cx = fminf(fmaxf(__fmul_rn(__fmul_rn(x - a.x0, ivx), is), 0.0f), (float)a.W - 0.5f);
    *cy = fminf(fmaxf(__fmul_rn(__fmul_rn(y - a.y0, ivy), is), 0.0f), (float)a.H - 0.5f);
}

// the box's size in cells; false for a degenerate box (dx <= 0 or dy <= 0, NaN included)
__device__ __forceinline__ bool hm_size_cells(const HmGrid &a, float dx, float dy, float *dxc, float *dyc) {
    const float ivx = __fdiv_rn(1.0f, a.vx), ivy = __fdiv_rn(1.0f, a.vy), is = __fdiv_rn(1.0f, a.stride);
    *dxc = __fmul_rn(__fmul_rn(dx, ivx), is);
    *dyc = __fmul_rn(__fmul_rn(dy, ivy), is);
    return *dxc > 0.0f && *dyc > 0.0f;
}

// The (2 r + 1)^2 window of radius r around cell (ix, iy) on class plane c, max-merged; called by all NT threads of a
// workgroup with the same arguments.  Each cell's value depends on the cell alone, so the order in which the threads visit
// the window does not matter.
template <int NT>
__device__ __forceinline__ void hm_draw_window(const HmGrid &a, int ix, int iy, int r, int c, float *map) {
    const float rt = (float)r;
    const int rw = r < a.max_radius ? r : a.max_radius;
    const float sigma = __fmul_rn(__fadd_rn(__fmul_rn(2.0f, rt), 1.0f), __fdiv_rn(1.0f, 6.0f));
    const float den = __fmul_rn(__fmul_rn(2.0f, sigma), sigma);
    const int K = 2 * rw + 1;
    int *plane = reinterpret_cast<int *>(map + (size_t)c * a.H * a.W);
    for (int e = threadIdx.x; e < K * K; e += NT) {
        const int ddy = e / K - rw, ddx = e % K - rw;
        const int px = ix + ddx, py = iy + ddy;
        if (px < 0 || px >= a.W || py < 0 || py >= a.H) continue;
        const float v = expf(-__fdiv_rn((float)(ddx * ddx + ddy * ddy), den));
        if (v < 1.1920928955078125e-07f) continue;               // h[h < eps * h.max()] = 0 (the window's maximum is 1)
        atomicMax(plane + (size_t)py * a.W + px, __float_as_int(v));
    }
}

// Called by all NT threads of a workgroup with the same box: (x, y) centre, (dx, dy) size in metres, cls = class channel
// + 1 as a float (< 1 = padding); map = the sample's (C, H, W) planes.  Each cell's value depends on the cell alone, so
// the order in which the threads visit the window does not matter.
template <int NT>
__device__ __forceinline__ void hm_draw_box(const HmGrid &a, float x, float y, float dx, float dy, float cls, float *map) {
    float dxc, dyc, cx, cy;
    if (!hm_size_cells(a, dx, dy, &dxc, &dyc) || !(cls >= 1.0f)) return;   // padding / degenerate box (uniform over the workgroup)
    const int c = (int)cls - 1;
    if (c >= a.C) return;
    hm_center_cells(a, x, y, &cx, &cy);
    int r = (int)hm_gaussian_radius(dxc, dyc, a.min_overlap);     // (height, width) = (dx, dy) cells as the head passes them
    if (r < a.min_radius) r = a.min_radius;
    hm_draw_window<NT>(a, (int)cx, (int)cy, r, c, map);
}

// TransFusionHead's rule for the same gaussian (pdm_tf_assign, tf_assign.hip): the centre cell is the TRUNCATED, unclamped
// (x - x0) / vx / stride, and a box whose centre cell lies outside the map draws nothing; the radius takes (height, width) =
// (dy, dx) cells, as that head passes them.  Same calling convention as hm_draw_box.
template <int NT>
__device__ __forceinline__ void hm_draw_box_unclamped(const HmGrid &a, float x, float y, float dx, float dy, float cls, float *map) {
    float dxc, dyc;
    if (!hm_size_cells(a, dx, dy, &dxc, &dyc) || !(cls >= 1.0f)) return;
    const int c = (int)cls - 1;
    if (c >= a.C) return;
    const float ivx = __fdiv_rn(1.0f, a.vx), ivy = __fdiv_rn(1.0f, a.vy), is = __fdiv_rn(1.0f, a.stride);
    const float cx = __fmul_rn(__fmul_rn(x - a.x0, ivx), is), cy = __fmul_rn(__fmul_rn(y - a.y0, ivy), is);
    if (!(cx > -1.0f && cx < (float)a.W && cy > -1.0f && cy < (float)a.H)) return;       // trunc(c) in [0, n); NaN draws nothing
    int r = (int)fminf(hm_gaussian_radius(dyc, dxc, a.min_overlap), 1e9f);
    if (r < a.min_radius) r = a.min_radius;
    hm_draw_window<NT>(a, (int)cx, (int)cy, r, c, map);
}

}  // namespace pdm

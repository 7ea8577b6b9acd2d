// The geometry of Voxel R-CNN's RoI-grid pooling, shared by the eval kernel (roi_grid_pool.hip) and the training
// form's query (roi_grid_train.hip): the grid points of a tile of 16, their cells, and the walk over the voxel window with the
// ballot compaction of the hits into the first nsample.  One definition, so both form the same bits in the same fp32 operation
// order.  `A` is the kernel's argument structure; the functions read its fields
//     M, n, G, roi_stride, D, H, W, P, stride, vox[3], r0[3], rz, ry, rx, nsample, radius, rois, bits, gprefix, row_of_rank.
#pragma once
#include "sc_index.h"

namespace pdm {

constexpr int RGP_TILE = 16;        // grid points per wave tile: the MFMA's 16 columns
constexpr int RGP_MAXS = 32;        // nsample at most
constexpr int RGP_MAXG = 8;         // grid size at most
constexpr int RGP_MAXR = 4;         // window half-width at most: 9 x 9 x 9 cells

// floor(a / s) for s >= 1
__device__ __forceinline__ int floor_div(int a, int s) {
    const int q = a / s;
    return (a % s != 0 && a < 0) ? q - 1 : q;
}
// floor((g - r0) / voxel) as an int; far outside (and NaN) -> a cell no window reaches
__device__ __forceinline__ int rgp_cell0(float g, float r0, float voxel) {
    const float c = floorf(__fdiv_rn(__fsub_rn(g, r0), voxel));
    return (c > -1.0e9f && c < 1.0e9f) ? (int)c : -(1 << 30);
}

// what a kernel derives once from its arguments
struct RgpWalk {
    float r2, sx, sy, sz;           // radius^2 and the level's voxel size
    int wy, wx, window, mzyx, mx;   // window extents; w / d = (w m) >> 20 exactly for w < 1024, d <= 81
    int G, G3;
};
template <class A>
__device__ __forceinline__ RgpWalk rgp_walk_of(const A &a) {
    RgpWalk k;
    k.r2 = __fmul_rn(a.radius, a.radius);
    k.sx = __fmul_rn(a.vox[0], (float)a.stride); k.sy = __fmul_rn(a.vox[1], (float)a.stride); k.sz = __fmul_rn(a.vox[2], (float)a.stride);
    k.wy = 2 * a.ry + 1; k.wx = 2 * a.rx + 1; k.window = (2 * a.rz + 1) * k.wy * k.wx;
    k.mzyx = (1 << 20) / (k.wy * k.wx) + 1; k.mx = (1 << 20) / k.wx + 1;
    k.G = a.G; k.G3 = a.G * a.G * a.G;
    return k;
}

// grid point gi (0 <= gi < G^3, the lattice in nonzero()'s order: x index slowest, z fastest) of the RoI row `roi`
// (x, y, z, dx, dy, dz, heading, ...): (i + 0.5) / G size - size / 2 per axis, turned by the heading, plus the centre.  The one
// definition of the fp32 operation order, for the voxel pooling (below) and PV-RCNN's keypoint query (pv_rcnn.hip) alike.
__device__ __forceinline__ void rgp_grid_point(const float *roi, int G, int gi, float &gx, float &gy, float &gz) {
    const int ix = gi / (G * G), iy = (gi / G) % G, iz = gi % G;
    const float dxs = roi[3], dys = roi[4], dzs = roi[5], head = roi[6];
    const float lx = __fsub_rn(__fmul_rn(__fdiv_rn(__fadd_rn((float)ix, 0.5f), (float)G), dxs), __fdiv_rn(dxs, 2.0f));
    const float ly = __fsub_rn(__fmul_rn(__fdiv_rn(__fadd_rn((float)iy, 0.5f), (float)G), dys), __fdiv_rn(dys, 2.0f));
    const float lz = __fsub_rn(__fmul_rn(__fdiv_rn(__fadd_rn((float)iz, 0.5f), (float)G), dzs), __fdiv_rn(dzs, 2.0f));
    const float cs = cosf(head), sn = sinf(head);
    gx = __fadd_rn(__fsub_rn(__fmul_rn(lx, cs), __fmul_rn(ly, sn)), roi[0]);
    gy = __fadd_rn(__fadd_rn(__fmul_rn(lx, sn), __fmul_rn(ly, cs)), roi[1]);
    gz = __fadd_rn(lz, roi[2]);
}

// the tile's 16 grid points, one per lane (lanes 16 and up repeat them): the trigonometry runs once a point, not once a lane
template <class A>
__device__ __forceinline__ void rgp_tile_points(const A &a, const RgpWalk &k, long long tile, int lane, float &pgx, float &pgy, float &pgz,
                                                int &pcx, int &pcy, int &pcz, int &pb) {
    const int G3 = k.G3;
    const int m = (int)min(tile * RGP_TILE + (lane & 15), a.M - 1);
    const int r = m / G3, gi = m - r * G3;
    rgp_grid_point(a.rois + (size_t)r * a.roi_stride, k.G, gi, pgx, pgy, pgz);
    pb = r / a.n;
    pcx = floor_div(rgp_cell0(pgx, a.r0[0], a.vox[0]), a.stride);
    pcy = floor_div(rgp_cell0(pgy, a.r0[1], a.vox[1]), a.stride);
    pcz = floor_div(rgp_cell0(pgz, a.r0[2], a.vox[2]), a.stride);
}

// the first nsample in-radius voxels of the window around cell (cx, cy, cz) of sample b, in window order: 64 cells a step, the
// sphere tested first (it needs no memory), then the bit, the rank for set cells only, a ballot compaction, early exit at
// nsample.  hrow[slot] = the row, hd[3 slot ..] = centre - g as (x, y, z); returns the group's size (<= nsample).  All 64
// lanes call it; the caller puts a wave barrier between this and its reads of hrow / hd.
template <class A>
__device__ __forceinline__ int rgp_window_hits(const A &a, const RgpWalk &k, int lane, float gx, float gy, float gz, int cx, int cy, int cz, int b,
                                               int *hrow, float *hd) {
    const int wy = k.wy, wx = k.wx, window = k.window;
    int cnt = 0;
    for (int base = 0; base < window && cnt < a.nsample; base += 64) {
        const int w = base + lane;
        bool hit = false;
        int row = -1;
        float ddx = 0.f, ddy = 0.f, ddz = 0.f;
        if (w < window) {
            const int wz = (w * k.mzyx) >> 20, rem = w - wz * (wy * wx), wyy = (rem * k.mx) >> 20;
            const int z = cz + wz - a.rz, y = cy + wyy - a.ry, x = cx + (rem - wyy * wx) - a.rx;
            if (z >= 0 && z < a.D && y >= 0 && y < a.H && x >= 0 && x < a.W) {
                // the sphere first: it needs no memory, and most cells of a window fail it
                ddx = __fsub_rn(__fadd_rn(__fmul_rn(__fadd_rn((float)x, 0.5f), k.sx), a.r0[0]), gx);
                ddy = __fsub_rn(__fadd_rn(__fmul_rn(__fadd_rn((float)y, 0.5f), k.sy), a.r0[1]), gy);
                ddz = __fsub_rn(__fadd_rn(__fmul_rn(__fadd_rn((float)z, 0.5f), k.sz), a.r0[2]), gz);
                if (!(sqdist(ddx, ddy, ddz) > k.r2)) {
                    const long long key = rb_key(b, z, y, x, a.D, a.H, a.W);
                    if (sc_test(a.bits, key)) {
                        row = a.row_of_rank[sc_rank(a.bits, a.gprefix, key)];
                        hit = row >= 0 && row < a.P;
                    }
                }
            }
        }
        const unsigned long long mask = __ballot(hit);
        if (mask == 0) continue;
        const int slot = cnt + lanes_below(mask, lane);
        if (hit && slot < a.nsample) {
            hrow[slot] = row;
            hd[slot * 3] = ddx; hd[slot * 3 + 1] = ddy; hd[slot * 3 + 2] = ddz;
        }
        cnt += __popcll(mask);
    }
    return min(cnt, a.nsample);
}

}  // namespace pdm

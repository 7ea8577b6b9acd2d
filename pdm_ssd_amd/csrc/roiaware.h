// RoI-aware pooling's decisions, owned once so that pdm_roiaware_pool3d_forward (roi_pool.hip) and the batched sparse form
// pdm_roiaware_pool_sparse (roiaware_sparse.hip) make them identically by construction:
//   roiaware_cell_of       the in-box test (bounding-circle reject, point_in_box3d_cs) and the cell of a point
//   roiaware_append_block  the ordered append of one block of RA_NT tested points to their cells' lists by the first wave: a
//                          list takes its cell's points in ascending index order; the caller's `put` applies the cap
//   roiaware_list_max      strict > from -inf over a list: first index wins ties, NaN and -inf never win
//   roiaware_list_avg      the sum in list order, divided once by float(count)
// Built with -ffp-contract=off: one rounding per operation.
#pragma once
#include "box_geometry.h"

namespace pdm {

constexpr int RA_NT = 256;   // threads of a pooling workgroup, one workgroup per box

// the cell (x * oy + y) * oz + z of point p in the box, or -1 outside it
__device__ __forceinline__ int roiaware_cell_of(const float *__restrict__ pts, size_t p, const float *bx, float c, float s, float reach2,
                                                int ox, int oy, int oz) {
    const float x = pts[p * 3], y = pts[p * 3 + 1], z = pts[p * 3 + 2];
    const float sx = x - bx[0], sy = y - bx[1];
    float lx, ly;
    if (!(sx * sx + sy * sy > reach2) && point_in_box3d_cs(x, y, z, bx, c, s, &lx, &ly)) return roiaware_voxel(lx, ly, z, bx, ox, oy, oz);
    return -1;
}

// s_vox[0 .. RA_NT): the cell of point p0 + t, or -1 (complete and visible on entry).  Called by the FIRST WAVE only, all 64
// lanes.  cnt[v]: points appended to cell v so far (LDS or global; lane 0 alone reads and advances every counter, whichever
// lane leads the cell, so all accesses to a counter are one thread's, in program order).  put(cell, slot, point) is called
// once per hit with slot = its rank in the cell, in ascending point order.
template <class Put>
__device__ __forceinline__ void roiaware_append_block(const int *s_vox, int p0, int *cnt, Put put) {
    const int lane = threadIdx.x & 63;
    for (int j = 0; j < RA_NT / 64; ++j) {
        const int vv = s_vox[j * 64 + lane];
        unsigned long long todo = __ballot(vv >= 0);
        while (todo) {
            const int leader = __ffsll((long long)todo) - 1;
            const int lv = __shfl(vv, leader, 64);
            const unsigned long long same = __ballot(vv == lv);
            int base = 0;
            if (lane == 0) {
                base = cnt[lv];
                cnt[lv] = base + __popcll(same);
            }
            base = __shfl(base, 0, 64);
            if (vv == lv) put(lv, base + lanes_below(same, lane), p0 + j * 64 + lane);
            todo &= ~same;
        }
    }
}

// l[0 .. n): point rows; feats rows of C floats.  *arg = the winner or -1 (then the returned value is not a pooled value)
__device__ __forceinline__ float roiaware_list_max(const int *l, int n, const float *__restrict__ feats, int C, unsigned ch, int *arg) {
    float best = -INFINITY;
    int a = -1;
    for (int q = 0; q < n; ++q) {
        const int idx = l[q];
        const float f = feats[(size_t)idx * C + ch];
        if (f > best) { best = f; a = idx; }
    }
    *arg = a;
    return best;
}

// n >= 1
__device__ __forceinline__ float roiaware_list_avg(const int *l, int n, const float *__restrict__ feats, int C, unsigned ch) {
    float sum = 0.f;
    for (int q = 0; q < n; ++q) sum += feats[(size_t)l[q] * C + ch];
    return sum / (float)n;
}

}  // namespace pdm

// The two device steps of NMS over boxes in score order, shared by pdm_nms (iou3d_nms.hip) and the batched
// post-processing (post_process.hip) so that both keep the same boxes by construction: the 64 x 64 tile of the
// suppression mask and the one-wave walk over the mask with the `removed` set in registers.
#pragma once
#include "box_geometry.h"

namespace pdm {

// One workgroup of 64 threads, tile (row_start, col_start) with col_start >= row_start, of n boxes: thread t returns the
// mask word of box cur = 64 row_start + t: bit j set iff box 64 col_start + j comes after cur and overlaps it above the
// threshold (strict).  Threads with cur >= n return 0 and own no word.  prefilter (valid for thresh >= 0 only): a pair
// whose BEV bounding circles are disjoint has overlap 0, hence IoU 0, and is not evaluated.
__device__ __forceinline__ unsigned long long nms_mask_tile(int n, const float *__restrict__ boxes, int row_start,
                                                            int col_start, float thresh, bool normal, bool prefilter) {
    __shared__ float col[64 * 7];
    __shared__ float crad[64];
    const int row_size = min(n - row_start * 64, 64), col_size = min(n - col_start * 64, 64);
    for (int e = threadIdx.x; e < col_size * 7; e += 64) col[e] = boxes[(size_t)col_start * 64 * 7 + e];
    __syncthreads();
    if (prefilter) {
        if ((int)threadIdx.x < col_size) crad[threadIdx.x] = bev_radius(col + threadIdx.x * 7);
        __syncthreads();
    }
    if ((int)threadIdx.x >= row_size) return 0ull;
    float me[7];
#pragma unroll
    for (int f = 0; f < 7; ++f) me[f] = boxes[(size_t)(row_start * 64 + threadIdx.x) * 7 + f];
    const float mr = bev_radius(me);
    unsigned long long t = 0;
    const int start = row_start == col_start ? threadIdx.x + 1 : 0;   // only later boxes can be suppressed by this one
    for (int i = start; i < col_size; ++i) {
        const float *o = col + i * 7;
        if (prefilter && bev_circles_disjoint(me[0], me[1], mr, o[0], o[1], crad[i])) continue;
        const float v = normal ? iou_normal(me, o) : iou_bev(me, o);
        if (v > thresh) t |= 1ull << i;
    }
    return t;
}

// One wave walks n <= 16384 boxes in score order: lane l owns the `removed` words of 64-box blocks l, l + 64, ...;
// box i is kept unless an earlier kept box suppressed it, keep(k, i) records the k-th kept box (lane 0 calls it), the
// walk ends after `limit` keeps.  mask rows are `stride` words apart.  Returns the number kept.
template <class Keep>
__device__ __forceinline__ int nms_walk(int n, int limit, const unsigned long long *__restrict__ mask, int stride, Keep keep) {
    constexpr int WPL = 4;   // words per lane: up to 64 * 4 * 64 = 16384 boxes
    const int lane = threadIdx.x, ncb = (n + 63) / 64;
    unsigned long long remv[WPL] = {0ull, 0ull, 0ull, 0ull};
    int kept = 0;
    for (int i = 0; i < n && kept < limit; ++i) {
        const int nblock = i >> 6, inblock = i & 63;
        const int owner = nblock & 63, slot = nblock >> 6;
        const unsigned long long w = slot == 0 ? remv[0] : slot == 1 ? remv[1] : slot == 2 ? remv[2] : remv[3];
        const unsigned lo = __builtin_amdgcn_readlane((int)(unsigned)w, owner);
        const unsigned hi = __builtin_amdgcn_readlane((int)(unsigned)(w >> 32), owner);
        const unsigned long long word = ((unsigned long long)hi << 32) | lo;
        if ((word >> inblock) & 1ull) continue;   // wave-uniform
        if (lane == 0) keep(kept, i);
        ++kept;
        const unsigned long long *row = mask + (size_t)i * stride;
#pragma unroll
        for (int s = 0; s < WPL; ++s) {
            const int cb = s * 64 + lane;
            if (cb < ncb && cb >= nblock) remv[s] |= row[cb];
        }
    }
    return kept;
}

}  // namespace pdm

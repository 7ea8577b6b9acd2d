// The per-point pillar features and the single PFN layer of eval mode, shared by pillar.hip (dynamic pillars: the rows of a
// pillar come from its CSR segment) and hard_voxel.hip (hard voxels: the rows come from the voxel's T slots).
#pragma once
#include "common.h"

namespace pdm {

constexpr int PL_MAXF = 16;                // input columns of the fused PFN layer (the reference's is 10 or 11 wide)

struct PlFeat {
    int C1, abs_xyz, with_dist, F;
    float vx, vy, xoff, yoff, zoff;
    float vz;                              // read only where the cell's z index takes part (ZC below)
};

// The derived columns of one kept row, after its raw ones (points[:, 1:] or points[:, 4:]): f_cluster = xyz - pillar mean,
// f_center = xyz - cell centre as the reference orders it, x - (float(cx) * vx + x_offset) with the product and the sum
// rounded separately, and |xyz| = sqrt(fma(z, z, fma(y, y, x * x))), what torch.norm's CPU kernel rounds to (0 without it).
// ZC: the z centre is float(cz) * vz + z_offset (the hard-voxel PillarVFE); without it z_offset alone (a pillar grid's cz = 0).
template <bool ZC = false>
__device__ __forceinline__ void pl_derived(const PlFeat &a, const float *__restrict__ p, const float *__restrict__ mean,
                                           const int *__restrict__ vc, float d[7]) {
    const float x = p[1], y = p[2], z = p[3];
    d[0] = __fsub_rn(x, mean[0]);
    d[1] = __fsub_rn(y, mean[1]);
    d[2] = __fsub_rn(z, mean[2]);
    d[3] = __fsub_rn(x, __fadd_rn(__fmul_rn((float)vc[3], a.vx), a.xoff));
    d[4] = __fsub_rn(y, __fadd_rn(__fmul_rn((float)vc[2], a.vy), a.yoff));
    d[5] = __fsub_rn(z, ZC ? __fadd_rn(__fmul_rn((float)vc[1], a.vz), a.zoff) : a.zoff);
    d[6] = a.with_dist ? sqrtf(sqdist(x, y, z)) : 0.0f;      // sqrtf is correctly rounded here; __fsqrt_rn is the 1-ulp native one
}

// one output channel of the PFN layer: its weights in registers under static indices, the raw columns' and the seven derived
// columns' (0 for an absent |xyz|), and the folded BatchNorm (or 1 and the bias)
struct PlChannel {
    float w_raw[PL_MAXF - 6], w_der[7], sc, sh;
};
__device__ __forceinline__ void pl_channel_load(const PlFeat &a, int k, const float *__restrict__ weight, const float *__restrict__ scale,
                                                const float *__restrict__ shift, PlChannel &w) {
    const int first = a.abs_xyz ? 1 : 4, nraw = a.C1 - first;
#pragma unroll
    for (int c = 0; c < PL_MAXF - 6; ++c) w.w_raw[c] = c < nraw ? weight[(size_t)k * a.F + c] : 0.0f;
#pragma unroll
    for (int j = 0; j < 7; ++j) w.w_der[j] = (j < 6 || a.with_dist) ? weight[(size_t)k * a.F + nraw + j] : 0.0f;
    w.sc = scale[k];
    w.sh = shift[k];
}
// relu((features of the row . w) * scale + shift): one fma chain over the columns in order
template <bool ZC = false>
__device__ __forceinline__ float pl_channel_row(const PlFeat &a, const PlChannel &w, const float *__restrict__ row,
                                                const float *__restrict__ mean, const int *__restrict__ vc) {
    const int first = a.abs_xyz ? 1 : 4, nraw = a.C1 - first;
    float d[7];
    pl_derived<ZC>(a, row, mean, vc, d);
    float acc = 0.0f;
#pragma unroll
    for (int c = 0; c < PL_MAXF - 6; ++c)
        if (c < nraw) acc = __fmaf_rn(row[first + c], w.w_raw[c], acc);
#pragma unroll
    for (int j = 0; j < 7; ++j) acc = __fmaf_rn(d[j], w.w_der[j], acc);
    return fmaxf(__fmaf_rn(acc, w.sc, w.sh), 0.0f);
}

static int pl_feat_args(const char *who, PlFeat *a, int C1, int abs_xyz, int with_dist, float vx, float vy, float xoff, float yoff, float zoff,
                        float vz = 0.0f) {
    PDM_REQUIRE(C1 >= 4, PDM_E_BADARG, "%s: rows are (batch_idx, x, y, z, ...)", who);
    *a = PlFeat{C1, abs_xyz != 0, with_dist != 0, (abs_xyz ? C1 - 1 : C1 - 4) + 6 + (with_dist ? 1 : 0), vx, vy, xoff, yoff, zoff, vz};
    return 0;
}

}  // namespace pdm

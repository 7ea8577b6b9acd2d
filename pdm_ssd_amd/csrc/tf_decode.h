// The box of one TransFusion query from the prediction head's maps, shared by pdm_tf_decode (transfusion.hip) and
// pdm_tf_assign (tf_assign.hip), so that the boxes the assigner matches are bit for bit the boxes the decode returns:
//   x = (center_x * stride) * vx + x0 (each step one fp32 rounding), y likewise, z = height, sizes exp(dim),
//   angle atan2(rot[0], rot[1]) (rot = [sin, cos]), velocity as it is (zero without the map)
#pragma once
#include "common.h"

namespace pdm {

struct TfBoxMaps {
    int P, E;                                            // queries per sample; 2 with a velocity map, else 0
    const float *center, *height, *dim, *rot, *vel;      // (B, c, P) each, contiguous
    float x0, y0, vx, vy, stride;
};

__device__ __forceinline__ void tf_decode_box(const TfBoxMaps &m, int b, int p, float *box /* 9 */) {
    const int P = m.P;
    const float *ctr = m.center + (size_t)b * 2 * P + p, *dm = m.dim + (size_t)b * 3 * P + p, *rt = m.rot + (size_t)b * 2 * P + p;
    box[0] = __fadd_rn(__fmul_rn(__fmul_rn(ctr[0], m.stride), m.vx), m.x0);
    box[1] = __fadd_rn(__fmul_rn(__fmul_rn(ctr[P], m.stride), m.vy), m.y0);
    box[2] = m.height[(size_t)b * P + p];
    box[3] = expf(dm[0]); box[4] = expf(dm[P]); box[5] = expf(dm[2 * P]);
    box[6] = atan2f(rt[0], rt[P]);                            // [sin, cos]
    box[7] = box[8] = 0.0f;
    if (m.E == 2) { box[7] = m.vel[(size_t)b * 2 * P + p]; box[8] = m.vel[(size_t)b * 2 * P + P + p]; }
}

}  // namespace pdm

// The last launch of the two "first shared FC without its dense operand" operators (sparse_fc.hip, bev_roi_crop.hip):
// out = epilogue(partial[0] + partial[1] + ...), the partials added in ascending order, epilogue(v) = relu(v scale + shift) as
// one multiply and one add.
#pragma once
#include "common.h"

namespace pdm {

constexpr int FCR_NT = 256;

static __global__ __launch_bounds__(FCR_NT) void fc_reduce_kernel(int R, int Cout, int nchunk, const float *__restrict__ partial,
                                                                 const float *__restrict__ scale, const float *__restrict__ shift, int relu,
                                                                 float *__restrict__ out) {
    const size_t n = (size_t)R * Cout, e = (size_t)blockIdx.x * FCR_NT + threadIdx.x;
    if (e >= n) return;
    float v = 0.f;
    for (int k = 0; k < nchunk; ++k) v += partial[(size_t)k * n + e];
    if (scale) v = v * scale[e % Cout] + shift[e % Cout];
    if (relu) v = v < 0.0f ? 0.0f : v;      // a NaN stays, as torch's ReLU keeps it
    out[e] = v;
}

}  // namespace pdm

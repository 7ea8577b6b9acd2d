// The last launch of the two "first shared FC without its dense operand" operators (sparse_fc.hip, bev_roi_crop.hip):
// out = epilogue(partial[0] + partial[1] + ...), the partials added in ascending order, epilogue(v) = relu(v scale + shift) as
// one multiply and one add; and the split of the contraction into the chunks that make those partials.
#pragma once
#include <algorithm>

#include "common.h"

namespace pdm {

constexpr int FCR_NT = 256;
constexpr int FCR_TARGET_WGS = 1024;    // workgroups the main kernel's grid aims at

// `units` of the contraction (cells, LDS stages) split into chunks so that other_wgs x nchunk workgroups reach the target;
// a function of the sizes alone, so two runs add the same partials in the same order
struct SplitK {
    int chunk, nchunk;      // units a chunk, chunks
};
static inline SplitK split_k_plan(int units, long long other_wgs) {
    const int want = std::min(units, std::max(1, divup(FCR_TARGET_WGS, other_wgs)));
    SplitK p;
    p.chunk = divup(units, want);
    p.nchunk = divup(units, p.chunk);
    return p;
}

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

// What the fused loss operators share (head_loss.hip, heatmap_loss.hip, roi_targets.hip, center_head.hip, anchor_head.hip;
// the flat loader also in interpolate.hip, the sigmoid in bev_head.hip): strided fp32 / bf16 map reads, the elementwise loss
// terms, the residual box code, and the two fixed-order sums every loss ends in.  One definition each: operators that must
// round alike run the same code.  Nothing here chooses a reduction order for its caller: the orders are spelled out below.
#pragma once
#include "bf16.h"
#include "common.h"

namespace pdm {

// ---- maps ------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float load_f32_or_bf16(const void *p, long long i, int bf16) {
    return bf16 ? bf16_to_f32(static_cast<const unsigned short *>(p)[i]) : static_cast<const float *>(p)[i];
}

// a (B, C, H, W) map as it leaves a convolution: fp32 or bf16, any element strides.  A single (B, H, W) plane is the same
// thing with sc = 0, read at c = 0.
struct MapRef {
    const void *p;
    int bf16;
    long long sb, sc, sh, sw;
};

__device__ __forceinline__ long long map_offset(const MapRef &m, long long b, long long c, long long y, long long x) {
    return b * m.sb + c * m.sc + y * m.sh + x * m.sw;
}

__device__ __forceinline__ float map_load(const MapRef &m, long long b, long long c, long long y, long long x) {
    return load_f32_or_bf16(m.p, map_offset(m, b, c, y, x), m.bf16);
}

// host: entry k of the (pointer, flag, 4 strides) tables an entry point receives is map_ref(maps[k], bf16[k], strides + 4 * k)
static inline MapRef map_ref(const void *p, int bf16, const long long *strides) {
    return MapRef{p, bf16, strides[0], strides[1], strides[2], strides[3]};
}

// ---- elementwise terms -------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float sigmoid_rn(float x) { return __fdiv_rn(1.0f, 1.0f + expf(-x)); }

// binary_cross_entropy_with_logits
__device__ __forceinline__ float bce_with_logits(float x, float t) { return fmaxf(x, 0.0f) - x * t + log1pf(expf(-fabsf(x))); }

// smooth-L1 of the residual r and its derivative; beta < 1e-5 is plain L1 (WeightedSmoothL1Loss)
__device__ __forceinline__ void smooth_l1(float r, float beta, float *loss, float *dloss) {
    const float mag = fabsf(r);
    if (beta < 1e-5f) { *loss = mag; *dloss = r > 0.0f ? 1.0f : r < 0.0f ? -1.0f : 0.0f; }
    else if (mag < beta) { *loss = mag * mag * (0.5f / beta); *dloss = r / beta; }
    else { *loss = mag - 0.5f * beta; *dloss = r > 0.0f ? 1.0f : -1.0f; }
}

// The residual code of box g = [x y z dx dy dz ..] against an anchor at `centre` with extents (dxa, dya, dza): t[0..5].  The
// caller clamps the anchor's extents where its coder does and passes diag = sqrt(dxa^2 + dya^2) in ITS square root (sqrtf is
// the correctly rounded one, __fsqrt_rn the native one: they differ in the last bit); heading columns stay with the caller.
__device__ __forceinline__ void residual_encode(const float *g, const float *centre, float dxa, float dya, float dza, float diag, float *t) {
    const float dxg = fmaxf(g[3], 1e-5f), dyg = fmaxf(g[4], 1e-5f), dzg = fmaxf(g[5], 1e-5f);
    t[0] = __fdiv_rn(__fsub_rn(g[0], centre[0]), diag);
    t[1] = __fdiv_rn(__fsub_rn(g[1], centre[1]), diag);
    t[2] = __fdiv_rn(__fsub_rn(g[2], centre[2]), dza);
    t[3] = logf(__fdiv_rn(dxg, dxa));
    t[4] = logf(__fdiv_rn(dyg, dya));
    t[5] = logf(__fdiv_rn(dzg, dza));
}

// ---- sums in a fixed order -----------------------------------------------------------------------------------------------------
// N accumulators per thread summed over a workgroup of NT threads: a butterfly over each wave, lane 0 of each wave to LDS, a
// barrier, then total(j) adds the waves' values of accumulator j.  The order over the waves is part of each result's bits
// and is chosen at compile time: in index order from zero, ((0 + w0) + w1) + ..., or PAIRWISE, (w0 + w1) + (w2 + w3).
template <int NT, int N, typename T, bool PAIRWISE = false>
struct BlockSum {
    static_assert(NT % 64 == 0 && (!PAIRWISE || NT == 256), "whole waves; the pairwise order is written for four of them");
    T w[N][NT / 64];

    // every thread of the workgroup calls it; total() is valid in every thread on return
    __device__ __forceinline__ void reduce(const T (&v)[N]) {
#pragma unroll
        for (int j = 0; j < N; ++j) {
            T s = v[j];
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) s += __shfl_xor(s, off, 64);
            if ((threadIdx.x & 63) == 0) w[j][threadIdx.x >> 6] = s;
        }
        __syncthreads();
    }

    __device__ __forceinline__ T total(int j) const {
        if (PAIRWISE) return (w[j][0] + w[j][1]) + (w[j][2] + w[j][3]);
        T s = T(0);
        for (int k = 0; k < NT / 64; ++k) s += w[j][k];
        return s;
    }
};

// `count` rows of N block partials (floats or doubles) folded by ONE workgroup of NT threads in double: thread t adds rows
// t, t + NT, ... in order, then an LDS halving tree over the threads.  total(j) is valid in every thread on return.
template <int NT, int N>
struct FoldSum {
    double v[N][NT];

    template <typename P>
    __device__ __forceinline__ void fold(const P *__restrict__ partials, int count) {
        const int tid = threadIdx.x;
        double acc[N];
#pragma unroll
        for (int j = 0; j < N; ++j) acc[j] = 0.0;
        for (int k = tid; k < count; k += NT)
#pragma unroll
            for (int j = 0; j < N; ++j) acc[j] += partials[(size_t)k * N + j];
#pragma unroll
        for (int j = 0; j < N; ++j) v[j][tid] = acc[j];
        __syncthreads();
        for (int half = NT / 2; half >= 1; half >>= 1) {
            if (tid < half)
#pragma unroll
                for (int j = 0; j < N; ++j) v[j][tid] += v[j][tid + half];
            __syncthreads();
        }
    }

    __device__ __forceinline__ double total(int j) const { return v[j][0]; }
};

}  // namespace pdm

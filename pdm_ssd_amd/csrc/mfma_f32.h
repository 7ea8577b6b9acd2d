// The leaf pieces every fp32 mfma_f32_16x16x4f32 kernel here is made of: the float x 4 vector, the four-step K = 16 product,
// the fragment addresses, the guarded four-channel row load and store, and the four-lane epilogues.  Nothing in this file
// launches, allocates or owns LDS; the pipelines, tilings and LDS layouts stay with the kernels.
//
// Fragment layout (one 16 x 16 output block, 16-deep K block kb, lane = 16 g + pos, register j = 0..3):
//     A[lane][j] = W[16 nb + (lane & 15)][16 kb + 4 (lane >> 4) + j]          weights, packed on the host in this order
//     B[lane][j] = X[row (lane & 15)][16 kb + 4 (lane >> 4) + j]              activations, a 16-byte piece of a row
//     D register j = out[row (lane & 15)][16 nb + 4 (lane >> 4) + j]          four consecutive channels of one row
// so an A or B fragment is one 16-byte load a lane, D is one 16-byte row store a lane, and D of one layer is the B fragment
// of the next.  The four MFMAs of a K block consume components x, y, z, w of both fragments in that order.
#pragma once
#include "common.h"

namespace pdm {

typedef float f4 __attribute__((ext_vector_type(4)));

// LDS row stride in floats of a 16-channel slice of staged rows that is read back as B fragments (16 + 8 pad): with 6 slots
// of 16 B per row the 16 lanes of every ds_read_b128 group ({0-3, 12-15, 20-27}, ...: MI355X_MICROARCH.md, LDS) land on 16
// different slots of the 256-B bank row; with 5 (a 4-float pad) rows p and p + 4 of neighbouring k-quads shared a slot:
// SQ_LDS_BANK_CONFLICT / SQ_LDS_IDX_ACTIVE = 0.375
constexpr int MFMA_ROW_STRIDE = 24;

// One 16-deep K block into one accumulator: the x, y, z, w products in that order (the results' bits depend on it).
__device__ __forceinline__ f4 mfma4(f4 acc, f4 a, f4 b) {
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, b.x, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, b.y, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, b.z, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, b.w, acc, 0, 0, 0);
    return acc;
}

// The same K block for NA x NB independent accumulators, component-outer: every (i, t) product of .x, then of .y, .z, .w,
// so that consecutive MFMAs never depend on each other.  Each accumulator still sees x, y, z, w in order.
template <int NA, int NB>
__device__ __forceinline__ void mfma4_grid(f4 (&acc)[NA][NB], const f4 (&fa)[NA], const f4 (&fb)[NB]) {
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int i = 0; i < NA; ++i)
#pragma unroll
            for (int t = 0; t < NB; ++t) acc[i][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(fa[i][c], fb[t][c], acc[i][t], 0, 0, 0);
}
// one output block over NB row tiles
template <int NB>
__device__ __forceinline__ void mfma4_grid(f4 (&acc)[NB], f4 fa, const f4 (&fb)[NB]) {
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int t = 0; t < NB; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(fa[c], fb[t][c], acc[t], 0, 0, 0);
}
// the first n of NA output blocks over one row tile (n a constant once the caller is unrolled)
template <int NA>
__device__ __forceinline__ void mfma4_grid(f4 *acc, const f4 (&fa)[NA], f4 fb, int n = NA) {
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int i = 0; i < NA; ++i)
            if (i < n) acc[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(fa[i][c], fb[c], acc[i], 0, 0, 0);
}

// A fragment of packed block `block` (the caller's block order: [nb][kb], [kb][nb], ...), from global memory or LDS
__device__ __forceinline__ f4 a_frag(const float *wpack, size_t block, int lane) {
    return reinterpret_cast<const f4 *>(wpack)[block * 64 + lane];
}
// B fragment of K block kb from row-major rows of `stride` floats (16-byte aligned pieces)
__device__ __forceinline__ f4 b_frag(const float *rows, int row, int stride, int kb, int g) {
    return *reinterpret_cast<const f4 *>(rows + row * stride + 16 * kb + 4 * g);
}

// p[0..3]; vec: p is 16-byte aligned
__device__ __forceinline__ f4 load_quad(const float *p, int vec) {
    if (vec) return *reinterpret_cast<const f4 *>(p);
    f4 r;
    r[0] = p[0]; r[1] = p[1]; r[2] = p[2]; r[3] = p[3];
    return r;
}
// channels [c, c + 4) of a row of `width` channels, p = &row[c]; zero past the width, and nothing past it is read
__device__ __forceinline__ f4 load_quad_ragged(const float *p, int c, int width, bool vec) {
    if (vec && c + 4 <= width) return *reinterpret_cast<const f4 *>(p);
    f4 v = {0.f, 0.f, 0.f, 0.f};
    if (c < width) v.x = p[0];
    if (c + 1 < width) v.y = p[1];
    if (c + 2 < width) v.z = p[2];
    if (c + 3 < width) v.w = p[3];
    return v;
}

__device__ __forceinline__ void store_quad(float *p, f4 v, int vec) {
    if (vec) { *reinterpret_cast<f4 *>(p) = v; return; }
    p[0] = v[0]; p[1] = v[1]; p[2] = v[2]; p[3] = v[3];
}
// channels [c0, c0 + 4) of a 16-byte aligned row of `width` channels (c0 a multiple of 4); nothing past the width is written
__device__ __forceinline__ void store_quad_ragged(float *row, int c0, int width, f4 v) {
    if (c0 + 4 <= width) {
        *reinterpret_cast<f4 *>(row + c0) = v;
    } else {
        if (c0 < width) row[c0] = v.x;
        if (c0 + 1 < width) row[c0 + 1] = v.y;
        if (c0 + 2 < width) row[c0 + 2] = v.z;
    }
}

// max(v, floor) as one v_med3_f32 (fmaxf() costs a canonicalising v_max v,v,v on top; inline asm would hide the
// MFMA -> VALU read hazard from the compiler).  floor = 0 for ReLU, -inf for a linear last layer.
__device__ __forceinline__ float max1(float v, float floor) { return __builtin_amdgcn_fmed3f(v, floor, __builtin_inff()); }
__device__ __forceinline__ f4 floor4(f4 v, float floor) {
    v.x = max1(v.x, floor); v.y = max1(v.y, floor); v.z = max1(v.z, floor); v.w = max1(v.w, floor);
    return v;
}

// v * scale[c0 + j] + shift[c0 + j] as one fma (scale null: v as it is), then ReLU; a NaN stays, as torch's ReLU keeps it
__device__ __forceinline__ f4 scale_shift_relu4(f4 v, const float *scale, const float *shift, int c0, bool relu) {
    if (scale) {
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = __fmaf_rn(v[j], scale[c0 + j], shift[c0 + j]);
    }
    if (relu) {
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = v[j] < 0.0f ? 0.0f : v[j];
    }
    return v;
}

}  // namespace pdm

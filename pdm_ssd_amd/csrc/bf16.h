// bf16 <-> fp32 as bit patterns (unsigned short), shared by every kernel that reads or writes bf16 rows.
#pragma once
#include <hip/hip_runtime.h>

namespace pdm {

// round to nearest even, the rounding of torch's .bfloat16(); a NaN stays a (quiet) NaN
__device__ __forceinline__ unsigned short f32_to_bf16(float f) {
    unsigned u = __float_as_uint(f);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (unsigned short)((u >> 16) | 0x0040u);
    u += 0x7fffu + ((u >> 16) & 1u);
    return (unsigned short)(u >> 16);
}

__device__ __forceinline__ float bf16_to_f32(unsigned short h) { return __uint_as_float((unsigned)h << 16); }

// eight consecutive channels as one 16-byte word, channel 0 in the low half of .x
__device__ __forceinline__ uint4 pack_bf16x8(const float (&v)[8]) {
    uint4 o;
    o.x = (unsigned)f32_to_bf16(v[0]) | ((unsigned)f32_to_bf16(v[1]) << 16);
    o.y = (unsigned)f32_to_bf16(v[2]) | ((unsigned)f32_to_bf16(v[3]) << 16);
    o.z = (unsigned)f32_to_bf16(v[4]) | ((unsigned)f32_to_bf16(v[5]) << 16);
    o.w = (unsigned)f32_to_bf16(v[6]) | ((unsigned)f32_to_bf16(v[7]) << 16);
    return o;
}

}  // namespace pdm

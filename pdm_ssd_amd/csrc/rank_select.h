// The score rank order of pdm_topk_sampling, shared with post_process.hip (the batched post-processing selects its
// NMS candidates in the same order): score descending on the order-preserving integer image of the float, equal
// images by lower index.  One workgroup of TK_THREADS threads per list.
#pragma once
#include "common.h"

namespace pdm {

constexpr int TK_THREADS = 1024;
constexpr int TK_MAXK = 16384;   // 128 KB of 8-byte items

// smaller key = higher rank
__device__ __host__ __forceinline__ unsigned topk_key(unsigned bits) {
    if ((bits & 0x7fffffffu) > 0x7f800000u) return 0u;                     // NaN: ranks first
    const unsigned mono = (bits & 0x80000000u) ? ~bits : (bits | 0x80000000u);   // ascending with the float order
    return ~mono;
}

__device__ __forceinline__ int tk_block_scan(int v, int *s_wave, int *total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int incl = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int t = __shfl_up(incl, off, 64);
        if (lane >= off) incl += t;
    }
    __syncthreads();
    if (lane == 63) s_wave[wave] = incl;
    __syncthreads();
    int base = 0, tot = 0;
    for (int w = 0; w < TK_THREADS / 64; ++w) {
        const int x = s_wave[w];
        if (w < wave) base += x;
        tot += x;
    }
    *total = tot;
    return base + incl - v;
}

}  // namespace pdm

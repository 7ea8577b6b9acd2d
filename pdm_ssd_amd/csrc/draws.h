// Counter-based draws shared by the operators that replace the reference's global numpy / torch RNGs with build-defined,
// replayable ones (augment.hip, roi_targets.hip).  Everything is a pure function of (seed, step, position): no state
// but the step counter, which the operator's own kernel advances on the device.
//   fmix32 (common.h) = the murmur3 finaliser
//   draw_key(seed, step, b, s) = fmix32(fmix32(seed ^ step * 0x85EBCA6B) ^ b * 0x9E3779B1 ^ s * 0x7F4A7C15)
//   feistel_perm(i, n, kp): position i of a keyed permutation of [0, n) — a 4-round balanced Feistel network on 2w bits
//     (2^(2w) >= n, w >= 1), round r: (L, R) -> (R, L ^ (fmix32(kp ^ R * 0x9E3779B1 ^ (r + 1) * 0x7F4A7C15) & (2^w - 1))),
//     cycle-walked into [0, n).  A bijection of [0, n) for every key.
#pragma once
#include "common.h"

namespace pdm {

__device__ __forceinline__ unsigned draw_key(unsigned seed, unsigned step, unsigned b, unsigned s) {
    return fmix32(fmix32(seed ^ step * 0x85EBCA6Bu) ^ b * 0x9E3779B1u ^ s * 0x7F4A7C15u);
}

// The attention dropout (attention.hip, attention_bwd.hip): weight (sample b, head h, query i, key j) is kept iff
//   fmix32(draw_key(seed, step, b * H + h, i) ^ j * 0x9E3779B1) >= floor(p * 2^32),   0 <= p < 1
// qkey = the query's draw_key, evaluated once per query; a kept weight is multiplied by 1.0f / (1.0f - p).
__device__ __forceinline__ bool attn_keep(unsigned qkey, unsigned j, unsigned thresh) {
    return fmix32(qkey ^ j * 0x9E3779B1u) >= thresh;
}

__device__ __forceinline__ unsigned feistel_perm(unsigned i, unsigned n, unsigned kp) {
    int w = 1;
    while ((1ull << (2 * w)) < (unsigned long long)n) ++w;
    const unsigned mask = (1u << w) - 1u;
    unsigned x = i;
    do {
        unsigned L = x >> w, R = x & mask;
        for (unsigned r = 0; r < 4; ++r) {
            const unsigned f = fmix32(kp ^ R * 0x9E3779B1u ^ (r + 1u) * 0x7F4A7C15u) & mask;
            const unsigned t = L ^ f;
            L = R;
            R = t;
        }
        x = (L << w) | R;
    } while (x >= n);
    return x;
}

}  // namespace pdm

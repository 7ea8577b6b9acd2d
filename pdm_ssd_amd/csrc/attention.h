// What the attention forward (attention.hip) and backward (attention_bwd.hip) share: the supported set, the default
// chunking and the host side of the dropout parameters.
#pragma once
#include <math.h>

#include "mfma_f32.h"

namespace pdm {

constexpr int MHA_DEFAULT_CHUNK = 1024;

static inline int mha_chunk(int keys_per_chunk) { return keys_per_chunk > 0 ? keys_per_chunk : MHA_DEFAULT_CHUNK; }

static inline bool mha_supported(int B, int P, int N, int C, int nheads, int keys_per_chunk) {
    if (B < 0 || P < 1 || N < 1 || C < 1 || C > 256 || nheads < 1 || keys_per_chunk < 0 || C % nheads != 0) return false;
    const int d = C / nheads;
    return d == 16 || d == 32;
}

// 0 <= p < 1 (NaN fails)
static inline bool mha_dropout_ok(double p) { return p >= 0.0 && p < 1.0; }
// a weight is kept iff its draw >= floor(p 2^32)
static inline unsigned mha_dropout_thresh(double p) { return (unsigned)floor(p * 4294967296.0); }
static inline float mha_dropout_rinv(double p) { return 1.0f / (1.0f - (float)p); }

static inline bool mha_aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace pdm

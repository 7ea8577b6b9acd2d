// Rank select in one workgroup of TK_THREADS threads: the K smallest 32-bit keys of a list, ties by lower index, as
// sorted 8-byte (key, index) items in LDS.  Owns the whole algorithm, so that every operator that ranks this way makes
// the same decisions by construction:
//   topk_key           the score rank order of pdm_topk_sampling (post_process.hip selects its NMS candidates in it)
//   radix_kth_key      4 rounds of 8-bit radix select (radix_pick256, common.h) -> the K-th smallest key
//   rank_select        the rounds, the emission in index order and the sort (topk_sampling.hip, post_process.hip)
//   bitonic_sort_items the LDS sort
// input_path.hip emits items of its own (far points, copies, a second key) between radix_kth_key and the sort.
#pragma once
#include "common.h"

namespace pdm {

constexpr int TK_THREADS = 1024;
constexpr int TK_MAXK = 16384;   // 128 KB of 8-byte items

// smaller key = higher rank: score descending on the order-preserving integer image of the float, equal images by
// lower index
__device__ __host__ __forceinline__ unsigned topk_key(unsigned bits) {
    if ((bits & 0x7fffffffu) > 0x7f800000u) return 0u;                     // NaN: ranks first
    const unsigned mono = (bits & 0x80000000u) ? ~bits : (bits | 0x80000000u);   // ascending with the float order
    return ~mono;
}

// static LDS of a selecting workgroup; declare it alignas(16): the scans then read the wave totals 16 bytes at a time
struct RankLds {
    int hist[256];
    int wave[TK_THREADS / 64];
    int digit, before;
};

// The K-th smallest key (1 <= K <= number of elements that take part).  key(i, &k) says whether element i of [0, n)
// takes part and, if so, its key; *remaining = how many elements with exactly that key are among the K smallest (they are
// taken by lower index).
template <class Key>
__device__ __forceinline__ unsigned radix_kth_key(int n, int K, Key key, RankLds &lds, int *remaining) {
    const int tid = threadIdx.x;
    unsigned prefix = 0, pmask = 0;
    int left = K;                          // rank still to locate inside the current prefix bucket
    for (int round = 0; round < 4; ++round) {
        const int shift = 24 - 8 * round;
        for (int d = tid; d < 256; d += TK_THREADS) lds.hist[d] = 0;
        __syncthreads();
        for (int i = tid; i < n; i += TK_THREADS) {
            unsigned k;
            if (!key(i, k)) continue;
            if ((k & pmask) == prefix) atomicAdd(&lds.hist[(k >> shift) & 255u], 1);
        }
        __syncthreads();
        if (tid < 64) radix_pick256(lds.hist, left, &lds.digit, &lds.before);
        __syncthreads();
        prefix |= (unsigned)lds.digit << shift;
        pmask |= 255u << shift;
        left -= lds.before;
        __syncthreads();
    }
    *remaining = left;
    return prefix;
}

// ascending bitonic sort of K2 (a power of two) 8-byte items; the items must be visible to the workgroup on entry
__device__ __forceinline__ void bitonic_sort_items(unsigned long long *s_items, int K2) {
    for (int k = 2; k <= K2; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int q = threadIdx.x; q < K2; q += TK_THREADS) {
                const int partner = q ^ j;
                if (partner > q) {
                    const unsigned long long a = s_items[q], b = s_items[partner];
                    const bool up = (q & k) == 0;
                    if ((a > b) == up) { s_items[q] = b; s_items[partner] = a; }
                }
            }
            __syncthreads();
        }
    }
}

// s_items[r] = (key << 32 | index) of the r-th ranked element, r = 0 .. K - 1 (1 <= K <= n); key(i) -> unsigned for
// every i in [0, n).  s_items holds the next power of two >= max(K, 2) items.
template <class Key>
__device__ __forceinline__ void rank_select(int n, int K, Key key, unsigned long long *s_items, RankLds &lds) {
    const int tid = threadIdx.x;
    int remaining;
    const unsigned T = radix_kth_key(n, K, [&](int i, unsigned &k) { k = key(i); return true; }, lds, &remaining);

    const int K2 = 1 << (32 - __builtin_clz(max(K, 2) - 1));
    for (int q = tid; q < K2; q += TK_THREADS) s_items[q] = ~0ull;   // padding sorts last
    __syncthreads();
    // keys below T are all taken, keys equal to T in index order until `remaining` of them are in: one block scan per
    // 1024 elements carries both counts (equal-key count in the high half; n <= 2^31 / 65536 per chunk is trivially met)
    int lt_seen = 0, eq_seen = 0;
    for (int c0 = 0; c0 < n; c0 += TK_THREADS) {
        const int i = c0 + tid;
        unsigned k = 0xffffffffu;
        bool is_lt = false, is_eq = false;
        if (i < n) {
            k = key(i);
            is_lt = k < T;
            is_eq = k == T;
        }
        int tot;
        const int both = block_scan<TK_THREADS>((is_lt ? 1 : 0) | (is_eq ? 1 << 16 : 0), lds.wave, &tot);
        const int lt_rank = both & 0xffff, eq_rank = both >> 16;
        const int eq_before = min(eq_seen + eq_rank, remaining);        // equal-key elements taken in front of this one
        const bool take = is_lt || (is_eq && eq_seen + eq_rank < remaining);
        const int pos = lt_seen + lt_rank + eq_before;
        if (take && pos < K) s_items[pos] = ((unsigned long long)k << 32) | (unsigned)i;
        lt_seen += tot & 0xffff;
        eq_seen += tot >> 16;
    }
    __syncthreads();
    bitonic_sort_items(s_items, K2);
}

}  // namespace pdm

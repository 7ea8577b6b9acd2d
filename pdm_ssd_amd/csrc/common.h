// Shared device/host helpers for libpdmssd_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/pdmssd_hip.h"

#define PDM_WAVE 64

namespace pdm {

// Thread-local error text behind pdm_last_error().
void set_error(const char *fmt, ...);
int check_launch(const char *what);
// Clears `bytes` bytes at p (any alignment) on the stream with a kernel; 0 bytes launch nothing.  Returns check_launch(who).
int zero_fill(void *stream, const char *who, void *p, size_t bytes);
// More than 64 KB of dynamic LDS has to be granted per kernel function AND per device (hipFuncSetAttribute acts on the
// CURRENT device's copy of the function; entry points may be called for any device).  Remembers (function, device)
// pairs, thread-safe; returns hipSuccess (0) or the runtime's error code.
int grant_lds(const void *fn, size_t bytes);

// Ragged compaction in W segments per frame (augment.hip, kitti_data.hip; defined in augment.hip): seg_count (B, W) ->
// seg_base (B, W) the exclusive prefix inside the frame, out_counts (B) the frame totals, offsets (B + 1) their exclusive
// prefix over the frames, overflow[0] = offsets[B] > capacity.  B <= 1024.
int segment_scan_launch(void *stream, const char *what, int B, int W, const int *seg_count, int *seg_base, int *out_counts,
                        long long *offsets, int *overflow, long long capacity);

static inline hipStream_t as_stream(void *s) { return reinterpret_cast<hipStream_t>(s); }

static inline int divup(long long a, long long b) { return (int)((a + b - 1) / b); }

// workspace sections start on 256-byte boundaries
static inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

// the murmur3 finaliser behind every counter-based draw (input_path.hip, augment.hip)
__device__ __host__ __forceinline__ unsigned fmix32(unsigned h) {
    h ^= h >> 16; h *= 0x85ebca6bu; h ^= h >> 13; h *= 0xc2b2ae35u; h ^= h >> 16;
    return h;
}

// how many lanes below `lane` are set in a ballot: the lane's rank among the hits
__device__ __forceinline__ int lanes_below(unsigned long long mask, int lane) {
    return __popcll(mask & ((1ull << lane) - 1ull));
}

// the sum of one value per lane over the wave, to every lane (all 64 lanes call it)
template <class T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// inclusive scan of one int per lane over the wave (all 64 lanes call it)
__device__ __forceinline__ int wave_scan_incl(int v) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int t = __shfl_up(v, off, 64);
        if (lane >= off) v += t;
    }
    return v;
}

// block-wide exclusive scan of one int per thread (NT threads, every one calls it); returns the exclusive prefix,
// *total = block sum.  s_wave: NT / 64 ints of LDS, reusable by the next call at once.
template <int NT>
__device__ __forceinline__ int block_scan(int v, int *s_wave, int *total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int incl = wave_scan_incl(v);
    __syncthreads();                      // s_wave reuse across calls
    if (lane == 63) s_wave[wave] = incl;
    __syncthreads();
    int base = 0, tot = 0;
    for (int w = 0; w < NT / 64; ++w) {
        const int x = s_wave[w];
        if (w < wave) base += x;
        tot += x;
    }
    *total = tot;
    return base + incl - v;
}

// Exclusive scan of n totals in global memory in place by ONE workgroup of NT threads (the middle launch of a multi-launch
// scan, between tile_reduce and tile_scan below); returns the grand total to every thread.  s_wave: NT / 64 ints of LDS.
template <int NT>
__device__ __forceinline__ int scan_totals(int n, int *__restrict__ v, int *s_wave) {
    int carry = 0;
    for (int base = 0; base < n; base += NT) {
        const int i = base + threadIdx.x;
        const int x = i < n ? v[i] : 0;
        int total;
        const int excl = block_scan<NT>(x, s_wave, &total);
        if (i < n) v[i] = carry + excl;
        carry += total;
    }
    return carry;
}

// ---- the outer launches of a multi-launch scan: scan_totals is the middle one -----------------------------------------
// A workgroup of NT threads owns a tile of NT * ITEMS items; item j of thread t is blockIdx.x * NT * ITEMS + j * NT + t.
// Both passes carry K values an item (K = 1 or 2, deduced from the braced list of tiles / bases).
constexpr int SCAN_T = 256;                        // the voxelizers' tiles (pillar.hip, sc_index.h, hard_voxel.hip)
constexpr int SCAN_ITEMS = 8;
constexpr int SCAN_TILE = SCAN_T * SCAN_ITEMS;

// Pass one: tiles[k][blockIdx.x] = the tile's sum of value k.  value(i, sum) adds item i < n to sum[0 .. K); it is not called
// past n and may have side effects of its own (the first read of a row is where its key and its atomics belong).
template <int NT, int ITEMS, int K, class F>
__device__ __forceinline__ void tile_reduce(long long n, int *const (&tiles)[K], F value) {
    __shared__ int s_total[K];
    if (threadIdx.x == 0)
        for (int k = 0; k < K; ++k) s_total[k] = 0;
    __syncthreads();
    int sum[K] = {};
    for (int j = 0; j < ITEMS; ++j) {
        const long long i = (long long)blockIdx.x * (NT * ITEMS) + j * NT + threadIdx.x;
        if (i >= n) break;
        value(i, sum);
    }
    for (int k = 0; k < K; ++k)
        if (sum[k]) atomicAdd(&s_total[k], sum[k]);
    __syncthreads();
    if (threadIdx.x == 0)
        for (int k = 0; k < K; ++k) tiles[k][blockIdx.x] = s_total[k];
}

// Pass three: base[k] is the tile's entry of the scanned totals.  value(i, v) sets v[0 .. K) of item i < n (an item past n
// counts as zeros), then body(i, at) runs for the same item with at[k] = base[k] + the exclusive prefix of value k inside
// the tile: the two may share a captured local.  The block_scans hold barriers, so every thread reaches every one of them:
// the loop has no break, and a body that has nothing to do returns.
template <int NT, int ITEMS, int K, class V, class F>
__device__ __forceinline__ void tile_scan(long long n, const int (&base)[K], V value, F body) {
    __shared__ int s_wave[NT / 64];
    int run[K];
    for (int k = 0; k < K; ++k) run[k] = base[k];
    for (int j = 0; j < ITEMS; ++j) {
        const long long i = (long long)blockIdx.x * (NT * ITEMS) + j * NT + threadIdx.x;
        int v[K] = {}, at[K];
        if (i < n) value(i, v);
        for (int k = 0; k < K; ++k) {
            int total;
            at[k] = run[k] + block_scan<NT>(v[k], s_wave, &total);
            run[k] += total;
        }
        if (i < n) body(i, at);
    }
}

// scan_totals as a launch of its own, ONE workgroup of NT threads: v[0 .. n) -> its exclusive prefix in place, v[n] = the total
// (v holds n + 1 ints).  record, when not null: record[slot] = the total, and record[clear] = 0 when clear >= 0 (the words of
// a caller's host read).  roiaware_sparse.hip, sparse_fc.hip.
template <int NT>
__global__ __launch_bounds__(NT) void scan_totals_kernel(int n, int *v, int *record, int slot, int clear) {
    __shared__ int s_wave[NT / 64];
    const int total = scan_totals<NT>(n, v, s_wave);
    if (threadIdx.x == 0) {
        v[n] = total;
        if (record) record[slot] = total;
        if (record && clear >= 0) record[clear] = 0;
    }
}

// Exclusive scan of an LDS histogram in place: counts become running cursors (the fill positions of a counting sort).
// Every thread of the workgroup (NT threads) calls it after the barrier that completes hist[0..ncells); a thread owns a
// contiguous chunk of cells (a compile-time ncells gives constant-trip loops, which unroll).  start_out, when not null,
// receives the ncells + 1 starts.  s_wave: NT / 64 ints of LDS.  Ends with a barrier: the cursors are ready on return.
template <int NT>
__device__ __forceinline__ void hist_to_cursors(int *hist, int ncells, int *s_wave, int *__restrict__ start_out) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int per = (ncells + NT - 1) / NT;
    const int c0 = threadIdx.x * per, c1 = min(c0 + per, ncells);
    int local = 0;
    for (int c = c0; c < c1; ++c) local += hist[c];
    const int incl = wave_scan_incl(local);
    if (lane == 63) s_wave[wave] = incl;
    __syncthreads();
    if (wave == 0) {
        const int v = lane < NT / 64 ? s_wave[lane] : 0;
        const int inc = wave_scan_incl(v);
        if (lane < NT / 64) s_wave[lane] = inc - v;   // exclusive wave offsets
    }
    __syncthreads();
    int run = s_wave[wave] + incl - local;
    for (int c = c0; c < c1; ++c) {
        const int cnt = hist[c];
        hist[c] = run;
        if (start_out) start_out[c] = run;
        run += cnt;
    }
    if (start_out && threadIdx.x == NT - 1) start_out[ncells] = run;   // the last thread ends on the total
    __syncthreads();
}

// Cell of one coordinate as the reference's dynamic voxel encoders compute it (voxel_grid.h's voxel_key):
// floor((x - x0) / v) in fp32 with an IEEE division (not a reciprocal multiply: 0.16 is no power of two).  Returns -1
// outside [0, n) and for NaN.
__device__ __forceinline__ int cell_1d(float x, float x0, float v, int n) {
    const float c = floorf(__fdiv_rn(__fsub_rn(x, x0), v));
    return (c >= 0.0f && c < (float)n) ? (int)c : -1;
}

// Squared distance with the rounding sequence pinned:
//   d = fma(dz,dz, fma(dy,dy, rn(dx*dx)))
// The translation units are also built with -ffp-contract=off so nothing else is fused.
__device__ __forceinline__ float sqdist(float dx, float dy, float dz) {
    return __fmaf_rn(dz, dz, __fmaf_rn(dy, dy, __fmul_rn(dx, dx)));
}

// One radix-select round, run by the FIRST WAVE of the workgroup (all 64 lanes): the first of 256 histogram bins at
// which the running count reaches `remaining` (>= 1), and the count in front of it.  Four bins per lane, one wave scan
// (a single thread walking the bins is a chain of 256 dependent LDS reads, ~10 us per round).
__device__ __forceinline__ void radix_pick256(const int *hist, int remaining, int *digit, int *before) {
    const int lane = threadIdx.x & 63;
    const int h0 = hist[4 * lane], h1 = hist[4 * lane + 1], h2 = hist[4 * lane + 2], h3 = hist[4 * lane + 3];
    const int sum = h0 + h1 + h2 + h3;
    const int incl = wave_scan_incl(sum);
    const int excl = incl - sum;
    const unsigned long long hit = __ballot(excl < remaining && incl >= remaining);
    const int src = hit ? __ffsll((long long)hit) - 1 : 63;   // no lane reaches it only if remaining > total: last bins
    if (lane == src) {
        int acc = excl, d = 4 * lane;
        if (acc + h0 < remaining) { acc += h0; ++d;
            if (acc + h1 < remaining) { acc += h1; ++d;
                if (acc + h2 < remaining) { acc += h2; ++d; } } }
        *digit = d;
        *before = acc;
    }
}

// ---- ragged ("stacked") batches: per-sample counts -> LDS prefix tables (stack_ops.hip, vector_pool.hip) -------
constexpr int ST_MAXB = 1024;   // samples per call held as LDS prefix tables

// prefix[k] = sum of cnt[0..k) for k = 0..B, built once per workgroup
__device__ __forceinline__ void build_prefix(int B, const int *__restrict__ cnt, int *prefix) {
    if (threadIdx.x == 0) {
        int acc = 0;
        for (int k = 0; k < B; ++k) { prefix[k] = acc; acc += cnt[k]; }
        prefix[B] = acc;
    }
}
// the reference's linear scan (ball_query_gpu.cu:27-32): the last sample absorbs elements past the total
__device__ __forceinline__ int sample_of(int i, int B, const int *prefix) {
    int bs = 0;
    for (int k = 1; k < B; ++k) {
        if (i < prefix[k]) break;
        bs = k;
    }
    return bs;
}

// both tables of a (centres, points) pair: wave 0 builds one, wave 1 the other; the caller syncs the workgroup
__device__ __forceinline__ void build_prefix_pair(int B, const int *__restrict__ cnt_a, int *prefix_a,
                                                  const int *__restrict__ cnt_b, int *prefix_b) {
    build_prefix(B, cnt_a, prefix_a);
    if (threadIdx.x == 64) {
        int acc = 0;
        for (int k = 0; k < B; ++k) { prefix_b[k] = acc; acc += cnt_b[k]; }
        prefix_b[B] = acc;
    }
}

}  // namespace pdm

#define PDM_REQUIRE(cond, code, ...)      \
    do {                                  \
        if (!(cond)) {                    \
            pdm::set_error(__VA_ARGS__);  \
            return (code);                \
        }                                 \
    } while (0)
// every void *workspace holds ints, floats and 64-bit words of the library's own: 8-byte aligned, or rejected
#define PDM_WS_ALIGNED(who, ws) \
    PDM_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 7) == 0, PDM_E_BADARG, "%s: workspace must be 8-byte aligned", who)

// DSVT (Dynamic Sparse Voxel Transformer) on the device: the set partition of one stage and the fused set attention.
//
// ---- pdm_dsvt_partition_count / pdm_dsvt_partition ------------------------------------------------------------------------
// The partition is a pure function of the voxel coordinates.  For each of the two shifts a voxel (b, z, y, x) lies in the window
//     win = ((b MX + X / wx) MY + Y / wy) MZ + Z / wz,   (X, Y, Z) = (x, y, z) + shift,   M* = ceil(shape / w) + 1
// at the in-window position (X % wx, Y % wy, Z % wz), and has two sort keys there,
//     ykey = (iy wx + ix) wz + iz,        xkey = (ix wy + iy) wz + iz.
// ONE occupancy bitmap (sc_index.h) holds four sections, (shift, axis), each over the cells win * max_voxel + key, with scanned
// group popcounts.  Ranks only ever enter as differences inside one section, so the sections need no scan of their own:
//     n_w    = rank(end of window) - rank(start of window)         voxels of the window
//     r      = rank(the voxel's cell) - rank(start of window)      the voxel's number under that key
// A second tiled scan runs over the windows of both shifts (plus one closing item) with ceil(n_w / ss) as the value: the window's
// first set, in ascending window order, which is torch.unique's; its entry at the first window of shift 1 and its total are
// the two set counts, the one host read.  Then every (voxel, shift, axis) writes its own slots: slot k of the window's
// sets_w ss slots holds the voxel of number floor(k n_w / (sets_w ss)), an onto map, so voxel r owns the k in
// [ceil(r T / n), ceil((r + 1) T / n)), T = sets_w ss, and is the only writer of each; the mask (slot equals its left neighbour
// in the set) is k != the first of them and k % ss != 0.  No sort, no hash, no cursor; every product of k and n is 64-bit.
//
// ---- pdm_set_attention -----------------------------------------------------------------------------------------------------
// One wave per (set, head), four to a workgroup, no LDS and no barrier.  The set's rows are gathered ONCE, straight into MFMA
// fragments: the head's k rows as A fragments, its v rows as the A fragments of the second product, the q rows tile by tile as B
// fragments.  The products are attention.hip's, oriented so that nothing changes lanes between them:
//     S^T = K Q^T    a lane ends with 4 scores of ONE query (column lane & 15) against the keys 4 (lane >> 4) + r of each tile
//     O^T = V^T P^T  A = v[key 4 (lane >> 4) + r][channel lane & 15], B = the lane's own weights
// with the whole score row of a query in registers (ss <= 128: 8 tiles), so the softmax is the plain one: maximum, exp2, sum.
// The contraction index of the first product is free as long as A and B name it alike: lane group g holds the d / 4 consecutive
// channels g d / 4 .. of its row, and step u multiplies channel g d / 4 + u, which serves d = 24 in 6 steps without padding.
// A slot is dead when it is past ss or equals its left neighbour (derived here from the indices, the mask is not read): dead keys
// get the score -inf, dead queries are computed on a real row and not written.  Each voxel has one live slot, so each out row
// has one writer: no atomics, two runs give the same bits.
#include <math.h>

#include "mfma_f32.h"
#include "sc_index.h"

namespace pdm {

// ---- partition ----------------------------------------------------------------------------------------------------------
struct DpShift {
    int wx, wy, wz;          // window
    int hx, hy, hz;          // shift (hz = 0 when the window spans z)
    int mx, my, mz;          // windows per axis, the shift's extra one included
    int nwin, mv;            // B mx my mz; wx wy wz
    int win0;                // this shift's first entry of the window table
    long long cell[2];       // first cell of the ykey / xkey section of the bitmap
};
struct DpArgs {
    int N, B, sx, sy, sz, ss, nwin_all;
    DpShift sh[2];
};
struct DpWorkspace {
    size_t record, index, wtiles, setbase, total;
    ScIndexSize isz;
    int nwt;
};
constexpr int DP_RECORD = 4;        // S of shift 0, S of both, a coordinate outside the grid, set bits

static bool dp_geometry(DpArgs &a, int N, int B, int sx, int sy, int sz, const int *win, const int *shift, int ss) {
    a.N = N; a.B = B; a.sx = sx; a.sy = sy; a.sz = sz; a.ss = ss;
    long long cells = 0, nwin_all = 0;
    for (int s = 0; s < 2; ++s) {
        DpShift &h = a.sh[s];
        h.wx = win[3 * s]; h.wy = win[3 * s + 1]; h.wz = win[3 * s + 2];
        if (h.wx < 1 || h.wy < 1 || h.wz < 1) return false;
        h.hx = shift ? shift[3 * s] : 0; h.hy = shift ? shift[3 * s + 1] : 0; h.hz = shift ? shift[3 * s + 2] : 0;
        if (sz == h.wz) h.hz = 0;
        if (h.hx < 0 || h.hx > h.wx || h.hy < 0 || h.hy > h.wy || h.hz < 0 || h.hz > h.wz) return false;
        h.mx = divup(sx, h.wx) + 1; h.my = divup(sy, h.wy) + 1; h.mz = divup(sz, h.wz) + 1;
        const long long nwin = (long long)B * h.mx * h.my * h.mz, mv = (long long)h.wx * h.wy * h.wz;
        if (nwin > 0x3fffffffll || mv > 0x3fffffffll || nwin * mv > SC_MAXCELL / 4) return false;
        h.nwin = (int)nwin; h.mv = (int)mv; h.win0 = (int)nwin_all;
        nwin_all += nwin;
        for (int ax = 0; ax < 2; ++ax) {                     // one spare cell: the rank at a section's end reads a word of its own
            h.cell[ax] = cells;
            cells += (nwin * mv + 1 + 32 * SC_GW - 1) / (32 * SC_GW) * (32 * SC_GW);
        }
    }
    if (nwin_all > 0x3fffffffll) return false;
    a.nwin_all = (int)nwin_all;
    return true;
}
static bool dp_sizes_ok(int N, int B, int sx, int sy, int sz) {
    return N >= 0 && B >= 0 && sx >= 1 && sy >= 1 && sz >= 1 && (long long)N * 4 <= 0x7fffffffll;
}
static DpWorkspace dp_workspace(const DpArgs &a) {
    DpWorkspace w{};
    const DpShift &l = a.sh[1];
    const long long cells = l.cell[1] + ((long long)l.nwin * l.mv + 1 + 32 * SC_GW - 1) / (32 * SC_GW) * (32 * SC_GW);
    w.isz = sc_index_size(cells);
    w.nwt = divup((long long)a.nwin_all + 1, SCAN_TILE);
    size_t at = 0;
    w.record = at; at += 256;
    w.index = at; at += w.isz.bits + w.isz.gprefix + w.isz.tiles;
    w.wtiles = at; at += align256(sizeof(int) * ((size_t)w.nwt + 1));
    w.setbase = at; at += align256(sizeof(int) * ((size_t)a.nwin_all + 1));
    w.total = at;
    return w;
}

struct DpPlace { int win, key[2], iz, iy, ix; };
__device__ __forceinline__ DpPlace dp_place(const DpShift &h, const int *__restrict__ c) {
    const int X = c[3] + h.hx, Y = c[2] + h.hy, Z = c[1] + h.hz;
    const int gx = X / h.wx, gy = Y / h.wy, gz = Z / h.wz;
    DpPlace p;
    p.ix = X - gx * h.wx; p.iy = Y - gy * h.wy; p.iz = Z - gz * h.wz;
    p.win = ((c[0] * h.mx + gx) * h.my + gy) * h.mz + gz;
    p.key[0] = (p.iy * h.wx + p.ix) * h.wz + p.iz;
    p.key[1] = (p.ix * h.wy + p.iy) * h.wz + p.iz;
    return p;
}
__device__ __forceinline__ bool dp_inside(const DpArgs &a, const int *__restrict__ c) {
    return c[0] >= 0 && c[0] < a.B && c[1] >= 0 && c[1] < a.sz && c[2] >= 0 && c[2] < a.sy && c[3] >= 0 && c[3] < a.sx;
}

__global__ __launch_bounds__(SC_T) void dp_mark_kernel(DpArgs a, const int *__restrict__ coords, unsigned *__restrict__ bits,
                                                       int *__restrict__ coors_in_win, int *__restrict__ record) {
    const int i = blockIdx.x * SC_T + threadIdx.x;
    if (i >= a.N) return;
    const int *c = coords + 4 * (size_t)i;
    if (!dp_inside(a, c)) { record[2] = 1; return; }
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        const DpShift &h = a.sh[s];
        const DpPlace p = dp_place(h, c);
        sc_set(bits, h.cell[0] + (long long)p.win * h.mv + p.key[0]);
        sc_set(bits, h.cell[1] + (long long)p.win * h.mv + p.key[1]);
        int *o = coors_in_win + 3 * ((size_t)s * a.N + i);
        o[0] = p.iz; o[1] = p.iy; o[2] = p.ix;
    }
}

// sets of entry i of the window table (both shifts in a row, then one closing item of value 0)
__device__ __forceinline__ int dp_win_sets(const DpArgs &a, const unsigned *__restrict__ bits, const int *__restrict__ gprefix, long long i) {
    if (i >= a.nwin_all) return 0;
    const DpShift &h = a.sh[i >= a.sh[1].win0 ? 1 : 0];
    const long long k0 = h.cell[0] + (i - h.win0) * h.mv;
    const int n = sc_rank(bits, gprefix, k0 + h.mv) - sc_rank(bits, gprefix, k0);
    return (n + a.ss - 1) / a.ss;
}
__global__ __launch_bounds__(SC_T) void dp_win_total_kernel(DpArgs a, const unsigned *__restrict__ bits, const int *__restrict__ gprefix,
                                                            int *__restrict__ wtiles) {
    tile_reduce<SC_T, SCAN_ITEMS>((long long)a.nwin_all + 1, {wtiles}, [&](long long i, int *sum) { sum[0] += dp_win_sets(a, bits, gprefix, i); });
}
__global__ __launch_bounds__(SC_T) void dp_win_fill_kernel(DpArgs a, const unsigned *__restrict__ bits, const int *__restrict__ gprefix,
                                                           const int *__restrict__ wtiles, int *__restrict__ setbase, int *__restrict__ record) {
    tile_scan<SC_T, SCAN_ITEMS>((long long)a.nwin_all + 1, {wtiles[blockIdx.x]},
                                [&](long long i, int *v) { v[0] = dp_win_sets(a, bits, gprefix, i); },
                                [&](long long i, const int *at) {
                                    setbase[i] = at[0];
                                    if (i == a.sh[1].win0) record[0] = at[0];
                                });
}

struct DpOut {
    long long *inds[2];
    unsigned char *mask[2];
    int S[2];
};
// thread = (voxel, shift, axis)
__global__ __launch_bounds__(SC_T) void dp_slots_kernel(DpArgs a, const int *__restrict__ coords, const unsigned *__restrict__ bits,
                                                        const int *__restrict__ gprefix, const int *__restrict__ setbase, DpOut o) {
    const long long t = (long long)blockIdx.x * SC_T + threadIdx.x;
    const int i = (int)(t >> 2), s = (int)(t >> 1) & 1, ax = (int)t & 1;
    if (i >= a.N) return;
    const int *c = coords + 4 * (size_t)i;
    if (!dp_inside(a, c)) return;
    const DpShift &h = a.sh[s];
    const DpPlace p = dp_place(h, c);
    const long long k0 = h.cell[ax] + (long long)p.win * h.mv;
    const int w0 = sc_rank(bits, gprefix, k0);
    const long long n = sc_rank(bits, gprefix, k0 + h.mv) - w0, r = sc_rank(bits, gprefix, k0 + p.key[ax]) - w0;
    if (n < 1 || r < 0 || r >= n) return;                              // (the voxel's own bit is set: never on a bitmap of this call)
    const long long T = (n + a.ss - 1) / a.ss * a.ss;
    const long long ka = (r * T + n - 1) / n, kb = ((r + 1) * T + n - 1) / n;
    // the window table runs through both shifts: shift 1 counts its sets from the end of shift 0's
    const long long base = (long long)(setbase[h.win0 + p.win] - (s ? o.S[0] : 0)) * a.ss, slots = (long long)o.S[s] * a.ss;
    if (base < 0 || base + kb > slots) return;                         // set counts that are not this bitmap's
    long long *inds = o.inds[s] + ax * slots + base;
    unsigned char *mask = o.mask[s] + ax * slots + base;
    for (long long k = ka; k < kb; ++k) {
        inds[k] = i;
        mask[k] = (k != ka && k % a.ss != 0) ? 1 : 0;
    }
}

// ---- set attention ------------------------------------------------------------------------------------------------------
constexpr int SA_T = 256;           // 4 waves, one (set, head) each

struct SaArgs {
    int S, ss, N, C, H, vec, ovec;
    const float *q, *k, *v;
    long long qs, ks, vs;
    const long long *inds;
    float c;                         // log2(e) / sqrt(d)
    float *out;
};

// DS consecutive floats at p; vec: p is aligned to 16 bytes (DS = 4, 8) or 8 bytes (DS = 6)
template <int DS>
__device__ __forceinline__ void sa_load_run(float (&f)[DS], const float *__restrict__ p, int vec) {
    if (vec) {
        if constexpr (DS == 6) {
            typedef float f2 __attribute__((ext_vector_type(2)));
#pragma unroll
            for (int u = 0; u < 3; ++u) {
                const f2 x = reinterpret_cast<const f2 *>(p)[u];
                f[2 * u] = x.x; f[2 * u + 1] = x.y;
            }
        } else {
#pragma unroll
            for (int u = 0; u < DS / 4; ++u) {
                const f4 x = reinterpret_cast<const f4 *>(p)[u];
                f[4 * u] = x.x; f[4 * u + 1] = x.y; f[4 * u + 2] = x.z; f[4 * u + 3] = x.w;
            }
        }
    } else {
#pragma unroll
        for (int u = 0; u < DS; ++u) f[u] = p[u];
    }
}

template <int D, int NT>
__global__ __launch_bounds__(SA_T) void set_attention_kernel(SaArgs a) {
    constexpr int DS = D / 4;               // steps of q k^T; a lane group's run of channels
    constexpr int VT = (D + 15) / 16;       // 16-channel tiles of the head's output
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, col = lane & 15, grp = lane >> 4;
    const long long w = (long long)blockIdx.x * (SA_T / 64) + wave;
    if (w >= (long long)a.S * a.H) return;                             // the whole wave; nothing below synchronises waves
    const int set = (int)(w / a.H), h = (int)(w - (long long)set * a.H);
    const long long *ind = a.inds + (long long)set * a.ss;

    int row[NT];
    unsigned dead_keys[NT];
    bool dead[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const int j = 16 * t + col, jc = min(j, a.ss - 1);
        const long long r = ind[jc], left = jc > 0 ? ind[jc - 1] : -1;
        dead[t] = j >= a.ss || r == left;
        row[t] = (int)min(max(r, 0ll), (long long)a.N - 1);            // an index outside the rows reads a real row
        dead_keys[t] = (unsigned)(__ballot(dead[t]) & 0xffffull);
    }
    // the head's k rows (A of S^T = K Q^T) and v rows (A of O^T = V^T P^T), once
    float kf[NT][DS], vf[NT][VT][4];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        sa_load_run<DS>(kf[t], a.k + (size_t)row[t] * a.ks + h * D + grp * DS, a.vec);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int vrow = __shfl(row[t], 4 * grp + r, 64);
            const float *vp = a.v + (size_t)vrow * a.vs + h * D + col;
#pragma unroll
            for (int u = 0; u < VT; ++u) vf[t][u][r] = 16 * u + col < D ? vp[16 * u] : 0.0f;
        }
    }
#pragma unroll
    for (int qt = 0; qt < NT; ++qt) {
        if (16 * qt >= a.ss) break;
        float qf[DS];
        sa_load_run<DS>(qf, a.q + (size_t)row[qt] * a.qs + h * D + grp * DS, a.vec);
        f4 s[NT];
        float m = -INFINITY;
#pragma unroll
        for (int kt = 0; kt < NT; ++kt) {
            s[kt] = f4{0, 0, 0, 0};
#pragma unroll
            for (int u = 0; u < DS; ++u) s[kt] = __builtin_amdgcn_mfma_f32_16x16x4f32(kf[kt][u], qf[u], s[kt], 0, 0, 0);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                if ((dead_keys[kt] >> (4 * grp + r)) & 1u) s[kt][r] = -INFINITY;
                m = fmaxf(m, s[kt][r]);
            }
        }
        m = fmaxf(m, __shfl_xor(m, 16, 64));
        m = fmaxf(m, __shfl_xor(m, 32, 64));                           // finite: slot 0 of a set is never dead
        float l = 0.0f;
#pragma unroll
        for (int kt = 0; kt < NT; ++kt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                s[kt][r] = exp2f((s[kt][r] - m) * a.c);
                l += s[kt][r];
            }
        l += __shfl_xor(l, 16, 64);
        l += __shfl_xor(l, 32, 64);
        f4 acc[VT][2];
#pragma unroll
        for (int u = 0; u < VT; ++u) { acc[u][0] = f4{0, 0, 0, 0}; acc[u][1] = f4{0, 0, 0, 0}; }
#pragma unroll
        for (int kt = 0; kt < NT; ++kt)
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int u = 0; u < VT; ++u)
                    acc[u][kt & 1] = __builtin_amdgcn_mfma_f32_16x16x4f32(vf[kt][u][r], s[kt][r], acc[u][kt & 1], 0, 0, 0);
        if (dead[qt]) continue;
        float *o = a.out + (size_t)row[qt] * a.C + h * D + 4 * grp;    // O^T: row = channel 4 grp + r, column = the query
#pragma unroll
        for (int u = 0; u < VT; ++u) {
            if (16 * u + 4 * grp >= D) continue;                       // d = 24: the upper half of the second tile
            const f4 x = (acc[u][0] + acc[u][1]) / l;
            store_quad(o + 16 * u, x, a.ovec);
        }
    }
}

static inline bool sa_supported(int S, int ss, int N, int C, int H) {
    if (S < 0 || N < 0 || ss < 1 || ss > 128 || C < 1 || C > 256 || H < 1 || C % H != 0) return false;
    const int d = C / H;
    return d == 16 || d == 24 || d == 32;
}
static inline bool sa_aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

template <int D>
static void sa_launch(int nt, dim3 grid, hipStream_t s, const SaArgs &a) {
    switch (nt) {
        case 1: hipLaunchKernelGGL((set_attention_kernel<D, 1>), grid, dim3(SA_T), 0, s, a); break;
        case 2: hipLaunchKernelGGL((set_attention_kernel<D, 2>), grid, dim3(SA_T), 0, s, a); break;
        case 3: hipLaunchKernelGGL((set_attention_kernel<D, 3>), grid, dim3(SA_T), 0, s, a); break;
        case 4: hipLaunchKernelGGL((set_attention_kernel<D, 4>), grid, dim3(SA_T), 0, s, a); break;
        case 5: case 6: hipLaunchKernelGGL((set_attention_kernel<D, 6>), grid, dim3(SA_T), 0, s, a); break;
        default: hipLaunchKernelGGL((set_attention_kernel<D, 8>), grid, dim3(SA_T), 0, s, a); break;
    }
}

}  // namespace pdm

using namespace pdm;

extern "C" size_t pdm_dsvt_partition_workspace_bytes(int N, int B, int sx, int sy, int sz, const int *windows) {
    DpArgs a{};
    if (!windows || !dp_sizes_ok(N, B, sx, sy, sz) || !dp_geometry(a, N, B, sx, sy, sz, windows, nullptr, 1)) return 0;
    return dp_workspace(a).total;
}

static int dp_check(const char *who, DpArgs &a, DpWorkspace &w, int N, const int *voxel_coords, int B, int sx, int sy, int sz,
                    const int *windows, const int *shifts, int set_size, void *workspace, size_t workspace_bytes) {
    PDM_REQUIRE(dp_sizes_ok(N, B, sx, sy, sz), PDM_E_BADARG, "%s: N = %d, B = %d, sparse shape (%d, %d, %d)", who, N, B, sx, sy, sz);
    PDM_REQUIRE(set_size >= 1 && set_size <= 0xffff, PDM_E_BADARG, "%s: set_size = %d, needs 1 .. 65535", who, set_size);
    PDM_REQUIRE(windows && shifts && workspace && (N == 0 || voxel_coords), PDM_E_BADARG, "%s: null pointer", who);
    PDM_REQUIRE(dp_geometry(a, N, B, sx, sy, sz, windows, shifts, set_size), PDM_E_BADARG,
                "%s: windows (%d, %d, %d), (%d, %d, %d): sizes >= 1, 0 <= shift <= window, at most 2^33 window cells a shift", who,
                windows[0], windows[1], windows[2], windows[3], windows[4], windows[5]);
    PDM_WS_ALIGNED(who, workspace);
    w = dp_workspace(a);
    PDM_REQUIRE(workspace_bytes >= w.total, PDM_E_BADARG, "%s: window volumes %d and %d need a workspace of %zu bytes, got %zu", who,
                a.sh[0].mv, a.sh[1].mv, w.total, workspace_bytes);
    return 0;
}

// Launches: zero, mark, three of the bitmap scan, three of the window scan; then the one host read.
extern "C" int pdm_dsvt_partition_count(void *stream, int N, const int *voxel_coords, int B, int sx, int sy, int sz, const int *windows,
                                        const int *shifts, int set_size, int *coors_in_win, int *set_counts, void *workspace,
                                        size_t workspace_bytes) {
    const char *who = "dsvt_partition_count";
    DpArgs a{};
    DpWorkspace w{};
    if (int rc = dp_check(who, a, w, N, voxel_coords, B, sx, sy, sz, windows, shifts, set_size, workspace, workspace_bytes)) return rc;
    PDM_REQUIRE(set_counts && (N == 0 || coors_in_win), PDM_E_BADARG, "%s: null pointer", who);
    char *ws = static_cast<char *>(workspace);
    int *record = reinterpret_cast<int *>(ws + w.record);
    const ScIndex ix = sc_index_at(ws + w.index, w.isz);
    int *wtiles = reinterpret_cast<int *>(ws + w.wtiles), *setbase = reinterpret_cast<int *>(ws + w.setbase);
    hipStream_t s = as_stream(stream);
    if (int rc = zero_fill(stream, who, record, 256 + w.isz.bits)) return rc;           // the record and the bitmap lie in a row
    if (N) {
        hipLaunchKernelGGL(dp_mark_kernel, dim3((unsigned)divup(N, SC_T)), dim3(SC_T), 0, s, a, voxel_coords, ix.bits, coors_in_win, record);
        if (int rc = check_launch(who)) return rc;
    }
    if (int rc = sc_index_scan(s, who, ix, record + 3, nullptr, nullptr)) return rc;
    hipLaunchKernelGGL(dp_win_total_kernel, dim3((unsigned)w.nwt), dim3(SC_T), 0, s, a, ix.bits, ix.gprefix, wtiles);
    if (int rc = check_launch(who)) return rc;
    hipLaunchKernelGGL(scan_totals_kernel<SC_T>, dim3(1), dim3(SC_T), 0, s, w.nwt, wtiles, record, 1, -1);
    if (int rc = check_launch(who)) return rc;
    hipLaunchKernelGGL(dp_win_fill_kernel, dim3((unsigned)w.nwt), dim3(SC_T), 0, s, a, ix.bits, ix.gprefix, wtiles, setbase, record);
    if (int rc = check_launch(who)) return rc;
    int host[DP_RECORD] = {0, 0, 0, 0};
    hipError_t e = hipMemcpyAsync(host, record, sizeof(host), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    PDM_REQUIRE(e == hipSuccess, (int)e, "%s: reading the set counts: %s", who, hipGetErrorString(e));
    PDM_REQUIRE(host[2] == 0, PDM_E_BADARG, "%s: a voxel coordinate outside the sparse shape (%d, %d, %d) of %d samples", who, sx, sy, sz, B);
    set_counts[0] = host[0];
    set_counts[1] = host[1] - host[0];
    return 0;
}

// One launch: every (voxel, shift, axis) writes its slots of set_voxel_inds (2, S, ss) int64 and of the masks (2, S, ss) bytes.
extern "C" int pdm_dsvt_partition(void *stream, int N, const int *voxel_coords, int B, int sx, int sy, int sz, const int *windows,
                                  const int *shifts, int set_size, int S0, int S1, long long *set_voxel_inds0, unsigned char *set_voxel_mask0,
                                  long long *set_voxel_inds1, unsigned char *set_voxel_mask1, void *workspace, size_t workspace_bytes) {
    const char *who = "dsvt_partition";
    DpArgs a{};
    DpWorkspace w{};
    if (int rc = dp_check(who, a, w, N, voxel_coords, B, sx, sy, sz, windows, shifts, set_size, workspace, workspace_bytes)) return rc;
    PDM_REQUIRE(S0 >= 0 && S1 >= 0 && (long long)S0 * set_size <= 0x3fffffffll && (long long)S1 * set_size <= 0x3fffffffll, PDM_E_TOOLARGE,
                "%s: %d and %d sets of %d", who, S0, S1, set_size);
    PDM_REQUIRE((S0 == 0 || (set_voxel_inds0 && set_voxel_mask0)) && (S1 == 0 || (set_voxel_inds1 && set_voxel_mask1)), PDM_E_BADARG,
                "%s: null pointer", who);
    if (N == 0) return 0;
    char *ws = static_cast<char *>(workspace);
    const ScIndex ix = sc_index_at(ws + w.index, w.isz);
    DpOut o{{set_voxel_inds0, set_voxel_inds1}, {set_voxel_mask0, set_voxel_mask1}, {S0, S1}};
    hipLaunchKernelGGL(dp_slots_kernel, dim3((unsigned)divup((long long)N * 4, SC_T)), dim3(SC_T), 0, as_stream(stream), a, voxel_coords, ix.bits,
                       ix.gprefix, reinterpret_cast<const int *>(ws + w.setbase), o);
    return check_launch(who);
}

extern "C" int pdm_set_attention(void *stream, int S, int set_size, int N, int C, int nheads, const float *q, long long q_stride,
                                 const float *k, long long k_stride, const float *v, long long v_stride, const long long *set_voxel_inds,
                                 float *out) {
    const char *who = "set_attention";
    PDM_REQUIRE(sa_supported(S, set_size, N, C, nheads), PDM_E_BADARG,
                "%s: S = %d, set_size = %d, N = %d, C = %d, heads = %d: needs 1 <= set_size <= 128, C <= 256 and C / heads in {16, 24, 32}", who,
                S, set_size, N, C, nheads);
    PDM_REQUIRE(q_stride >= C && k_stride >= C && v_stride >= C, PDM_E_BADARG, "%s: a row stride below C = %d", who, C);
    if (S == 0) return 0;
    PDM_REQUIRE(N >= 1, PDM_E_BADARG, "%s: %d sets over no rows", who, S);
    PDM_REQUIRE(q && k && v && set_voxel_inds && out, PDM_E_BADARG, "%s: null pointer", who);
    PDM_REQUIRE((reinterpret_cast<uintptr_t>(set_voxel_inds) & 7) == 0, PDM_E_BADARG, "%s: set_voxel_inds must be 8-byte aligned", who);
    const long long waves = (long long)S * nheads;
    PDM_REQUIRE(divup(waves, SA_T / 64) <= 0x7fffffffll && (long long)N * C <= 0x7fffffffll * 4ll, PDM_E_TOOLARGE, "%s: %lld (set, head) pairs", who, waves);
    SaArgs a{};
    a.S = S; a.ss = set_size; a.N = N; a.C = C; a.H = nheads;
    a.q = q; a.k = k; a.v = v; a.qs = q_stride; a.ks = k_stride; a.vs = v_stride;
    a.vec = sa_aligned16(q) && sa_aligned16(k) && q_stride % 4 == 0 && k_stride % 4 == 0;
    a.ovec = sa_aligned16(out);
    a.inds = set_voxel_inds;
    const int d = C / nheads, nt = divup(set_size, 16);
    a.c = (float)(1.4426950408889634 / sqrt((double)d));
    a.out = out;
    const dim3 grid((unsigned)divup(waves, SA_T / 64));
    hipStream_t s = as_stream(stream);
    if (d == 16) sa_launch<16>(nt, grid, s, a);
    else if (d == 24) sa_launch<24>(nt, grid, s, a);
    else sa_launch<32>(nt, grid, s, a);
    return check_launch(who);
}

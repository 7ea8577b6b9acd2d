// The occupancy index of a sparse grid (DESIGN.md "Voxel path"), shared by sparse_conv.hip (voxels, rulebooks, the site index
// operator) and roi_grid_pool.hip (the RoI-grid pooling reads it).  An occupancy BITMAP, one bit per cell in key order
//     key = ((b * W + x) * H + y) * D + z                        (64-bit; z innermost, x-major: torch.unique's order)
// with the number of set bits in front of every group of 256 cells (a multi-launch scan of the groups' popcounts).  The rank
// of a cell, prefix[group] + popcount(bits below it), is its number in ascending key order; row_of_rank[rank(key)] = row turns
// the bitmap into a lookup for rows that arrive in any order.
#pragma once
#include "common.h"

namespace pdm {

constexpr int SC_T = SCAN_T;               // threads per workgroup of every kernel here; a scan tile is SCAN_TILE groups
constexpr int SC_GW = 8;                   // 32-bit words per group: 256 cells
constexpr long long SC_MAXCELL = 1ll << 35;    // 2^30 words

// ---- the occupancy index ------------------------------------------------------------------------------------------
struct ScIndex {
    unsigned *bits;     // nwords, a multiple of SC_GW
    int *gprefix;       // ngroups: set bits in front of the group
    int *tiles;         // ntiles: scan scratch
    int nwords, ngroups, ntiles;
};
struct ScIndexSize {
    size_t bits, gprefix, tiles;    // bytes of each section, 256-byte multiples
    int nwords, ngroups, ntiles;
};
static ScIndexSize sc_index_size(long long ncell) {
    ScIndexSize z{};
    z.ngroups = (int)((ncell + 32 * SC_GW - 1) / (32 * SC_GW));
    z.nwords = z.ngroups * SC_GW;
    z.ntiles = divup(z.ngroups, SCAN_TILE);
    z.bits = align256(sizeof(unsigned) * (size_t)z.nwords);
    z.gprefix = align256(sizeof(int) * (size_t)z.ngroups);
    z.tiles = align256(sizeof(int) * (size_t)z.ntiles);
    return z;
}
static ScIndex sc_index_at(char *base, const ScIndexSize &z) {
    return ScIndex{reinterpret_cast<unsigned *>(base), reinterpret_cast<int *>(base + z.bits),
                   reinterpret_cast<int *>(base + z.bits + z.gprefix), z.nwords, z.ngroups, z.ntiles};
}

__device__ __forceinline__ int sc_group_pop(const unsigned *__restrict__ bits, int g) {
    const uint2 *p = reinterpret_cast<const uint2 *>(bits) + 4 * (size_t)g;      // a workspace is 8-byte aligned, no more
    int n = 0;
#pragma unroll
    for (int q = 0; q < SC_GW / 2; ++q) n += __popc(p[q].x) + __popc(p[q].y);
    return n;
}
__device__ __forceinline__ bool sc_test(const unsigned *__restrict__ bits, long long key) {
    return (bits[key >> 5] >> (unsigned)(key & 31)) & 1u;
}
// number of set cells in front of `key`: the cell's number in ascending key order when its own bit is set
__device__ __forceinline__ int sc_rank(const unsigned *__restrict__ bits, const int *__restrict__ gprefix, long long key) {
    const int w = (int)(key >> 5), g = w / SC_GW;
    int r = gprefix[g];
    for (int q = g * SC_GW; q < w; ++q) r += __popc(bits[q]);
    return r + __popc(bits[w] & ((1u << (unsigned)(key & 31)) - 1u));
}
__device__ __forceinline__ void sc_set(unsigned *__restrict__ bits, long long key) {
    atomicOr(&bits[key >> 5], 1u << (unsigned)(key & 31));
}

// set cells of every tile of groups
static __global__ __launch_bounds__(SC_T) void sc_tile_total_kernel(int ngroups, const unsigned *__restrict__ bits, int *__restrict__ tiles) {
    tile_reduce<SC_T, SCAN_ITEMS>(ngroups, {tiles}, [&](long long g, int *sum) { sum[0] += sc_group_pop(bits, (int)g); });
}

// workgroup w scans array w (two arrays at most) and leaves its total in slot w
static __global__ __launch_bounds__(SC_T) void sc_scan_tiles_kernel(int n0, int *__restrict__ v0, int *__restrict__ slot0, int n1,
                                                                    int *__restrict__ v1, int *__restrict__ slot1) {
    __shared__ int s_wave[SC_T / 64];
    const int total = blockIdx.x == 0 ? scan_totals<SC_T>(n0, v0, s_wave) : scan_totals<SC_T>(n1, v1, s_wave);
    if (threadIdx.x == 0) *(blockIdx.x == 0 ? slot0 : slot1) = total;
}

static __global__ __launch_bounds__(SC_T) void sc_group_fill_kernel(int ngroups, const unsigned *__restrict__ bits, const int *__restrict__ tiles,
                                                                    int *__restrict__ gprefix) {
    tile_scan<SC_T, SCAN_ITEMS>(ngroups, {tiles[blockIdx.x]}, [&](long long g, int *v) { v[0] = sc_group_pop(bits, (int)g); },
                                [&](long long g, const int *at) { gprefix[g] = at[0]; });
}

// the scan of one or two indices: tile totals, one scan launch, group prefixes
static int sc_index_scan(hipStream_t s, const char *who, const ScIndex &a, int *slot_a, const ScIndex *b, int *slot_b) {
    const ScIndex *both[2] = {&a, b};
    for (int i = 0; i < 2; ++i)
        if (both[i] && both[i]->ntiles) {
            hipLaunchKernelGGL(sc_tile_total_kernel, dim3((unsigned)both[i]->ntiles), dim3(SC_T), 0, s, both[i]->ngroups, both[i]->bits, both[i]->tiles);
            if (int rc = check_launch(who)) return rc;
        }
    hipLaunchKernelGGL(sc_scan_tiles_kernel, dim3(b ? 2 : 1), dim3(SC_T), 0, s, a.ntiles, a.tiles, slot_a, b ? b->ntiles : 0,
                       b ? b->tiles : nullptr, slot_b);
    if (int rc = check_launch(who)) return rc;
    for (int i = 0; i < 2; ++i)
        if (both[i] && both[i]->ntiles) {
            hipLaunchKernelGGL(sc_group_fill_kernel, dim3((unsigned)both[i]->ntiles), dim3(SC_T), 0, s, both[i]->ngroups, both[i]->bits, both[i]->tiles,
                               both[i]->gprefix);
            if (int rc = check_launch(who)) return rc;
        }
    return 0;
}

// ---- rows (b, z, y, x) on a grid (B, D, H, W) ---------------------------------------------------------------------------
__device__ __forceinline__ long long rb_key(int b, int z, int y, int x, int D, int H, int W) {
    return (((long long)b * W + x) * H + y) * D + z;
}
__device__ __forceinline__ bool rb_inside(const int *c, int B, int D, int H, int W) {
    return c[0] >= 0 && c[0] < B && c[1] >= 0 && c[1] < D && c[2] >= 0 && c[2] < H && c[3] >= 0 && c[3] < W;
}

// ---- the site index as an object of its own (pdm_sparse_index): the index of the grid, row_of_rank (P), one scan slot -----
struct SiWorkspace {
    size_t index, row_of_rank, slot, total;
    ScIndexSize isz;
};
static bool si_grid_ok(int B, int D, int H, int W) {
    return B >= 0 && D >= 1 && H >= 1 && W >= 1 && (long long)H * W <= 0x7fffffffll && (long long)D * H * W <= SC_MAXCELL &&
           (long long)B * D * H * W <= SC_MAXCELL;
}
static SiWorkspace si_workspace(long long P, int B, int D, int H, int W) {
    SiWorkspace w{};
    w.isz = sc_index_size((long long)B * D * H * W);
    size_t at = 0;
    w.index = at; at += w.isz.bits + w.isz.gprefix + w.isz.tiles;
    w.row_of_rank = at; at += align256(sizeof(int) * (size_t)P);
    w.slot = at; at += 256;
    w.total = at;
    return w;
}

}  // namespace pdm

// What the point-to-cell front ends share (pillar.hip, sparse_conv.hip, hard_voxel.hip): the grid, the cell key of a point row
// and its inverse, the 2^20 fixed-point sums with their mean, and the host-side checks of a grid's size.  The tiled scan
// passes they run over rows and cells are common.h's tile_reduce / tile_scan.
#pragma once
#include "common.h"

namespace pdm {

constexpr double FIXED20 = 1048576.0;      // 2^20: one step of the fixed-point sums is about a micrometre

struct VoxelGrid {                         // pillars: nz = 1, the z fields unused
    int B, nx, ny, nz;
    float x0, y0, z0, vx, vy, vz;
};

// key = ((b * nx + cx) * ny + cy) * nz + cz of the row's cell (z innermost, x-major: torch.unique's order of the reference's
// merged coordinates), or -1 when the row is dropped: outside on an axis (z only with TEST_Z; without it the key has no z
// term), a sample index outside [0, B), NaN
template <bool TEST_Z>
__device__ __forceinline__ long long voxel_key(const float *__restrict__ row, const VoxelGrid &g) {
    const float bf = row[0];
    if (!(bf >= 0.0f && bf < (float)g.B)) return -1;
    const int cx = cell_1d(row[1], g.x0, g.vx, g.nx), cy = cell_1d(row[2], g.y0, g.vy, g.ny), cz = TEST_Z ? cell_1d(row[3], g.z0, g.vz, g.nz) : 0;
    if (cx < 0 || cy < 0 || cz < 0) return -1;
    const long long plane = ((long long)(int)bf * g.nx + cx) * g.ny + cy;
    return TEST_Z ? plane * g.nz + cz : plane;
}

// the inverse: c = (b, z, y, x), a row of voxel_coords.  K is the key's own width (the pillars' keys are ints).
template <class K>
__device__ __forceinline__ void voxel_key_coords(K key, int nx, int ny, int nz, int *c) {
    c[1] = (int)(key % nz); key /= nz;
    c[2] = (int)(key % ny); key /= ny;
    c[0] = (int)(key / nx); c[3] = (int)(key % nx);
}

// sums are 64-bit fixed point, llrint(v * 2^20), added with integer atomics, which commute: no float atomics.
// Two's complement: the unsigned add is the signed one.
__device__ __forceinline__ void fixed20_add(unsigned long long *sum, float v) {
    atomicAdd(sum, (unsigned long long)llrint((double)v * FIXED20));
}
__device__ __forceinline__ float fixed20_mean(long long sum, int count) {
    return (float)((double)sum * (1.0 / FIXED20) / (double)count);
}
// sums (P, C), count (P) -> mean (P, C) with P = record[1]: launched at capacity, the count of cells is read on the device
static __global__ __launch_bounds__(SCAN_T) void fixed20_mean_kernel(const int *__restrict__ record, int C, const long long *__restrict__ sums,
                                                                   const int *__restrict__ count, float *__restrict__ mean) {
    const long long t = (long long)blockIdx.x * SCAN_T + threadIdx.x;
    if (t >= (long long)record[1] * C) return;
    mean[t] = fixed20_mean(sums[t], count[t / C]);
}

// sizes non-negative, a plane of nx ny cells within int32, a sample's cells and the grid's within max_cells: what the
// *_workspace_bytes functions ask before they size anything
static bool voxel_grid_cells_ok(int B, int nx, int ny, int nz, long long max_cells) {
    return B >= 0 && nx >= 1 && ny >= 1 && nz >= 1 && (long long)nx * ny <= 0x7fffffffll && (long long)nx * ny * nz <= max_cells &&
           (long long)B * nx * ny * nz <= max_cells;
}
// the same for an entry point, with the rows: too_many is the operator's own wording of the cell limit
static int voxel_grid_check(const char *who, long long N, int C1, int B, int nx, int ny, int nz, long long max_cells, const char *too_many) {
    PDM_REQUIRE(N >= 0 && B >= 0 && nx >= 1 && ny >= 1 && nz >= 1 && C1 >= 4, PDM_E_BADARG, "%s: bad size", who);
    PDM_REQUIRE(voxel_grid_cells_ok(B, nx, ny, nz, max_cells), PDM_E_TOOLARGE, "%s: %s", who, too_many);
    PDM_REQUIRE(N * C1 <= 0x7fffffffll, PDM_E_TOOLARGE, "%s: %lld point elements exceed int32", who, N * C1);
    return 0;
}

}  // namespace pdm

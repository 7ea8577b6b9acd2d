// The pillar front end (DESIGN.md "Pillar path"): points -> dynamic pillars, per-point pillar features, the per-pillar max
// with its winner, the fused single-layer PFN of eval mode, and the BEV canvas scatter with its gather backward.
//
// count -> scan -> fill, no host loop, no float atomics: every result is a function of the input alone.
//   * a cell's key is b * nx * ny + cx * ny + cy (x-major: torch.unique's order of the reference's merge_coords), and the
//     pillar ids are the exclusive scan of the cells' occupancy in key order;
//   * the scans are multi-launch (tile totals, one workgroup over the totals, tiles again): no workgroup waits for another;
//   * xyz sums are 64-bit fixed point (voxel_grid.h), added with integer atomics, which commute;
//   * the rows of a pillar are listed in a CSR whose slot order is arbitrary (an integer atomic cursor): the only readers
//     take a max with ties to the lower row, or an integer sum, neither of which depends on the order.
#include "pillar_feat.h"
#include "voxel_grid.h"

namespace pdm {

constexpr int PL_T = SCAN_T;               // threads per workgroup of every kernel here; a scan tile is SCAN_TILE items

// ---- a. assign ----------------------------------------------------------------------------------------------------
// rows -> cell keys (voxel_grid.h on the nz = 1 grid, z not tested; the host bounds the cells, and so the keys, by int32),
// per-cell counts (integer atomics) and the kept rows of every tile
__global__ __launch_bounds__(PL_T) void pl_key_kernel(int N, int C1, const float *__restrict__ points, VoxelGrid g, int *__restrict__ point_key,
                                                      int *__restrict__ cell_count, int *__restrict__ ptile) {
    tile_reduce<PL_T, SCAN_ITEMS>(N, {ptile}, [&](long long i, int *kept) {
        const int key = (int)voxel_key<false>(points + (size_t)i * C1, g);
        point_key[i] = key;
        if (key >= 0) {
            atomicAdd(&cell_count[key], 1);
            ++kept[0];
        }
    });
}

// per tile of cells: how many are occupied and how many rows they hold
__global__ __launch_bounds__(PL_T) void pl_cell_total_kernel(int ncell, const int *__restrict__ cell_count, int *__restrict__ ctile_occ,
                                                             int *__restrict__ ctile_cnt) {
    tile_reduce<PL_T, SCAN_ITEMS>(ncell, {ctile_occ, ctile_cnt}, [&](long long c, int *sum) {
        const int n = cell_count[c];
        sum[0] += n > 0;
        sum[1] += n;
    });
}

// workgroup 0: the point tiles -> record[0] = N'; workgroup 1: the cell tiles -> record[1] = P, seg_start[P] = N'
__global__ __launch_bounds__(PL_T) void pl_scan_totals_kernel(int ntp, int *__restrict__ ptile, int ntc, int *__restrict__ ctile_occ,
                                                              int *__restrict__ ctile_cnt, int *__restrict__ record, int *__restrict__ seg_start) {
    __shared__ int s_wave[PL_T / 64];
    if (blockIdx.x == 0) {
        const int kept = scan_totals<PL_T>(ntp, ptile, s_wave);
        if (threadIdx.x == 0) record[0] = kept;
    } else {
        const int P = scan_totals<PL_T>(ntc, ctile_occ, s_wave);
        const int kept = scan_totals<PL_T>(ntc, ctile_cnt, s_wave);
        if (threadIdx.x == 0) { record[1] = P; seg_start[P] = kept; }
    }
}

// every cell: its pillar id (or -1), and per pillar its coordinates, count, first CSR slot, a cleared cursor and cleared sums
__global__ __launch_bounds__(PL_T) void pl_cell_fill_kernel(int ncell, VoxelGrid g, const int *__restrict__ cell_count, const int *__restrict__ ctile_occ,
                                                            const int *__restrict__ ctile_cnt, int *__restrict__ cell_table,
                                                            int *__restrict__ voxel_coords, int *__restrict__ pillar_count, int *__restrict__ seg_start,
                                                            int *__restrict__ cursor, long long *__restrict__ sums) {
    int n;
    tile_scan<PL_T, SCAN_ITEMS>(ncell, {ctile_occ[blockIdx.x], ctile_cnt[blockIdx.x]}, [&](long long c, int *v) {
        n = cell_count[c];
        v[0] = n > 0;
        v[1] = n;
    }, [&](long long c, const int *at) {
        const int pid = at[0];
        cell_table[c] = n > 0 ? pid : -1;
        if (n > 0) {
            voxel_key_coords((int)c, g.nx, g.ny, 1, voxel_coords + (size_t)pid * 4);
            pillar_count[pid] = n;
            seg_start[pid] = at[1];
            cursor[pid] = 0;
            sums[(size_t)pid * 3] = 0; sums[(size_t)pid * 3 + 1] = 0; sums[(size_t)pid * 3 + 2] = 0;
        }
    });
}

// every kept row: its place in input order, its pillar, a CSR slot, and its xyz added to the pillar's fixed-point sums
__global__ __launch_bounds__(PL_T) void pl_point_fill_kernel(int N, int C1, const float *__restrict__ points, const int *__restrict__ point_key,
                                                             const int *__restrict__ ptile, const int *__restrict__ cell_table,
                                                             const int *__restrict__ seg_start, int *__restrict__ cursor,
                                                             unsigned long long *__restrict__ sums, int *__restrict__ kept_idx,
                                                             int *__restrict__ unq_inv, int *__restrict__ seg_rows) {
    int key;
    tile_scan<PL_T, SCAN_ITEMS>(N, {ptile[blockIdx.x]}, [&](long long i, int *v) { key = point_key[i]; v[0] = key >= 0; },
                                [&](long long i, const int *at) {
        if (key < 0) return;
        const int row = at[0], pid = cell_table[key];
        kept_idx[row] = (int)i;
        unq_inv[row] = pid;
        seg_rows[seg_start[pid] + atomicAdd(&cursor[pid], 1)] = row;
        const float *p = points + (size_t)i * C1;
        for (int d = 0; d < 3; ++d) fixed20_add(&sums[(size_t)pid * 3 + d], p[1 + d]);
    });
}

// ---- b. features ----------------------------------------------------------------------------------------------------
// PlFeat, pl_derived and the PFN channel: pillar_feat.h (shared with hard_voxel.hip)
__global__ __launch_bounds__(PL_T) void pl_features_kernel(int n_kept, PlFeat a, const float *__restrict__ points, const int *__restrict__ kept_idx,
                                                           const int *__restrict__ unq_inv, const int *__restrict__ voxel_coords,
                                                           const float *__restrict__ pillar_mean, float *__restrict__ out) {
    const long long r = (long long)blockIdx.x * PL_T + threadIdx.x;
    if (r >= n_kept) return;
    const int pid = unq_inv[r];
    const float *p = points + (size_t)kept_idx[r] * a.C1;
    float *o = out + (size_t)r * a.F;
    const int first = a.abs_xyz ? 1 : 4, nraw = a.C1 - first;
    for (int c = 0; c < nraw; ++c) o[c] = p[first + c];
    float d[7];
    pl_derived(a, p, pillar_mean + (size_t)pid * 3, voxel_coords + (size_t)pid * 4, d);
#pragma unroll
    for (int j = 0; j < 7; ++j)
        if (j < 6 || a.with_dist) o[nraw + j] = d[j];
}

// ---- c. segment max ---------------------------------------------------------------------------------------------------
// thread = (pillar, channel), channels fastest; ties go to the lower row whatever the slot order
__global__ __launch_bounds__(PL_T) void pl_segment_max_kernel(long long total, int K, const float *__restrict__ x, const int *__restrict__ seg_start,
                                                              const int *__restrict__ seg_rows, float *__restrict__ x_max, int *__restrict__ arg) {
    const long long t = (long long)blockIdx.x * PL_T + threadIdx.x;
    if (t >= total) return;
    const int p = (int)(t / K), k = (int)(t % K);
    const int lo = seg_start[p], hi = seg_start[p + 1];
    float best = 0.0f;
    int brow = -1;
    for (int s = lo; s < hi; ++s) {
        const int row = seg_rows[s];
        const float v = x[(size_t)row * K + k];
        if (brow < 0 || v > best || (v == best && row < brow)) { best = v; brow = row; }
    }
    x_max[t] = best;
    arg[t] = brow;
}

// thread = (row, channel): the pillar's gradient if this row won, else zero; every element written, no atomics
__global__ __launch_bounds__(PL_T) void pl_segment_max_grad_kernel(long long total, int K, const float *__restrict__ grad_max, const int *__restrict__ arg,
                                                                   const int *__restrict__ unq_inv, float *__restrict__ grad_x) {
    const long long t = (long long)blockIdx.x * PL_T + threadIdx.x;
    if (t >= total) return;
    const int row = (int)(t / K), k = (int)(t % K);
    const size_t at = (size_t)unq_inv[row] * K + k;
    grad_x[t] = arg[at] == row ? grad_max[at] : 0.0f;
}

// ---- d. fused eval PFN ------------------------------------------------------------------------------------------------
// thread = (pillar, channel): features of each row of the pillar -> dot with the channel's weights -> scale, shift, ReLU ->
// running max in a register.  The (N', K) activations are never stored.
__global__ __launch_bounds__(PL_T) void pl_fused_pfn_kernel(long long total, int K, PlFeat a, const float *__restrict__ points,
                                                            const int *__restrict__ kept_idx, const int *__restrict__ voxel_coords,
                                                            const float *__restrict__ pillar_mean, const int *__restrict__ seg_start,
                                                            const int *__restrict__ seg_rows, const float *__restrict__ weight,
                                                            const float *__restrict__ scale, const float *__restrict__ shift, float *__restrict__ out) {
    const long long t = (long long)blockIdx.x * PL_T + threadIdx.x;
    if (t >= total) return;
    const int p = (int)(t / K), k = (int)(t % K);
    PlChannel w;
    pl_channel_load(a, k, weight, scale, shift, w);
    const float *mean = pillar_mean + (size_t)p * 3;
    const int *vc = voxel_coords + (size_t)p * 4;
    float best = 0.0f;                     // after the ReLU nothing is below zero, and no pillar is empty
    for (int s = seg_start[p]; s < seg_start[p + 1]; ++s) {
        const float y = pl_channel_row(a, w, points + (size_t)kept_idx[seg_rows[s]] * a.C1, mean, vc);
        best = (y > best || y != y) ? y : best;        // a NaN stays, as torch's amax keeps it
    }
    out[t] = best;
}

// ---- e. scatter -------------------------------------------------------------------------------------------------------
constexpr int PL_SX = 64, PL_SY = 16;      // cells of one scatter workgroup: 64 along x (one wave's store) by 16 along y

// cell table from voxel_coords (b, 0, cy, cx) for a caller that has none; rows outside the grid are skipped
__global__ __launch_bounds__(PL_T) void pl_table_fill_kernel(long long ncell, int *__restrict__ cell_table) {
    const long long c = (long long)blockIdx.x * PL_T + threadIdx.x;
    if (c < ncell) cell_table[c] = -1;
}
__global__ __launch_bounds__(PL_T) void pl_table_set_kernel(int P, int B, int nx, int ny, const int *__restrict__ voxel_coords,
                                                            int *__restrict__ cell_table) {
    const long long p = (long long)blockIdx.x * PL_T + threadIdx.x;
    if (p >= P) return;
    const int *vc = voxel_coords + (size_t)p * 4;
    const int b = vc[0], cy = vc[2], cx = vc[3];
    if (b < 0 || b >= B || cy < 0 || cy >= ny || cx < 0 || cx >= nx) return;
    cell_table[((size_t)b * nx + cx) * ny + cy] = (int)p;
}

// One pass writes the whole (B, C, ny, nx) canvas, zeros included.  The table is x-major (cy fastest), the canvas y-major
// (x fastest): a 64 x 16 tile of pillar ids goes through LDS so that both the table reads and the canvas stores coalesce.
__global__ __launch_bounds__(PL_T) void pl_scatter_kernel(int P, int C, int nx, int ny, const float *__restrict__ feat, const int *__restrict__ cell_table,
                                                          float *__restrict__ out) {
    __shared__ int s_pid[PL_SY][PL_SX + 1];
    const int b = blockIdx.z, x_base = blockIdx.x * PL_SX, y_base = blockIdx.y * PL_SY;
    for (int q = threadIdx.x; q < PL_SX * PL_SY; q += PL_T) {
        const int ly = q % PL_SY, lx = q / PL_SY;
        const int x = x_base + lx, y = y_base + ly;
        int pid = -1;
        if (x < nx && y < ny) pid = cell_table[((size_t)b * nx + x) * ny + y];
        s_pid[ly][lx] = (pid >= 0 && pid < P) ? pid : -1;
    }
    __syncthreads();
    const int lx = threadIdx.x % PL_SX, x = x_base + lx;
    if (x >= nx) return;
    constexpr int ROWS = PL_SY / (PL_T / PL_SX);
    int pid[ROWS];
    for (int r = 0; r < ROWS; ++r) pid[r] = s_pid[(threadIdx.x / PL_SX) * ROWS + r][lx];
    for (int c = 0; c < C; ++c) {
        for (int r = 0; r < ROWS; ++r) {
            const int y = y_base + (threadIdx.x / PL_SX) * ROWS + r;
            if (y >= ny) break;
            out[(((size_t)b * C + c) * ny + y) * nx + x] = pid[r] >= 0 ? feat[(size_t)pid[r] * C + c] : 0.0f;
        }
    }
}

// thread = (pillar, channel): the canvas gradient at the pillar's cell; rows outside the grid get zero
__global__ __launch_bounds__(PL_T) void pl_scatter_grad_kernel(long long total, int B, int C, int nx, int ny, const float *__restrict__ grad_out,
                                                               const int *__restrict__ voxel_coords, float *__restrict__ grad_feat) {
    const long long t = (long long)blockIdx.x * PL_T + threadIdx.x;
    if (t >= total) return;
    const int p = (int)(t / C), c = (int)(t % C);
    const int *vc = voxel_coords + (size_t)p * 4;
    const int b = vc[0], cy = vc[2], cx = vc[3];
    const bool in = b >= 0 && b < B && cy >= 0 && cy < ny && cx >= 0 && cx < nx;
    grad_feat[t] = in ? grad_out[(((size_t)b * C + c) * ny + cy) * nx + cx] : 0.0f;
}

// workspace of pdm_pillar_assign, every section 256-byte aligned
struct PlWorkspace {
    size_t point_key, cell_count, ptile, ctile_occ, ctile_cnt, cursor, sums, total;
};
static long long pl_capacity(long long N, long long ncell) { return N < ncell ? N : ncell; }
static PlWorkspace pl_workspace(long long N, long long ncell) {
    const size_t ntp = (size_t)divup(N, SCAN_TILE), ntc = (size_t)divup(ncell, SCAN_TILE), cap = (size_t)pl_capacity(N, ncell);
    PlWorkspace w{};
    size_t at = 0;
    w.point_key = at; at += align256(sizeof(int) * (size_t)N);
    w.cell_count = at; at += align256(sizeof(int) * (size_t)ncell);
    w.ptile = at; at += align256(sizeof(int) * ntp);
    w.ctile_occ = at; at += align256(sizeof(int) * ntc);
    w.ctile_cnt = at; at += align256(sizeof(int) * ntc);
    w.cursor = at; at += align256(sizeof(int) * cap);
    w.sums = at; at += align256(sizeof(long long) * 3 * cap);
    w.total = at;
    return w;
}

static int pl_check_grid(const char *who, long long N, int C1, int B, int nx, int ny, int nz) {
    PDM_REQUIRE(nz == 1, PDM_E_BADARG, "%s: a pillar grid has nz = 1 (got %d)", who, nz);
    PDM_REQUIRE(N >= 0 && B >= 0 && nx >= 1 && ny >= 1 && C1 >= 4, PDM_E_BADARG, "%s: bad size", who);
    PDM_REQUIRE((long long)B * nx * ny <= 0x7fffffffll, PDM_E_TOOLARGE, "%s: %lld cells exceed int32", who, (long long)B * nx * ny);
    PDM_REQUIRE(N * C1 <= 0x7fffffffll, PDM_E_TOOLARGE, "%s: %lld point elements exceed int32", who, N * C1);
    return 0;
}

}  // namespace pdm

using namespace pdm;

extern "C" size_t pdm_pillar_assign_workspace_bytes(int N, int B, int nx, int ny) {
    if (N < 0 || !voxel_grid_cells_ok(B, nx, ny, 1, 0x7fffffffll)) return 0;
    return pl_workspace(N, (long long)B * nx * ny).total;
}

// points (N, C1) fp32 rows (batch_idx, x, y, z, ...), any row order, any 4-byte alignment.  Outputs at capacity: kept_idx,
// unq_inv, seg_rows (N); voxel_coords (cap, 4), pillar_count (cap), pillar_mean (cap, 3), seg_start (cap + 1) with cap =
// min(N, B nx ny); cell_table (B nx ny); record (2) = {N', P}.  Only the first N' / P entries are written.
extern "C" int pdm_pillar_assign(void *stream, int N, int C1, const float *points, int B, int nx, int ny, int nz, float x0, float y0,
                                 float vx, float vy, int *kept_idx, int *unq_inv, int *voxel_coords, int *pillar_count,
                                 float *pillar_mean, int *cell_table, int *seg_start, int *seg_rows, int *record, void *workspace,
                                 size_t workspace_bytes) {
    if (int rc = pl_check_grid("pillar_assign", N, C1, B, nx, ny, nz)) return rc;
    PDM_REQUIRE(vx > 0.0f && vy > 0.0f, PDM_E_BADARG, "pillar_assign: voxel size must be positive");
    PDM_REQUIRE(record && seg_start, PDM_E_BADARG, "pillar_assign: null pointer");
    const long long ncell = (long long)B * nx * ny;
    PDM_REQUIRE(N == 0 || (points && kept_idx && unq_inv && seg_rows), PDM_E_BADARG, "pillar_assign: null pointer");
    PDM_REQUIRE(ncell == 0 || cell_table, PDM_E_BADARG, "pillar_assign: null pointer");
    PDM_REQUIRE(pl_capacity(N, ncell) == 0 || (voxel_coords && pillar_count && pillar_mean), PDM_E_BADARG, "pillar_assign: null pointer");
    const PlWorkspace w = pl_workspace(N, ncell);
    PDM_REQUIRE(w.total == 0 || workspace, PDM_E_BADARG, "pillar_assign: null pointer");
    PDM_WS_ALIGNED("pillar_assign", workspace);
    PDM_REQUIRE(workspace_bytes >= w.total, PDM_E_BADARG, "pillar_assign: workspace too small (%zu bytes, need %zu)", workspace_bytes, w.total);
    char *ws = static_cast<char *>(workspace);
    int *point_key = reinterpret_cast<int *>(ws + w.point_key), *cell_count = reinterpret_cast<int *>(ws + w.cell_count);
    int *ptile = reinterpret_cast<int *>(ws + w.ptile), *ctile_occ = reinterpret_cast<int *>(ws + w.ctile_occ);
    int *ctile_cnt = reinterpret_cast<int *>(ws + w.ctile_cnt), *cursor = reinterpret_cast<int *>(ws + w.cursor);
    long long *sums = reinterpret_cast<long long *>(ws + w.sums);
    const VoxelGrid g{B, nx, ny, 1, x0, y0, 0.0f, vx, vy, 1.0f};
    const int ntp = divup(N, SCAN_TILE), ntc = divup(ncell, SCAN_TILE);
    hipStream_t s = as_stream(stream);
    if (int rc = zero_fill(stream, "pillar_assign(zero)", cell_count, sizeof(int) * (size_t)ncell)) return rc;
    if (ntp) {
        hipLaunchKernelGGL(pl_key_kernel, dim3((unsigned)ntp), dim3(PL_T), 0, s, N, C1, points, g, point_key, cell_count, ptile);
        if (int rc = check_launch("pillar_assign(keys)")) return rc;
    }
    if (ntc) {
        hipLaunchKernelGGL(pl_cell_total_kernel, dim3((unsigned)ntc), dim3(PL_T), 0, s, (int)ncell, cell_count, ctile_occ, ctile_cnt);
        if (int rc = check_launch("pillar_assign(cell totals)")) return rc;
    }
    hipLaunchKernelGGL(pl_scan_totals_kernel, dim3(2), dim3(PL_T), 0, s, ntp, ptile, ntc, ctile_occ, ctile_cnt, record, seg_start);
    if (int rc = check_launch("pillar_assign(scan)")) return rc;
    if (ntc) {
        hipLaunchKernelGGL(pl_cell_fill_kernel, dim3((unsigned)ntc), dim3(PL_T), 0, s, (int)ncell, g, cell_count, ctile_occ, ctile_cnt,
                           cell_table, voxel_coords, pillar_count, seg_start, cursor, sums);
        if (int rc = check_launch("pillar_assign(cells)")) return rc;
    }
    if (ntp && ntc) {
        hipLaunchKernelGGL(pl_point_fill_kernel, dim3((unsigned)ntp), dim3(PL_T), 0, s, N, C1, points, point_key, ptile, cell_table,
                           seg_start, cursor, reinterpret_cast<unsigned long long *>(sums), kept_idx, unq_inv, seg_rows);
        if (int rc = check_launch("pillar_assign(points)")) return rc;
        const long long cap3 = 3 * pl_capacity(N, ncell);
        hipLaunchKernelGGL(fixed20_mean_kernel, dim3((unsigned)divup(cap3, SCAN_T)), dim3(SCAN_T), 0, s, record, 3, sums, pillar_count, pillar_mean);
        if (int rc = check_launch("pillar_assign(mean)")) return rc;
    }
    return 0;
}

// out (n_kept, F): F = (abs_xyz ? C1 - 1 : C1 - 4) + 6 + (with_dist ? 1 : 0) columns in the reference's order
extern "C" int pdm_pillar_features(void *stream, int n_kept, int C1, const float *points, const int *kept_idx, const int *unq_inv,
                                   const int *voxel_coords, const float *pillar_mean, int abs_xyz, int with_dist, float vx, float vy,
                                   float xoff, float yoff, float zoff, float *out) {
    PlFeat a;
    if (int rc = pl_feat_args("pillar_features", &a, C1, abs_xyz, with_dist, vx, vy, xoff, yoff, zoff)) return rc;
    PDM_REQUIRE(n_kept >= 0, PDM_E_BADARG, "pillar_features: bad size");
    if (n_kept == 0) return 0;
    PDM_REQUIRE(points && kept_idx && unq_inv && voxel_coords && pillar_mean && out, PDM_E_BADARG, "pillar_features: null pointer");
    hipLaunchKernelGGL(pl_features_kernel, dim3((unsigned)divup(n_kept, PL_T)), dim3(PL_T), 0, as_stream(stream), n_kept, a, points, kept_idx,
                       unq_inv, voxel_coords, pillar_mean, out);
    return check_launch("pillar_features");
}

// x (n_kept, K), the CSR of pdm_pillar_assign -> x_max (P, K), arg (P, K) the winning row, ties to the lower row
extern "C" int pdm_pillar_segment_max(void *stream, int P, int K, const float *x, const int *seg_start, const int *seg_rows, float *x_max,
                                      int *arg) {
    PDM_REQUIRE(P >= 0 && K >= 1, PDM_E_BADARG, "pillar_segment_max: bad size");
    if (P == 0) return 0;
    PDM_REQUIRE(x && seg_start && seg_rows && x_max && arg, PDM_E_BADARG, "pillar_segment_max: null pointer");
    const long long total = (long long)P * K;
    PDM_REQUIRE(total <= 0x7fffffffll * PL_T, PDM_E_TOOLARGE, "pillar_segment_max: %lld outputs", total);
    hipLaunchKernelGGL(pl_segment_max_kernel, dim3((unsigned)divup(total, PL_T)), dim3(PL_T), 0, as_stream(stream), total, K, x, seg_start,
                       seg_rows, x_max, arg);
    return check_launch("pillar_segment_max");
}

// grad_max (P, K), arg (P, K), unq_inv (n_kept) -> grad_x (n_kept, K), every element written
extern "C" int pdm_pillar_segment_max_grad(void *stream, int n_kept, int K, const float *grad_max, const int *arg, const int *unq_inv,
                                           float *grad_x) {
    PDM_REQUIRE(n_kept >= 0 && K >= 1, PDM_E_BADARG, "pillar_segment_max_grad: bad size");
    if (n_kept == 0) return 0;
    PDM_REQUIRE(grad_max && arg && unq_inv && grad_x, PDM_E_BADARG, "pillar_segment_max_grad: null pointer");
    const long long total = (long long)n_kept * K;
    PDM_REQUIRE(total <= 0x7fffffffll * PL_T, PDM_E_TOOLARGE, "pillar_segment_max_grad: %lld outputs", total);
    hipLaunchKernelGGL(pl_segment_max_grad_kernel, dim3((unsigned)divup(total, PL_T)), dim3(PL_T), 0, as_stream(stream), total, K, grad_max, arg,
                       unq_inv, grad_x);
    return check_launch("pillar_segment_max_grad");
}

// features -> weight (K, F) -> * scale (K) + shift (K) -> ReLU -> max per pillar: out (P, K).  F <= 16.
extern "C" int pdm_pillar_fused_pfn(void *stream, int P, int K, int C1, const float *points, const int *kept_idx, const int *voxel_coords,
                                    const float *pillar_mean, const int *seg_start, const int *seg_rows, int abs_xyz, int with_dist,
                                    float vx, float vy, float xoff, float yoff, float zoff, const float *weight, const float *scale,
                                    const float *shift, float *out) {
    PlFeat a;
    if (int rc = pl_feat_args("pillar_fused_pfn", &a, C1, abs_xyz, with_dist, vx, vy, xoff, yoff, zoff)) return rc;
    PDM_REQUIRE(a.F <= PL_MAXF, PDM_E_TOOLARGE, "pillar_fused_pfn: %d feature columns, at most %d", a.F, PL_MAXF);
    PDM_REQUIRE(P >= 0 && K >= 1, PDM_E_BADARG, "pillar_fused_pfn: bad size");
    if (P == 0) return 0;
    PDM_REQUIRE(points && kept_idx && voxel_coords && pillar_mean && seg_start && seg_rows && weight && scale && shift && out, PDM_E_BADARG,
                "pillar_fused_pfn: null pointer");
    const long long total = (long long)P * K;
    PDM_REQUIRE(total <= 0x7fffffffll * PL_T, PDM_E_TOOLARGE, "pillar_fused_pfn: %lld outputs", total);
    hipLaunchKernelGGL(pl_fused_pfn_kernel, dim3((unsigned)divup(total, PL_T)), dim3(PL_T), 0, as_stream(stream), total, K, a, points, kept_idx,
                       voxel_coords, pillar_mean, seg_start, seg_rows, weight, scale, shift, out);
    return check_launch("pillar_fused_pfn");
}

// voxel_coords (P, 4) int32 (b, 0, cy, cx) -> cell_table (B nx ny): pillar id or -1, every entry written
extern "C" int pdm_pillar_cell_table(void *stream, int P, const int *voxel_coords, int B, int nx, int ny, int nz, int *cell_table) {
    if (int rc = pl_check_grid("pillar_cell_table", 0, 4, B, nx, ny, nz)) return rc;
    PDM_REQUIRE(P >= 0, PDM_E_BADARG, "pillar_cell_table: bad size");
    const long long ncell = (long long)B * nx * ny;
    if (ncell == 0) return 0;
    PDM_REQUIRE(cell_table && (P == 0 || voxel_coords), PDM_E_BADARG, "pillar_cell_table: null pointer");
    hipLaunchKernelGGL(pl_table_fill_kernel, dim3((unsigned)divup(ncell, PL_T)), dim3(PL_T), 0, as_stream(stream), ncell, cell_table);
    if (int rc = check_launch("pillar_cell_table(fill)")) return rc;
    if (P == 0) return 0;
    hipLaunchKernelGGL(pl_table_set_kernel, dim3((unsigned)divup(P, PL_T)), dim3(PL_T), 0, as_stream(stream), P, B, nx, ny, voxel_coords,
                       cell_table);
    return check_launch("pillar_cell_table(set)");
}

// pillar_features (P, C), cell_table (B nx ny) -> canvas (B, C, ny, nx), every element written in one pass
extern "C" int pdm_pillar_scatter(void *stream, int P, int C, const float *pillar_features, const int *cell_table, int B, int nx, int ny,
                                  int nz, float *canvas) {
    if (int rc = pl_check_grid("pillar_scatter", 0, 4, B, nx, ny, nz)) return rc;
    PDM_REQUIRE(P >= 0 && C >= 1, PDM_E_BADARG, "pillar_scatter: bad size");
    PDM_REQUIRE(B <= 65535 && divup(ny, PL_SY) <= 65535, PDM_E_TOOLARGE, "pillar_scatter: B and ny / %d at most 65535", PL_SY);
    if (B == 0) return 0;
    PDM_REQUIRE(cell_table && canvas && (P == 0 || pillar_features), PDM_E_BADARG, "pillar_scatter: null pointer");
    hipLaunchKernelGGL(pl_scatter_kernel, dim3((unsigned)divup(nx, PL_SX), (unsigned)divup(ny, PL_SY), (unsigned)B), dim3(PL_T), 0,
                       as_stream(stream), P, C, nx, ny, pillar_features, cell_table, canvas);
    return check_launch("pillar_scatter");
}

// grad_canvas (B, C, ny, nx), voxel_coords (P, 4) -> grad_features (P, C): a gather at the pillar cells
extern "C" int pdm_pillar_scatter_grad(void *stream, int P, int C, const float *grad_canvas, const int *voxel_coords, int B, int nx, int ny,
                                       int nz, float *grad_features) {
    if (int rc = pl_check_grid("pillar_scatter_grad", 0, 4, B, nx, ny, nz)) return rc;
    PDM_REQUIRE(P >= 0 && C >= 1, PDM_E_BADARG, "pillar_scatter_grad: bad size");
    if (P == 0) return 0;
    PDM_REQUIRE(grad_canvas && voxel_coords && grad_features, PDM_E_BADARG, "pillar_scatter_grad: null pointer");
    const long long total = (long long)P * C;
    PDM_REQUIRE(total <= 0x7fffffffll * PL_T, PDM_E_TOOLARGE, "pillar_scatter_grad: %lld outputs", total);
    hipLaunchKernelGGL(pl_scatter_grad_kernel, dim3((unsigned)divup(total, PL_T)), dim3(PL_T), 0, as_stream(stream), total, B, C, nx, ny,
                       grad_canvas, voxel_coords, grad_features);
    return check_launch("pillar_scatter_grad");
}

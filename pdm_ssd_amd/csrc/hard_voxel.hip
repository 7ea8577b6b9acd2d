// Hard voxelization (DESIGN.md "Hard voxels"): at most T points a voxel and at most max_voxels voxels a sample, voxels
// numbered in the order their first point appears, as the reference's CPU voxel generator does in a sequential loop.  Here
// it is the loop's closed form, with no host loop, no sort and no float atomic:
//   * a cell's APPEARANCE RANK is the rank of its first row among the first rows of the occupied cells of its sample; the
//     cell becomes voxel `rank` of the sample iff rank < max_voxels; a voxel keeps the T smallest rows of its cell, ascending;
//   * cells are found by the occupancy index of sc_index.h (64-bit keys, bitmap, scanned popcounts); the first row of a cell
//     is an integer atomicMin, the count an integer atomicAdd: both commute;
//   * a first-row flag per row, scanned over the rows, numbers the cells in appearance order; the samples' bases come from
//     per-sample counts of the flags (the rows of a sample are contiguous, samples ascending: checked on the device);
//   * the rows of every accepted cell are listed in a CSR whose slot order is arbitrary (an atomic cursor); the selection
//     pass CHOOSES the T smallest rows and writes them ascending, so the cursor's order never reaches a result.
// The encoders read slot_rows: MeanVFE as a sum in slot order and one division, PillarVFE with a single PFN layer in eval
// mode in one launch (pillar_feat.h), neither through the padded (M, T, C) tensor.
#include "pillar_feat.h"
#include "sc_index.h"
#include "voxel_grid.h"

namespace pdm {

constexpr int HV_T = SCAN_T;               // threads per workgroup of every kernel here; a scan tile is SCAN_TILE items
constexpr int HV_MAX_T = 128;              // points per voxel (pdm_hard_voxel_max_points)
constexpr int HV_SHORT = 32;               // the selection pass: a lane per list up to here, a wave per longer list
constexpr int HV_NONE = 0x7fffffff;
enum { HV_UNSORTED = 0, HV_CELLS = 1 };    // words of the workspace's `misc`

// rows -> keys (voxel_grid.h, z tested) and occupancy bits; batch_idx[i] <= batch_idx[i + 1] or the input counts as unsorted
// (a NaN does); the first-row table starts at "none"
__global__ __launch_bounds__(HV_T) void hv_key_kernel(int N, int C1, const float *__restrict__ points, VoxelGrid g, int capc,
                                                      long long *__restrict__ point_key, unsigned *__restrict__ bits,
                                                      int *__restrict__ first_row, int *__restrict__ misc) {
    const long long i = (long long)blockIdx.x * HV_T + threadIdx.x;
    if (i < capc) first_row[i] = HV_NONE;
    if (i >= N) return;
    const float *row = points + (size_t)i * C1;
    const long long key = voxel_key<true>(row, g);
    point_key[i] = key;
    if (key >= 0) sc_set(bits, key);
    if (i + 1 < N && !(row[0] <= row[C1])) atomicOr(&misc[HV_UNSORTED], 1);
}

// every kept row: the rank of its cell in key order, the cell's first row and its count
__global__ __launch_bounds__(HV_T) void hv_first_kernel(int N, const long long *__restrict__ point_key, const unsigned *__restrict__ bits,
                                                        const int *__restrict__ gprefix, int *__restrict__ point_rank,
                                                        int *__restrict__ first_row, int *__restrict__ cell_count) {
    const long long i = (long long)blockIdx.x * HV_T + threadIdx.x;
    if (i >= N) return;
    const long long key = point_key[i];
    int r = -1;
    if (key >= 0) {
        r = sc_rank(bits, gprefix, key);
        atomicMin(&first_row[r], (int)i);
        atomicAdd(&cell_count[r], 1);
    }
    point_rank[i] = r;
}

// per tile of rows: how many are the first of their cell; per sample: how many cells it owns (one atomic per wave and sample)
__global__ __launch_bounds__(HV_T) void hv_flag_total_kernel(int N, int C1, const float *__restrict__ points, const int *__restrict__ point_rank,
                                                             const int *__restrict__ first_row, int *__restrict__ ptile,
                                                             int *__restrict__ sample_cnt) {
    const int lane = threadIdx.x & 63;
    tile_reduce<HV_T, SCAN_ITEMS>(N, {ptile}, [&](long long i, int *flags) {
        const int r = point_rank[i];
        const bool f = r >= 0 && first_row[r] == (int)i;
        const int b = f ? (int)points[(size_t)i * C1] : -1;
        flags[0] += f;
        unsigned long long left = __ballot(f);          // of the wave's lanes that have a row
        while (left) {                                  // wave-uniform: the flagged lanes of one sample at a time
            const int leader = __ffsll((long long)left) - 1;
            const int lb = __shfl(b, leader, 64);
            const unsigned long long same = __ballot(f && b == lb);
            if (lane == leader) atomicAdd(&sample_cnt[lb], __popcll(same));
            left &= ~same;
        }
    });
}

// rows of every tile of cells (cells in key order; entries past the occupied cells are zero)
__global__ __launch_bounds__(HV_T) void hv_cell_total_kernel(int capc, const int *__restrict__ cell_count, int *__restrict__ ctile) {
    tile_reduce<HV_T, SCAN_ITEMS>(capc, {ctile}, [&](long long c, int *rows) { rows[0] += cell_count[c]; });
}

// workgroup 0: the row tiles; 1: the cell tiles; 2: the samples -> sample_cnt becomes the cells in front of every sample,
// sample_vox the voxels in front of it, record = {M, unsorted} (M = 0 for an unsorted input: nothing after this is valid)
__global__ __launch_bounds__(HV_T) void hv_scan_kernel(int ntp, int *__restrict__ ptile, int ntc, int *__restrict__ ctile, int B, int max_voxels,
                                                       int *__restrict__ sample_cnt, int *__restrict__ sample_vox, const int *__restrict__ misc,
                                                       int *__restrict__ record) {
    __shared__ int s_wave[HV_T / 64];
    if (blockIdx.x == 0) {
        scan_totals<HV_T>(ntp, ptile, s_wave);
    } else if (blockIdx.x == 1) {
        scan_totals<HV_T>(ntc, ctile, s_wave);
    } else {
        for (int b = threadIdx.x; b < B; b += HV_T) sample_vox[b] = min(sample_cnt[b], max_voxels);
        __syncthreads();
        scan_totals<HV_T>(B, sample_cnt, s_wave);
        const int M = scan_totals<HV_T>(B, sample_vox, s_wave);
        if (threadIdx.x == 0) {
            const int unsorted = misc[HV_UNSORTED] != 0;
            record[0] = unsorted ? 0 : M;
            record[1] = unsorted;
        }
    }
}

// every first row: its cell's appearance rank in the sample -> the voxel (or none), its coordinates and its point count
__global__ __launch_bounds__(HV_T) void hv_voxel_kernel(int N, VoxelGrid g, int T, int max_voxels, int cap, const long long *__restrict__ point_key,
                                                        const int *__restrict__ point_rank, const int *__restrict__ first_row,
                                                        const int *__restrict__ cell_count, const int *__restrict__ ptile,
                                                        const int *__restrict__ sample_cnt, const int *__restrict__ sample_vox,
                                                        const int *__restrict__ misc, int *__restrict__ cell_vid, int *__restrict__ voxel_rank,
                                                        int *__restrict__ voxel_coords, int *__restrict__ voxel_num_points) {
    if (misc[HV_UNSORTED]) return;
    int r;
    bool f;
    tile_scan<HV_T, SCAN_ITEMS>(N, {ptile[blockIdx.x]}, [&](long long i, int *v) {
        r = point_rank[i];
        v[0] = f = r >= 0 && first_row[r] == (int)i;
    }, [&](long long i, const int *seen) {              // seen: first rows in front of this one, all samples
        if (!f) return;
        int c[4];
        voxel_key_coords(point_key[i], g.nx, g.ny, g.nz, c);
        const int b = c[0], rank = seen[0] - sample_cnt[b];
        const int vid = (rank >= 0 && rank < max_voxels) ? sample_vox[b] + rank : -1;
        if (vid < 0 || vid >= cap) { cell_vid[r] = -1; return; }
        cell_vid[r] = vid;
        voxel_rank[vid] = r;
        int *vc = voxel_coords + (size_t)vid * 4;
        vc[0] = b; vc[1] = c[1]; vc[2] = c[2]; vc[3] = c[3];
        voxel_num_points[vid] = min(cell_count[r], T);
    });
}

// the first CSR slot of every cell
__global__ __launch_bounds__(HV_T) void hv_cell_start_kernel(int capc, const int *__restrict__ cell_count, const int *__restrict__ ctile,
                                                             int *__restrict__ seg_start) {
    tile_scan<HV_T, SCAN_ITEMS>(capc, {ctile[blockIdx.x]}, [&](long long c, int *v) { v[0] = cell_count[c]; },
                                [&](long long c, const int *at) { seg_start[c] = at[0]; });
}

// every row of an accepted cell takes a CSR slot of the cell (slot order arbitrary)
__global__ __launch_bounds__(HV_T) void hv_list_kernel(int N, const int *__restrict__ point_rank, const int *__restrict__ cell_vid,
                                                       const int *__restrict__ seg_start, const int *__restrict__ misc, int *__restrict__ cursor,
                                                       int *__restrict__ seg_rows) {
    const long long i = (long long)blockIdx.x * HV_T + threadIdx.x;
    if (i >= N || misc[HV_UNSORTED]) return;
    const int r = point_rank[i];
    if (r < 0 || cell_vid[r] < 0) return;
    seg_rows[seg_start[r] + atomicAdd(&cursor[r], 1)] = (int)i;
}

// The T smallest rows of every voxel's cell, ascending, -1 behind them.  A list of up to HV_SHORT rows is one lane's: round k
// takes the smallest row above round k - 1's.  A longer list is the whole wave's, one list after another: the lanes stride
// over it, the wave takes the minimum.  Either way the result is the set's, whatever order the CSR holds it in.
__global__ __launch_bounds__(HV_T) void hv_select_kernel(int T, const int *__restrict__ record, const int *__restrict__ voxel_rank,
                                                         const int *__restrict__ seg_start, const int *__restrict__ cell_count,
                                                         const int *__restrict__ seg_rows, int *__restrict__ slot_rows) {
    const int M = record[0], lane = threadIdx.x & 63;
    const long long v = (long long)blockIdx.x * HV_T + threadIdx.x;
    const bool valid = v < M;
    int lo = 0, n = 0;
    if (valid) {
        const int r = voxel_rank[v];
        lo = seg_start[r];
        n = cell_count[r];
    }
    if (valid && n <= HV_SHORT) {
        int *out = slot_rows + (size_t)v * T;
        const int m = min(n, T);
        int prev = -1;
        for (int k = 0; k < m; ++k) {
            int best = HV_NONE;
            for (int s = 0; s < n; ++s) {
                const int x = seg_rows[lo + s];
                if (x > prev && x < best) best = x;
            }
            out[k] = best;
            prev = best;
        }
        for (int k = m; k < T; ++k) out[k] = -1;
    }
    unsigned long long left = __ballot(valid && n > HV_SHORT);
    while (left) {
        const int src = __ffsll((long long)left) - 1;
        left &= left - 1;
        const int wlo = __shfl(lo, src, 64), wn = __shfl(n, src, 64);
        int *out = slot_rows + (size_t)(v - lane + src) * T;
        const int m = min(wn, T);
        int prev = -1;
        for (int k = 0; k < m; ++k) {
            int best = HV_NONE;
            for (int s = lane; s < wn; s += 64) {
                const int x = seg_rows[wlo + s];
                if (x > prev && x < best) best = x;
            }
#pragma unroll
            for (int off = 32; off; off >>= 1) best = min(best, __shfl_xor(best, off, 64));
            if (lane == 0) out[k] = best;
            prev = best;
        }
        for (int k = m + lane; k < T; k += 64) out[k] = -1;
    }
}

// voxels (M, T, C) = the slots' rows past batch_idx, zeros in the padding: every element written, values are bit copies.
// M from the record when there is one (a launch at capacity), else the argument.
__global__ __launch_bounds__(HV_T) void hv_gather_kernel(int M_arg, const int *__restrict__ record, int T, int C1, const float *__restrict__ points,
                                                         const int *__restrict__ slot_rows, float *__restrict__ voxels) {
    const int C = C1 - 1, M = record ? record[0] : M_arg;
    const long long e = (long long)blockIdx.x * HV_T + threadIdx.x;
    if (e >= (long long)M * T * C) return;
    const int row = slot_rows[e / C];
    voxels[e] = row >= 0 ? points[(size_t)row * C1 + 1 + (int)(e % C)] : 0.0f;
}

// thread = (voxel, column): the fp32 sum of the slots in slot order, then one IEEE division by max(num, 1)
__global__ __launch_bounds__(HV_T) void hv_mean_kernel(long long total, int T, int C1, const float *__restrict__ points,
                                                       const int *__restrict__ slot_rows, const int *__restrict__ voxel_num_points,
                                                       float *__restrict__ out) {
    const long long t = (long long)blockIdx.x * HV_T + threadIdx.x;
    if (t >= total) return;
    const int C = C1 - 1, c = (int)(t % C);
    const long long v = t / C;
    const int n = min(voxel_num_points[v], T);
    const int *slots = slot_rows + (size_t)v * T;
    float acc = 0.0f;
    for (int s = 0; s < n; ++s) {
        const int row = slots[s];
        if (row < 0) break;
        acc = __fadd_rn(acc, points[(size_t)row * C1 + 1 + c]);
    }
    out[t] = __fdiv_rn(acc, (float)max(n, 1));
}

// thread = (voxel, channel): the mean of the kept slots, then per slot features -> dot -> scale, shift, ReLU -> running max;
// a voxel with fewer than T points also takes the padding rows' value, relu(0 * scale + shift)
__global__ __launch_bounds__(HV_T) void hv_pfn_kernel(long long total, int K, int T, PlFeat a, const float *__restrict__ points,
                                                      const int *__restrict__ slot_rows, const int *__restrict__ voxel_num_points,
                                                      const int *__restrict__ voxel_coords, const float *__restrict__ weight,
                                                      const float *__restrict__ scale, const float *__restrict__ shift, float *__restrict__ out) {
    const long long t = (long long)blockIdx.x * HV_T + threadIdx.x;
    if (t >= total) return;
    const long long v = t / K;
    const int k = (int)(t % K);
    PlChannel w;
    pl_channel_load(a, k, weight, scale, shift, w);
    const int *slots = slot_rows + (size_t)v * T;
    int n = min(voxel_num_points[v], T);
    float sum[3] = {0.0f, 0.0f, 0.0f};
    for (int s = 0; s < n; ++s) {
        const int row = slots[s];
        if (row < 0) { n = s; break; }
        const float *p = points + (size_t)row * a.C1;
        sum[0] = __fadd_rn(sum[0], p[1]); sum[1] = __fadd_rn(sum[1], p[2]); sum[2] = __fadd_rn(sum[2], p[3]);
    }
    const float den = (float)max(n, 1);
    const float mean[3] = {__fdiv_rn(sum[0], den), __fdiv_rn(sum[1], den), __fdiv_rn(sum[2], den)};
    const int *vc = voxel_coords + (size_t)v * 4;
    float best = n < T ? fmaxf(__fmaf_rn(0.0f, w.sc, w.sh), 0.0f) : 0.0f;
    for (int s = 0; s < n; ++s) {
        const float y = pl_channel_row<true>(a, w, points + (size_t)slots[s] * a.C1, mean, vc);
        best = (y > best || y != y) ? y : best;        // a NaN stays, as torch's max keeps it
    }
    out[t] = best;
}

// workspace of pdm_hard_voxelize, every section 256-byte aligned; [zeroed .. zeroed_end) is cleared by one launch
struct HvWorkspace {
    size_t point_key, index, point_rank, first_row, cell_vid, seg_start, seg_rows, voxel_rank, ptile, ctile, sample_vox;
    size_t zeroed, cell_count, cursor, sample_cnt, misc, zeroed_end, total;
    ScIndexSize isz;
};
static long long hv_cells(int B, int nx, int ny, int nz) { return (long long)B * nx * ny * nz; }
static long long hv_capacity(long long N, int B, int max_voxels, long long ncell) {
    const long long a = N < ncell ? N : ncell, b = (long long)B * max_voxels;
    return a < b ? a : b;
}
static HvWorkspace hv_workspace(long long N, int B, long long ncell) {
    const size_t capc = (size_t)(N < ncell ? N : ncell), ntp = (size_t)divup(N, SCAN_TILE), ntc = (size_t)divup((long long)capc, SCAN_TILE);
    HvWorkspace w{};
    w.isz = sc_index_size(ncell);
    size_t at = 0;
    w.point_key = at; at += align256(sizeof(long long) * (size_t)N);
    w.index = at; at += w.isz.bits + w.isz.gprefix + w.isz.tiles;
    w.point_rank = at; at += align256(sizeof(int) * (size_t)N);
    w.first_row = at; at += align256(sizeof(int) * capc);
    w.cell_vid = at; at += align256(sizeof(int) * capc);
    w.seg_start = at; at += align256(sizeof(int) * capc);
    w.seg_rows = at; at += align256(sizeof(int) * (size_t)N);
    w.voxel_rank = at; at += align256(sizeof(int) * capc);
    w.ptile = at; at += align256(sizeof(int) * ntp);
    w.ctile = at; at += align256(sizeof(int) * ntc);
    w.sample_vox = at; at += align256(sizeof(int) * (size_t)B);
    w.zeroed = at;
    w.cell_count = at; at += align256(sizeof(int) * capc);
    w.cursor = at; at += align256(sizeof(int) * capc);
    w.sample_cnt = at; at += align256(sizeof(int) * (size_t)B);
    w.misc = at; at += 256;
    w.zeroed_end = at;
    w.total = at;
    return w;
}

static int hv_check_slots(const char *who, long long M, int T, int C1) {
    PDM_REQUIRE(M >= 0 && C1 >= 4, PDM_E_BADARG, "%s: bad size", who);
    PDM_REQUIRE(T >= 1 && T <= HV_MAX_T, PDM_E_BADARG, "%s: %d points per voxel, between 1 and %d", who, T, HV_MAX_T);
    PDM_REQUIRE(M * T * (C1 - 1) <= 0x7fffffffll * HV_T, PDM_E_TOOLARGE, "%s: %lld voxel elements", who, M * T * (C1 - 1));
    return 0;
}

}  // namespace pdm

using namespace pdm;

extern "C" int pdm_hard_voxel_max_points(void) { return HV_MAX_T; }

extern "C" size_t pdm_hard_voxelize_workspace_bytes(int N, int B, int nx, int ny, int nz) {
    if (N < 0 || !voxel_grid_cells_ok(B, nx, ny, nz, SC_MAXCELL)) return 0;
    return hv_workspace(N, B, hv_cells(B, nx, ny, nz)).total;
}

// points (N, C1) fp32 rows (batch_idx, x, y, z, ...), the rows of a sample contiguous and samples ascending, any 4-byte
// alignment.  Outputs at capacity cap = min(N, B max_voxels, cells): slot_rows (cap, T), voxel_coords (cap, 4) = (b, cz, cy, cx),
// voxel_num_points (cap), voxels (cap, T, C1 - 1) or null; record (2) = {M, unsorted}.  Only the first M voxels are written.
extern "C" int pdm_hard_voxelize(void *stream, int N, int C1, const float *points, int B, int nx, int ny, int nz, float x0, float y0, float z0,
                                 float vx, float vy, float vz, int T, int max_voxels, int *slot_rows, int *voxel_coords,
                                 int *voxel_num_points, float *voxels, int *record, void *workspace, size_t workspace_bytes) {
    if (int rc = voxel_grid_check("hard_voxelize", N, C1, B, nx, ny, nz, SC_MAXCELL, "the grid exceeds 2^35 cells")) return rc;
    PDM_REQUIRE(vx > 0.0f && vy > 0.0f && vz > 0.0f, PDM_E_BADARG, "hard_voxelize: voxel size must be positive");
    PDM_REQUIRE(max_voxels >= 1, PDM_E_BADARG, "hard_voxelize: max_voxels must be at least 1 (got %d)", max_voxels);
    const long long ncell = hv_cells(B, nx, ny, nz), cap = hv_capacity(N, B, max_voxels, ncell);
    if (int rc = hv_check_slots("hard_voxelize", cap, T, C1)) return rc;
    PDM_REQUIRE(record, PDM_E_BADARG, "hard_voxelize: null pointer");
    PDM_REQUIRE(N == 0 || points, PDM_E_BADARG, "hard_voxelize: null pointer");
    PDM_REQUIRE(cap == 0 || (slot_rows && voxel_coords && voxel_num_points), PDM_E_BADARG, "hard_voxelize: null pointer");
    const HvWorkspace w = hv_workspace(N, B, ncell);
    PDM_REQUIRE(workspace, PDM_E_BADARG, "hard_voxelize: null pointer");
    PDM_WS_ALIGNED("hard_voxelize", workspace);
    PDM_REQUIRE(workspace_bytes >= w.total, PDM_E_BADARG, "hard_voxelize: workspace too small (%zu bytes, need %zu)", workspace_bytes, w.total);
    char *ws = static_cast<char *>(workspace);
    auto ints = [ws](size_t at) { return reinterpret_cast<int *>(ws + at); };
    long long *point_key = reinterpret_cast<long long *>(ws + w.point_key);
    const ScIndex ix = sc_index_at(ws + w.index, w.isz);
    int *point_rank = ints(w.point_rank), *first_row = ints(w.first_row), *cell_vid = ints(w.cell_vid), *seg_start = ints(w.seg_start);
    int *seg_rows = ints(w.seg_rows), *voxel_rank = ints(w.voxel_rank), *ptile = ints(w.ptile), *ctile = ints(w.ctile);
    int *sample_vox = ints(w.sample_vox), *cell_count = ints(w.cell_count), *cursor = ints(w.cursor), *sample_cnt = ints(w.sample_cnt);
    int *misc = ints(w.misc);
    const VoxelGrid g{B, nx, ny, nz, x0, y0, z0, vx, vy, vz};
    const int capc = (int)(N < ncell ? N : ncell), ntp = divup(N, SCAN_TILE), ntc = divup(capc, SCAN_TILE), nbp = divup(N, HV_T);
    hipStream_t s = as_stream(stream);
    if (int rc = zero_fill(stream, "hard_voxelize(zero)", ix.bits, w.isz.bits)) return rc;
    if (int rc = zero_fill(stream, "hard_voxelize(zero)", ws + w.zeroed, w.zeroed_end - w.zeroed)) return rc;
    const bool rows = N > 0 && ncell > 0;
    if (rows) {
        hipLaunchKernelGGL(hv_key_kernel, dim3((unsigned)nbp), dim3(HV_T), 0, s, N, C1, points, g, capc, point_key, ix.bits, first_row, misc);
        if (int rc = check_launch("hard_voxelize(keys)")) return rc;
        if (int rc = sc_index_scan(s, "hard_voxelize(index)", ix, misc + HV_CELLS, nullptr, nullptr)) return rc;
        hipLaunchKernelGGL(hv_first_kernel, dim3((unsigned)nbp), dim3(HV_T), 0, s, N, point_key, ix.bits, ix.gprefix, point_rank, first_row,
                           cell_count);
        if (int rc = check_launch("hard_voxelize(first rows)")) return rc;
        hipLaunchKernelGGL(hv_flag_total_kernel, dim3((unsigned)ntp), dim3(HV_T), 0, s, N, C1, points, point_rank, first_row, ptile, sample_cnt);
        if (int rc = check_launch("hard_voxelize(flags)")) return rc;
        hipLaunchKernelGGL(hv_cell_total_kernel, dim3((unsigned)ntc), dim3(HV_T), 0, s, capc, cell_count, ctile);
        if (int rc = check_launch("hard_voxelize(cell totals)")) return rc;
    }
    hipLaunchKernelGGL(hv_scan_kernel, dim3(3), dim3(HV_T), 0, s, rows ? ntp : 0, ptile, rows ? ntc : 0, ctile, rows ? B : 0, max_voxels, sample_cnt,
                       sample_vox, misc, record);
    if (int rc = check_launch("hard_voxelize(scan)")) return rc;
    if (!rows || cap == 0) return 0;
    hipLaunchKernelGGL(hv_voxel_kernel, dim3((unsigned)ntp), dim3(HV_T), 0, s, N, g, T, max_voxels, (int)cap, point_key, point_rank, first_row,
                       cell_count, ptile, sample_cnt, sample_vox, misc, cell_vid, voxel_rank, voxel_coords, voxel_num_points);
    if (int rc = check_launch("hard_voxelize(voxels)")) return rc;
    hipLaunchKernelGGL(hv_cell_start_kernel, dim3((unsigned)ntc), dim3(HV_T), 0, s, capc, cell_count, ctile, seg_start);
    if (int rc = check_launch("hard_voxelize(cell starts)")) return rc;
    hipLaunchKernelGGL(hv_list_kernel, dim3((unsigned)nbp), dim3(HV_T), 0, s, N, point_rank, cell_vid, seg_start, misc, cursor, seg_rows);
    if (int rc = check_launch("hard_voxelize(lists)")) return rc;
    hipLaunchKernelGGL(hv_select_kernel, dim3((unsigned)divup(cap, HV_T)), dim3(HV_T), 0, s, T, record, voxel_rank, seg_start, cell_count, seg_rows,
                       slot_rows);
    if (int rc = check_launch("hard_voxelize(select)")) return rc;
    if (voxels) {
        hipLaunchKernelGGL(hv_gather_kernel, dim3((unsigned)divup(cap * T * (C1 - 1), HV_T)), dim3(HV_T), 0, s, 0, record, T, C1, points, slot_rows,
                           voxels);
        if (int rc = check_launch("hard_voxelize(gather)")) return rc;
    }
    return 0;
}

// slot_rows (M, T) -> voxels (M, T, C1 - 1): the reference's padded tensor, every element written
extern "C" int pdm_hard_voxel_materialize(void *stream, int M, int T, int C1, const float *points, const int *slot_rows, float *voxels) {
    if (int rc = hv_check_slots("hard_voxel_materialize", M, T, C1)) return rc;
    if (M == 0) return 0;
    PDM_REQUIRE(points && slot_rows && voxels, PDM_E_BADARG, "hard_voxel_materialize: null pointer");
    hipLaunchKernelGGL(hv_gather_kernel, dim3((unsigned)divup((long long)M * T * (C1 - 1), HV_T)), dim3(HV_T), 0, as_stream(stream), M, nullptr, T, C1,
                       points, slot_rows, voxels);
    return check_launch("hard_voxel_materialize");
}

// out (M, C1 - 1): MeanVFE without the padded tensor
extern "C" int pdm_hard_voxel_mean(void *stream, int M, int T, int C1, const float *points, const int *slot_rows, const int *voxel_num_points,
                                   float *out) {
    if (int rc = hv_check_slots("hard_voxel_mean", M, T, C1)) return rc;
    if (M == 0) return 0;
    PDM_REQUIRE(points && slot_rows && voxel_num_points && out, PDM_E_BADARG, "hard_voxel_mean: null pointer");
    const long long total = (long long)M * (C1 - 1);
    hipLaunchKernelGGL(hv_mean_kernel, dim3((unsigned)divup(total, HV_T)), dim3(HV_T), 0, as_stream(stream), total, T, C1, points, slot_rows,
                       voxel_num_points, out);
    return check_launch("hard_voxel_mean");
}

// the reference's PillarVFE with one PFN layer in eval mode: out (M, K).  F <= 16.
extern "C" int pdm_hard_pillar_pfn(void *stream, int M, int K, int T, int C1, const float *points, const int *slot_rows,
                                   const int *voxel_num_points, const int *voxel_coords, int abs_xyz, int with_dist, float vx, float vy, float vz,
                                   float xoff, float yoff, float zoff, const float *weight, const float *scale, const float *shift, float *out) {
    PlFeat a;
    if (int rc = pl_feat_args("hard_pillar_pfn", &a, C1, abs_xyz, with_dist, vx, vy, xoff, yoff, zoff, vz)) return rc;
    PDM_REQUIRE(a.F <= PL_MAXF, PDM_E_TOOLARGE, "hard_pillar_pfn: %d feature columns, at most %d", a.F, PL_MAXF);
    if (int rc = hv_check_slots("hard_pillar_pfn", M, T, C1)) return rc;
    PDM_REQUIRE(K >= 1, PDM_E_BADARG, "hard_pillar_pfn: bad size");
    if (M == 0) return 0;
    PDM_REQUIRE(points && slot_rows && voxel_num_points && voxel_coords && weight && scale && shift && out, PDM_E_BADARG,
                "hard_pillar_pfn: null pointer");
    const long long total = (long long)M * K;
    PDM_REQUIRE(total <= 0x7fffffffll * HV_T, PDM_E_TOOLARGE, "hard_pillar_pfn: %lld outputs", total);
    hipLaunchKernelGGL(hv_pfn_kernel, dim3((unsigned)divup(total, HV_T)), dim3(HV_T), 0, as_stream(stream), total, K, T, a, points, slot_rows,
                       voxel_num_points, voxel_coords, weight, scale, shift, out);
    return check_launch("hard_pillar_pfn");
}

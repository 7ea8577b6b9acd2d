// The training form of Voxel R-CNN's RoI-grid pooling, three operators per (level, scale):
//   pdm_roi_grid_query       roi_grid_geom.h's walk, kept: grp_row (M, S), grp_off (M, S, 3) and the nine float64 moments of the
//                            reference's PADDED offset tensor (what its BatchNorm2d takes its batch statistics over);
//   pdm_roi_grid_pool_train  pooled (M, C1) with the eval kernel's arithmetic per slot and arg (M, C1), the winning slot;
//   pdm_roi_grid_pool_grad   the gradients of the features, of Wp and of scale_p / shift_p.
// No dense table, no grouped tensors, no float atomics, no host read: many grid points write one voxel row, so the features'
// gradient is summed in 64-bit fixed point with integer atomics, which commute (pillar.hip, sparse_conv.hip), at a scale taken
// from max|gpool| on the device; the parameter sums go through per-workgroup partials whose partition is a function of the sizes
// alone, added in ascending order.  Two runs and a graph replay give the same bits.
#include "roi_grid_geom.h"

namespace pdm {

constexpr int RGT_T = 256;
constexpr long long RGT_MAXM = 1ll << 22;       // grid points at most: 2^22 addends below 2^41 stay inside 64 bits
constexpr int RGT_MAXBLOCKS = 2048;             // query workgroups at most; waves walk the tiles with this stride
constexpr int RGT_PARTS = 1024;                 // parameter-gradient partials at most
constexpr int RGT_FIXBITS = 40;                 // max|gpool| is scaled into [2^40, 2^41)

// ---- the query -----------------------------------------------------------------------------------------------------------
struct RgqArgs {
    long long M;
    int n, G, roi_stride;
    int B, D, H, W, P, stride;
    float vox[3], r0[3];
    int rz, ry, rx, nsample;
    float radius;
    const float *rois;
    const unsigned *bits;
    const int *gprefix, *row_of_rank;
    int *grp_row;       // (M, S)
    float *grp_off;     // (M, S, 3)
    double *part;       // (tiles, 9)
};

// A wave owns a tile of 16 grid points.  Lane s of the wave holds slot s of the current group: it stores the slot and adds its
// offset, weighted by the slot's multiplicity in the padded tensor (slot 0 also stands for the S - cnt padding slots), to nine
// float64 sums; after the tile one butterfly adds the lanes and lane 0 writes the tile's partial.
__global__ __launch_bounds__(RGT_T) void roi_grid_query_kernel(RgqArgs a) {
    __shared__ int s_hrow[RGT_T / 64][RGP_MAXS];
    __shared__ float s_hd[RGT_T / 64][RGP_MAXS * 3];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const RgpWalk k = rgp_walk_of(a);
    const long long ntiles = (a.M + RGP_TILE - 1) / RGP_TILE;
    const int S = a.nsample;
    int *hrow = s_hrow[wave];
    float *hd = s_hd[wave];

    for (long long tile = (long long)blockIdx.x * (RGT_T / 64) + wave; tile < ntiles; tile += (long long)gridDim.x * (RGT_T / 64)) {
        float pgx, pgy, pgz;
        int pcx, pcy, pcz, pb;
        rgp_tile_points(a, k, tile, lane, pgx, pgy, pgz, pcx, pcy, pcz, pb);
        double m[9];
#pragma unroll
        for (int j = 0; j < 9; ++j) m[j] = 0.0;
        for (int i = 0; i < RGP_TILE; ++i) {
            const long long pt = tile * RGP_TILE + i;
            if (pt >= a.M) break;
            const float gx = __shfl(pgx, i, 64), gy = __shfl(pgy, i, 64), gz = __shfl(pgz, i, 64);
            const int cx = __shfl(pcx, i, 64), cy = __shfl(pcy, i, 64), cz = __shfl(pcz, i, 64), b = __shfl(pb, i, 64);
            const int cnt = rgp_window_hits(a, k, lane, gx, gy, gz, cx, cy, cz, b, hrow, hd);
            __builtin_amdgcn_wave_barrier();
            if (lane < S) {
                const bool used = lane < cnt;
                const float dx = used ? hd[lane * 3] : 0.0f, dy = used ? hd[lane * 3 + 1] : 0.0f, dz = used ? hd[lane * 3 + 2] : 0.0f;
                a.grp_row[pt * S + lane] = used ? hrow[lane] : -1;
                float *o = a.grp_off + (pt * S + lane) * 3;
                o[0] = dx; o[1] = dy; o[2] = dz;
                if (used) {
                    const double w = lane == 0 ? (double)(1 + S - cnt) : 1.0;
                    const double x = dx, y = dy, z = dz, wx = w * x, wy = w * y, wz = w * z;
                    m[0] += wx; m[1] += wy; m[2] += wz;
                    m[3] += wx * x; m[4] += wx * y; m[5] += wx * z; m[6] += wy * y; m[7] += wy * z; m[8] += wz * z;
                }
            }
            __builtin_amdgcn_wave_barrier();        // the next group overwrites hrow / hd
        }
#pragma unroll
        for (int j = 0; j < 9; ++j) {
            const double t = wave_sum(m[j]);
            if (lane == 0) a.part[tile * 9 + j] = t;
        }
    }
}

// moments[j] = the tiles' partials in ascending order: thread t adds its run of ceil(ntiles / 256) consecutive tiles, then
// thread j adds the 256 runs.  One workgroup; the partition is a function of ntiles alone.
__global__ __launch_bounds__(RGT_T) void roi_grid_moments_kernel(long long ntiles, const double *__restrict__ part, double *__restrict__ moments) {
    __shared__ double s_run[RGT_T][9];
    const long long per = (ntiles + RGT_T - 1) / RGT_T;
    const long long t0 = min(threadIdx.x * per, ntiles), t1 = min(t0 + per, ntiles);
    double m[9];
#pragma unroll
    for (int j = 0; j < 9; ++j) m[j] = 0.0;
    for (long long t = t0; t < t1; ++t)
#pragma unroll
        for (int j = 0; j < 9; ++j) m[j] += part[t * 9 + j];
#pragma unroll
    for (int j = 0; j < 9; ++j) s_run[threadIdx.x][j] = m[j];
    __syncthreads();
    if (threadIdx.x < 9) {
        double s = 0.0;
        for (int t = 0; t < RGT_T; ++t) s += s_run[t][threadIdx.x];
        moments[threadIdx.x] = s;
    }
}

// ---- the pooling over the saved groups -------------------------------------------------------------------------------------
// thread = (grid point, channel), the channel fastest: a gathered feature row and a pooled row are contiguous across lanes, the
// group's rows and offsets are the same address for the C1 lanes of a point
template <int C1>
__global__ __launch_bounds__(RGT_T) void roi_grid_pool_train_kernel(long long M, int S, int P, const int *__restrict__ grp_row,
                                                                    const float *__restrict__ grp_off, const float *__restrict__ feat,
                                                                    const float *__restrict__ wp, const float *__restrict__ scale_p,
                                                                    const float *__restrict__ shift_p, float *__restrict__ pooled,
                                                                    unsigned char *__restrict__ arg) {
    const long long t = (long long)blockIdx.x * RGT_T + threadIdx.x;
    const long long m = t / C1;
    const int c = (int)(t % C1);
    if (m >= M) return;
    const float wpx = wp[c * 3], wpy = wp[c * 3 + 1], wpz = wp[c * 3 + 2], sp = scale_p[c], hp = shift_p[c];
    const int *rows = grp_row + m * S;
    const float *offs = grp_off + m * S * 3;
    float v = 0.0f;
    unsigned char best = 0xFF;
    const int row0 = rows[0];
    if (row0 < 0 || row0 >= P) {        // an empty group: relu(shift_p), slot 0 when that is positive
        if (hp > 0.0f) { v = hp; best = 0; }
    } else {
        for (int s = 0; s < S; ++s) {
            const int row = rows[s];
            if (row < 0 || row >= P) break;
            const float f = feat[(size_t)row * C1 + c];
            const float dot = __fmaf_rn(wpz, offs[s * 3 + 2], __fmaf_rn(wpy, offs[s * 3 + 1], __fmul_rn(wpx, offs[s * 3])));
            const float x = __fadd_rn(f, __fmaf_rn(dot, sp, hp));
            if (x > v) { v = x; best = (unsigned char)s; }      // strict: the lowest slot keeps a tie, and 0 keeps 0xFF
        }
    }
    pooled[t] = v;
    arg[t] = best;
}

// ---- the gradients ---------------------------------------------------------------------------------------------------------
struct RggWorkspace {
    size_t maxword, fixed, part, total;
    int chunk, nparts;
};
// grid points of one parameter-gradient partial: a multiple of the 256 / C1 points a workgroup holds at a time, and at most
// RGT_PARTS partials
static int rgg_chunk(long long M, int C1) {
    const long long sub = RGT_T / C1;
    return (int)(sub * max(1ll, (M + sub * RGT_PARTS - 1) / (sub * RGT_PARTS)));
}
static RggWorkspace rgg_workspace(long long M, long long P, int C1) {
    RggWorkspace w{};
    w.chunk = rgg_chunk(M, C1);
    w.nparts = (int)((M + w.chunk - 1) / w.chunk);
    size_t at = 0;
    w.maxword = at; at += 256;
    w.fixed = at; at += align256(sizeof(long long) * (size_t)P * C1);
    w.part = at; at += align256(sizeof(float) * (size_t)w.nparts * 5 * C1);
    w.total = at;
    return w;
}

// max |gpool| as an integer maximum on the bit patterns (non-negative floats order as their bits do; NaN and inf sort last)
__global__ __launch_bounds__(RGT_T) void roi_grid_absmax_kernel(long long count, const float *__restrict__ g, unsigned *__restrict__ maxword) {
    unsigned best = 0;
    for (long long i = (long long)blockIdx.x * RGT_T + threadIdx.x; i < count; i += (long long)gridDim.x * RGT_T)
        best = max(best, __float_as_uint(g[i]) & 0x7fffffffu);
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) best = max(best, (unsigned)__shfl_xor((int)best, off, 64));
    if ((threadIdx.x & 63) == 0 && best) atomicMax(maxword, best);
}

// 2^k with max|gpool| 2^k in [2^40, 2^41); 1 for a zero gradient; 0 (nothing is added, the conversion writes NaN) when
// max|gpool| is inf or NaN
__device__ __forceinline__ double rgg_scale(unsigned maxword, bool *finite) {
    const int e = (int)(maxword >> 23);
    *finite = e != 255;
    if (e == 255) return 0.0;
    if (maxword == 0) return 1.0;
    return ldexp(1.0, RGT_FIXBITS - (max(e, 1) - 127));
}

// workgroup = partial `blockIdx.x`: its chunk of grid points, 256 / C1 at a time, thread = (point, channel).  The features'
// gradient goes to the fixed-point sums; the five parameter sums stay in registers over the chunk, are added across the
// workgroup's points in ascending order through LDS and written as the partial (5, C1): dwp x, y, z, dscale_p, dshift_p.
template <int C1>
__global__ __launch_bounds__(RGT_T) void roi_grid_pool_grad_kernel(long long M, int S, int P, int chunk, const float *__restrict__ gpool,
                                                                   const unsigned char *__restrict__ arg, const int *__restrict__ grp_row,
                                                                   const float *__restrict__ grp_off, const float *__restrict__ wp,
                                                                   const float *__restrict__ scale_p, const unsigned *__restrict__ maxword,
                                                                   unsigned long long *__restrict__ fixed, float *__restrict__ part) {
    constexpr int SUB = RGT_T / C1;
    __shared__ float s_sum[SUB][5][C1];
    const int c = threadIdx.x % C1, sub = threadIdx.x / C1;
    const float wpx = wp[c * 3], wpy = wp[c * 3 + 1], wpz = wp[c * 3 + 2], sp = scale_p[c];
    bool finite;
    const double scale = rgg_scale(*maxword, &finite);
    const long long m0 = (long long)blockIdx.x * chunk, m1 = min(m0 + chunk, M);
    float acc[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
    for (long long m = m0 + sub; m < m1; m += SUB) {
        const int s = arg[m * C1 + c];
        if (s >= S) continue;                   // 0xFF: the pooled value is 0 and passes no gradient
        const float g = gpool[m * C1 + c];
        acc[4] += g;
        const int row = grp_row[m * S + s];
        if (row < 0 || row >= P) continue;      // an empty group: shift_p alone
        const float *d = grp_off + (m * S + s) * 3;
        const float dx = d[0], dy = d[1], dz = d[2];
        const float dot = __fmaf_rn(wpz, dz, __fmaf_rn(wpy, dy, __fmul_rn(wpx, dx)));
        const float gs = g * sp;
        acc[0] += gs * dx; acc[1] += gs * dy; acc[2] += gs * dz;
        acc[3] += g * dot;
        if (finite) atomicAdd(&fixed[(size_t)row * C1 + c], (unsigned long long)llrint((double)g * scale));
    }
#pragma unroll
    for (int j = 0; j < 5; ++j) s_sum[sub][j][c] = acc[j];
    __syncthreads();
    for (int q = threadIdx.x; q < 5 * C1; q += RGT_T) {
        const int j = q / C1, cc = q % C1;
        float s = 0.0f;
        for (int u = 0; u < SUB; ++u) s += s_sum[u][j][cc];
        part[(size_t)blockIdx.x * 5 * C1 + q] = s;
    }
}

// every element of dfeatures_in (P, C1) from its fixed-point sum, zeros included, and (the first workgroup) the parameter
// gradients from the partials in ascending order
__global__ __launch_bounds__(RGT_T) void roi_grid_pool_grad_finish_kernel(long long count, int C1, int nparts, const unsigned *__restrict__ maxword,
                                                                          const unsigned long long *__restrict__ fixed,
                                                                          const float *__restrict__ part, float *__restrict__ dfeat,
                                                                          float *__restrict__ dwp, float *__restrict__ dscale,
                                                                          float *__restrict__ dshift) {
    bool finite;
    const double scale = rgg_scale(*maxword, &finite);
    const long long i = (long long)blockIdx.x * RGT_T + threadIdx.x;
    if (i < count) dfeat[i] = finite ? (float)((double)(long long)fixed[i] / scale) : __uint_as_float(0x7fc00000u);
    if (blockIdx.x != 0) return;
    for (int q = threadIdx.x; q < 5 * C1; q += RGT_T) {
        float s = 0.0f;
        for (int p = 0; p < nparts; ++p) s += part[(size_t)p * 5 * C1 + q];
        const int j = q / C1, c = q % C1;
        if (j < 3) dwp[c * 3 + j] = s;
        else if (j == 3) dscale[c] = s;
        else dshift[c] = s;
    }
}

static bool rgt_groups_ok(long long M, int nsample, int P, int C1) {
    return M >= 0 && P >= 0 && nsample >= 1 && nsample <= RGP_MAXS && (C1 == 16 || C1 == 32 || C1 == 64);
}

}  // namespace pdm

using namespace pdm;

extern "C" size_t pdm_roi_grid_query_workspace_bytes(long long M) {
    if (M < 0 || M > RGT_MAXM) return 0;
    return align256(sizeof(double) * 9 * (size_t)((M + RGP_TILE - 1) / RGP_TILE)) + 256;
}

// The geometry arguments and site_index as pdm_roi_grid_pool.  grp_row (M, nsample) int32, grp_off (M, nsample, 3) fp32, moments
// (9) float64 [sum x, y, z, xx, xy, xz, yy, yz, zz] over the padded tensor's M nsample slots; every element of the three is
// written.
extern "C" int pdm_roi_grid_query(void *stream, int B, int n, int roi_stride, const float *rois, int G, int D, int H, int W, int stride, float vx,
                                  float vy, float vz, float x0, float y0, float z0, int P, const void *site_index, size_t site_index_bytes, int rz,
                                  int ry, int rx, float radius, int nsample, int *grp_row, float *grp_off, double *moments, void *workspace,
                                  size_t workspace_bytes) {
    PDM_REQUIRE(B >= 0 && n >= 0 && P >= 0 && D >= 1 && H >= 1 && W >= 1 && roi_stride >= 7, PDM_E_BADARG, "roi_grid_query: bad size");
    PDM_REQUIRE(G >= 1 && G <= RGP_MAXG, PDM_E_BADARG, "roi_grid_query: grid size %d (1 to 8)", G);
    PDM_REQUIRE(rz >= 0 && ry >= 0 && rx >= 0 && rz <= RGP_MAXR && ry <= RGP_MAXR && rx <= RGP_MAXR, PDM_E_BADARG,
                "roi_grid_query: query range (%d, %d, %d): a window of at most 9 x 9 x 9", rz, ry, rx);
    PDM_REQUIRE(nsample >= 1 && nsample <= RGP_MAXS, PDM_E_BADARG, "roi_grid_query: nsample %d (1 to %d)", nsample, RGP_MAXS);
    PDM_REQUIRE(stride >= 1 && vx > 0.0f && vy > 0.0f && vz > 0.0f && radius >= 0.0f, PDM_E_BADARG, "roi_grid_query: bad stride, voxel size or radius");
    PDM_REQUIRE(si_grid_ok(B, D, H, W), PDM_E_TOOLARGE, "roi_grid_query: more than 2^35 cells");
    const long long M = (long long)B * n * G * G * G;
    PDM_REQUIRE(M <= RGT_MAXM, PDM_E_TOOLARGE, "roi_grid_query: %lld grid points exceed 2^22", M);
    PDM_REQUIRE((long long)B * n * roi_stride <= 0x7fffffffll, PDM_E_TOOLARGE, "roi_grid_query: roi elements exceed int32");
    PDM_REQUIRE(moments, PDM_E_BADARG, "roi_grid_query: null pointer");
    PDM_REQUIRE((reinterpret_cast<uintptr_t>(moments) & 7) == 0, PDM_E_BADARG, "roi_grid_query: moments must be 8-byte aligned");
    if (M == 0) return zero_fill(stream, "roi_grid_query", moments, 9 * sizeof(double));
    PDM_REQUIRE(rois && site_index && grp_row && grp_off && workspace, PDM_E_BADARG, "roi_grid_query: null pointer");
    PDM_WS_ALIGNED("roi_grid_query", site_index);
    PDM_WS_ALIGNED("roi_grid_query", workspace);
    const SiWorkspace w = si_workspace(P, B, D, H, W);
    PDM_REQUIRE(site_index_bytes >= w.total, PDM_E_BADARG, "roi_grid_query: site index too small (%zu bytes, need %zu)", site_index_bytes, w.total);
    const size_t need = pdm_roi_grid_query_workspace_bytes(M);
    PDM_REQUIRE(workspace_bytes >= need, PDM_E_BADARG, "roi_grid_query: workspace too small (%zu bytes, need %zu)", workspace_bytes, need);
    char *ws = const_cast<char *>(static_cast<const char *>(site_index));
    const ScIndex ix = sc_index_at(ws + w.index, w.isz);
    RgqArgs a{};
    a.M = M; a.n = n; a.G = G; a.roi_stride = roi_stride;
    a.B = B; a.D = D; a.H = H; a.W = W; a.P = P; a.stride = stride;
    a.vox[0] = vx; a.vox[1] = vy; a.vox[2] = vz; a.r0[0] = x0; a.r0[1] = y0; a.r0[2] = z0;
    a.rz = rz; a.ry = ry; a.rx = rx; a.nsample = nsample; a.radius = radius;
    a.rois = rois; a.bits = ix.bits; a.gprefix = ix.gprefix; a.row_of_rank = reinterpret_cast<const int *>(ws + w.row_of_rank);
    a.grp_row = grp_row; a.grp_off = grp_off; a.part = static_cast<double *>(workspace);
    const long long ntiles = (M + RGP_TILE - 1) / RGP_TILE;
    const dim3 grid((unsigned)min((long long)RGT_MAXBLOCKS, (ntiles + RGT_T / 64 - 1) / (RGT_T / 64)));
    hipStream_t s = as_stream(stream);
    hipLaunchKernelGGL(roi_grid_query_kernel, grid, dim3(RGT_T), 0, s, a);
    if (int rc = check_launch("roi_grid_query")) return rc;
    hipLaunchKernelGGL(roi_grid_moments_kernel, dim3(1), dim3(RGT_T), 0, s, ntiles, a.part, moments);
    return check_launch("roi_grid_query");
}

// grp_row / grp_off: what pdm_roi_grid_query left; a row outside [0, P) ends its group.  pooled (M, C1) fp32, arg (M, C1) uint8.
extern "C" int pdm_roi_grid_pool_train(void *stream, long long M, int nsample, int P, int C1, const int *grp_row, const float *grp_off,
                                       const float *features_in, const float *wp, const float *scale_p, const float *shift_p, float *pooled,
                                       unsigned char *arg) {
    PDM_REQUIRE(C1 == 16 || C1 == 32 || C1 == 64, PDM_E_BADARG, "roi_grid_pool_train: %d pooled channels (16, 32 or 64)", C1);
    PDM_REQUIRE(nsample >= 1 && nsample <= RGP_MAXS, PDM_E_BADARG, "roi_grid_pool_train: nsample %d (1 to %d)", nsample, RGP_MAXS);
    PDM_REQUIRE(rgt_groups_ok(M, nsample, P, C1), PDM_E_BADARG, "roi_grid_pool_train: bad size");
    PDM_REQUIRE(M <= RGT_MAXM, PDM_E_TOOLARGE, "roi_grid_pool_train: %lld grid points exceed 2^22", M);
    PDM_REQUIRE((long long)P * C1 <= 0x7fffffffll, PDM_E_TOOLARGE, "roi_grid_pool_train: feature elements exceed int32");
    if (M == 0) return 0;
    PDM_REQUIRE(grp_row && grp_off && wp && scale_p && shift_p && pooled && arg && (P == 0 || features_in), PDM_E_BADARG,
                "roi_grid_pool_train: null pointer");
    const dim3 grid((unsigned)((M * C1 + RGT_T - 1) / RGT_T));
    hipStream_t s = as_stream(stream);
    switch (C1) {
        case 16: hipLaunchKernelGGL(roi_grid_pool_train_kernel<16>, grid, dim3(RGT_T), 0, s, M, nsample, P, grp_row, grp_off, features_in, wp, scale_p, shift_p, pooled, arg); break;
        case 32: hipLaunchKernelGGL(roi_grid_pool_train_kernel<32>, grid, dim3(RGT_T), 0, s, M, nsample, P, grp_row, grp_off, features_in, wp, scale_p, shift_p, pooled, arg); break;
        default: hipLaunchKernelGGL(roi_grid_pool_train_kernel<64>, grid, dim3(RGT_T), 0, s, M, nsample, P, grp_row, grp_off, features_in, wp, scale_p, shift_p, pooled, arg); break;
    }
    return check_launch("roi_grid_pool_train");
}

extern "C" int pdm_roi_grid_pool_grad_chunk_points(long long M, int C1) {
    if (M < 0 || M > RGT_MAXM || !(C1 == 16 || C1 == 32 || C1 == 64)) return 0;
    return rgg_chunk(M, C1);
}

extern "C" size_t pdm_roi_grid_pool_grad_workspace_bytes(long long M, int P, int C1) {
    if (M < 0 || M > RGT_MAXM || P < 0 || !(C1 == 16 || C1 == 32 || C1 == 64) || (long long)P * C1 > 0x7fffffffll) return 0;
    return rgg_workspace(M, P, C1).total;
}

// gpool (M, C1): the gradient of pooled -> dfeatures_in (P, C1), dwp (C1, 3), dscale_p, dshift_p (C1), every element written.
extern "C" int pdm_roi_grid_pool_grad(void *stream, long long M, int nsample, int P, int C1, const float *gpool, const unsigned char *arg,
                                      const int *grp_row, const float *grp_off, const float *wp, const float *scale_p, float *dfeatures_in,
                                      float *dwp, float *dscale_p, float *dshift_p, void *workspace, size_t workspace_bytes) {
    PDM_REQUIRE(C1 == 16 || C1 == 32 || C1 == 64, PDM_E_BADARG, "roi_grid_pool_grad: %d pooled channels (16, 32 or 64)", C1);
    PDM_REQUIRE(nsample >= 1 && nsample <= RGP_MAXS, PDM_E_BADARG, "roi_grid_pool_grad: nsample %d (1 to %d)", nsample, RGP_MAXS);
    PDM_REQUIRE(rgt_groups_ok(M, nsample, P, C1), PDM_E_BADARG, "roi_grid_pool_grad: bad size");
    PDM_REQUIRE(M <= RGT_MAXM, PDM_E_TOOLARGE, "roi_grid_pool_grad: %lld grid points exceed 2^22", M);
    PDM_REQUIRE((long long)P * C1 <= 0x7fffffffll, PDM_E_TOOLARGE, "roi_grid_pool_grad: feature elements exceed int32");
    PDM_REQUIRE(dwp && dscale_p && dshift_p && workspace && (P == 0 || dfeatures_in), PDM_E_BADARG, "roi_grid_pool_grad: null pointer");
    PDM_REQUIRE(M == 0 || (gpool && arg && grp_row && grp_off && wp && scale_p), PDM_E_BADARG, "roi_grid_pool_grad: null pointer");
    PDM_WS_ALIGNED("roi_grid_pool_grad", workspace);
    const RggWorkspace w = rgg_workspace(M, P, C1);
    PDM_REQUIRE(workspace_bytes >= w.total, PDM_E_BADARG, "roi_grid_pool_grad: workspace too small (%zu bytes, need %zu)", workspace_bytes, w.total);
    char *ws = static_cast<char *>(workspace);
    unsigned *maxword = reinterpret_cast<unsigned *>(ws + w.maxword);
    unsigned long long *fixed = reinterpret_cast<unsigned long long *>(ws + w.fixed);
    float *part = reinterpret_cast<float *>(ws + w.part);
    hipStream_t s = as_stream(stream);
    const long long count = (long long)P * C1;
    if (int rc = zero_fill(stream, "roi_grid_pool_grad", ws, w.part)) return rc;        // the maximum and the fixed-point sums
    if (M > 0) {
        const long long gcount = M * C1;
        const dim3 mgrid((unsigned)min(1024ll, (gcount + RGT_T - 1) / RGT_T));
        hipLaunchKernelGGL(roi_grid_absmax_kernel, mgrid, dim3(RGT_T), 0, s, gcount, gpool, maxword);
        if (int rc = check_launch("roi_grid_pool_grad")) return rc;
        const dim3 grid((unsigned)w.nparts);
        switch (C1) {
            case 16: hipLaunchKernelGGL(roi_grid_pool_grad_kernel<16>, grid, dim3(RGT_T), 0, s, M, nsample, P, w.chunk, gpool, arg, grp_row, grp_off, wp, scale_p, maxword, fixed, part); break;
            case 32: hipLaunchKernelGGL(roi_grid_pool_grad_kernel<32>, grid, dim3(RGT_T), 0, s, M, nsample, P, w.chunk, gpool, arg, grp_row, grp_off, wp, scale_p, maxword, fixed, part); break;
            default: hipLaunchKernelGGL(roi_grid_pool_grad_kernel<64>, grid, dim3(RGT_T), 0, s, M, nsample, P, w.chunk, gpool, arg, grp_row, grp_off, wp, scale_p, maxword, fixed, part); break;
        }
        if (int rc = check_launch("roi_grid_pool_grad")) return rc;
    }
    const dim3 fgrid((unsigned)max(1ll, (count + RGT_T - 1) / RGT_T));
    hipLaunchKernelGGL(roi_grid_pool_grad_finish_kernel, fgrid, dim3(RGT_T), 0, s, count, C1, w.nparts, maxword, fixed, part, dfeatures_in, dwp, dscale_p,
                       dshift_p);
    return check_launch("roi_grid_pool_grad");
}

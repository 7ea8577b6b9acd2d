// Voxel R-CNN's RoI-grid pooling over one level of the voxel backbone, one launch per (level, scale): for every
// grid point of every RoI, the voxel-window query, the gather of the level's features after mlps_in, the position term, ReLU,
// the max over the group and the output layer.  None of the composed formulation's intermediates exists: no dense
// (B, Z, Y, X) table (the level's occupancy index of sc_index.h answers "which row is at this cell"), no (M, nsample) index
// rows, no grouped (M, C, nsample) tensors.
//
// A wave owns a tile of 16 consecutive grid points, formed one per lane and handed round by shuffles.  Per point: 64 window
// cells a step in the reference's order (z outer, x inner), the sphere tested first (it needs no memory), then the bit, the rank
// taken for set cells only, a ballot compaction of the hits into the first nsample, early exit at nsample.  Then the lanes turn
// into channels: lane c gathers channel c of every hit row, adds the position term and keeps the maximum of the ReLUs (C1 < 64:
// 64 / C1 hits at a time and a cross-lane maximum, which is exact).  The pooled row goes to LDS; after 16 rows the wave runs C1 -> C2 on mfma_f32_16x16x4f32 (weights in the packed
// fragment order of sparse_conv_mfma.hip, staged once per workgroup) and the epilogue relu(acc * scale + shift), written at
// a column offset into rows of the full stride.  No atomics and nothing summed across waves: two runs and a graph replay give
// the same bits.
#include "mfma_f32.h"
#include "roi_grid_geom.h"

namespace pdm {

constexpr int RGP_T = 256;          // 4 waves
constexpr int RGP_MAXBLOCKS = 2048; // workgroups at most; waves walk the tiles with this stride

struct RgpArgs {
    long long M;            // B n G^3 grid points
    int n, G, roi_stride;   // rois per sample, grid size, floats per roi row
    int B, D, H, W, P, stride;
    float vox[3], r0[3];    // (x, y, z): the BASE voxel size and the range minimum
    int rz, ry, rx, nsample;
    float radius;
    int out_stride, out_offset;
    const float *rois;
    const unsigned *bits;
    const int *gprefix, *row_of_rank;
    const float *feat;      // (P, C1)
    const float *wp, *scale_p, *shift_p;    // (C1, 3), (C1), (C1)
    const float *wout, *scale_o, *shift_o;  // packed (C2, C1), (C2), (C2)
    float *out;
};

template <int C1, int NB>
__global__ __launch_bounds__(RGP_T) void roi_grid_pool_kernel(RgpArgs a) {
    constexpr int NKB = C1 / 16, SUB = 64 / C1;
    __shared__ __attribute__((aligned(16))) float s_w[NKB * NB * 256];
    __shared__ __attribute__((aligned(16))) float s_pool[RGP_T / 64][NKB * RGP_TILE * MFMA_ROW_STRIDE];
    __shared__ int s_hrow[RGP_T / 64][RGP_MAXS];
    __shared__ float s_hd[RGP_T / 64][RGP_MAXS * 3];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);

    for (int q = tid; q < NKB * NB * 64; q += RGP_T) reinterpret_cast<f4 *>(s_w)[q] = reinterpret_cast<const f4 *>(a.wout)[q];
    __syncthreads();

    const int c = lane % C1, sub = lane / C1;       // gather role: channel c of the hits sub, sub + SUB, ...
    const float wpx = a.wp[c * 3], wpy = a.wp[c * 3 + 1], wpz = a.wp[c * 3 + 2], sp = a.scale_p[c], hp = a.shift_p[c];
    const RgpWalk k = rgp_walk_of(a);
    const long long ntiles = (a.M + RGP_TILE - 1) / RGP_TILE;
    float *pool = s_pool[wave];
    int *hrow = s_hrow[wave];
    float *hd = s_hd[wave];

    for (long long tile = (long long)blockIdx.x * (RGP_T / 64) + wave; tile < ntiles; tile += (long long)gridDim.x * (RGP_T / 64)) {
        float pgx, pgy, pgz;
        int pcx, pcy, pcz, pb;
        rgp_tile_points(a, k, tile, lane, pgx, pgy, pgz, pcx, pcy, pcz, pb);
        for (int i = 0; i < RGP_TILE; ++i) {
            if (tile * RGP_TILE + i >= a.M) break;
            const float gx = __shfl(pgx, i, 64), gy = __shfl(pgy, i, 64), gz = __shfl(pgz, i, 64);
            const int cx = __shfl(pcx, i, 64), cy = __shfl(pcy, i, 64), cz = __shfl(pcz, i, 64), b = __shfl(pb, i, 64);

            const int cnt = rgp_window_hits(a, k, lane, gx, gy, gz, cx, cy, cz, b, hrow, hd);
            __builtin_amdgcn_wave_barrier();

            // lanes are channels: max over the group of relu(feature + position term); an empty group is relu(shift_p)
            float v = 0.0f;
            if (cnt == 0) {
                v = hp < 0.0f ? 0.0f : hp;
            } else {
#pragma unroll 4
                for (int h = sub; h < cnt; h += SUB) {
                    const float f = a.feat[(size_t)hrow[h] * C1 + c];
                    const float dot = __fmaf_rn(wpz, hd[h * 3 + 2], __fmaf_rn(wpy, hd[h * 3 + 1], __fmul_rn(wpx, hd[h * 3])));
                    const float t = __fadd_rn(f, __fmaf_rn(dot, sp, hp));
                    v = fmaxf(v, t < 0.0f ? 0.0f : t);
                }
#pragma unroll
                for (int off = C1; off < 64; off <<= 1) v = fmaxf(v, __shfl_xor(v, off, 64));
            }
            if (lane < C1) pool[((c >> 4) * RGP_TILE + i) * MFMA_ROW_STRIDE + (c & 15)] = v;
            __builtin_amdgcn_wave_barrier();
        }

        // out rows of the tile: C1 -> C2 on the exact f32 MFMA (fragment layout: mfma_f32.h)
        const int pos = lane & 15, g = lane >> 4;
        f4 acc[NB];
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) acc[nb] = f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kb = 0; kb < NKB; ++kb) {
            const f4 fb = b_frag(pool, kb * RGP_TILE + pos, MFMA_ROW_STRIDE, 0, g);
#pragma unroll
            for (int nb = 0; nb < NB; ++nb) acc[nb] = mfma4(acc[nb], a_frag(s_w, kb * NB + nb, lane), fb);
        }
        __builtin_amdgcn_wave_barrier();        // the next tile's rows overwrite `pool`
        const long long m = tile * RGP_TILE + pos;
        if (m >= a.M) continue;
        float *orow = a.out + (size_t)m * a.out_stride + a.out_offset;
        const bool vec_o = ((reinterpret_cast<uintptr_t>(a.out) & 15) | ((a.out_stride | a.out_offset) & 3)) == 0;
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) {
            const int c0 = 16 * nb + 4 * g;
            store_quad(orow + c0, scale_shift_relu4(acc[nb], a.scale_o, a.shift_o, c0, true), vec_o);
        }
    }
}

template <int C1>
static void rgp_launch(int C2, dim3 grid, hipStream_t s, const RgpArgs &a) {
    switch (C2 / 16) {
        case 1: hipLaunchKernelGGL((roi_grid_pool_kernel<C1, 1>), grid, dim3(RGP_T), 0, s, a); break;
        case 2: hipLaunchKernelGGL((roi_grid_pool_kernel<C1, 2>), grid, dim3(RGP_T), 0, s, a); break;
        default: hipLaunchKernelGGL((roi_grid_pool_kernel<C1, 4>), grid, dim3(RGP_T), 0, s, a); break;
    }
}

}  // namespace pdm

using namespace pdm;

// rois (B, n, roi_stride >= 7) fp32 rows (x, y, z, dx, dy, dz, heading, ...); the level's grid (B, D, H, W) at `stride` times
// the base voxel (vx, vy, vz) from the range minimum (x0, y0, z0); site_index: the workspace pdm_sparse_index filled for the
// level's P rows on that grid; features_in (P, C1): the level's features after mlps_in; wp (C1, 3), scale_p, shift_p (C1): the
// folded mlps_pos; window half-widths (rz, ry, rx), radius, nsample; wout: the folded mlps_out weight (C2, C1) in
// pdm_sparse_conv's packed order (kvol = 1), scale_o, shift_o (C2).  Writes columns [out_offset, out_offset + C2) of the rows
// r G^3 + g of out (B n G^3, out_stride).
extern "C" int pdm_roi_grid_pool(void *stream, int B, int n, int roi_stride, const float *rois, int G, int D, int H, int W, int stride, float vx,
                                 float vy, float vz, float x0, float y0, float z0, int P, const void *site_index, size_t site_index_bytes, int C1,
                                 const float *features_in, const float *wp, const float *scale_p, const float *shift_p, int rz, int ry, int rx,
                                 float radius, int nsample, int C2, const float *wout, const float *scale_o, const float *shift_o, float *out,
                                 int out_stride, int out_offset) {
    PDM_REQUIRE(B >= 0 && n >= 0 && P >= 0 && D >= 1 && H >= 1 && W >= 1 && roi_stride >= 7, PDM_E_BADARG, "roi_grid_pool: bad size");
    PDM_REQUIRE(G >= 1 && G <= 8, PDM_E_BADARG, "roi_grid_pool: grid size %d (1 to 8)", G);
    PDM_REQUIRE(C1 == 16 || C1 == 32 || C1 == 64, PDM_E_BADARG, "roi_grid_pool: %d pooled channels (16, 32 or 64)", C1);
    PDM_REQUIRE(C2 == 16 || C2 == 32 || C2 == 64, PDM_E_BADARG, "roi_grid_pool: %d output channels (16, 32 or 64)", C2);
    PDM_REQUIRE(rz >= 0 && ry >= 0 && rx >= 0 && rz <= 4 && ry <= 4 && rx <= 4, PDM_E_BADARG,
                "roi_grid_pool: query range (%d, %d, %d): a window of at most 9 x 9 x 9", rz, ry, rx);
    PDM_REQUIRE(nsample >= 1 && nsample <= RGP_MAXS, PDM_E_BADARG, "roi_grid_pool: nsample %d (1 to %d)", nsample, RGP_MAXS);
    PDM_REQUIRE(stride >= 1 && vx > 0.0f && vy > 0.0f && vz > 0.0f && radius >= 0.0f, PDM_E_BADARG, "roi_grid_pool: bad stride, voxel size or radius");
    PDM_REQUIRE(out_offset >= 0 && out_stride >= 1 && (long long)out_offset + C2 <= out_stride, PDM_E_BADARG,
                "roi_grid_pool: columns [%d, %d) do not fit rows of %d", out_offset, out_offset + C2, out_stride);
    PDM_REQUIRE(si_grid_ok(B, D, H, W), PDM_E_TOOLARGE, "roi_grid_pool: more than 2^35 cells");
    const long long M = (long long)B * n * G * G * G;
    PDM_REQUIRE(M <= 0x7fffffffll && (long long)B * n * roi_stride <= 0x7fffffffll && (long long)P * C1 <= 0x7fffffffll, PDM_E_TOOLARGE,
                "roi_grid_pool: %lld grid points, roi or feature elements exceed int32", M);
    if (M == 0) return 0;
    PDM_REQUIRE(rois && site_index && wp && scale_p && shift_p && wout && scale_o && shift_o && out && (P == 0 || features_in), PDM_E_BADARG,
                "roi_grid_pool: null pointer");
    PDM_WS_ALIGNED("roi_grid_pool", site_index);
    PDM_REQUIRE((reinterpret_cast<uintptr_t>(wout) & 15) == 0, PDM_E_BADARG, "roi_grid_pool: packed weights must be 16-byte aligned");
    const SiWorkspace w = si_workspace(P, B, D, H, W);
    PDM_REQUIRE(site_index_bytes >= w.total, PDM_E_BADARG, "roi_grid_pool: site index too small (%zu bytes, need %zu)", site_index_bytes, w.total);
    char *ws = const_cast<char *>(static_cast<const char *>(site_index));
    const ScIndex ix = sc_index_at(ws + w.index, w.isz);
    RgpArgs a{};
    a.M = M; a.n = n; a.G = G; a.roi_stride = roi_stride;
    a.B = B; a.D = D; a.H = H; a.W = W; a.P = P; a.stride = stride;
    a.vox[0] = vx; a.vox[1] = vy; a.vox[2] = vz; a.r0[0] = x0; a.r0[1] = y0; a.r0[2] = z0;
    a.rz = rz; a.ry = ry; a.rx = rx; a.nsample = nsample; a.radius = radius;
    a.out_stride = out_stride; a.out_offset = out_offset;
    a.rois = rois; a.bits = ix.bits; a.gprefix = ix.gprefix; a.row_of_rank = reinterpret_cast<const int *>(ws + w.row_of_rank);
    a.feat = features_in; a.wp = wp; a.scale_p = scale_p; a.shift_p = shift_p; a.wout = wout; a.scale_o = scale_o; a.shift_o = shift_o;
    a.out = out;
    const long long ntiles = (M + RGP_TILE - 1) / RGP_TILE;
    const dim3 grid((unsigned)min((long long)RGP_MAXBLOCKS, (ntiles + RGP_T / 64 - 1) / (RGP_T / 64)));
    hipStream_t s = as_stream(stream);
    switch (C1) {
        case 16: rgp_launch<16>(C2, grid, s, a); break;
        case 32: rgp_launch<32>(C2, grid, s, a); break;
        default: rgp_launch<64>(C2, grid, s, a); break;
    }
    return check_launch("roi_grid_pool");
}

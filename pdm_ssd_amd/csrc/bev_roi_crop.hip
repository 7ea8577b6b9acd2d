// SECOND-IoU's RoI pooling: the rotated G x G crop of the 2-D backbone's map under every RoI of the batch, and the
// same crop followed by the head's first shared FC without the (R, C G^2) tensor in between.
//
// crop_tap / crop_blend are the ONE definition of where grid cell (i, j) of a RoI lies on the map and what is read there; both
// operators call them, so the fused form's crop has the bits of the stand-alone one.  The reference builds theta, an
// affine_grid and a grid_sample(align_corners=True, zeros) per sample; multiplied out, its pixel position is
//     px = hx cos(a) u - hx sin(a) v + cx,   py = hy sin(a) u + hy cos(a) v + cy
//     cx = (x - x0) / cell_x, hx = (dx / 2) / cell_x, cy = (y - y0) / cell_y, hy = (dy / 2) / cell_y,
//     u = (2 j - (G - 1)) / (G - 1), v = (2 i - (G - 1)) / (G - 1)
// (the terms (W - 1) and (H - 1) of theta cancel; hx multiplies BOTH terms of px and hy both of py: the reference's rule, not a
// rotation of the box's own axes).  fp32, one rounding per operation, in exactly the order written in crop_tap; nothing is
// contracted.  The value is ((v00 w00 + v01 w01) + v10 w10) + v11 w11 with w00 = (1 - fx)(1 - fy), w01 = fx (1 - fy),
// w10 = (1 - fx) fy, w11 = fx fy, fx = px - floor(px), fy likewise, and a corner outside the map is 0 and is not read.
//
// pdm_bev_roi_crop: a workgroup per (RoI, block of 64 channels).  The G^2 taps go to LDS once; the threads then walk the
// block's (channel, cell) pairs in output order, so the stores are one contiguous run and the reads of a wave fall on the few
// rows of a channel plane the RoI covers.  The map is read NCHW where it lies.
//
// pdm_bev_roi_crop_fc: a workgroup owns (32 RoIs) x (a chunk of the contraction) x (256 output channels).  The contraction index
// k = c G^2 + i G + j is the Conv1d's own column order, walked in stages of 128: the crop of the stage goes to LDS (32 x 128) and
// is the B operand of mfma_f32_16x16x4f32 against the weight's A fragments (packed [k / 16][Cout / 16][lane][4], sparse_fc.hip's
// layout with one cell).  A wave keeps its 4 x 2 accumulator tiles in registers over the whole chunk and writes them to
// partial[chunk]; fc_reduce.h adds the partials in ascending order and applies the epilogue.  The chunk boundaries are a function
// of (R, C, G, Cout) alone: no atomics, two runs give the same bits.
#include <algorithm>

#include "fc_reduce.h"
#include "mfma_f32.h"

namespace pdm {

constexpr int CROP_MAXG = 8;
constexpr int CROP_MAXSIDE = 32768;     // H, W at most: a plane's offsets stay below 2^30
struct CropGeom {
    float x0, y0, cell_x, cell_y;
    int H, W, G;
};
struct __align__(16) CropTap {
    int ix, iy;       // floor of the pixel position, -1 .. n - 1; (-4, -4) for a position no corner of which is on the map
    float fx, fy;     // the position's fraction
};

__device__ __forceinline__ CropTap crop_tap(const float *__restrict__ roi, const CropGeom &g, int i, int j) {
    const float cx = __fdiv_rn(__fsub_rn(roi[0], g.x0), g.cell_x), hx = __fdiv_rn(__fmul_rn(roi[3], 0.5f), g.cell_x);
    const float cy = __fdiv_rn(__fsub_rn(roi[1], g.y0), g.cell_y), hy = __fdiv_rn(__fmul_rn(roi[4], 0.5f), g.cell_y);
    float s, c;
    sincosf(roi[6], &s, &c);
    const float gm = (float)(g.G - 1);
    const float u = __fdiv_rn((float)(2 * j - (g.G - 1)), gm), v = __fdiv_rn((float)(2 * i - (g.G - 1)), gm);
    const float px = __fadd_rn(__fsub_rn(__fmul_rn(__fmul_rn(hx, c), u), __fmul_rn(__fmul_rn(hx, s), v)), cx);
    const float py = __fadd_rn(__fadd_rn(__fmul_rn(__fmul_rn(hy, s), u), __fmul_rn(__fmul_rn(hy, c), v)), cy);
    CropTap t{-4, -4, 0.0f, 0.0f};
    // (a NaN position fails the test: zeros)
    if (px > -1.0f && px < (float)g.W && py > -1.0f && py < (float)g.H) {
        const float flx = floorf(px), fly = floorf(py);
        t.ix = (int)flx;
        t.iy = (int)fly;
        t.fx = __fsub_rn(px, flx);
        t.fy = __fsub_rn(py, fly);
    }
    return t;
}

// im: one channel's (H, W) plane
__device__ __forceinline__ float crop_blend(const float *__restrict__ im, int H, int W, const CropTap &t) {
    const bool xl = (unsigned)t.ix < (unsigned)W, xr = (unsigned)(t.ix + 1) < (unsigned)W;
    const bool yt = (unsigned)t.iy < (unsigned)H, yb = (unsigned)(t.iy + 1) < (unsigned)H;
    const int o = t.iy * W + t.ix;
    const float v00 = (yt && xl) ? im[o] : 0.0f, v01 = (yt && xr) ? im[o + 1] : 0.0f;
    const float v10 = (yb && xl) ? im[o + W] : 0.0f, v11 = (yb && xr) ? im[o + W + 1] : 0.0f;
    const float wx0 = __fsub_rn(1.0f, t.fx), wy0 = __fsub_rn(1.0f, t.fy);
    const float top = __fadd_rn(__fmul_rn(v00, __fmul_rn(wx0, wy0)), __fmul_rn(v01, __fmul_rn(t.fx, wy0)));
    return __fadd_rn(__fadd_rn(top, __fmul_rn(v10, __fmul_rn(wx0, t.fy))), __fmul_rn(v11, __fmul_rn(t.fx, t.fy)));
}

// ---------------------------------------------------------------------------------------------------------------- the crop

constexpr int CROP_NT = 256;
constexpr int CROP_CCH = 64;            // channels a workgroup writes

__global__ __launch_bounds__(CROP_NT) void bev_roi_crop_kernel(int n, int roi_stride, const float *__restrict__ rois, int C,
                                                               const float *__restrict__ feat, CropGeom g, float *__restrict__ out,
                                                               long long ld) {
    __shared__ CropTap s_tap[CROP_MAXG * CROP_MAXG];
    const int r = blockIdx.x, GG = g.G * g.G, tid = threadIdx.x;
    if (tid < GG) s_tap[tid] = crop_tap(rois + (size_t)r * roi_stride, g, tid / g.G, tid % g.G);
    __syncthreads();
    const int c0 = blockIdx.y * CROP_CCH, total = min(CROP_CCH, C - c0) * GG;
    const size_t HW = (size_t)g.H * g.W;
    const float *plane0 = feat + ((size_t)(r / n) * C + c0) * HW;
    float *orow = out + (size_t)r * ld + (size_t)c0 * GG;
    // element e = (channel e / GG, cell e % GG) of the block, the output's own order; the pair is stepped, not divided
    int cl = tid / GG, p = tid % GG;
    const int dc = CROP_NT / GG, dp = CROP_NT % GG;
    for (int e = tid; e < total; e += CROP_NT) {
        orow[e] = crop_blend(plane0 + (size_t)cl * HW, g.H, g.W, s_tap[p]);
        cl += dc;
        p += dp;
        if (p >= GG) { p -= GG; ++cl; }
    }
}

// ------------------------------------------------------------------------------------------------------ crop + first FC

constexpr int CFC_NT = 256;
constexpr int CFC_TR = 32;              // RoIs a workgroup owns: two 16-wide B tiles
constexpr int CFC_KS = 128;             // contraction indices a stage holds in LDS
constexpr int CFC_XS = CFC_KS + 4;      // the staged rows' stride in floats
constexpr int CFC_NCO = 256;            // output channels a workgroup owns: 4 blocks of 16 per wave

struct CfcPlan {
    int tiles, cblocks, nstage, chunk_stages, nchunk;
};

static CfcPlan cfc_plan(int R, int C, int G, int Cout) {
    CfcPlan p;
    p.tiles = divup(std::max(R, 1), CFC_TR);
    p.cblocks = divup(Cout, CFC_NCO);
    p.nstage = divup((long long)C * G * G, CFC_KS);
    const SplitK k = split_k_plan(p.nstage, (long long)p.tiles * p.cblocks);
    p.chunk_stages = k.chunk;
    p.nchunk = k.nchunk;
    return p;
}

static size_t cfc_bytes(int R, int C, int G, int Cout) {
    return align256((size_t)cfc_plan(R, C, G, Cout).nchunk * R * Cout * sizeof(float));
}

struct CfcArgs {
    int R, n, roi_stride, C, Cout, K, nstage, chunk_stages;
    const float *rois, *feat, *wpack;
    CropGeom g;
    float *partial;
};

__global__ __launch_bounds__(CFC_NT) void bev_roi_crop_fc_kernel(CfcArgs a) {
    __shared__ CropTap s_tap[CFC_TR * CROP_MAXG * CROP_MAXG];     // 32 KiB
    __shared__ __align__(16) float s_x[CFC_TR * CFC_XS];          // 16.5 KiB: the stage's crop, (RoI, k)
    __shared__ int s_sample[CFC_TR];
    const int tid = threadIdx.x, lane = tid & 63, pos = lane & 15, gq = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int GG = a.g.G * a.g.G, NB = a.Cout / 16;
    const int r_lo = blockIdx.x * CFC_TR;
    const size_t HW = (size_t)a.g.H * a.g.W;
    for (int e = tid; e < CFC_TR * GG; e += CFC_NT) {
        const int t = e / GG, p = e - t * GG, r = r_lo + t;
        CropTap tap{-4, -4, 0.0f, 0.0f};            // a row past the last RoI: zeros, nothing read
        if (r < a.R) tap = crop_tap(a.rois + (size_t)r * a.roi_stride, a.g, p / a.g.G, p % a.g.G);
        s_tap[e] = tap;
    }
    if (tid < CFC_TR) s_sample[tid] = min(r_lo + tid, a.R - 1) / a.n;

    f4 acc[4][2];
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int t = 0; t < 2; ++t) acc[q][t] = f4{0.f, 0.f, 0.f, 0.f};
    const int nb0 = blockIdx.z * (CFC_NCO / 16) + wave;        // the wave's blocks of 16 channels: nb0 + 4 q

    const int s_lo = blockIdx.y * a.chunk_stages, s_hi = min(a.nstage, s_lo + a.chunk_stages);
    for (int s = s_lo; s < s_hi; ++s) {
        const int k0 = s * CFC_KS, ks = min(CFC_KS, a.K - k0);      // ks: a multiple of 16, as K is
        __syncthreads();        // the taps; the previous stage's reads of s_x
        for (int e = tid; e < CFC_TR * CFC_KS; e += CFC_NT) {
            const int t = e / CFC_KS, kk = e % CFC_KS;
            if (kk < ks) {
                const int k = k0 + kk, c = k / GG, p = k - c * GG;
                s_x[t * CFC_XS + kk] = crop_blend(a.feat + ((size_t)s_sample[t] * a.C + c) * HW, a.g.H, a.g.W, s_tap[t * GG + p]);
            }
        }
        __syncthreads();
        for (int kb = 0; kb < ks / 16; ++kb) {
            const f4 fb[2] = {b_frag(s_x, pos, CFC_XS, kb, gq), b_frag(s_x, 16 + pos, CFC_XS, kb, gq)};
            const size_t kbg = (size_t)(k0 / 16 + kb) * NB;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int nb = nb0 + 4 * q;
                if (nb < NB) {          // wave-uniform
                    mfma4_grid(acc[q], a_frag(a.wpack, kbg + nb, lane), fb);
                }
            }
        }
    }
    // D layout of mfma_f32.h: tile t is RoI r_lo + 16 t + pos, g = gq
    float *part = a.partial + (size_t)blockIdx.y * a.R * a.Cout;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int nb = nb0 + 4 * q;
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const int r = r_lo + 16 * t + pos;
            if (nb < NB && r < a.R) *reinterpret_cast<f4 *>(part + (size_t)r * a.Cout + 16 * nb + 4 * gq) = acc[q][t];
        }
    }
}

}  // namespace pdm

using namespace pdm;

static int crop_args(const char *who, int B, int n, int roi_stride, int C, int H, int W, float cell_x, float cell_y, int G) {
    PDM_REQUIRE(B >= 0 && n >= 0 && roi_stride >= 7, PDM_E_BADARG, "%s: bad size (B=%d n=%d roi_stride=%d)", who, B, n, roi_stride);
    PDM_REQUIRE(G >= 2 && G <= CROP_MAXG, PDM_E_BADARG, "%s: grid size %d (2 to %d; one cell has no corner-aligned lattice)", who, G, CROP_MAXG);
    PDM_REQUIRE(C >= 1 && H >= 2 && W >= 2, PDM_E_BADARG, "%s: map of C=%d H=%d W=%d (at least one channel and 2 x 2 cells)", who, C, H, W);
    PDM_REQUIRE(H <= CROP_MAXSIDE && W <= CROP_MAXSIDE && C <= 65536, PDM_E_TOOLARGE, "%s: map of C=%d H=%d W=%d (sides up to %d, 65536 channels)",
                who, C, H, W, CROP_MAXSIDE);
    PDM_REQUIRE(cell_x > 0.0f && cell_y > 0.0f && cell_x <= 3.0e38f && cell_y <= 3.0e38f, PDM_E_BADARG, "%s: cell size (%g, %g)", who, (double)cell_x,
                (double)cell_y);
    PDM_REQUIRE((long long)B * n * roi_stride <= 0x7fffffffll, PDM_E_TOOLARGE, "%s: %lld roi elements exceed int32", who, (long long)B * n * roi_stride);
    return 0;
}

extern "C" int pdm_bev_roi_crop(void *stream, int B, int n, int roi_stride, const float *rois, int C, int H, int W,
                                const float *spatial_features_2d, float x0, float y0, float cell_x, float cell_y, int G, float *pooled,
                                long long ld) {
    const int rc = crop_args("bev_roi_crop", B, n, roi_stride, C, H, W, cell_x, cell_y, G);
    if (rc) return rc;
    PDM_REQUIRE(ld >= (long long)C * G * G, PDM_E_BADARG, "bev_roi_crop: rows of %lld floats do not hold C G^2 = %lld", ld, (long long)C * G * G);
    const long long R = (long long)B * n;
    if (R == 0) return 0;
    PDM_REQUIRE(rois && spatial_features_2d && pooled, PDM_E_BADARG, "bev_roi_crop: null pointer");
    const CropGeom g{x0, y0, cell_x, cell_y, H, W, G};
    hipLaunchKernelGGL(bev_roi_crop_kernel, dim3((unsigned)R, (unsigned)divup(C, CROP_CCH)), dim3(CROP_NT), 0, as_stream(stream), n, roi_stride,
                       rois, C, spatial_features_2d, g, pooled, ld);
    return check_launch("bev_roi_crop");
}

static bool cfc_sizes_ok(int C, int G, int Cout) {
    return G >= 2 && G <= CROP_MAXG && C >= 16 && C % 16 == 0 && C <= 512 && Cout >= 16 && Cout % 16 == 0 && Cout <= 1024;
}

extern "C" size_t pdm_bev_roi_crop_fc_packed_floats(int C, int G, int Cout) {
    return cfc_sizes_ok(C, G, Cout) ? (size_t)C * G * G * Cout : 0;
}

extern "C" int pdm_bev_roi_crop_fc_chunks(int R, int C, int G, int Cout) {
    return (R >= 0 && cfc_sizes_ok(C, G, Cout)) ? cfc_plan(R, C, G, Cout).nchunk : 0;
}

extern "C" size_t pdm_bev_roi_crop_fc_workspace_bytes(int R, int C, int G, int Cout) {
    return (R > 0 && cfc_sizes_ok(C, G, Cout)) ? cfc_bytes(R, C, G, Cout) : 0;
}

extern "C" int pdm_bev_roi_crop_fc(void *stream, int B, int n, int roi_stride, const float *rois, int C, int H, int W,
                                   const float *spatial_features_2d, float x0, float y0, float cell_x, float cell_y, int G, int Cout,
                                   const float *wpack, const float *scale, const float *shift, int relu, float *out, void *workspace,
                                   size_t workspace_bytes) {
    const int rc = crop_args("bev_roi_crop_fc", B, n, roi_stride, C, H, W, cell_x, cell_y, G);
    if (rc) return rc;
    PDM_REQUIRE(C % 16 == 0 && C <= 512, PDM_E_BADARG, "bev_roi_crop_fc: C=%d (a multiple of 16 up to 512)", C);
    PDM_REQUIRE(Cout >= 16 && Cout % 16 == 0 && Cout <= 1024, PDM_E_BADARG, "bev_roi_crop_fc: Cout=%d (a multiple of 16 up to 1024)", Cout);
    const long long R = (long long)B * n;
    PDM_REQUIRE(R * Cout < (1ll << 31), PDM_E_TOOLARGE, "bev_roi_crop_fc: R * Cout = %lld", R * Cout);
    PDM_REQUIRE((scale == nullptr) == (shift == nullptr), PDM_E_BADARG, "bev_roi_crop_fc: one of scale and shift without the other");
    if (R == 0) return 0;
    PDM_REQUIRE(rois && spatial_features_2d && wpack && out, PDM_E_BADARG, "bev_roi_crop_fc: null pointer");
    PDM_REQUIRE((reinterpret_cast<uintptr_t>(wpack) & 15) == 0, PDM_E_BADARG, "bev_roi_crop_fc: the packed weight is read 16 bytes at a time: 16-byte aligned");
    const size_t need = cfc_bytes((int)R, C, G, Cout);
    PDM_REQUIRE(workspace && workspace_bytes >= need, PDM_E_BADARG, "bev_roi_crop_fc: workspace of %zu bytes, need %zu", workspace_bytes, need);
    PDM_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 15) == 0, PDM_E_BADARG, "bev_roi_crop_fc: workspace must be 16-byte aligned");
    const CfcPlan plan = cfc_plan((int)R, C, G, Cout);
    CfcArgs a{(int)R, n, roi_stride, C, Cout, C * G * G, plan.nstage, plan.chunk_stages, rois, spatial_features_2d, wpack,
              CropGeom{x0, y0, cell_x, cell_y, H, W, G}, static_cast<float *>(workspace)};
    hipStream_t st = as_stream(stream);
    hipLaunchKernelGGL(bev_roi_crop_fc_kernel, dim3(plan.tiles, plan.nchunk, plan.cblocks), dim3(CFC_NT), 0, st, a);
    hipLaunchKernelGGL(fc_reduce_kernel, dim3(divup(R * Cout, FCR_NT)), dim3(FCR_NT), 0, st, (int)R, Cout, plan.nchunk, a.partial, scale, shift, relu,
                       out);
    return check_launch("bev_roi_crop_fc");
}

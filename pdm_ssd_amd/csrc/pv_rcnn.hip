// PV-RCNN's two operators.
//
// pdm_bev_interpolate: the bilinear sample of the BEV map at every keypoint of the batch, one launch, straight from the NCHW
// map HeightCompression leaves and into a column range of the keypoints' wider feature rows.  A wave owns a keypoint, a lane
// a channel: the four corner loads are strided by H W floats across the lanes in either mapping (every (keypoint, channel)
// pair is two cache lines of its own, the x0 / x1 corners of a row sharing one), so the mapping is chosen for the store, which
// is then one contiguous run of C floats, and for the index arithmetic, which is wave-uniform.  The arithmetic is
// bilinear_interpolate_torch's, operation for operation: IEEE divisions for the indices, the floor, both corners clamped, the
// weights taken from the CLAMPED corners (negative ones beyond the border included), Ia wa + Ib wb + Ic wc + Id wd summed left
// to right, nothing contracted.
//
// pdm_roi_keypoint_query: the grid points of every RoI (roi_grid_geom.h's rgp_grid_point: Voxel R-CNN's lattice and fp32
// operation order) and, for up to two radii at once, stack_ball_query_kernel's neighbour rows over the keypoints of the RoI's
// sample.  A workgroup serves 64 grid points of ONE sample and stages that sample's keypoint coordinates in LDS once (struct
// of arrays: lane k of a step reads word base + k, no bank conflict); a wave owns 16 of the points, formed one per lane and
// handed round by shuffles, and walks the staged keypoints 64 candidates a step, testing every candidate against all radii in
// the one pass: pinned squared distance, strict <, ballot-ordered writes of the first nsample by index, early exit once every
// scale is full, padding with the first hit, an empty ball flagged and given row 0 of its sample.  The rows hold GLOBAL
// (stacked-row) indices.  No atomics, nothing summed: two runs and a graph replay give the same bits.
#include "roi_grid_geom.h"

namespace pdm {

constexpr int BEVI_T = 256;             // 4 waves, a keypoint each
constexpr int BEVI_MAXBLOCKS = 8192;

__global__ __launch_bounds__(BEVI_T) void bev_interpolate_kernel(int K, const float *__restrict__ kp, int B, int C, int H, int W,
                                                                 const float *__restrict__ feat, float x0, float y0, float vx, float vy,
                                                                 float stride, float *__restrict__ out, int ld, int col0) {
    const int lane = threadIdx.x & 63;
    const size_t HW = (size_t)H * W;
    for (int k = blockIdx.x * (BEVI_T / 64) + (threadIdx.x >> 6); k < K; k += gridDim.x * (BEVI_T / 64)) {
        const float *p = kp + (size_t)k * 4;
        const float bf = p[0];
        float *orow = out + (size_t)k * ld + col0;
        if (!(bf >= 0.0f && bf < (float)B)) {        // a row of no sample (or NaN): zeros, no load
            for (int c = lane; c < C; c += 64) orow[c] = 0.0f;
            continue;
        }
        const int b = (int)bf;
        const float x = __fdiv_rn(__fdiv_rn(__fsub_rn(p[1], x0), vx), stride);
        const float y = __fdiv_rn(__fdiv_rn(__fsub_rn(p[2], y0), vy), stride);
        const float fx = floorf(x), fy = floorf(y);
        const float wm = (float)(W - 1), hm = (float)(H - 1);
        // clamp(floor, 0, n - 1) and clamp(floor + 1, 0, n - 1) as the integers they are (NaN -> 0)
        const float x0f = fx > 0.0f ? (fx < wm ? fx : wm) : 0.0f, x1c = __fadd_rn(fx, 1.0f), x1f = x1c > 0.0f ? (x1c < wm ? x1c : wm) : 0.0f;
        const float y0f = fy > 0.0f ? (fy < hm ? fy : hm) : 0.0f, y1c = __fadd_rn(fy, 1.0f), y1f = y1c > 0.0f ? (y1c < hm ? y1c : hm) : 0.0f;
        const float wa = __fmul_rn(__fsub_rn(x1f, x), __fsub_rn(y1f, y));
        const float wb = __fmul_rn(__fsub_rn(x1f, x), __fsub_rn(y, y0f));
        const float wc = __fmul_rn(__fsub_rn(x, x0f), __fsub_rn(y1f, y));
        const float wd = __fmul_rn(__fsub_rn(x, x0f), __fsub_rn(y, y0f));
        const int ix0 = (int)x0f, ix1 = (int)x1f, iy0 = (int)y0f, iy1 = (int)y1f;
        const size_t oa = (size_t)iy0 * W + ix0, ob = (size_t)iy1 * W + ix0, oc = (size_t)iy0 * W + ix1, od = (size_t)iy1 * W + ix1;
        const float *plane = feat + (size_t)b * C * HW;
        for (int c = lane; c < C; c += 64) {
            const float *im = plane + (size_t)c * HW;
            const float ia = im[oa], ib = im[ob], ic = im[oc], id = im[od];
            orow[c] = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(ia, wa), __fmul_rn(ib, wb)), __fmul_rn(ic, wc)), __fmul_rn(id, wd));
        }
    }
}

constexpr int RKQ_T = 256;              // 4 waves of 16 grid points
constexpr int RKQ_POINTS = (RKQ_T / 64) * RGP_TILE;
constexpr int RKQ_CAP = 4096;           // keypoints of one sample at most: 48 KiB of LDS (the reference's 2048: 24 KiB)
constexpr int RKQ_MAXS = 64;            // nsample at most: the padding is one pass of the wave

struct RkqArgs {
    int B, n, G, roi_stride, K, cap;    // cap: the caller's bound on a sample's keypoints = the LDS staged
    int nscales, nsample[2];
    float radius[2];
    const float *rois, *xyz;
    const int *cnt;
    float *grid;
    int *idx[2];
    unsigned char *empty[2];
};

__global__ __launch_bounds__(RKQ_T) void roi_keypoint_query_kernel(RkqArgs a) {
    extern __shared__ float s_kp[];     // x[cap], y[cap], z[cap]
    __shared__ int s_start;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int b = blockIdx.y;
    if (wave == 0) {                    // the sample's first stacked row: the sum of the counts in front of it
        int acc = 0;
        for (int k = lane; k < b; k += 64) acc += max(a.cnt[k], 0);
#pragma unroll
        for (int off = 32; off; off >>= 1) acc += __shfl_xor(acc, off, 64);
        if (lane == 0) s_start = acc;
    }
    __syncthreads();
    const int start = min(s_start, a.K);
    // never past the stacked rows, never past what the caller said a sample holds (a bound that does not hold cuts the sample)
    const int nk = min(min(max(a.cnt[b], 0), a.K - start), a.cap);
    float *sx = s_kp, *sy = s_kp + a.cap, *sz = s_kp + 2 * a.cap;
    for (int k = tid; k < nk; k += RKQ_T) {
        const float *p = a.xyz + (size_t)(start + k) * 3;
        sx[k] = p[0]; sy[k] = p[1]; sz[k] = p[2];
    }
    __syncthreads();

    const int G3 = a.G * a.G * a.G, per = a.n * G3;                 // grid points of one sample
    const int local0 = blockIdx.x * RKQ_POINTS + wave * RGP_TILE;   // the wave's first point within the sample
    if (local0 >= per) return;
    const int mine = min(local0 + (lane & 15), per - 1);
    const int r = mine / G3;
    float pgx, pgy, pgz;
    rgp_grid_point(a.rois + ((size_t)b * a.n + r) * a.roi_stride, a.G, mine - r * G3, pgx, pgy, pgz);
    const size_t m0 = (size_t)b * per + local0;
    if (lane < RGP_TILE && local0 + lane < per) {
        float *g = a.grid + (m0 + lane) * 3;
        g[0] = pgx; g[1] = pgy; g[2] = pgz;
    }
    const float r2a = __fmul_rn(a.radius[0], a.radius[0]), r2b = __fmul_rn(a.radius[1], a.radius[1]);
    const int nsa = a.nsample[0], nsb = a.nscales > 1 ? a.nsample[1] : 0;
    const int row0 = min(start, max(a.K - 1, 0));                   // row 0 of the sample (of an empty last sample: the last row there is)

    for (int i = 0; i < RGP_TILE && local0 + i < per; ++i) {
        const float gx = __shfl(pgx, i, 64), gy = __shfl(pgy, i, 64), gz = __shfl(pgz, i, 64);
        int *outa = a.idx[0] + (m0 + i) * nsa;
        int *outb = nsb ? a.idx[1] + (m0 + i) * nsb : nullptr;
        int ca = 0, cb = 0, fa = -1, fb = -1;
        for (int base = 0; base < nk && (ca < nsa || cb < nsb); base += 64) {
            const int k = base + lane;
            bool ha = false, hb = false;
            if (k < nk) {
                const float d = sqdist(gx - sx[k], gy - sy[k], gz - sz[k]);
                ha = d < r2a;
                hb = nsb && d < r2b;
            }
            const unsigned long long ma = __ballot(ha), mb = __ballot(hb);
            if (ma && ca < nsa) {
                if (ca == 0) fa = base + __ffsll((long long)ma) - 1;
                const int rank = ca + lanes_below(ma, lane);
                if (ha && rank < nsa) outa[rank] = start + k;
                ca += __popcll(ma);
            }
            if (mb && cb < nsb) {
                if (cb == 0) fb = base + __ffsll((long long)mb) - 1;
                const int rank = cb + lanes_below(mb, lane);
                if (hb && rank < nsb) outb[rank] = start + k;
                cb += __popcll(mb);
            }
        }
        // padding with the first hit; an empty ball: every slot row 0 of the sample, and the flag
        for (int l = ca + lane; l < nsa; l += 64) outa[l] = ca ? start + fa : row0;
        if (lane == 0) a.empty[0][m0 + i] = ca == 0;
        if (nsb) {
            for (int l = cb + lane; l < nsb; l += 64) outb[l] = cb ? start + fb : row0;
            if (lane == 0) a.empty[1][m0 + i] = cb == 0;
        }
    }
}

}  // namespace pdm

using namespace pdm;

// keypoints (K, 4) fp32 rows (b, x, y, z); spatial_features (B, C, H, W) fp32, contiguous; writes columns [col0, col0 + C) of
// the rows of out (K, ld).
extern "C" int pdm_bev_interpolate(void *stream, int K, const float *keypoints, int B, int C, int H, int W, const float *spatial_features,
                                   float x0, float y0, float vx, float vy, int bev_stride, float *out, int ld, int col0) {
    PDM_REQUIRE(K >= 0 && B >= 1 && C >= 1 && H >= 1 && W >= 1, PDM_E_BADARG, "bev_interpolate: bad size (K=%d B=%d C=%d H=%d W=%d)", K, B, C, H, W);
    PDM_REQUIRE(vx > 0.0f && vy > 0.0f && bev_stride >= 1, PDM_E_BADARG, "bev_interpolate: bad voxel size or stride");
    PDM_REQUIRE(col0 >= 0 && ld >= 1 && (long long)col0 + C <= ld, PDM_E_BADARG, "bev_interpolate: columns [%d, %d) do not fit rows of %d", col0,
                col0 + C, ld);
    PDM_REQUIRE(H <= (1 << 20) && W <= (1 << 20), PDM_E_TOOLARGE, "bev_interpolate: a map side above 2^20");
    if (K == 0) return 0;
    PDM_REQUIRE(keypoints && spatial_features && out, PDM_E_BADARG, "bev_interpolate: null pointer");
    const int blocks = (int)min((long long)BEVI_MAXBLOCKS, ((long long)K + BEVI_T / 64 - 1) / (BEVI_T / 64));
    hipLaunchKernelGGL(bev_interpolate_kernel, dim3(blocks), dim3(BEVI_T), 0, as_stream(stream), K, keypoints, B, C, H, W, spatial_features, x0, y0,
                       vx, vy, (float)bev_stride, out, ld, col0);
    return check_launch("bev_interpolate");
}

// the most keypoints a sample may hold (max_per_sample) for pdm_roi_keypoint_query to serve it
extern "C" int pdm_roi_keypoint_query_cap(void) { return RKQ_CAP; }

// rois (B, n, roi_stride >= 7); xyz (K, 3): the keypoints of all samples, stacked; xyz_batch_cnt (B) int32 on the device, at
// most max_per_sample each (a host bound: it sizes the LDS; a sample above it is cut to its first max_per_sample keypoints).
// grid_points (B n G^3, 3); per scale s < nscales: idx_s (B n G^3, nsample_s) int32 global rows, empty_s (B n G^3) bytes.
extern "C" int pdm_roi_keypoint_query(void *stream, int B, int n, int roi_stride, const float *rois, int G, int K, const float *xyz,
                                      const int *xyz_batch_cnt, int max_per_sample, int nscales, float radius0, int nsample0, float radius1,
                                      int nsample1, float *grid_points, int *idx0, unsigned char *empty0, int *idx1, unsigned char *empty1) {
    PDM_REQUIRE(B >= 0 && B <= ST_MAXB && n >= 0 && K >= 0 && roi_stride >= 7, PDM_E_BADARG, "roi_keypoint_query: bad size (B=%d n=%d K=%d)", B, n, K);
    PDM_REQUIRE(G >= 1 && G <= RGP_MAXG, PDM_E_BADARG, "roi_keypoint_query: grid size %d (1 to %d)", G, RGP_MAXG);
    PDM_REQUIRE(nscales == 1 || nscales == 2, PDM_E_BADARG, "roi_keypoint_query: %d scales (1 or 2)", nscales);
    PDM_REQUIRE(nsample0 >= 1 && nsample0 <= RKQ_MAXS && radius0 >= 0.0f, PDM_E_BADARG, "roi_keypoint_query: scale 0: nsample %d (1 to %d) or a negative radius",
                nsample0, RKQ_MAXS);
    PDM_REQUIRE(nscales == 1 || (nsample1 >= 1 && nsample1 <= RKQ_MAXS && radius1 >= 0.0f), PDM_E_BADARG,
                "roi_keypoint_query: scale 1: nsample %d (1 to %d) or a negative radius", nsample1, RKQ_MAXS);
    PDM_REQUIRE(max_per_sample >= 0, PDM_E_BADARG, "roi_keypoint_query: negative max_per_sample");
    PDM_REQUIRE(max_per_sample <= RKQ_CAP, PDM_E_TOOLARGE,
                "roi_keypoint_query: up to %d keypoints a sample exceed the cap of %d the workgroup stages in LDS: use the composed query",
                max_per_sample, RKQ_CAP);
    const long long per = (long long)n * G * G * G, M = per * B;
    PDM_REQUIRE(M * RKQ_MAXS <= 0x7fffffffll && (long long)B * n * roi_stride <= 0x7fffffffll && (long long)K * 3 <= 0x7fffffffll, PDM_E_TOOLARGE,
                "roi_keypoint_query: %lld grid points, roi or keypoint elements exceed int32", M);
    if (M == 0) return 0;
    PDM_REQUIRE(K >= 1, PDM_E_BADARG, "roi_keypoint_query: no keypoint at all (K = 0): an empty ball would have no row to point at");
    PDM_REQUIRE(rois && xyz_batch_cnt && grid_points && idx0 && empty0 && xyz && (nscales == 1 || (idx1 && empty1)), PDM_E_BADARG,
                "roi_keypoint_query: null pointer");
    RkqArgs a{};
    a.B = B; a.n = n; a.G = G; a.roi_stride = roi_stride; a.K = K; a.cap = max(min(max_per_sample, K), 1);
    a.nscales = nscales; a.nsample[0] = nsample0; a.nsample[1] = nscales > 1 ? nsample1 : 0;
    a.radius[0] = radius0; a.radius[1] = nscales > 1 ? radius1 : 0.0f;
    a.rois = rois; a.xyz = xyz; a.cnt = xyz_batch_cnt; a.grid = grid_points;
    a.idx[0] = idx0; a.idx[1] = idx1; a.empty[0] = empty0; a.empty[1] = empty1;
    const dim3 grid((unsigned)((per + RKQ_POINTS - 1) / RKQ_POINTS), (unsigned)B);
    hipLaunchKernelGGL(roi_keypoint_query_kernel, grid, dim3(RKQ_T), (size_t)a.cap * 3 * sizeof(float), as_stream(stream), a);
    return check_launch("roi_keypoint_query");
}

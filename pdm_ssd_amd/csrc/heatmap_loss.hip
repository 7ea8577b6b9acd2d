// Heat-map head (the dense half of the hybrid head) in training: gaussian targets, penalty-reduced focal loss and its gradient
// in FOUR launches instead of ~75 elementwise torch kernels per step.
//
// Restates pdm_ssd_amd/dense_heads/pdm_heatmap_head.py::assign_targets + utils/centernet_utils.py (behaviour of
// /root/reference/pcdet/models/model_utils/centernet_utils.py:9-70 gaussian_radius / gaussian2D / draw_gaussian_to_heatmap as
// /root/reference/pcdet/models/dense_heads/center_head.py:100-160 calls them) and utils/loss_utils.py::neg_loss_cornernet on
// clamp(sigmoid(logits), 1e-4, 1 - 1e-4) (center_head.py:232, /root/reference/pcdet/utils/loss_utils.py:266-304):
//
//   target[b, c, y, x] = max over the boxes of (b, c) of exp(-(dx^2 + dy^2) / (2 sigma^2)) inside the box's (2 r + 1)^2 window,
//                        r = max(int(gaussian_radius(dy_cells, dx_cells, overlap)), min_radius), sigma = (2 r + 1) / 6,
//                        values under fp32 eps dropped
//   S      = sum_{target == 1} (1 - p)^2 log p + sum_{target < 1} (1 - target)^4 p^2 log(1 - p),   p = clamp(sigmoid(x))
//   L      = - weight * S / max(#{target == 1}, 1)
//
// Launch 1 (after a memset) draws the gaussians with integer atomic max (the values are non-negative floats: their bit patterns
// order like the values).  Launch 2 forms per-workgroup partial sums of the two terms and the peak count, and d S / d x per
// element; launch 3 (one workgroup) folds the partials in double in a fixed order (bit-reproducible), leaving L and the factor
// - weight / max(#peaks, 1) that backward() multiplies the stored d S / d x by.
#include "heatmap_draw.h"
#include "loss_kit.h"

namespace pdm {

constexpr int HM_T = 256;

struct HmTargetArgs {
    int B, M, C, H, W;
    const float *gt_boxes;          // (B, M, 8) [x y z dx dy dz heading class], zero rows = padding
    float x0, y0, vx, vy, stride;   // point-cloud range minimum, voxel size, feature-map stride: cell = (x - x0) / vx / stride
    double min_overlap;
    int min_radius, max_radius;
    float *heatmap;                 // (B, C, H, W), zero on entry
};

// one workgroup per box; the threads share the cells of its window (heatmap_draw.h)
__global__ __launch_bounds__(HM_T) void hm_target_kernel(HmTargetArgs a) {
    const int bm = blockIdx.x, b = bm / a.M;
    const float *g = a.gt_boxes + (size_t)bm * 8;
    const HmGrid grid{a.C, a.H, a.W, a.x0, a.y0, a.vx, a.vy, a.stride, a.min_overlap, a.min_radius, a.max_radius};
    hm_draw_box<HM_T>(grid, g[0], g[1], g[3], g[4], g[7], a.heatmap + (size_t)b * a.C * a.H * a.W);
}

struct HmLossArgs {
    long long n;                    // B C H W
    int C, H, W;
    MapRef logits;                  // (B, C, H, W) fp32 or bf16, any strides
    const float *heatmap;           // (B, C, H, W) contiguous
    float *dlogits;                 // (B, C, H, W) contiguous fp32: d S / d logit
    double *partials;               // (blocks, 3): peak term, other term, peaks
    float weight;
    float *out;                     // [0] loss, [1] - weight / max(peaks, 1), [2] peaks
};

__global__ __launch_bounds__(HM_T) void hm_loss_kernel(HmLossArgs a) {
    __shared__ BlockSum<HM_T, 3, double> red;
    double acc[3] = {0.0, 0.0, 0.0};                     // peak term, other term, peaks
    const long long hw = (long long)a.H * a.W, chw = hw * a.C;
    for (long long i = (long long)blockIdx.x * HM_T + threadIdx.x; i < a.n; i += (long long)gridDim.x * HM_T) {
        const long long b = i / chw, r0 = i - b * chw, c = r0 / hw, r1 = r0 - c * hw, y = r1 / a.W, x = r1 - y * a.W;
        const float gt = a.heatmap[i];
        const float praw = sigmoid_rn(map_load(a.logits, b, c, y, x));
        const float lo = 1e-4f, hi = 1.0f - 1e-4f;
        const float p = fminf(fmaxf(praw, lo), hi);
        const float dp = (praw >= lo && praw <= hi) ? praw * (1.0f - praw) : 0.0f;      // clamp passes the gradient inside [lo, hi]
        const float q = 1.0f - p;
        float ds;
        if (gt == 1.0f) {
            const float lp = logf(p);
            acc[0] += (double)(q * q * lp);
            acc[2] += 1.0;
            ds = -2.0f * q * lp + q * q / p;
        } else {
            const float w4 = powf(1.0f - gt, 4.0f), lq = logf(q);
            acc[1] += (double)(w4 * (p * p) * lq);
            ds = w4 * (2.0f * p * lq - p * p / q);
        }
        a.dlogits[i] = ds * dp;
    }
    red.reduce(acc);
    if (threadIdx.x < 3) a.partials[(size_t)blockIdx.x * 3 + threadIdx.x] = red.total(threadIdx.x);
}

__global__ __launch_bounds__(64) void hm_loss_finalize_kernel(int blocks, const double *__restrict__ partials, float weight, float *__restrict__ out) {
    // lane l adds partials l, l + 64, ... in order, then a butterfly over the wave: a fixed order (bit-reproducible) without the
    // 2048-step dependent chain one thread walked (180 us of a training step)
    double s_peak = 0.0, s_else = 0.0, n_peak = 0.0;
    for (int k = threadIdx.x; k < blocks; k += 64) { s_peak += partials[3 * k]; s_else += partials[3 * k + 1]; n_peak += partials[3 * k + 2]; }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        s_peak += __shfl_xor(s_peak, off, 64); s_else += __shfl_xor(s_else, off, 64); n_peak += __shfl_xor(n_peak, off, 64);
    }
    if (threadIdx.x != 0) return;
    const double den = n_peak > 1.0 ? n_peak : 1.0;
    out[0] = (float)(-(s_peak + s_else) / den * (double)weight);
    out[1] = (float)(-(double)weight / den);
    out[2] = (float)n_peak;
}

static inline int hm_blocks(long long n) {
    const long long want = (n + HM_T * 8 - 1) / (HM_T * 8);
    return (int)(want < 1 ? 1 : want > 2048 ? 2048 : want);
}

}  // namespace pdm

using namespace pdm;

// heatmap (B, C, H, W) fp32, fully written (zeroed here, then max-merged gaussians).  gt_boxes (B, M, 8) fp32.
extern "C" int pdm_heatmap_targets(void *stream, int B, int M, int C, int H, int W, const float *gt_boxes, float x0, float y0, float vx,
                                   float vy, float stride, double min_overlap, int min_radius, int max_radius, float *heatmap) {
    PDM_REQUIRE(B >= 0 && M >= 0 && C >= 1 && H >= 1 && W >= 1 && max_radius >= 0 && max_radius <= 64 && vx > 0.0f && vy > 0.0f && stride > 0.0f,
                PDM_E_BADARG, "heatmap_targets: bad size");
    if (B == 0) return 0;
    PDM_REQUIRE(heatmap && (M == 0 || gt_boxes), PDM_E_BADARG, "heatmap_targets: null pointer");
    if (int rc = zero_fill(stream, "heatmap_targets(zero)", heatmap, sizeof(float) * (size_t)B * C * H * W)) return rc;
    if (M == 0) return 0;
    PDM_REQUIRE((long long)B * M <= 0x7fffffffll, PDM_E_TOOLARGE, "heatmap_targets: %lld boxes", (long long)B * M);
    HmTargetArgs a{B, M, C, H, W, gt_boxes, x0, y0, vx, vy, stride, min_overlap, min_radius, max_radius, heatmap};
    hipLaunchKernelGGL(hm_target_kernel, dim3((unsigned)(B * M)), dim3(HM_T), 0, as_stream(stream), a);
    return check_launch("heatmap_targets");
}

extern "C" size_t pdm_heatmap_focal_loss_workspace_bytes(long long n) { return n <= 0 ? 0 : (size_t)hm_blocks(n) * 3 * sizeof(double); }

// logits (B, C, H, W) fp32 or bf16 with element strides (sb, sc, sh, sw); heatmap and dlogits (B, C, H, W) contiguous fp32;
// out[0] = loss, out[1] = the factor backward multiplies dlogits by, out[2] = number of peaks.
extern "C" int pdm_heatmap_focal_loss(void *stream, int B, int C, int H, int W, const void *logits, int logits_bf16, long long sb, long long sc,
                                      long long sh, long long sw, const float *heatmap, float weight, float *dlogits, float *out,
                                      void *workspace, size_t workspace_bytes) {
    PDM_REQUIRE(B >= 0 && C >= 1 && H >= 1 && W >= 1, PDM_E_BADARG, "heatmap_focal_loss: bad size");
    PDM_REQUIRE(out, PDM_E_BADARG, "heatmap_focal_loss: null pointer");
    const long long n = (long long)B * C * H * W;
    const int blocks = hm_blocks(n);
    if (n > 0) {
        PDM_REQUIRE(logits && heatmap && dlogits && workspace, PDM_E_BADARG, "heatmap_focal_loss: null pointer");
        PDM_REQUIRE(workspace_bytes >= pdm_heatmap_focal_loss_workspace_bytes(n) && (reinterpret_cast<uintptr_t>(workspace) & 7) == 0,
                    PDM_E_BADARG, "heatmap_focal_loss: workspace of %zu bytes, need %zu (8-byte aligned)", workspace_bytes,
                    pdm_heatmap_focal_loss_workspace_bytes(n));
        HmLossArgs a{n, C, H, W, MapRef{logits, logits_bf16, sb, sc, sh, sw}, heatmap, dlogits, static_cast<double *>(workspace), weight, out};
        hipLaunchKernelGGL(hm_loss_kernel, dim3((unsigned)blocks), dim3(HM_T), 0, as_stream(stream), a);
        if (int rc = check_launch("heatmap_focal_loss")) return rc;
    }
    hipLaunchKernelGGL(hm_loss_finalize_kernel, dim3(1), dim3(64), 0, as_stream(stream), n > 0 ? blocks : 0, static_cast<const double *>(workspace),
                       weight, out);
    return check_launch("heatmap_focal_loss(finalize)");
}

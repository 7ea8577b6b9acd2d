// Second-stage training on the device: proposal targets and the rcnn losses.
//
// pdm_proposal_targets restates, for a whole batch in one pass, ProposalTargetLayer.forward
// (pcdet/models/roi_heads/target_assigner/proposal_target_layer.py:13-228) and the canonical transformation of
// RoIHeadTemplate.assign_targets (pcdet/models/roi_heads/roi_head_template.py:104-134).  One workgroup per sample; the
// rois x boxes IoU matrix is never stored (each lane keeps the running maximum of its RoIs).  Per sample:
//   ground truth  rows (M, 8) [box7, class]; the trailing rows whose 8 elements sum to 0 (fp32, summed left to right) are
//                 dropped, interior ones stay; no row left: one all-zero box.
//   assignment    iou(r, m) = ov * h / max(vol_r + vol_m - ov * h, 1e-6), ov = box_overlap_bev(roi, gt) (box_geometry.h; the
//                 bounding-circle prefilter only skips pairs whose overlap is exactly 0), h = max(min(zr + dzr / 2, zm + dzm / 2) -
//                 max(zr - dzr / 2, zm - dzm / 2), 0), vol = (dx * dy) * dz: iou3d_nms_utils._iou3d_from_overlap, operation for
//                 operation (min / max / clamp hand a NaN on, as torch's do).  max_overlaps = the maximum over the ground truth
//                 whose class (fp32 -> int64, truncated) equals the RoI's label (SAMPLE_ROI_BY_EACH_CLASS), or over all of it;
//                 gt_assignment = the LOWEST index that reaches the maximum (torch.max leaves the order of ties open: this is
//                 build-defined); a NaN beats every number.  A RoI whose label has no ground truth: overlap 0, assignment 0.
//   split         fg: mo >= min(REG_FG_THRESH, CLS_FG_THRESH); easy bg: mo < CLS_BG_THRESH_LO; hard bg: mo < REG_FG_THRESH and
//                 mo >= CLS_BG_THRESH_LO (thresholds as fp32), each set compacted in RoI order.
//   counts        subsample_rois / sample_bg_inds (:117-192), S = ROI_PER_IMAGE, F = int(np.round(FG_RATIO * S)) (from the host):
//                 fg and bg: min(F, n_fg) fg, the rest bg; fg only: S fg; bg only: S bg; within bg, both kinds present:
//                 min(int(n_bg_wanted * HARD_BG_RATIO), n_hard) hard (the product in double), the rest easy; else all from the
//                 kind that exists.  Neither fg nor bg (NaN overlaps): state[1] |= 1 and every slot holds RoI 0.
//   order         fg slots first, then hard bg, then easy bg (the reference's cat order).
//
// Draws (the reference's global numpy / torch RNGs cannot be replayed; these are build-defined, as augment.hip's):
//   K(b, p) = draw_key(seed, step, b, p) (draws.h), step = state[0] read before the call's own increment
//   index(k, j, n) = (fmix32(k + j * 0x9E3779B1) * n) >> 32   (64-bit product: a value in [0, n))
//   fg, bg present   fg slot j in [0, min(F, n_fg)):  fg[feistel_perm(j, n_fg, K(b, 1))]      no repetition
//   fg only          fg slot j in [0, S):             fg[index(K(b, 2), j, n_fg)]             with repetition
//   hard bg slot j:  hard[index(K(b, 3), j, n_hard)]; easy bg slot j:  easy[index(K(b, 4), j, n_easy)]   with repetition
// A second, one-lane launch advances state[0] by 1 after all samples have read it.
//
// Targets of a drawn RoI (iou = its max_overlaps, g = its assigned ground-truth row; thresholds as fp32):
//   reg_valid_mask = iou > REG_FG_THRESH;  'cls' label = iou > CLS_FG_THRESH, -1 where CLS_BG_THRESH < iou < CLS_FG_THRESH;
//   'roi_iou' label = 1 above CLS_FG_THRESH, 0 below CLS_BG_THRESH, else (iou - CLS_BG_THRESH) / fp32(CLS_FG_THRESH -
//   CLS_BG_THRESH) (the difference in double, a true division).
//   canonical g (this file is built with -ffp-contract=off; nothing is fused), mod(a, b) = fmodf(a, b), plus b when negative
//   (torch.remainder); every constant is the fp32 nearest to the double the reference writes:
//     ry = mod(roi_heading, 2 pi);  x = gx - rx, y = gy - ry_, z = gz - rz;  h = g_heading - ry
//     c = cosf(-ry), s = sinf(-ry);  x' = x * c + y * (-s),  y' = x * s + y * c,  z' = z   (rotate_points_along_z's matmul,
//     summed left to right, without its + z * 0 terms)
//     h = mod(h, 2 pi);  if pi / 2 < h < 3 pi / 2: h = mod(h + pi, 2 pi);  if h > pi: h = h - 2 pi;  h = clamp(h, -pi / 2, pi / 2)
//   sizes and the class column pass through.
// Every output element is written by a kernel: no memset, no float atomics (the error flag is an integer OR).
//
// pdm_rcnn_loss restates get_box_cls_layer_loss (BinaryCrossEntropy) and get_box_reg_layer_loss (smooth-l1 +
// CORNER_LOSS_REGULARIZATION) of roi_head_template.py:136-218 with utils/box_coder_utils.py:5-77 (ResidualCoder) and
// utils/loss_utils.py:211-234 (get_corner_loss_lidar), and leaves their gradients:
//   L_cls    = w_cls * sum_{label >= 0} bce(x, label) / max(#valid, 1),  bce = max(x, 0) - x t + log1p(exp(-|x|)): the logit form
//              of F.binary_cross_entropy(sigmoid(x), t), equal to it while its clamp of the logs at -100 is idle (|x| < 88).
//   L_reg    = w_reg * sum_{fg, k} smooth_l1(cw_k (pred_k - t_k), beta) / max(#fg, 1), t = encode(canonical gt | RoI with centre
//              and heading zeroed): (x / d, y / d, z / dza, log(dxg / dxa), .., heading), sizes clamped at 1e-5, d = sqrt(dxa^2 + dya^2);
//              a NaN target switches its element off (WeightedSmoothL1Loss).  Rows outside fg are SKIPPED (the reference multiplies
//              them by 0, so an inf there would be a NaN in its sum).
//   L_corner = w_corner * sum_{fg} mean_{8 corners} smooth_l1(min(|P - G|, |P - G_flipped|), 1) / #fg (0 without fg): P the
//              corners of decode(pred | RoI at the origin) turned by the RoI's heading and moved to its centre, G those of the
//              source ground truth, G_flipped with heading + pi.  d L / d pred is analytic: through min (the nearer one; on a tie the
//              unflipped), norm (0 at distance 0), corners, rotation and decode.
// Sums: one (L_cls, L_reg, L_corner) triple per workgroup from a fixed shuffle tree, folded in double in index order by the
// second launch: bit-reproducible.  Every workgroup counts #fg and #valid itself over all rows (integers; n <= 262144).
#include "box_geometry.h"
#include "draws.h"
#include "loss_kit.h"

namespace pdm {

constexpr int PT_MAXR = 1024;      // RoIs per sample
constexpr int PT_MAXM = 256;       // ground-truth rows per sample
constexpr int PT_T = 256;
constexpr float PT_PI = 3.14159265358979323846f;
constexpr float PT_2PI = 6.28318530717958647692f;
constexpr float PT_HALF_PI = 1.57079632679489661923f;
constexpr float PT_3HALF_PI = 4.71238898038468985769f;

struct PTArgs {
    int B, R, M, S, by_class, fg_per_image, score_type;
    double hard_ratio;
    float reg_fg, cls_fg, cls_bg, bg_lo, ramp_den;
    unsigned seed;
    const float *rois, *scores;
    const long long *labels;
    const float *gt;
    int *state;
    float *o_rois;
    long long *o_labels;
    float *o_scores, *o_iou, *o_src, *o_canon;
    long long *o_mask;
    void *o_cls;
    int *o_idx, *o_ga;
};

// torch.min / torch.max / clamp(min=): a NaN operand is the result
__device__ __forceinline__ float pt_min(float a, float b) { return a != a ? a : (b != b ? b : (a < b ? a : b)); }
__device__ __forceinline__ float pt_max(float a, float b) { return a != a ? a : (b != b ? b : (a > b ? a : b)); }

// torch.remainder(a, b) for b > 0
__device__ __forceinline__ float pt_mod(float a, float b) {
    float m = fmodf(a, b);
    if (m != 0.f && m < 0.f) m = m + b;
    return m;
}

__device__ __forceinline__ int pt_index(unsigned k, unsigned j, unsigned n) {
    return (int)(((unsigned long long)fmix32(k + j * 0x9E3779B1u) * (unsigned long long)n) >> 32);
}

__global__ __launch_bounds__(PT_T) void proposal_targets_kernel(PTArgs a) {
    __shared__ float s_gt[PT_MAXM * 8];
    __shared__ float s_rad[PT_MAXM];
    __shared__ int s_gcls[PT_MAXM];
    __shared__ float s_mo[PT_MAXR];
    __shared__ short s_ga[PT_MAXR];
    __shared__ short s_list[3][PT_MAXR];
    __shared__ int s_wave[PT_T / 64];
    __shared__ int s_last;
    const int b = blockIdx.x, tid = threadIdx.x;
    const unsigned step = (unsigned)a.state[0];

    // ---- ground-truth rows: the last one whose elements do not sum to 0 ends the list
    if (tid == 0) s_last = -1;
    __syncthreads();
    for (int m = tid; m < a.M; m += PT_T) {
        const float *src = a.gt + ((size_t)b * a.M + m) * 8;
        float sum = 0.f;
        for (int f = 0; f < 8; ++f) {
            const float v = src[f];
            s_gt[m * 8 + f] = v;
            sum = sum + v;
        }
        if (!(sum == 0.f)) atomicMax(&s_last, m);
    }
    __syncthreads();
    int n_gt = s_last + 1;
    if (n_gt == 0) {
        if (tid < 8) s_gt[tid] = 0.f;
        n_gt = 1;
    }
    __syncthreads();
    for (int m = tid; m < n_gt; m += PT_T) {
        s_rad[m] = bev_radius(s_gt + m * 8);
        s_gcls[m] = (int)(long long)s_gt[m * 8 + 7];
    }
    __syncthreads();

    // ---- assignment: the running maximum per RoI
    for (int r = tid; r < a.R; r += PT_T) {
        const float *ro = a.rois + ((size_t)b * a.R + r) * 7;
        float bx[7];
        for (int f = 0; f < 7; ++f) bx[f] = ro[f];
        const long long lab = a.labels[(size_t)b * a.R + r];
        const float rr = bev_radius(bx);
        const float a_max = bx[2] + bx[5] / 2, a_min = bx[2] - bx[5] / 2;
        const float vol_a = bx[3] * bx[4] * bx[5];
        float best = 0.f;
        int arg = -1;
        for (int m = 0; m < n_gt; ++m) {
            if (a.by_class && (long long)s_gcls[m] != lab) continue;
            const float *g = s_gt + m * 8;
            float ov = 0.f;
            if (!bev_circles_disjoint(bx[0], bx[1], rr, g[0], g[1], s_rad[m])) ov = box_overlap_bev(bx, g);
            const float b_max = g[2] + g[5] / 2, b_min = g[2] - g[5] / 2;
            const float h = pt_max(pt_min(a_max, b_max) - pt_max(a_min, b_min), 0.f);
            const float o3 = ov * h;
            const float vol_b = g[3] * g[4] * g[5];
            const float iou = o3 / pt_max(vol_a + vol_b - o3, 1e-6f);
            if (arg < 0 || iou > best || (iou != iou && best == best)) {
                best = iou;
                arg = m;
            }
        }
        if (arg < 0) {
            best = 0.f;
            arg = 0;
        }
        s_mo[r] = best;
        s_ga[r] = (short)arg;
    }
    __syncthreads();

    // ---- split: three compactions in RoI order, one scan per 256 RoIs (the three counts share an int, 10 bits each)
    const float fg_t = fminf(a.reg_fg, a.cls_fg);
    int n_fg = 0, n_hard = 0, n_easy = 0;
    for (int r0 = 0; r0 < a.R; r0 += PT_T) {
        const int r = r0 + tid;
        const bool in = r < a.R;
        const float mo = in ? s_mo[r] : 0.f;
        const int f = in && mo >= fg_t ? 1 : 0;
        const int e = in && mo < a.bg_lo ? 1 : 0;
        const int h = in && mo < a.reg_fg && mo >= a.bg_lo ? 1 : 0;
        int tot;
        const int pre = block_scan<PT_T>(f | (h << 10) | (e << 20), s_wave, &tot);
        if (f) s_list[0][n_fg + (pre & 1023)] = (short)r;
        if (h) s_list[1][n_hard + ((pre >> 10) & 1023)] = (short)r;
        if (e) s_list[2][n_easy + (pre >> 20)] = (short)r;
        n_fg += tot & 1023;
        n_hard += (tot >> 10) & 1023;
        n_easy += tot >> 20;
    }
    __syncthreads();

    // ---- counts
    const int n_bg = n_hard + n_easy;
    int take_fg = 0, take_bg = 0, fg_rep = 0;
    bool err = false;
    if (n_fg > 0 && n_bg > 0) {
        take_fg = min(a.fg_per_image, n_fg);
        take_bg = a.S - take_fg;
    } else if (n_fg > 0) {
        take_fg = a.S;
        fg_rep = 1;
    } else if (n_bg > 0) {
        take_bg = a.S;
    } else {
        err = true;
    }
    int take_hard = 0;
    if (n_hard > 0 && n_easy > 0) take_hard = min((int)((double)take_bg * a.hard_ratio), n_hard);
    else if (n_hard > 0) take_hard = take_bg;
    if (err && tid == 0) atomicOr(&a.state[1], 1);

    // ---- draws, gather and targets: one lane per output slot
    const unsigned k_fg = draw_key(a.seed, step, (unsigned)b, 1u), k_rep = draw_key(a.seed, step, (unsigned)b, 2u);
    const unsigned k_hard = draw_key(a.seed, step, (unsigned)b, 3u), k_easy = draw_key(a.seed, step, (unsigned)b, 4u);
    for (int s = tid; s < a.S; s += PT_T) {
        int r = 0;
        if (err) r = 0;
        else if (s < take_fg) r = s_list[0][fg_rep ? pt_index(k_rep, (unsigned)s, (unsigned)n_fg)
                                                   : (int)feistel_perm((unsigned)s, (unsigned)n_fg, k_fg)];
        else if (s < take_fg + take_hard) r = s_list[1][pt_index(k_hard, (unsigned)(s - take_fg), (unsigned)n_hard)];
        else r = s_list[2][pt_index(k_easy, (unsigned)(s - take_fg - take_hard), (unsigned)n_easy)];
        const size_t o = (size_t)b * a.S + s;
        const float *ro = a.rois + ((size_t)b * a.R + r) * 7;
        float bx[7];
        for (int f = 0; f < 7; ++f) {
            bx[f] = ro[f];
            a.o_rois[o * 7 + f] = bx[f];
        }
        const int ga = s_ga[r];
        const float iou = s_mo[r];
        const float *g = s_gt + ga * 8;
        a.o_labels[o] = a.labels[(size_t)b * a.R + r];
        a.o_scores[o] = a.scores[(size_t)b * a.R + r];
        a.o_iou[o] = iou;
        a.o_idx[o] = r;
        a.o_ga[o] = ga;
        for (int f = 0; f < 8; ++f) a.o_src[o * 8 + f] = g[f];
        a.o_mask[o] = iou > a.reg_fg ? 1 : 0;
        if (a.score_type == 0) {
            long long lab = iou > a.cls_fg ? 1 : 0;
            if (iou > a.cls_bg && iou < a.cls_fg) lab = -1;
            static_cast<long long *>(a.o_cls)[o] = lab;
        } else {
            const bool fgm = iou > a.cls_fg, bgm = iou < a.cls_bg;
            float v = fgm ? 1.f : 0.f;
            if (!fgm && !bgm) v = (iou - a.cls_bg) / a.ramp_den;
            static_cast<float *>(a.o_cls)[o] = v;
        }
        // the ground truth in the RoI's frame
        const float ry = pt_mod(bx[6], PT_2PI);
        const float x = g[0] - bx[0], y = g[1] - bx[1], z = g[2] - bx[2];
        float h = g[6] - ry;
        const float c = cosf(-ry), sn = sinf(-ry);
        float *oc = a.o_canon + o * 8;
        oc[0] = x * c + y * (-sn);
        oc[1] = x * sn + y * c;
        oc[2] = z;
        oc[3] = g[3];
        oc[4] = g[4];
        oc[5] = g[5];
        h = pt_mod(h, PT_2PI);
        if (h > PT_HALF_PI && h < PT_3HALF_PI) h = pt_mod(h + PT_PI, PT_2PI);
        if (h > PT_PI) h = h - PT_2PI;
        h = pt_min(pt_max(h, -PT_HALF_PI), PT_HALF_PI);
        oc[6] = h;
        oc[7] = g[7];
    }
}

__global__ void proposal_targets_advance_kernel(int *state) { state[0] = (int)((unsigned)state[0] + 1u); }

// ---- rcnn losses ---------------------------------------------------------------------------------------------------------
constexpr int RL_T = 256;
constexpr long long RL_MAXN = 262144;

struct RLArgs {
    long long n;
    const float *cls, *reg, *rois, *gt, *src;
    const long long *mask;
    const void *labels;
    int labels_float, use_corner;
    float cw[7];
    float beta, w_cls, w_reg, w_corner;
    float *dcls, *dreg, *dcorner;
    int *counts;        // [0] #fg, [1] #valid (written by workgroup 0)
    float *partials;    // (workgroups, 3)
    float *o_cls, *o_reg, *o_corner, *o_fg;
};

__device__ __forceinline__ float rl_label(const RLArgs &a, long long i) {
    return a.labels_float ? static_cast<const float *>(a.labels)[i] : (float)static_cast<const long long *>(a.labels)[i];
}

__global__ __launch_bounds__(RL_T) void rcnn_loss_main_kernel(RLArgs a) {
    __shared__ BlockSum<RL_T, 2, int, true> s_cnt;
    __shared__ BlockSum<RL_T, 3, float, true> red;
    const int tid = threadIdx.x;
    int cnt[2] = {0, 0};                                 // #fg, #valid
    for (long long k = tid; k < a.n; k += RL_T) {
        cnt[0] += a.mask[k] > 0 ? 1 : 0;
        cnt[1] += rl_label(a, k) >= 0.f ? 1 : 0;
    }
    s_cnt.reduce(cnt);
    const int nf = s_cnt.total(0), nv = s_cnt.total(1);
    if (blockIdx.x == 0 && tid == 0) { a.counts[0] = nf; a.counts[1] = nv; }
    const float den_fg = fmaxf((float)nf, 1.f), den_valid = fmaxf((float)nv, 1.f);

    const long long i = (long long)blockIdx.x * RL_T + tid;
    float acc[3] = {0.f, 0.f, 0.f};                      // classification, regression, corner
    if (i < a.n) {
        // ---- classification
        const float x = a.cls[i], t = rl_label(a, i);
        if (t >= 0.f) {
            acc[0] = bce_with_logits(x, t);
            const float p = sigmoid_rn(x);
            a.dcls[i] = (p - t) / den_valid * a.w_cls;
        } else {
            a.dcls[i] = 0.f;
        }
        // ---- regression
        float dr[7], dk[7];
        for (int k = 0; k < 7; ++k) dr[k] = dk[k] = 0.f;
        if (a.mask[i] > 0) {
            const float *ro = a.rois + i * 7, *g = a.gt + i * 8, *sr = a.src + i * 8, *pr = a.reg + i * 7;
            float p[7];
            for (int k = 0; k < 7; ++k) p[k] = pr[k];
            const float dxa = fmaxf(ro[3], 1e-5f), dya = fmaxf(ro[4], 1e-5f), dza = fmaxf(ro[5], 1e-5f);
            const float diag = sqrtf(dxa * dxa + dya * dya);
            const float origin[3] = {0.f, 0.f, 0.f};               // the ground truth is already canonical
            float tg[7];
            residual_encode(g, origin, dxa, dya, dza, diag, tg);
            tg[6] = g[6];
            for (int k = 0; k < 7; ++k) {
                const float r = tg[k] != tg[k] ? 0.f : (p[k] - tg[k]) * a.cw[k];
                float l, d;
                smooth_l1(r, a.beta, &l, &d);
                acc[1] += l;
                dr[k] = tg[k] != tg[k] ? 0.f : d * a.cw[k] / den_fg * a.w_reg;
            }
            if (a.use_corner) {
                // decode against the RoI at the origin (sizes as they are), turn by its heading, move to its centre
                const float adx = ro[3], ady = ro[4], adz = ro[5];
                const float dg = sqrtf(adx * adx + ady * ady);
                const float xl = p[0] * dg, yl = p[1] * dg, zl = p[2] * adz;
                const float sx = expf(p[3]) * adx, sy = expf(p[4]) * ady, sz = expf(p[5]) * adz;
                const float rg = p[6] + ro[6];
                const float c = cosf(ro[6]), s = sinf(ro[6]);
                const float cx = xl * c - yl * s + ro[0], cy = xl * s + yl * c + ro[1], cz = zl + ro[2];
                const float ch = cosf(rg), sh = sinf(rg);
                const float gc = cosf(sr[6]), gs = sinf(sr[6]);
                const float hf = sr[6] + PT_PI;
                const float fc = cosf(hf), fs = sinf(hf);
                float dC[3] = {0.f, 0.f, 0.f}, dS[3] = {0.f, 0.f, 0.f}, dR = 0.f, sum = 0.f;
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    // boxes_to_corners_3d's template: x + + - - | + + - -, y + - - + | + - - +, z - - - - | + + + +
                    const float ux = (k & 3) < 2 ? 0.5f : -0.5f;
                    const float uy = (k & 3) == 0 || (k & 3) == 3 ? 0.5f : -0.5f;
                    const float uz = k < 4 ? -0.5f : 0.5f;
                    const float qx = sx * ux, qy = sy * uy;
                    const float px = qx * ch - qy * sh + cx, py = qx * sh + qy * ch + cy, pz = sz * uz + cz;
                    const float wx = sr[3] * ux, wy = sr[4] * uy, gz = sr[5] * uz + sr[2];
                    float ex = px - (wx * gc - wy * gs + sr[0]), ey = py - (wx * gs + wy * gc + sr[1]);
                    const float ez = pz - gz;
                    const float fx = px - (wx * fc - wy * fs + sr[0]), fy = py - (wx * fs + wy * fc + sr[1]);
                    float d = sqrtf(ex * ex + ey * ey + ez * ez);
                    const float d2 = sqrtf(fx * fx + fy * fy + ez * ez);
                    if (d2 < d) { d = d2; ex = fx; ey = fy; }
                    sum += d < 1.f ? d * d * 0.5f : d - 0.5f;
                    const float gsc = d < 1.f ? 1.f : 1.f / d;
                    const float gx = ex * gsc, gy = ey * gsc, gzz = ez * gsc;
                    dC[0] += gx; dC[1] += gy; dC[2] += gzz;
                    dS[0] += ux * (gx * ch + gy * sh);
                    dS[1] += uy * (gy * ch - gx * sh);
                    dS[2] += uz * gzz;
                    dR += gx * (-sh * qx - ch * qy) + gy * (ch * qx - sh * qy);
                }
                acc[2] = sum / 8.f;
                const float sc = a.w_corner / 8.f / den_fg;
                dk[0] = sc * dg * (dC[0] * c + dC[1] * s);
                dk[1] = sc * dg * (dC[1] * c - dC[0] * s);
                dk[2] = sc * adz * dC[2];
                dk[3] = sc * dS[0] * sx;
                dk[4] = sc * dS[1] * sy;
                dk[5] = sc * dS[2] * sz;
                dk[6] = sc * dR;
            }
        }
        for (int k = 0; k < 7; ++k) { a.dreg[i * 7 + k] = dr[k]; a.dcorner[i * 7 + k] = dk[k]; }
    }
    red.reduce(acc);
    if (tid < 3) a.partials[(size_t)blockIdx.x * 3 + tid] = red.total(tid);
}

__global__ __launch_bounds__(RL_T) void rcnn_loss_finalize_kernel(RLArgs a, int nblocks) {
    __shared__ FoldSum<RL_T, 3> sum;
    sum.fold(a.partials, nblocks);
    if (threadIdx.x == 0) {
        const int nf = a.counts[0], nv = a.counts[1];
        *a.o_cls = (float)sum.total(0) / fmaxf((float)nv, 1.f) * a.w_cls;
        *a.o_reg = (float)sum.total(1) / fmaxf((float)nf, 1.f) * a.w_reg;
        *a.o_corner = nf > 0 && a.use_corner ? (float)sum.total(2) / (float)nf * a.w_corner : 0.f;
        *a.o_fg = (float)nf;
    }
}

}  // namespace pdm

using namespace pdm;

extern "C" int pdm_proposal_targets(void *stream, int B, int R, int M, int S, const float *rois, const float *roi_scores,
                                    const long long *roi_labels, const float *gt_boxes, int by_class, int fg_per_image,
                                    double hard_bg_ratio, double reg_fg_thresh, double cls_fg_thresh, double cls_bg_thresh,
                                    double cls_bg_thresh_lo, int score_type, unsigned seed, int *state, float *out_rois,
                                    long long *out_labels, float *out_scores, float *out_iou, float *out_gt_src,
                                    float *out_gt_canon, long long *reg_valid_mask, void *cls_labels, int *sampled_inds,
                                    int *gt_assignment) {
    PDM_REQUIRE(B >= 0 && R >= 1 && M >= 0 && S >= 1 && fg_per_image >= 0 && fg_per_image <= S && (score_type == 0 || score_type == 1) &&
                hard_bg_ratio >= 0.0 && hard_bg_ratio <= 1.0,
                PDM_E_BADARG, "proposal_targets: B=%d R=%d M=%d S=%d fg_per_image=%d score_type=%d hard_bg_ratio=%g", B, R, M, S,
                fg_per_image, score_type, hard_bg_ratio);
    PDM_REQUIRE(R <= PT_MAXR && M <= PT_MAXM && B <= 65535 && S <= (1 << 20), PDM_E_TOOLARGE,
                "proposal_targets: B=%d R=%d M=%d S=%d (limits 65535, %d, %d, %d)", B, R, M, S, PT_MAXR, PT_MAXM, 1 << 20);
    if (B == 0) return 0;
    PDM_REQUIRE(rois && roi_scores && roi_labels && (M == 0 || gt_boxes) && state && out_rois && out_labels && out_scores && out_iou &&
                out_gt_src && out_gt_canon && reg_valid_mask && cls_labels && sampled_inds && gt_assignment,
                PDM_E_BADARG, "proposal_targets: null pointer");
    PTArgs a{};
    a.B = B; a.R = R; a.M = M; a.S = S; a.by_class = by_class ? 1 : 0; a.fg_per_image = fg_per_image; a.score_type = score_type;
    a.hard_ratio = hard_bg_ratio;
    a.reg_fg = (float)reg_fg_thresh; a.cls_fg = (float)cls_fg_thresh; a.cls_bg = (float)cls_bg_thresh; a.bg_lo = (float)cls_bg_thresh_lo;
    a.ramp_den = (float)(cls_fg_thresh - cls_bg_thresh);
    a.seed = seed;
    a.rois = rois; a.scores = roi_scores; a.labels = roi_labels; a.gt = gt_boxes; a.state = state;
    a.o_rois = out_rois; a.o_labels = out_labels; a.o_scores = out_scores; a.o_iou = out_iou; a.o_src = out_gt_src;
    a.o_canon = out_gt_canon; a.o_mask = reg_valid_mask; a.o_cls = cls_labels; a.o_idx = sampled_inds; a.o_ga = gt_assignment;
    hipLaunchKernelGGL(proposal_targets_kernel, dim3(B), dim3(PT_T), 0, as_stream(stream), a);
    int e = check_launch("proposal_targets");
    if (e) return e;
    hipLaunchKernelGGL(proposal_targets_advance_kernel, dim3(1), dim3(1), 0, as_stream(stream), state);
    return check_launch("proposal_targets(advance)");
}

extern "C" size_t pdm_rcnn_loss_workspace_bytes(long long n) {
    if (n < 0) return 0;
    const long long blocks = (n + RL_T - 1) / RL_T;
    return (size_t)(16 + blocks * 3 * (long long)sizeof(float));
}

extern "C" int pdm_rcnn_loss(void *stream, long long n, const float *rcnn_cls, const float *rcnn_reg, const float *rois,
                             const float *gt_of_rois, const float *gt_of_rois_src, const long long *reg_valid_mask,
                             const void *cls_labels, int labels_float, const float *code_weights, float beta, float cls_weight,
                             float reg_weight, float corner_weight, int use_corner, float *dcls, float *dreg, float *dcorner,
                             float *loss_cls, float *loss_reg, float *loss_corner, float *fg_count, void *workspace, size_t workspace_bytes) {
    PDM_REQUIRE(n >= 1, PDM_E_BADARG, "rcnn_loss: n=%lld rows", n);
    PDM_REQUIRE(n <= RL_MAXN, PDM_E_TOOLARGE, "rcnn_loss: n=%lld rows (limit %lld)", n, RL_MAXN);
    PDM_REQUIRE(rcnn_cls && rcnn_reg && rois && gt_of_rois && gt_of_rois_src && reg_valid_mask && cls_labels && code_weights && dcls &&
                dreg && dcorner && loss_cls && loss_reg && loss_corner && fg_count, PDM_E_BADARG, "rcnn_loss: null pointer");
    PDM_REQUIRE(workspace && workspace_bytes >= pdm_rcnn_loss_workspace_bytes(n), PDM_E_BADARG,
                "rcnn_loss: workspace too small (%zu < %zu bytes)", workspace_bytes, pdm_rcnn_loss_workspace_bytes(n));
    PDM_WS_ALIGNED("rcnn_loss", workspace);
    RLArgs a{};
    a.n = n;
    a.cls = rcnn_cls; a.reg = rcnn_reg; a.rois = rois; a.gt = gt_of_rois; a.src = gt_of_rois_src; a.mask = reg_valid_mask;
    a.labels = cls_labels; a.labels_float = labels_float ? 1 : 0; a.use_corner = use_corner ? 1 : 0;
    for (int k = 0; k < 7; ++k) a.cw[k] = code_weights[k];     // host array
    a.beta = beta; a.w_cls = cls_weight; a.w_reg = reg_weight; a.w_corner = corner_weight;
    a.dcls = dcls; a.dreg = dreg; a.dcorner = dcorner;
    a.counts = static_cast<int *>(workspace);
    a.partials = reinterpret_cast<float *>(static_cast<char *>(workspace) + 16);
    a.o_cls = loss_cls; a.o_reg = loss_reg; a.o_corner = loss_corner; a.o_fg = fg_count;
    const int blocks = (int)((n + RL_T - 1) / RL_T);
    hipLaunchKernelGGL(rcnn_loss_main_kernel, dim3(blocks), dim3(RL_T), 0, as_stream(stream), a);
    int e = check_launch("rcnn_loss");
    if (e) return e;
    hipLaunchKernelGGL(rcnn_loss_finalize_kernel, dim3(1), dim3(RL_T), 0, as_stream(stream), a, blocks);
    return check_launch("rcnn_loss(finalize)");
}

// TransFusionHead in training on the device (the reference's pcdet/models/dense_heads/transfusion_head.py:235-382 and
// target_assigner/hungarian_assigner.py): a batched linear-sum-assignment solver, the assigner's costs, matching and
// targets for the whole batch, and the three losses with their gradients.  No host read, no atomics on results except
// the integer max that merges the heat-map gaussians (order-free); two runs give the same bits.
//
// pdm_lsap       one workgroup per sample.  The Jonker-Volgenant shortest-augmenting-path form of Crouse ("On implementing
//                2D rectangular assignment algorithms", 2016; scipy's rectangular_lsap): rows are the SMALLER side (scipy
//                transposes when it has more rows than columns), one augmentation per row.  An augmentation is a Dijkstra
//                search over the columns: every step relaxes the free columns in parallel from the current row, takes the
//                column of least path length (an arg-min reduction, ties by LOWER COLUMN INDEX) and retires it; the search
//                ends at an unassigned column.  Duals and path lengths are fp64, as scipy's are after its cast.
//                LOOP BOUNDS: nr = min(P, G) augmentations; a step retires one column, so a search takes at most nc =
//                max(P, G) steps; the walk back along the path visits at most nr rows.  Every loop is a counted `for` over
//                one of these; none waits for a condition.  A cost that is not finite (NaN, +Inf, -Inf) is read as FLT_MAX,
//                so every path length is finite and a free column always exists: the trip counts depend on (P, G) alone.
// pdm_tf_assign  prepare (one workgroup per sample: the valid boxes, dx > 0 && dy > 0, compacted in order; the P decoded boxes,
//                tf_decode.h) -> cost (one thread per (proposal, valid gt): focal + L1 + IoU3D cost, fp32 in the reference's
//                operation order) -> match (one workgroup per sample: the solver above, then the targets of its P proposals)
//                -> finish (num_pos, matched_ious) -> heat map (one workgroup per box, heatmap_draw.h).
// pdm_tf_loss    one thread per element of the (B, C + code, P) maps: sigmoid focal and L1 terms with their gradients already
//                divided by max(num_pos, 1) (read on the device), block partials folded in double in a fixed order; the dense
//                heat-map term is pdm_heatmap_focal_loss (heatmap_loss.hip) as it stands.
#include <float.h>

#include "box_geometry.h"
#include "heatmap_draw.h"
#include "loss_kit.h"
#include "tf_decode.h"

namespace pdm {

constexpr int LS_T = 256;
constexpr int LS_MAX = 1024;         // rows and columns the solver holds in LDS

struct LsapLds {
    double u[LS_MAX], v[LS_MAX], sh[LS_MAX];             // row duals, column duals, shortest path length to a column
    int path[LS_MAX], col4row[LS_MAX], row4col[LS_MAX];
    unsigned char sr[LS_MAX], sc[LS_MAX];                // rows visited, columns retired in the current search
    double wv[LS_T / 64];
    int wi[LS_T / 64];
};

// entry (i, j) of the solver's matrix: rows are the smaller side, `tr` = the rows are the caller's columns
__device__ __forceinline__ double lsap_cost(const float *cost, long long stride, bool tr, int i, int j) {
    const float c = tr ? cost[(long long)j * stride + i] : cost[(long long)i * stride + j];
    return (double)(fabsf(c) <= FLT_MAX ? c : FLT_MAX);          // NaN, +Inf and -Inf alike
}

// cost: one sample's (P, >= G) fp32 matrix with row stride `stride`; 1 <= P <= LS_MAX, 0 <= G <= Gmax <= LS_MAX.
// gt_of_row (P) = the matched column or -1, row_of_gt (Gmax) = the matched row or -1.  All LS_T threads call it.
__device__ void lsap_solve(const float *cost, long long stride, int P, int G, int Gmax, int *gt_of_row, int *row_of_gt, LsapLds &s) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int p = tid; p < P; p += LS_T) gt_of_row[p] = -1;
    for (int g = tid; g < Gmax; g += LS_T) row_of_gt[g] = -1;
    if (G <= 0) return;                                          // (uniform over the workgroup)
    const bool tr = G < P;
    const int nr = tr ? G : P, nc = tr ? P : G;
    const double INF = __longlong_as_double(0x7ff0000000000000ll);
    for (int i = tid; i < nr; i += LS_T) { s.u[i] = 0.0; s.col4row[i] = -1; }
    for (int j = tid; j < nc; j += LS_T) { s.v[j] = 0.0; s.row4col[j] = -1; }
    for (int cur = 0; cur < nr; ++cur) {
        for (int j = tid; j < nc; j += LS_T) { s.sh[j] = INF; s.sc[j] = 0; }
        for (int i = tid; i < nr; i += LS_T) s.sr[i] = 0;
        __syncthreads();
        double min_val = 0.0;
        int i = cur, sink = -1;
        for (int step = 0; step < nc; ++step) {                  // a step retires one column
            if (tid == 0) s.sr[i] = 1;
            const double ui = s.u[i];
            double bv = INF;
            int bi = 0x7fffffff;
            for (int j = tid; j < nc; j += LS_T) {
                if (s.sc[j]) continue;
                const double r = ((min_val + lsap_cost(cost, stride, tr, i, j)) - ui) - s.v[j];
                if (r < s.sh[j]) { s.path[j] = i; s.sh[j] = r; }
                const double d = s.sh[j];
                if (d < bv) { bv = d; bi = j; }                  // j ascends: the lower index stays on a tie
            }
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) {
                const double ov = __shfl_xor(bv, off, 64);
                const int oi = __shfl_xor(bi, off, 64);
                if (ov < bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
            }
            if (lane == 0) { s.wv[wave] = bv; s.wi[wave] = bi; }
            __syncthreads();
            bv = s.wv[0]; bi = s.wi[0];
#pragma unroll
            for (int w = 1; w < LS_T / 64; ++w) {
                const double ov = s.wv[w];
                const int oi = s.wi[w];
                if (ov < bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
            }
            if (bi >= nc) break;                                 // no free column: cannot happen with finite costs (uniform)
            min_val = bv;
            const int r4c = s.row4col[bi];
            if (tid == 0) s.sc[bi] = 1;
            __syncthreads();                                     // sc, sr, and wv / wi free for the next step
            if (r4c < 0) { sink = bi; break; }
            i = r4c;
        }
        __syncthreads();
        if (sink >= 0) {
            // the duals of the visited rows and retired columns (col4row is still the matching before this augmentation)
            for (int k = tid; k < nr; k += LS_T) {
                if (k == cur) s.u[k] += min_val;
                else if (s.sr[k]) s.u[k] += min_val - s.sh[s.col4row[k]];
            }
            for (int j = tid; j < nc; j += LS_T)
                if (s.sc[j]) s.v[j] -= min_val - s.sh[j];
            __syncthreads();
            if (tid == 0) {
                int j = sink;
                for (int k = 0; k < nr; ++k) {                   // the path back to `cur` visits each row at most once
                    const int pi = s.path[j];
                    s.row4col[j] = pi;
                    const int t = s.col4row[pi];
                    s.col4row[pi] = j;
                    j = t;
                    if (pi == cur || j < 0) break;
                }
            }
        }
        __syncthreads();
    }
    for (int i = tid; i < nr; i += LS_T) {
        const int j = s.col4row[i];
        if (j < 0) continue;
        const int row = tr ? j : i, col = tr ? i : j;
        gt_of_row[row] = col;
        row_of_gt[col] = row;
    }
}

__global__ __launch_bounds__(LS_T) void lsap_kernel(int P, int Gmax, const float *cost, long long sb, long long stride, const int *num_gt,
                                                    int *gt_of_row, int *row_of_gt) {
    __shared__ LsapLds lds;
    const int b = blockIdx.x;
    int G = num_gt[b];
    G = G < 0 ? 0 : G > Gmax ? Gmax : G;
    lsap_solve(cost + (long long)b * sb, stride, P, G, Gmax, gt_of_row + (size_t)b * P, row_of_gt + (size_t)b * Gmax, lds);
}

// ---- pdm_tf_assign ----------------------------------------------------------------------------------------------------------
constexpr int TFA_GT = 10;           // a compacted box: [x y z dx dy dz yaw vx vy class]

struct TfaArgs {
    int B, C, P, M, D, E;            // D = columns of a gt row (8 | 10), E = 2 with a velocity map
    const float *heatmap;            // (B, C, P) logits
    TfBoxMaps maps;
    const float *gt_boxes;           // (B, M, D)
    float cls_w, cls_alpha, cls_1malpha, cls_gamma, cls_eps, reg_w, iou_w;
    float rx0, ry0, rdx, rdy;        // range minimum and extent in x, y
    float tx, ty;                    // stride * voxel size: the divisor of the centre targets
    int num_classes;
    // workspace
    float *boxes, *gts, *cost, *stats;    // (B, P, 9), (B, M, TFA_GT), (B, P, M), (B, 2)
    int *num_gt, *row_of_gt;              // (B), (B, M)
    // outputs
    long long *labels;               // (B, P)
    float *label_weights, *bbox_targets, *bbox_weights, *ious, *matched_ious;   // (B, P), (B, P, 8 + E) x 2, (B, P), (1)
    int *assigned, *num_pos;         // (B, P): index among the sample's valid boxes or -1; (1)
};

// the reference's overlaps(): BEV overlap x height overlap over the union, z read as the box's BOTTOM
__device__ __forceinline__ float tf_iou3d(const float *a, const float *g) {
    float ov = 0.0f;
    if (!bev_circles_disjoint(a[0], a[1], bev_radius(a), g[0], g[1], bev_radius(g))) ov = box_overlap_bev(a, g);
    const float top = fminf(a[2] + a[5], g[2] + g[5]), bottom = fmaxf(a[2], g[2]);
    const float o3 = ov * fmaxf(top - bottom, 0.0f);
    const float v1 = a[3] * a[4] * a[5], v2 = g[3] * g[4] * g[5];
    return o3 / fmaxf(v1 + v2 - o3, 1e-8f);
}

__global__ __launch_bounds__(LS_T) void tfa_prepare_kernel(TfaArgs a) {
    __shared__ int s_wave[LS_T / 64];
    const int b = blockIdx.x, tid = threadIdx.x;
    int kept = 0;
    for (int m0 = 0; m0 < a.M; m0 += LS_T) {
        const int m = m0 + tid;
        const float *g = a.gt_boxes + ((size_t)b * a.M + (m < a.M ? m : 0)) * a.D;
        const bool valid = m < a.M && g[3] > 0.0f && g[4] > 0.0f;
        int tot;
        const int pos = kept + block_scan<LS_T>(valid ? 1 : 0, s_wave, &tot);
        kept += tot;
        if (valid) {
            float *o = a.gts + ((size_t)b * a.M + pos) * TFA_GT;
            for (int d = 0; d < 7; ++d) o[d] = g[d];
            o[7] = a.D == 10 ? g[7] : 0.0f;
            o[8] = a.D == 10 ? g[8] : 0.0f;
            o[9] = g[a.D - 1];
        }
    }
    if (tid == 0) a.num_gt[b] = kept;
    for (int p = tid; p < a.P; p += LS_T) tf_decode_box(a.maps, b, p, a.boxes + ((size_t)b * a.P + p) * 9);
}

__global__ __launch_bounds__(LS_T) void tfa_cost_kernel(TfaArgs a) {
    const int b = blockIdx.y, e = blockIdx.x * LS_T + threadIdx.x;
    if (e >= a.P * a.M) return;
    const int p = e / a.M, g = e - p * a.M;
    if (g >= a.num_gt[b]) return;
    const float *box = a.boxes + ((size_t)b * a.P + p) * 9, *gt = a.gts + ((size_t)b * a.M + g) * TFA_GT;
    int c = (int)gt[9] - 1;
    c = c < 0 ? 0 : c >= a.C ? a.C - 1 : c;
    // focal_loss_cost: pos - neg at the gt's class
    const float s = sigmoid_rn(a.heatmap[((size_t)b * a.C + c) * a.P + p]), q = 1.0f - s;
    const float sg = a.cls_gamma == 2.0f ? s * s : powf(s, a.cls_gamma), qg = a.cls_gamma == 2.0f ? q * q : powf(q, a.cls_gamma);
    const float neg = -logf(q + a.cls_eps) * a.cls_1malpha * sg;
    const float pos = -logf(s + a.cls_eps) * a.cls_alpha * qg;
    const float cls = (pos - neg) * a.cls_w;
    // bevbox_cost: L1 of the range-normalised centres
    const float reg = (fabsf((box[0] - a.rx0) / a.rdx - (gt[0] - a.rx0) / a.rdx) + fabsf((box[1] - a.ry0) / a.rdy - (gt[1] - a.ry0) / a.rdy)) * a.reg_w;
    const float iou = -tf_iou3d(box, gt) * a.iou_w;
    a.cost[((size_t)b * a.P + p) * a.M + g] = (cls + reg) + iou;
}

__global__ __launch_bounds__(LS_T) void tfa_match_kernel(TfaArgs a) {
    __shared__ LsapLds lds;
    __shared__ BlockSum<LS_T, 1, double> red;
    const int b = blockIdx.x, tid = threadIdx.x, P = a.P, code = 8 + a.E;
    const int G = a.num_gt[b];                                   // <= M by construction
    int *assigned = a.assigned + (size_t)b * P;
    lsap_solve(a.cost + (size_t)b * P * a.M, a.M, P, G, a.M, assigned, a.row_of_gt + (size_t)b * a.M, lds);
    __syncthreads();
    double acc[1] = {0.0};
    for (int p = tid; p < P; p += LS_T) {
        const size_t at = (size_t)b * P + p;
        const int g = assigned[p];
        float t[10] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        float iou = 0.0f;
        long long label = a.num_classes;
        if (g >= 0) {
            const float *gt = a.gts + ((size_t)b * a.M + g) * TFA_GT;
            label = (long long)gt[9] - 1;
            t[0] = (gt[0] - a.rx0) / a.tx;                       // encode_bbox
            t[1] = (gt[1] - a.ry0) / a.ty;
            t[2] = gt[2];
            t[3] = logf(gt[3]); t[4] = logf(gt[4]); t[5] = logf(gt[5]);
            t[6] = sinf(gt[6]); t[7] = cosf(gt[6]);
            t[8] = gt[7]; t[9] = gt[8];
            iou = fminf(fmaxf(tf_iou3d(a.boxes + at * 9, gt), 0.0f), 1.0f);
            acc[0] += (double)iou;
        }
        a.labels[at] = label;
        a.label_weights[at] = 1.0f;
        a.ious[at] = iou;
        for (int d = 0; d < code; ++d) {
            a.bbox_targets[at * code + d] = t[d];
            a.bbox_weights[at * code + d] = g >= 0 ? 1.0f : 0.0f;
        }
    }
    red.reduce(acc);
    if (tid == 0) {
        const int npos = G < P ? G : P;
        a.stats[2 * b] = (float)npos;
        a.stats[2 * b + 1] = (float)red.total(0) / (float)(npos > 1 ? npos : 1);
    }
}

__global__ __launch_bounds__(64) void tfa_finish_kernel(int B, const float *__restrict__ stats, int *num_pos, float *matched_ious) {
    double n = 0.0, m = 0.0;
    for (int k = threadIdx.x; k < B; k += 64) { n += stats[2 * k]; m += stats[2 * k + 1]; }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) { n += __shfl_xor(n, off, 64); m += __shfl_xor(m, off, 64); }
    if (threadIdx.x != 0) return;
    num_pos[0] = (int)n;
    matched_ious[0] = (float)(m / (double)B);
}

struct TfaHmArgs {
    int M, D;
    const float *gt_boxes;
    HmGrid grid;
    float *heatmap;                  // (B, C, H, W), zero on entry
};

__global__ __launch_bounds__(LS_T) void tfa_heatmap_kernel(TfaHmArgs a) {
    const int bm = blockIdx.x, b = bm / a.M;
    const float *g = a.gt_boxes + (size_t)bm * a.D;
    hm_draw_box_unclamped<LS_T>(a.grid, g[0], g[1], g[3], g[4], g[a.D - 1], a.heatmap + (size_t)b * a.grid.C * a.grid.H * a.grid.W);
}

// ---- pdm_tf_loss ------------------------------------------------------------------------------------------------------------
struct TflArgs {
    int B, C, P, E;
    const float *heatmap, *maps[5];  // logits (B, C, P); center, height, dim, rot, vel (B, c, P)
    const long long *labels;         // (B, P)
    const float *label_weights, *bbox_targets, *bbox_weights;
    const int *num_pos;
    float code_w[10], cls_w, bbox_w, alpha, gamma;
    float *g_heatmap, *g_maps[5];
    double *partials;                // (blocks, 2)
};

__global__ __launch_bounds__(LS_T) void tfl_kernel(TflArgs a) {
    __shared__ BlockSum<LS_T, 2, double> red;
    const int code = 8 + a.E, rows = a.C + code;
    const long long total = (long long)a.B * rows * a.P;
    const long long e = (long long)blockIdx.x * LS_T + threadIdx.x;
    const int np = a.num_pos[0];
    const float den = (float)(np > 1 ? np : 1);
    double acc[2] = {0.0, 0.0};
    if (e < total) {
        const int p = (int)(e % a.P), ch = (int)((e / a.P) % rows), b = (int)(e / ((long long)a.P * rows));
        const size_t bp = (size_t)b * a.P + p;
        if (ch < a.C) {                                          // SigmoidFocalClassificationLoss against the one-hot of labels
            const size_t at = ((size_t)b * a.C + ch) * a.P + p;
            const float x = a.heatmap[at], t = a.labels[bp] == ch ? 1.0f : 0.0f, w = a.label_weights[bp];
            const float s = sigmoid_rn(x);
            const float aw = t * a.alpha + (1.0f - t) * (1.0f - a.alpha);
            const float pt = t * (1.0f - s) + (1.0f - t) * s;
            const float ptg = a.gamma == 2.0f ? pt * pt : powf(pt, a.gamma);
            const float dptg = a.gamma == 2.0f ? 2.0f * pt : (pt > 0.0f ? a.gamma * powf(pt, a.gamma - 1.0f) : 0.0f);
            const float bce = bce_with_logits(x, t);
            acc[0] += (double)(aw * ptg * bce * w);
            const float dpt = (1.0f - 2.0f * t) * s * (1.0f - s);
            a.g_heatmap[at] = (aw * dptg * dpt * bce + aw * ptg * (s - t)) * w * a.cls_w / den;
        } else {                                                 // L1 over the HEAD_ORDER maps
            const int d = ch - a.C;
            const int k = d < 2 ? 0 : d < 3 ? 1 : d < 6 ? 2 : d < 8 ? 3 : 4, base = k == 0 ? 0 : k == 1 ? 2 : k == 2 ? 3 : k == 3 ? 6 : 8;
            const int width = k == 0 ? 2 : k == 1 ? 1 : k == 2 ? 3 : 2;
            const size_t at = ((size_t)b * width + (d - base)) * a.P + p;
            const float r = a.maps[k][at] - a.bbox_targets[bp * code + d];
            const float w = a.bbox_weights[bp * code + d] * a.code_w[d];
            acc[1] += (double)(fabsf(r) * w);
            a.g_maps[k][at] = (r > 0.0f ? 1.0f : r < 0.0f ? -1.0f : 0.0f) * w * a.bbox_w / den;
        }
    }
    red.reduce(acc);
    if (threadIdx.x < 2) a.partials[(size_t)blockIdx.x * 2 + threadIdx.x] = red.total(threadIdx.x);
}

__global__ __launch_bounds__(LS_T) void tfl_finalize_kernel(int blocks, const double *__restrict__ partials, const int *num_pos, float cls_w,
                                                            float bbox_w, float *out) {
    __shared__ FoldSum<LS_T, 2> fold;
    fold.fold(partials, blocks);
    if (threadIdx.x != 0) return;
    const int np = num_pos[0];
    const double den = (double)(np > 1 ? np : 1);
    out[0] = (float)(fold.total(0) / den * (double)cls_w);
    out[1] = (float)(fold.total(1) / den * (double)bbox_w);
}

}  // namespace pdm

using namespace pdm;

extern "C" int pdm_lsap(void *stream, int B, int P, int Gmax, const float *cost, long long row_stride, const int *num_gt, int *gt_of_row,
                        int *row_of_gt) {
    PDM_REQUIRE(B >= 0 && B <= 0x7fffff && P >= 1 && P <= LS_MAX && Gmax >= 0 && Gmax <= LS_MAX, PDM_E_BADARG,
                "lsap: B = %d, P = %d, Gmax = %d (1 <= P <= %d, 0 <= Gmax <= %d)", B, P, Gmax, LS_MAX, LS_MAX);
    PDM_REQUIRE(row_stride >= Gmax, PDM_E_BADARG, "lsap: row stride %lld < Gmax = %d", row_stride, Gmax);
    if (B == 0) return 0;
    PDM_REQUIRE(num_gt && gt_of_row && (Gmax == 0 || (cost && row_of_gt)), PDM_E_BADARG, "lsap: null pointer");
    hipLaunchKernelGGL(lsap_kernel, dim3((unsigned)B), dim3(LS_T), 0, as_stream(stream), P, Gmax, cost, (long long)P * row_stride, row_stride,
                       num_gt, gt_of_row, row_of_gt);
    return check_launch("lsap");
}

static size_t tfa_sections(int B, int P, int M, size_t *off) {
    size_t at = 0;
    const size_t sizes[6] = {sizeof(float) * B * P * 9, sizeof(float) * B * M * TFA_GT, sizeof(float) * B * P * M, sizeof(float) * B * 2,
                             sizeof(int) * B, sizeof(int) * B * M};
    for (int k = 0; k < 6; ++k) { if (off) off[k] = at; at += align256(sizes[k]); }
    return at;
}

extern "C" size_t pdm_tf_assign_workspace_bytes(int B, int P, int M) {
    if (B <= 0 || P < 1 || P > LS_MAX || M < 0 || M > LS_MAX) return 0;
    return tfa_sections(B, P, M, nullptr);
}

// cost_cfg: HOST [cls weight, alpha, gamma, eps, reg weight, iou weight]; pc_range: HOST [x0 y0 z0 x1 y1 z1]
extern "C" int pdm_tf_assign(void *stream, int B, int C, int P, int M, int gt_cols, int H, int W, const float *heatmap, const float *center,
                             const float *height, const float *dim, const float *rot, const float *vel, const float *gt_boxes,
                             const double *cost_cfg, const float *pc_range, float vx, float vy, float stride, double gaussian_overlap,
                             int min_radius, int num_classes, long long *labels, float *label_weights, float *bbox_targets,
                             float *bbox_weights, float *ious, int *assigned, int *num_pos, float *matched_ious, float *heatmap_target,
                             void *workspace, size_t workspace_bytes) {
    PDM_REQUIRE(B >= 0 && B <= 65535 && C >= 1 && P >= 1 && P <= LS_MAX && M >= 0 && M <= LS_MAX && H >= 1 && W >= 1 && H <= 16384 && W <= 16384,
                PDM_E_BADARG, "tf_assign: bad size (1 <= P <= %d, 0 <= M <= %d)", LS_MAX, LS_MAX);
    PDM_REQUIRE((long long)B * C * P <= 0x7fffffffll && (long long)B * C * H * W <= 0x7fffffffll, PDM_E_TOOLARGE, "tf_assign: too large");
    const int E = vel ? 2 : 0;
    PDM_REQUIRE((gt_cols == 8 || gt_cols == 10) && gt_cols - 8 >= E, PDM_E_BADARG,
                "tf_assign: gt_boxes with %d columns (8, or 10 with velocities; a velocity map needs 10)", gt_cols);
    PDM_REQUIRE(cost_cfg && pc_range && vx > 0.0f && vy > 0.0f && stride > 0.0f && min_radius >= 0 && num_classes >= 1, PDM_E_BADARG,
                "tf_assign: bad table");
    if (B == 0) return 0;
    PDM_REQUIRE(heatmap && center && height && dim && rot && (M == 0 || gt_boxes) && labels && label_weights && bbox_targets && bbox_weights &&
                ious && assigned && num_pos && matched_ious && heatmap_target && workspace, PDM_E_BADARG, "tf_assign: null pointer");
    size_t off[6];
    const size_t need = tfa_sections(B, P, M, off);
    PDM_REQUIRE(workspace_bytes >= need && (reinterpret_cast<uintptr_t>(workspace) & 7) == 0, PDM_E_BADARG,
                "tf_assign: workspace of %zu bytes, need %zu (8-byte aligned)", workspace_bytes, need);
    char *ws = static_cast<char *>(workspace);
    TfaArgs a{};
    a.B = B; a.C = C; a.P = P; a.M = M; a.D = gt_cols; a.E = E;
    a.heatmap = heatmap;
    a.maps = TfBoxMaps{P, E, center, height, dim, rot, vel, pc_range[0], pc_range[1], vx, vy, stride};
    a.gt_boxes = gt_boxes;
    a.cls_w = (float)cost_cfg[0]; a.cls_alpha = (float)cost_cfg[1]; a.cls_1malpha = (float)(1.0 - cost_cfg[1]); a.cls_gamma = (float)cost_cfg[2];
    a.cls_eps = (float)cost_cfg[3]; a.reg_w = (float)cost_cfg[4]; a.iou_w = (float)cost_cfg[5];
    a.rx0 = pc_range[0]; a.ry0 = pc_range[1]; a.rdx = pc_range[3] - pc_range[0]; a.rdy = pc_range[4] - pc_range[1];
    a.tx = (float)((double)stride * (double)vx); a.ty = (float)((double)stride * (double)vy);
    a.num_classes = num_classes;
    a.boxes = reinterpret_cast<float *>(ws + off[0]); a.gts = reinterpret_cast<float *>(ws + off[1]);
    a.cost = reinterpret_cast<float *>(ws + off[2]); a.stats = reinterpret_cast<float *>(ws + off[3]);
    a.num_gt = reinterpret_cast<int *>(ws + off[4]); a.row_of_gt = reinterpret_cast<int *>(ws + off[5]);
    a.labels = labels; a.label_weights = label_weights; a.bbox_targets = bbox_targets; a.bbox_weights = bbox_weights; a.ious = ious;
    a.matched_ious = matched_ious; a.assigned = assigned; a.num_pos = num_pos;
    hipStream_t st = as_stream(stream);
    if (int rc = zero_fill(stream, "tf_assign(zero)", heatmap_target, sizeof(float) * (size_t)B * C * H * W)) return rc;
    hipLaunchKernelGGL(tfa_prepare_kernel, dim3((unsigned)B), dim3(LS_T), 0, st, a);
    if (int rc = check_launch("tf_assign(prepare)")) return rc;
    if (M > 0) {
        hipLaunchKernelGGL(tfa_cost_kernel, dim3((unsigned)divup((long long)P * M, LS_T), (unsigned)B), dim3(LS_T), 0, st, a);
        if (int rc = check_launch("tf_assign(cost)")) return rc;
    }
    hipLaunchKernelGGL(tfa_match_kernel, dim3((unsigned)B), dim3(LS_T), 0, st, a);
    if (int rc = check_launch("tf_assign(match)")) return rc;
    hipLaunchKernelGGL(tfa_finish_kernel, dim3(1), dim3(64), 0, st, B, a.stats, num_pos, matched_ious);
    if (int rc = check_launch("tf_assign(finish)")) return rc;
    if (M > 0) {
        const int reach = H > W ? H : W;                         // a window wider than the map adds nothing inside it
        TfaHmArgs h{M, gt_cols, gt_boxes, HmGrid{C, H, W, pc_range[0], pc_range[1], vx, vy, stride, gaussian_overlap, min_radius, reach},
                    heatmap_target};
        hipLaunchKernelGGL(tfa_heatmap_kernel, dim3((unsigned)(B * M)), dim3(LS_T), 0, st, h);
        if (int rc = check_launch("tf_assign(heatmap)")) return rc;
    }
    return 0;
}

static int tfl_blocks(int B, int C, int P, int E) { return divup((long long)B * (C + 8 + E) * P, LS_T); }

extern "C" size_t pdm_tf_loss_workspace_bytes(int B, int C, int P, int with_vel, int H, int W) {
    if (B <= 0 || C < 1 || P < 1 || H < 1 || W < 1) return 0;
    return align256(sizeof(double) * 2 * tfl_blocks(B, C, P, with_vel ? 2 : 0)) + pdm_heatmap_focal_loss_workspace_bytes((long long)B * C * H * W);
}

// code_weights: HOST array of 8 | 10.  out (6): [0] cls loss, [1] box loss, [2] heat-map loss (each weighted), [3] the factor the
// stored d S / d dense_heatmap is multiplied by, [4] the number of heat-map peaks, [5] unused.
extern "C" int pdm_tf_loss(void *stream, int B, int C, int P, int H, int W, const float *heatmap, const float *center, const float *height,
                           const float *dim, const float *rot, const float *vel, const float *dense_heatmap, const long long *labels,
                           const float *label_weights, const float *bbox_targets, const float *bbox_weights, const int *num_pos,
                           const float *heatmap_target, const float *code_weights, float cls_weight, float bbox_weight, float hm_weight,
                           float alpha, float gamma, float *out, float *g_heatmap, float *g_center, float *g_height, float *g_dim,
                           float *g_rot, float *g_vel, float *g_dense, void *workspace, size_t workspace_bytes) {
    PDM_REQUIRE(B >= 1 && C >= 1 && P >= 1 && H >= 1 && W >= 1 && (long long)B * (C + 10) * P <= 0x7fffffffll, PDM_E_BADARG, "tf_loss: bad size");
    PDM_REQUIRE((vel == nullptr) == (g_vel == nullptr), PDM_E_BADARG, "tf_loss: vel and its gradient go together");
    PDM_REQUIRE(heatmap && center && height && dim && rot && dense_heatmap && labels && label_weights && bbox_targets && bbox_weights && num_pos &&
                heatmap_target && code_weights && out && g_heatmap && g_center && g_height && g_dim && g_rot && g_dense && workspace,
                PDM_E_BADARG, "tf_loss: null pointer");
    const int E = vel ? 2 : 0, blocks = tfl_blocks(B, C, P, E);
    const size_t need = pdm_tf_loss_workspace_bytes(B, C, P, E, H, W), head = align256(sizeof(double) * 2 * blocks);
    PDM_REQUIRE(workspace_bytes >= need && (reinterpret_cast<uintptr_t>(workspace) & 7) == 0, PDM_E_BADARG,
                "tf_loss: workspace of %zu bytes, need %zu (8-byte aligned)", workspace_bytes, need);
    TflArgs a{};
    a.B = B; a.C = C; a.P = P; a.E = E;
    a.heatmap = heatmap;
    a.maps[0] = center; a.maps[1] = height; a.maps[2] = dim; a.maps[3] = rot; a.maps[4] = vel;
    a.labels = labels; a.label_weights = label_weights; a.bbox_targets = bbox_targets; a.bbox_weights = bbox_weights; a.num_pos = num_pos;
    for (int d = 0; d < 8 + E; ++d) a.code_w[d] = code_weights[d];
    a.cls_w = cls_weight; a.bbox_w = bbox_weight; a.alpha = alpha; a.gamma = gamma;
    a.g_heatmap = g_heatmap;
    a.g_maps[0] = g_center; a.g_maps[1] = g_height; a.g_maps[2] = g_dim; a.g_maps[3] = g_rot; a.g_maps[4] = g_vel;
    a.partials = static_cast<double *>(workspace);
    hipStream_t st = as_stream(stream);
    hipLaunchKernelGGL(tfl_kernel, dim3((unsigned)blocks), dim3(LS_T), 0, st, a);
    if (int rc = check_launch("tf_loss")) return rc;
    hipLaunchKernelGGL(tfl_finalize_kernel, dim3(1), dim3(LS_T), 0, st, blocks, a.partials, num_pos, cls_weight, bbox_weight, out);
    if (int rc = check_launch("tf_loss(finalize)")) return rc;
    // GaussianFocalLoss(eps = 1e-12) behind clip_sigmoid(1e-4) is the penalty-reduced focal loss of heatmap_loss.hip term for term
    return pdm_heatmap_focal_loss(stream, B, C, H, W, dense_heatmap, 0, (long long)C * H * W, (long long)H * W, W, 1, heatmap_target, hm_weight,
                                  g_dense, out + 2, static_cast<char *>(workspace) + head, workspace_bytes - head);
}

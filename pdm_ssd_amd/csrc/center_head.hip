// CenterHead on the device: target assignment, heat-map box decode and the L1 regression loss with its gradient, each
// one launch chain per head for the whole batch, with no host read and no float atomics on results or gradients.
//
// Restates the reference's pcdet/models/dense_heads/center_head.py:106-162, :189-226 (targets), :297-365 with
// pcdet/models/model_utils/centernet_utils.py:155-241 (decode) and pcdet/utils/loss_utils.py:347-419 with
// center_head.py:245-252 (regression loss).
//
// pdm_center_targets   zero fill -> assign (one workgroup per sample: the head's boxes compacted in their order by a block
//                      scan; slot k < NUM_MAX_OBJS gets inds / mask / target_boxes / target_boxes_src, the rest zeros) ->
//                      draw (one workgroup per slot: the gaussian of heatmap_draw.h, the code pdm_heatmap_targets runs)
// pdm_center_decode    one workgroup per sample: rank_select (rank_select.h) of the K highest sigmoid(hm) over the
//                      flattened (class, y, x), ties by lower flat index; per rank the regression channels gathered at
//                      the cell and decoded; the survivors of the limit range and the score threshold compacted in rank
//                      order by a block scan (count -> scan -> fill inside the workgroup), padding rows zeroed
// pdm_center_reg_loss  partial (one workgroup per sample: per-code sums of |pred m - gt m| and the mask count, in double,
//                      folded in a fixed order) -> finalize (one wave: the sums over the samples in order) -> zero fill ->
//                      grad (one workgroup per sample; the FIRST masked slot that names a cell owns it and adds the
//                      contributions of every masked slot of that cell in slot order: no atomics, two runs give the
//                      same bits; cells no slot names keep the fill's zeros)
#include "heatmap_draw.h"
#include "loss_kit.h"
#include "rank_select.h"

namespace pdm {

constexpr int CT_T = 256;
constexpr int CH_MAX_CLASSES = 32;   // global classes a head's tables hold
constexpr int CH_MAX_CODE = 16;      // 8 + E regression channels
constexpr int CH_MAX_OBJS = 8192;    // slots whose cells the gradient kernel holds in LDS

// ---- targets -------------------------------------------------------------------------------------------------------------
struct CtArgs {
    int B, M, cols, nmax;            // gt_boxes (B, M, cols), cols = 7 + E + 1, class last
    HmGrid grid;                     // grid.C = the head's classes
    const float *gt;
    int num_global;                  // global classes 1 .. num_global
    int local_of[CH_MAX_CLASSES + 1];   // global class -> the head's class, 1-based; 0 = not this head's
    float *heatmap, *target, *src;   // (B, C, H, W), (B, nmax, cols), (B, nmax, cols)
    long long *inds, *mask;          // (B, nmax)
};

__global__ __launch_bounds__(CT_T) void ct_assign_kernel(CtArgs a) {
    __shared__ int s_wave[CT_T / 64];
    const int b = blockIdx.x, tid = threadIdx.x, cols = a.cols;
    int seen = 0;
    for (int c0 = 0; c0 < a.M; c0 += CT_T) {
        const int i = c0 + tid;
        int loc = 0;
        const float *g = a.gt + ((size_t)b * a.M + (i < a.M ? i : 0)) * cols;
        if (i < a.M) {
            const float cls = g[cols - 1];
            if (cls >= 1.0f && cls < (float)(a.num_global + 1)) loc = a.local_of[(int)cls];
        }
        int tot;
        const int k = seen + block_scan<CT_T>(loc > 0 ? 1 : 0, s_wave, &tot);
        seen += tot;
        if (loc <= 0 || k >= a.nmax) continue;
        const size_t slot = (size_t)b * a.nmax + k;
        float *src = a.src + slot * cols, *t = a.target + slot * cols;
        for (int c = 0; c < cols - 1; ++c) src[c] = g[c];
        src[cols - 1] = (float)loc;
        float dxc, dyc;
        if (!hm_size_cells(a.grid, g[3], g[4], &dxc, &dyc)) {      // a used slot that stays empty (the reference `continue`s)
            for (int c = 0; c < cols; ++c) t[c] = 0.0f;
            a.inds[slot] = 0;
            a.mask[slot] = 0;
            continue;
        }
        float cx, cy;
        hm_center_cells(a.grid, g[0], g[1], &cx, &cy);
        const int ix = (int)cx, iy = (int)cy;
        a.inds[slot] = (long long)iy * a.grid.W + ix;
        a.mask[slot] = 1;
        t[0] = cx - (float)ix;
        t[1] = cy - (float)iy;
        t[2] = g[2];
        t[3] = logf(g[3]); t[4] = logf(g[4]); t[5] = logf(g[5]);
        t[6] = cosf(g[6]);
        t[7] = sinf(g[6]);
        for (int c = 8; c < cols; ++c) t[c] = g[c - 1];
    }
    const int used = seen < a.nmax ? seen : a.nmax;
    for (int k = used + tid; k < a.nmax; k += CT_T) {
        const size_t slot = (size_t)b * a.nmax + k;
        for (int c = 0; c < cols; ++c) { a.src[slot * cols + c] = 0.0f; a.target[slot * cols + c] = 0.0f; }
        a.inds[slot] = 0;
        a.mask[slot] = 0;
    }
}

// one workgroup per slot (launched behind ct_assign_kernel on the same stream)
__global__ __launch_bounds__(CT_T) void ct_draw_kernel(CtArgs a) {
    const int slot = blockIdx.x, b = slot / a.nmax;
    if (a.mask[slot] == 0) return;                                  // uniform over the workgroup
    const float *g = a.src + (size_t)slot * a.cols;
    hm_draw_box<CT_T>(a.grid, g[0], g[1], g[3], g[4], g[a.cols - 1], a.heatmap + (size_t)b * a.grid.C * a.grid.H * a.grid.W);
}

// ---- decode --------------------------------------------------------------------------------------------------------------
struct CdArgs {
    int B, C, H, W, K, E;
    MapRef hm, center, center_z, dim, rot, vel;   // vel.p == nullptr without velocity
    float score_thresh, lo[3], hi[3];
    float x0, y0, vx, vy, stride;
    int global_of[CH_MAX_CLASSES];   // the head's class -> global class, 0-based
    float *boxes, *scores;           // (B, K, 7 + E), (B, K)
    long long *labels;               // (B, K)
    int *count;                      // (B)
};

__device__ __forceinline__ float cd_score(const CdArgs &a, int b, int i) {
    const int hw = a.H * a.W, c = i / hw, cell = i - c * hw, y = cell / a.W, x = cell - y * a.W;
    return sigmoid_rn(map_load(a.hm, b, c, y, x));
}

__global__ __launch_bounds__(TK_THREADS) void cd_decode_kernel(CdArgs a) {
    extern __shared__ unsigned long long s_items[];
    __shared__ alignas(16) RankLds lds;
    const int b = blockIdx.x, tid = threadIdx.x;
    const int hw = a.H * a.W, n = a.C * hw, K = a.K, D = 7 + a.E;
    rank_select(n, K, [&](int i) { return topk_key(__float_as_uint(cd_score(a, b, i))); }, s_items, lds);
    __syncthreads();
    float *boxes = a.boxes + (size_t)b * K * D, *scores = a.scores + (size_t)b * K;
    long long *labels = a.labels + (size_t)b * K;
    int kept = 0;
    for (int r0 = 0; r0 < K; r0 += TK_THREADS) {
        const int r = r0 + tid;
        bool keep = false;
        float box[7 + 2], score = 0.0f;
        int c = 0;
        if (r < K) {
            const int i = (int)(unsigned)(s_items[r] & 0xffffffffull);
            c = i / hw;
            const int cell = i - c * hw, y = cell / a.W, x = cell - y * a.W;
            score = cd_score(a, b, i);
            const float px = __fadd_rn((float)x, map_load(a.center, b, 0, y, x)), py = __fadd_rn((float)y, map_load(a.center, b, 1, y, x));
            box[0] = __fadd_rn(__fmul_rn(__fmul_rn(px, a.stride), a.vx), a.x0);
            box[1] = __fadd_rn(__fmul_rn(__fmul_rn(py, a.stride), a.vy), a.y0);
            box[2] = map_load(a.center_z, b, 0, y, x);
            box[3] = expf(map_load(a.dim, b, 0, y, x));
            box[4] = expf(map_load(a.dim, b, 1, y, x));
            box[5] = expf(map_load(a.dim, b, 2, y, x));
            box[6] = atan2f(map_load(a.rot, b, 1, y, x), map_load(a.rot, b, 0, y, x));
            box[7] = box[8] = 0.0f;
            if (a.E == 2) { box[7] = map_load(a.vel, b, 0, y, x); box[8] = map_load(a.vel, b, 1, y, x); }
            keep = score > a.score_thresh;
#pragma unroll
            for (int d = 0; d < 3; ++d) keep = keep && box[d] >= a.lo[d] && box[d] <= a.hi[d];
        }
        int tot;
        const int pos = kept + block_scan<TK_THREADS>(keep ? 1 : 0, lds.wave, &tot);
        kept += tot;
        if (keep) {                                                 // pos <= r: a row is never written before its turn
            for (int d = 0; d < D; ++d) boxes[(size_t)pos * D + d] = box[d];
            scores[pos] = score;
            labels[pos] = (long long)a.global_of[c] + 1;
        }
    }
    for (int r = kept + tid; r < K; r += TK_THREADS) {
        for (int d = 0; d < D; ++d) boxes[(size_t)r * D + d] = 0.0f;
        scores[r] = 0.0f;
        labels[r] = 0;
    }
    if (tid == 0) a.count[b] = kept;
}

// ---- regression loss -------------------------------------------------------------------------------------------------------
struct RlArgs {
    int B, nmax, D, H, W;
    MapRef ch[CH_MAX_CODE];          // a regression channel's (B, H, W) plane: sc = 0
    const long long *inds, *mask;    // (B, nmax)
    const float *target;             // (B, nmax, D)
    float w[CH_MAX_CODE], loc_weight;
    double *partials;                // (B, D + 1): per-code sums, mask count
    float *loss_per_code, *out;      // (D); [0] loc_loss, [1] max(num, 1), [2] num
    float *grad;                     // (B, D, H, W)
};

__device__ __forceinline__ float rl_pred(const RlArgs &a, int d, int b, long long ind) {
    const long long y = ind / a.W, x = ind - y * a.W;
    return map_load(a.ch[d], b, 0, y, x);
}

__global__ __launch_bounds__(CT_T) void rl_partial_kernel(RlArgs a) {
    __shared__ BlockSum<CT_T, CH_MAX_CODE + 1, double> red;
    const int b = blockIdx.x, tid = threadIdx.x, D = a.D;
    const long long hw = (long long)a.H * a.W;
    double acc[CH_MAX_CODE + 1];
#pragma unroll
    for (int d = 0; d <= CH_MAX_CODE; ++d) acc[d] = 0.0;
    for (int k = tid; k < a.nmax; k += CT_T) {
        const size_t slot = (size_t)b * a.nmax + k;
        const float mf = (float)a.mask[slot];
        const long long ind = a.inds[slot];
        acc[CH_MAX_CODE] += (double)mf;
        if (mf == 0.0f || ind < 0 || ind >= hw) continue;
#pragma unroll
        for (int d = 0; d < CH_MAX_CODE; ++d) {
            if (d >= D) break;
            const float gt = a.target[slot * D + d];
            if (gt != gt) continue;                                 // the element's mask is mask * !isnan(target)
            acc[d] += (double)fabsf(__fsub_rn(__fmul_rn(rl_pred(a, d, b, ind), mf), __fmul_rn(gt, mf)));
        }
    }
    red.reduce(acc);                                                // all 17, whatever D is
    if (tid <= D) a.partials[(size_t)b * (D + 1) + tid] = red.total(tid < D ? tid : CH_MAX_CODE);
}

__global__ __launch_bounds__(64) void rl_finalize_kernel(RlArgs a) {
    __shared__ double s_loss[CH_MAX_CODE];
    const int tid = threadIdx.x, D = a.D;
    double num = 0.0;
    for (int b = 0; b < a.B; ++b) num += a.partials[(size_t)b * (D + 1) + D];
    const double den = num > 1.0 ? num : 1.0;
    if (tid < D) {
        double s = 0.0;
        for (int b = 0; b < a.B; ++b) s += a.partials[(size_t)b * (D + 1) + tid];
        const float l = (float)(s / den);
        a.loss_per_code[tid] = l;
        s_loss[tid] = (double)l * (double)a.w[tid];
    }
    __syncthreads();
    if (tid != 0) return;
    double loc = 0.0;
    for (int d = 0; d < D; ++d) loc += s_loss[d];
    a.out[0] = (float)(loc * (double)a.loc_weight);
    a.out[1] = (float)den;
    a.out[2] = (float)num;
}

__global__ __launch_bounds__(CT_T) void rl_grad_kernel(RlArgs a) {
    extern __shared__ int s_cell[];                                 // nmax: the slot's cell, -1 = takes no part
    const int b = blockIdx.x, tid = threadIdx.x, D = a.D;
    const long long hw = (long long)a.H * a.W;
    for (int k = tid; k < a.nmax; k += CT_T) {
        const size_t slot = (size_t)b * a.nmax + k;
        const long long ind = a.inds[slot];
        s_cell[k] = (a.mask[slot] != 0 && ind >= 0 && ind < hw) ? (int)ind : -1;
    }
    __syncthreads();
    const float den = a.out[1];
    for (int k = tid; k < a.nmax; k += CT_T) {
        const int cell = s_cell[k];
        if (cell < 0) continue;
        bool first = true;
        for (int j = 0; j < k; ++j) if (s_cell[j] == cell) { first = false; break; }
        if (!first) continue;                                       // an earlier slot owns the cell
        float acc[CH_MAX_CODE];
#pragma unroll
        for (int d = 0; d < CH_MAX_CODE; ++d) acc[d] = 0.0f;
        for (int j = k; j < a.nmax; ++j) {                          // slot order
            if (s_cell[j] != cell) continue;
            const size_t slot = (size_t)b * a.nmax + j;
            const float mf = (float)a.mask[slot];
#pragma unroll
            for (int d = 0; d < CH_MAX_CODE; ++d) {
                if (d >= D) break;
                const float gt = a.target[slot * D + d];
                if (gt != gt) continue;
                const float diff = __fsub_rn(__fmul_rn(rl_pred(a, d, b, cell), mf), __fmul_rn(gt, mf));
                const float sg = diff > 0.0f ? 1.0f : diff < 0.0f ? -1.0f : 0.0f;
                acc[d] = __fadd_rn(acc[d], __fdiv_rn(__fmul_rn(__fmul_rn(__fmul_rn(sg, mf), a.w[d]), a.loc_weight), den));
            }
        }
#pragma unroll
        for (int d = 0; d < CH_MAX_CODE; ++d) {
            if (d >= D) break;
            a.grad[((size_t)b * D + d) * hw + cell] = acc[d];
        }
    }
}

}  // namespace pdm

using namespace pdm;

// gt_boxes (B, M, cols) fp32, cols = 7 + E + 1 with the global class (1-based, 0 = padding) last; local_of: HOST array of
// num_global + 1 ints, local_of[g] = the head's 1-based class of global class g or 0.  Every output element is written.
extern "C" int pdm_center_targets(void *stream, int B, int M, int cols, int C, int H, int W, const float *gt_boxes, int num_global,
                                  const int *local_of, float x0, float y0, float vx, float vy, float stride, int num_max_objs,
                                  double min_overlap, int min_radius, float *heatmap, float *target_boxes, long long *inds,
                                  long long *mask, float *target_boxes_src) {
    PDM_REQUIRE(B >= 0 && M >= 0 && cols >= 8 && cols - 8 <= CH_MAX_CODE - 8 && C >= 1 && H >= 1 && W >= 1 && H <= 8192 && W <= 8192 &&
                num_max_objs >= 1 && vx > 0.0f && vy > 0.0f && stride > 0.0f && min_radius >= 0,
                PDM_E_BADARG, "center_targets: bad size");
    PDM_REQUIRE(num_global >= 1 && num_global <= CH_MAX_CLASSES && local_of, PDM_E_BADARG, "center_targets: 1 .. %d global classes", CH_MAX_CLASSES);
    if (B == 0) return 0;
    PDM_REQUIRE(heatmap && target_boxes && inds && mask && target_boxes_src && (M == 0 || gt_boxes), PDM_E_BADARG, "center_targets: null pointer");
    PDM_REQUIRE((long long)B * num_max_objs <= 0x7fffffffll, PDM_E_TOOLARGE, "center_targets: %lld slots", (long long)B * num_max_objs);
    CtArgs a{};
    a.B = B; a.M = M; a.cols = cols; a.nmax = num_max_objs;
    // the window is the box's own (2 r + 1)^2 cells: a radius is never clipped short of the map (max_radius = the map's side)
    a.grid = HmGrid{C, H, W, x0, y0, vx, vy, stride, min_overlap, min_radius, H > W ? H : W};
    a.gt = gt_boxes; a.num_global = num_global;
    for (int g = 0; g <= num_global; ++g) {
        PDM_REQUIRE(local_of[g] >= 0 && local_of[g] <= C, PDM_E_BADARG, "center_targets: class table entry %d = %d", g, local_of[g]);
        a.local_of[g] = local_of[g];
    }
    a.local_of[0] = 0;
    a.heatmap = heatmap; a.target = target_boxes; a.src = target_boxes_src; a.inds = inds; a.mask = mask;
    if (int rc = zero_fill(stream, "center_targets(zero)", heatmap, sizeof(float) * (size_t)B * C * H * W)) return rc;
    hipLaunchKernelGGL(ct_assign_kernel, dim3((unsigned)B), dim3(CT_T), 0, as_stream(stream), a);
    if (int rc = check_launch("center_targets(assign)")) return rc;
    hipLaunchKernelGGL(ct_draw_kernel, dim3((unsigned)(B * num_max_objs)), dim3(CT_T), 0, as_stream(stream), a);
    return check_launch("center_targets(draw)");
}

// maps: HOST array of 6 device pointers [hm, center, center_z, dim, rot, vel | NULL]; bf16: HOST array of 6 flags; strides:
// HOST array of 6 x 4 element strides (b, c, y, x).  limit_range: HOST array [x0 y0 z0 x1 y1 z1]; global_of: HOST array of C
// 0-based global classes.  Call once before capturing it in a graph (K > 4096 needs an LDS grant).
extern "C" int pdm_center_decode(void *stream, int B, int C, int H, int W, int K, const void *const *maps, const int *bf16,
                                 const long long *strides, float score_thresh, const float *limit_range, float x0, float y0,
                                 float vx, float vy, float stride, const int *global_of, float *boxes, float *scores,
                                 long long *labels, int *count) {
    PDM_REQUIRE(B >= 0 && C >= 1 && C <= CH_MAX_CLASSES && H >= 1 && W >= 1 && (long long)C * H * W <= 0x7fffffffll, PDM_E_BADARG,
                "center_decode: bad size");
    PDM_REQUIRE(K >= 1 && (long long)K <= (long long)H * W, PDM_E_BADARG, "center_decode: K = %d out of range (1 .. H * W = %lld)", K,
                (long long)H * W);
    PDM_REQUIRE(K <= TK_MAXK, PDM_E_TOOLARGE, "center_decode: K = %d > %d", K, TK_MAXK);
    PDM_REQUIRE(maps && bf16 && strides && limit_range && global_of, PDM_E_BADARG, "center_decode: null table");
    if (B == 0) return 0;
    for (int m = 0; m < 5; ++m) PDM_REQUIRE(maps[m], PDM_E_BADARG, "center_decode: null map %d", m);
    PDM_REQUIRE(boxes && scores && labels && count, PDM_E_BADARG, "center_decode: null output");
    CdArgs a{};
    a.B = B; a.C = C; a.H = H; a.W = W; a.K = K; a.E = maps[5] ? 2 : 0;
    MapRef *refs[6] = {&a.hm, &a.center, &a.center_z, &a.dim, &a.rot, &a.vel};
    for (int m = 0; m < 6; ++m) *refs[m] = map_ref(maps[m], bf16[m], strides + 4 * m);
    a.score_thresh = score_thresh;
    for (int d = 0; d < 3; ++d) { a.lo[d] = limit_range[d]; a.hi[d] = limit_range[3 + d]; }
    a.x0 = x0; a.y0 = y0; a.vx = vx; a.vy = vy; a.stride = stride;
    for (int c = 0; c < C; ++c) a.global_of[c] = global_of[c];
    a.boxes = boxes; a.scores = scores; a.labels = labels; a.count = count;
    const int k2 = 1 << (32 - __builtin_clz((K > 2 ? K : 2) - 1));
    const size_t lds = (size_t)k2 * sizeof(unsigned long long);
    if (lds > 48 * 1024) {   // granted per device (static LDS comes on top, as post_process.hip)
        const int e = grant_lds(reinterpret_cast<const void *>(&cd_decode_kernel), 156 * 1024);
        PDM_REQUIRE(e == 0, PDM_E_TOOLARGE, "center_decode: cannot obtain %zu bytes of LDS: %s", lds, hipGetErrorString((hipError_t)e));
    }
    hipLaunchKernelGGL(cd_decode_kernel, dim3((unsigned)B), dim3(TK_THREADS), lds, as_stream(stream), a);
    return check_launch("center_decode");
}

extern "C" size_t pdm_center_reg_loss_workspace_bytes(int B, int D) {
    return B <= 0 || D <= 0 ? 0 : (size_t)B * (D + 1) * sizeof(double);
}

// chans: HOST array of D device pointers, each the (B, H, W) plane of one regression channel in code order; bf16: HOST
// array of D flags; strides: HOST array of D x 3 element strides (b, y, x); code_weights: HOST array of D floats.
// inds / mask (B, nmax) int64, target (B, nmax, D) fp32.  loss_per_code (D); out[0] = loc_loss, out[1] = max(num, 1),
// out[2] = num; grad (B, D, H, W) fp32 = d loc_loss / d map, every element written.
extern "C" int pdm_center_reg_loss(void *stream, int B, int num_max_objs, int D, int H, int W, const void *const *chans, const int *bf16,
                                   const long long *strides, const long long *inds, const long long *mask, const float *target,
                                   const float *code_weights, float loc_weight, float *loss_per_code, float *out, float *grad,
                                   void *workspace, size_t workspace_bytes) {
    PDM_REQUIRE(B >= 0 && num_max_objs >= 1 && num_max_objs <= CH_MAX_OBJS && D >= 1 && D <= CH_MAX_CODE && H >= 1 && W >= 1 &&
                (long long)H * W <= 0x7fffffffll, PDM_E_BADARG, "center_reg_loss: bad size");
    PDM_REQUIRE(chans && bf16 && strides && code_weights && loss_per_code && out, PDM_E_BADARG, "center_reg_loss: null pointer");
    RlArgs a{};
    a.B = B; a.nmax = num_max_objs; a.D = D; a.H = H; a.W = W;
    for (int d = 0; d < D; ++d) {
        PDM_REQUIRE(B == 0 || chans[d], PDM_E_BADARG, "center_reg_loss: null channel %d", d);
        a.ch[d] = MapRef{chans[d], bf16[d], strides[3 * d], 0, strides[3 * d + 1], strides[3 * d + 2]};
        a.w[d] = code_weights[d];
    }
    a.inds = inds; a.mask = mask; a.target = target; a.loc_weight = loc_weight;
    a.partials = static_cast<double *>(workspace); a.loss_per_code = loss_per_code; a.out = out; a.grad = grad;
    if (B > 0) {
        PDM_REQUIRE(inds && mask && target && grad && workspace, PDM_E_BADARG, "center_reg_loss: null pointer");
        PDM_REQUIRE(workspace_bytes >= pdm_center_reg_loss_workspace_bytes(B, D) && (reinterpret_cast<uintptr_t>(workspace) & 7) == 0,
                    PDM_E_BADARG, "center_reg_loss: workspace of %zu bytes, need %zu (8-byte aligned)", workspace_bytes,
                    pdm_center_reg_loss_workspace_bytes(B, D));
        hipLaunchKernelGGL(rl_partial_kernel, dim3((unsigned)B), dim3(CT_T), 0, as_stream(stream), a);
        if (int rc = check_launch("center_reg_loss(partial)")) return rc;
    }
    hipLaunchKernelGGL(rl_finalize_kernel, dim3(1), dim3(64), 0, as_stream(stream), a);
    if (int rc = check_launch("center_reg_loss(finalize)")) return rc;
    if (B == 0) return 0;
    if (int rc = zero_fill(stream, "center_reg_loss(zero)", grad, sizeof(float) * (size_t)B * D * H * W)) return rc;
    hipLaunchKernelGGL(rl_grad_kernel, dim3((unsigned)B), dim3(CT_T), sizeof(int) * (size_t)num_max_objs, as_stream(stream), a);
    return check_launch("center_reg_loss(grad)");
}

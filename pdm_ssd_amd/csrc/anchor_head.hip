// The anchor head on the device: target assignment, the three loss terms with their gradients, and the box decode, each a
// short launch chain for the whole batch with no host read and no float atomics on any result.
//
// Restates the reference's pcdet/models/dense_heads/target_assigner/axis_aligned_target_assigner.py:36-210 with
// pcdet/utils/box_utils.py:291-340 (targets), pcdet/models/dense_heads/anchor_head_template.py:101-223 with
// pcdet/utils/loss_utils.py:10-141, :183-208 (losses) and anchor_head_template.py:225-272 with
// pcdet/utils/box_coder_utils.py:5-77 (decode).
//
// pdm_anchor_targets    zero fill (box_reg_targets) -> prepare (one workgroup per sample: the boxes that take part grouped by
//                       anchor set in their own order by block scans, each with its axis-aligned BEV box; the per-box
//                       maxima, the example counts and num_pos cleared) -> best (every anchor against the boxes of its set;
//                       the per-box maximum IoU as an integer atomicMax on the bit pattern, LDS first, one global atomic per
//                       box and workgroup) -> assign (the same IoUs again, bit for bit: arg-max box with the lowest index
//                       among equals, forced / matched / unmatched, label, weight, and the residual code of the positives)
//                       [-> norm, only with NORM_BY_NUM_EXAMPLES: positives get 1 / max(#labels >= 0 of the set, 1)].
//                       No (anchors x boxes) matrix exists in memory.
// pdm_anchor_head_loss  loss (a thread owns one cell, or two neighbours along W, and walks the anchor slots: channel reads and
//                       gradient writes are coalesced along W for a fixed channel; sums in double: wave -> LDS -> block
//                       partial) -> finish (one workgroup adds the partials in a fixed order).  Every gradient element is
//                       written, zeros included.
// pdm_anchor_decode     one launch: residual decode against the anchor table, arg-max direction bin (lower bin on equal
//                       logits), heading folded into the bin's period; a workgroup's piece of the table and of the output
//                       passes through LDS, so both move in whole lines.
#include "loss_kit.h"

namespace pdm {

constexpr int AH_T = 256;
constexpr int AH_MAX_GT = 1024;      // boxes of one sample held in LDS
constexpr int AH_MAX_SETS = 16;      // anchor sets
constexpr int AH_MAX_SLOTS = 32;     // anchors per location
constexpr int AH_MAX_CLASSES = 32;
constexpr int AH_MAX_BINS = 8;       // direction bins
constexpr int AH_PER_BLOCK = 4;      // anchors per thread of the best / assign kernels
constexpr int AH_REC = 8;            // words per prepared box: x1 y1 x2 y2 area | source row | class | unused

#define AH_PI 3.14159274101257324f           // fp32(pi): the period a fp32 tensor is divided by
#define AH_PI_4 0.785398185253143311f        // fp32(pi / 4)
#define AH_2PI 6.28318548202514648f          // fp32(2 pi)

// V cells along W from (b, c, y, x).  V = 2: two neighbours in one access (the host checked sw == 1, even strides and the
// alignment: ah_pair_ok)
template <int V>
__device__ __forceinline__ void ah_load(const MapRef &m, int b, int c, int y, int x, float *v) {
    const long long off = map_offset(m, b, c, y, x);
    if (V == 2) {
        if (m.bf16) {
            const unsigned u = *reinterpret_cast<const unsigned *>(static_cast<const unsigned short *>(m.p) + off);
            v[0] = __uint_as_float(u << 16);
            v[V - 1] = __uint_as_float(u & 0xffff0000u);
        } else {
            const float2 f = *reinterpret_cast<const float2 *>(static_cast<const float *>(m.p) + off);
            v[0] = f.x;
            v[V - 1] = f.y;
        }
    } else {
        v[0] = load_f32_or_bf16(m.p, off, m.bf16);
    }
}

template <int V>
__device__ __forceinline__ void ah_store(float *p, const float *v) {
    if (V == 2) *reinterpret_cast<float2 *>(p) = make_float2(v[0], v[V - 1]);
    else p[0] = v[0];
}

// limit_period(val, offset, period) = val - floor(val / period + offset) * period, every step rounded to fp32
__device__ __forceinline__ float ah_limit_period(float val, float offset, float period) {
    return __fsub_rn(val, __fmul_rn(floorf(__fadd_rn(__fdiv_rn(val, period), offset)), period));
}

// boxes3d_lidar_to_aligned_bev_boxes: |limit_period(heading, 0.5, pi)| >= pi / 4 swaps the extents
__device__ __forceinline__ void ah_bev(float x, float y, float dx, float dy, float heading, float *bev) {
    const float r = fabsf(ah_limit_period(heading, 0.5f, AH_PI));
    const bool keep = r < AH_PI_4;
    const float hx = __fmul_rn(keep ? dx : dy, 0.5f), hy = __fmul_rn(keep ? dy : dx, 0.5f);
    bev[0] = __fsub_rn(x, hx);
    bev[1] = __fsub_rn(y, hy);
    bev[2] = __fadd_rn(x, hx);
    bev[3] = __fadd_rn(y, hy);
}

__device__ __forceinline__ float ah_area(const float *bev) {
    return __fmul_rn(__fsub_rn(bev[2], bev[0]), __fsub_rn(bev[3], bev[1]));
}

// boxes_iou_normal for one pair: intersection / max(area_a + area_b - intersection, 1e-6).  Boxes that do not overlap along
// an axis give an intersection of exactly +0 and an IoU of exactly +0: the rest is skipped for them, same bits.  B: any
// type with x1 / y1 / x2 / y2 / area arrays (the staged boxes), read only as far as the pair gets.
template <typename B>
__device__ __forceinline__ float ah_iou(const float *a, float area_a, const B &l, int j) {
    const float xl = fmaxf(__fsub_rn(fminf(a[2], l.x2[j]), fmaxf(a[0], l.x1[j])), 0.0f);
    if (xl == 0.0f) return 0.0f;
    const float yl = fmaxf(__fsub_rn(fminf(a[3], l.y2[j]), fmaxf(a[1], l.y1[j])), 0.0f);
    if (yl == 0.0f) return 0.0f;
    const float inter = __fmul_rn(xl, yl);
    return __fdiv_rn(inter, fmaxf(__fsub_rn(__fadd_rn(area_a, l.area[j]), inter), 1e-6f));
}

// ---- targets -------------------------------------------------------------------------------------------------------------
struct AtArgs {
    int B, M, cols, A, A_loc, S, C, norm;
    const float *anchors;            // (A, 7)
    const float *gt;                 // (B, M, cols)
    int set_of_slot[AH_MAX_SLOTS];
    int set_of_class[AH_MAX_CLASSES + 1];   // global class (1-based) -> set, -1 = none
    float matched[AH_MAX_SETS], unmatched[AH_MAX_SETS];
    int *labels;                     // (B, A)
    float *targets;                  // (B, A, 7)
    float *weights;                  // (B, A)
    int *num_pos;                    // (B)
    // workspace
    int *starts;                     // (B, S + 1): the sets' ranges of the prepared boxes
    float *rec;                      // (B, M, AH_REC)
    unsigned *best;                  // (B, M): bit pattern of every prepared box's best IoU
    int *examples;                   // (B, S): labels >= 0 per set
};

__global__ __launch_bounds__(AH_T) void at_prepare_kernel(AtArgs a) {
    __shared__ int s_wave[AH_T / 64];
    const int b = blockIdx.x, tid = threadIdx.x;
    int placed = 0;
    for (int s = 0; s < a.S; ++s) {
        if (tid == 0) a.starts[b * (a.S + 1) + s] = placed;
        for (int c0 = 0; c0 < a.M; c0 += AH_T) {
            const int i = c0 + tid;
            const float *g = a.gt + ((size_t)b * a.M + (i < a.M ? i : 0)) * a.cols;
            bool mine = false;
            int cls = 0;
            if (i < a.M) {
                const float cf = g[a.cols - 1];
                if (cf >= 1.0f && cf < (float)(a.C + 1)) {
                    cls = (int)cf;
                    mine = a.set_of_class[cls] == s;
                }
            }
            int tot;
            const int k = placed + block_scan<AH_T>(mine ? 1 : 0, s_wave, &tot);
            placed += tot;
            if (!mine) continue;
            float *r = a.rec + ((size_t)b * a.M + k) * AH_REC;
            float bev[4];
            ah_bev(g[0], g[1], g[3], g[4], g[6], bev);
            r[0] = bev[0]; r[1] = bev[1]; r[2] = bev[2]; r[3] = bev[3];
            r[4] = ah_area(bev);
            r[5] = __int_as_float(i);
            r[6] = __int_as_float(cls);
            r[7] = 0.0f;
        }
    }
    if (tid == 0) {
        a.starts[b * (a.S + 1) + a.S] = placed;
        a.num_pos[b] = 0;
    }
    for (int i = tid; i < a.M; i += AH_T) a.best[(size_t)b * a.M + i] = 0u;
    for (int s = tid; s < a.S; s += AH_T) a.examples[b * a.S + s] = 0;
}

struct AtLds {
    float x1[AH_MAX_GT], y1[AH_MAX_GT], x2[AH_MAX_GT], y2[AH_MAX_GT], area[AH_MAX_GT];
    unsigned best[AH_MAX_GT];
    int starts[AH_MAX_SETS + 1];
};

// the sample's prepared boxes into LDS; n = how many (<= AH_MAX_GT: the host refused a larger M)
__device__ __forceinline__ int at_stage(const AtArgs &a, int b, AtLds &l, bool global_best) {
    const int tid = threadIdx.x;
    if (tid <= a.S) l.starts[tid] = a.starts[b * (a.S + 1) + tid];
    __syncthreads();
    const int n = l.starts[a.S];
    for (int j = tid; j < n; j += AH_T) {
        const float *r = a.rec + ((size_t)b * a.M + j) * AH_REC;
        l.x1[j] = r[0]; l.y1[j] = r[1]; l.x2[j] = r[2]; l.y2[j] = r[3]; l.area[j] = r[4];
        l.best[j] = global_best ? a.best[(size_t)b * a.M + j] : 0u;
    }
    __syncthreads();
    return n;
}

__global__ __launch_bounds__(AH_T) void at_best_kernel(AtArgs a) {
    __shared__ AtLds l;
    const int b = blockIdx.y, tid = threadIdx.x;
    const int n = at_stage(a, b, l, false);
    if (n == 0) return;                                             // uniform over the workgroup
    for (int k = 0; k < AH_PER_BLOCK; ++k) {
        const int i = ((int)blockIdx.x * AH_PER_BLOCK + k) * AH_T + tid;      // A * 7 fits int32: 32-bit index arithmetic
        if (i >= a.A) break;
        const int s = a.set_of_slot[i % a.A_loc];
        const int j0 = l.starts[s], j1 = l.starts[s + 1];
        if (j0 == j1) continue;
        const float *an = a.anchors + i * 7;
        float bev[4];
        ah_bev(an[0], an[1], an[3], an[4], an[6], bev);
        const float area = ah_area(bev);
        for (int j = j0; j < j1; ++j) {
            const unsigned bits = __float_as_uint(ah_iou(bev, area, l, j));
            if (bits > l.best[j]) atomicMax(&l.best[j], bits);      // an IoU is >= +0: its bits order as the value does
        }
    }
    __syncthreads();
    for (int j = tid; j < n; j += AH_T)
        if (l.best[j] != 0u) atomicMax(&a.best[(size_t)b * a.M + j], l.best[j]);
}

__global__ __launch_bounds__(AH_T) void at_assign_kernel(AtArgs a) {
    __shared__ AtLds l;
    __shared__ int s_src[AH_MAX_GT], s_cls[AH_MAX_GT];
    __shared__ int s_examples[AH_MAX_SETS], s_pos;
    const int b = blockIdx.y, tid = threadIdx.x;
    const int n = at_stage(a, b, l, true);
    for (int j = tid; j < n; j += AH_T) {
        const float *r = a.rec + ((size_t)b * a.M + j) * AH_REC;
        s_src[j] = __float_as_int(r[5]);
        s_cls[j] = __float_as_int(r[6]);
    }
    if (tid < AH_MAX_SETS) s_examples[tid] = 0;
    if (tid == 0) s_pos = 0;
    __syncthreads();
    for (int k = 0; k < AH_PER_BLOCK; ++k) {
        const int i = ((int)blockIdx.x * AH_PER_BLOCK + k) * AH_T + tid;      // A * 7 fits int32: 32-bit index arithmetic
        if (i >= a.A) break;
        const int s = a.set_of_slot[i % a.A_loc];
        const int j0 = l.starts[s], j1 = l.starts[s + 1];
        const float *an = a.anchors + i * 7;
        int label = 0, arg = -1;
        if (j0 < j1) {
            float bev[4];
            ah_bev(an[0], an[1], an[3], an[4], an[6], bev);
            const float area = ah_area(bev);
            float top = -1.0f;
            bool forced = false;
            for (int j = j0; j < j1; ++j) {
                const float iou = ah_iou(bev, area, l, j);
                if (iou > top) { top = iou; arg = j; }              // the first of equals: the lowest index
                const unsigned bits = __float_as_uint(iou);
                forced = forced || (bits != 0u && bits == l.best[j]);   // a best of exactly 0 forces no anchor
            }
            if (arg < 0) { arg = j0; top = 0.0f; }                  // (every IoU NaN)
            label = -1;
            if (top >= a.matched[s]) label = s_cls[arg];
            if (top < a.unmatched[s]) label = 0;
            if (forced) label = s_cls[arg];
        }
        const size_t o = (size_t)b * a.A + i;
        a.labels[o] = label;
        a.weights[o] = label > 0 ? 1.0f : 0.0f;
        if (a.norm && label >= 0) atomicAdd(&s_examples[s], 1);
        if (label > 0) {
            atomicAdd(&s_pos, 1);
            const float *g = a.gt + ((size_t)b * a.M + s_src[arg]) * a.cols;
            const float dxa = fmaxf(an[3], 1e-5f), dya = fmaxf(an[4], 1e-5f), dza = fmaxf(an[5], 1e-5f);
            const float diag = __fsqrt_rn(__fadd_rn(__fmul_rn(dxa, dxa), __fmul_rn(dya, dya)));
            float *t = a.targets + o * 7;
            residual_encode(g, an, dxa, dya, dza, diag, t);
            t[6] = __fsub_rn(g[6], an[6]);
        }
    }
    __syncthreads();
    if (tid == 0 && s_pos != 0) atomicAdd(&a.num_pos[b], s_pos);
    if (a.norm && tid < a.S && s_examples[tid] != 0) atomicAdd(&a.examples[b * a.S + tid], s_examples[tid]);
}

__global__ __launch_bounds__(AH_T) void at_norm_kernel(AtArgs a) {
    const int b = blockIdx.y;
    const int i = (int)blockIdx.x * AH_T + threadIdx.x;
    if (i >= a.A) return;
    const size_t o = (size_t)b * a.A + i;
    if (a.labels[o] <= 0) return;
    const int cnt = a.examples[b * a.S + a.set_of_slot[i % a.A_loc]];
    a.weights[o] = __fdiv_rn(1.0f, (float)(cnt > 1 ? cnt : 1));
}

// ---- loss ------------------------------------------------------------------------------------------------------------------
struct AlArgs {
    int B, H, W, A_loc, C, NB;
    MapRef cls, box, dir;            // dir.p == nullptr: no direction classifier
    const int *labels;               // (B, A)
    const float *targets;            // (B, A, 7)
    const int *num_pos;              // (B)
    float rot[AH_MAX_SLOTS], cw[7];
    float cls_weight, loc_weight, dir_weight, dir_offset, beta, alpha, gamma;
    double *partials;                // (B * gridDim.x, 3)
    int num_partials;
    float *out;                      // [cls_loss, loc_loss, dir_loss]
    float *g_cls, *g_box, *g_dir;    // (B, A_loc * C | 7 | NB, H, W)
};

template <int V>
__global__ __launch_bounds__(AH_T) void al_loss_kernel(AlArgs a) {
    __shared__ BlockSum<AH_T, 3, double> red;
    const int b = blockIdx.y, tid = threadIdx.x;
    const int Wg = a.W / V;
    const long long t = (long long)blockIdx.x * AH_T + tid, hw = (long long)a.H * a.W, A = hw * a.A_loc;
    double acc[3] = {0.0, 0.0, 0.0};
    if (t < (long long)a.H * Wg) {
        const int y = (int)(t / Wg), x = (int)(t - (long long)y * Wg) * V;
        const long long cell0 = (long long)y * a.W + x;
        const int np = a.num_pos[b];
        const float w = __fdiv_rn(1.0f, (float)(np > 1 ? np : 1));
        const float invB = __fdiv_rn(1.0f, (float)a.B);
        const float gs_cls = __fmul_rn(__fmul_rn(w, a.cls_weight), invB), gs_loc = __fmul_rn(__fmul_rn(w, a.loc_weight), invB),
                    gs_dir = __fmul_rn(__fmul_rn(w, a.dir_weight), invB);
        const int C = a.C, NB = a.NB;
        for (int s = 0; s < a.A_loc; ++s) {
            int lab[V];
            bool any_pos = false;
#pragma unroll
            for (int i = 0; i < V; ++i) {
                lab[i] = a.labels[(size_t)b * A + (cell0 + i) * a.A_loc + s];
                any_pos = any_pos || lab[i] > 0;
            }
            // sigmoid focal loss over the anchors with label >= 0
            for (int c = 0; c < C; ++c) {
                float xv[V], g[V];
                ah_load<V>(a.cls, b, s * C + c, y, x, xv);
#pragma unroll
                for (int i = 0; i < V; ++i) {
                    g[i] = 0.0f;
                    if (lab[i] < 0) continue;
                    const bool hit = lab[i] > 0 && (C == 1 || lab[i] == c + 1);
                    const float xx = xv[i], tt = hit ? 1.0f : 0.0f;
                    const float p = sigmoid_rn(xx);
                    const float miss = hit ? 1.0f - p : p, bal = hit ? a.alpha : 1.0f - a.alpha;
                    const float bce = bce_with_logits(xx, tt);
                    const float mg = powf(miss, a.gamma);
                    acc[0] += (double)(bal * mg * bce * w);
                    const float dmiss = (hit ? -1.0f : 1.0f) * p * (1.0f - p);
                    const float mg1 = a.gamma == 2.0f ? miss : powf(miss, a.gamma - 1.0f);
                    g[i] = bal * (a.gamma * mg1 * dmiss * bce + mg * (p - tt)) * gs_cls;
                }
                ah_store<V>(a.g_cls + ((size_t)b * a.A_loc * C + s * C + c) * hw + cell0, g);
            }
            // smooth-L1 and direction cross-entropy on the positives
            float gb[7][V], gd[AH_MAX_BINS][V];
#pragma unroll
            for (int k = 0; k < 7; ++k)
#pragma unroll
                for (int i = 0; i < V; ++i) gb[k][i] = 0.0f;
#pragma unroll
            for (int j = 0; j < AH_MAX_BINS; ++j)
#pragma unroll
                for (int i = 0; i < V; ++i) gd[j][i] = 0.0f;
            if (any_pos) {
                float pk[7][V], lg[AH_MAX_BINS][V];
#pragma unroll
                for (int k = 0; k < 7; ++k)
                    ah_load<V>(a.box, b, s * 7 + k, y, x, pk[k]);
                if (a.dir.p) {
#pragma unroll
                    for (int j = 0; j < AH_MAX_BINS; ++j) {
                        if (j >= NB) break;
                        ah_load<V>(a.dir, b, s * NB + j, y, x, lg[j]);
                    }
                }
#pragma unroll
                for (int i = 0; i < V; ++i) {
                    if (lab[i] <= 0) continue;
                    const float *tg = a.targets + ((size_t)b * A + (cell0 + i) * a.A_loc + s) * 7;
#pragma unroll
                    for (int k = 0; k < 7; ++k) {
                        float pv = pk[k][i], tv = tg[k], dpv = 1.0f;
                        if (k == 6) {                               // sin(p - t) = sin p cos t - cos p sin t
                            const float sp = sinf(pv), cp = cosf(pv), st = sinf(tv), ct = cosf(tv);
                            pv = sp * ct;
                            tv = cp * st;
                            dpv = cp * ct + sp * st;
                        }
                        if (tv != tv) continue;                     // a NaN target switches its element off
                        float loss, dl;
                        smooth_l1((pv - tv) * a.cw[k], a.beta, &loss, &dl);
                        acc[1] += (double)(loss * w);
                        gb[k][i] = dl * a.cw[k] * dpv * gs_loc;
                    }
                    if (a.dir.p) {
                        const float rot_gt = __fadd_rn(tg[6], a.rot[s]);
                        const float off = ah_limit_period(__fsub_rn(rot_gt, a.dir_offset), 0.0f, AH_2PI);
                        int bin = (int)floorf(__fdiv_rn(off, __fdiv_rn(AH_2PI, (float)NB)));
                        bin = bin < 0 ? 0 : bin > NB - 1 ? NB - 1 : bin;
                        float mx = lg[0][i];
#pragma unroll
                        for (int j = 1; j < AH_MAX_BINS; ++j) {
                            if (j >= NB) break;
                            mx = fmaxf(mx, lg[j][i]);
                        }
                        float se = 0.0f, hit_logit = 0.0f;
#pragma unroll
                        for (int j = 0; j < AH_MAX_BINS; ++j) {
                            if (j >= NB) break;
                            se += expf(lg[j][i] - mx);
                            if (j == bin) hit_logit = lg[j][i];
                        }
                        acc[2] += (double)((mx + logf(se) - hit_logit) * w);
#pragma unroll
                        for (int j = 0; j < AH_MAX_BINS; ++j) {
                            if (j >= NB) break;
                            gd[j][i] = (expf(lg[j][i] - mx) / se - (j == bin ? 1.0f : 0.0f)) * gs_dir;
                        }
                    }
                }
            }
#pragma unroll
            for (int k = 0; k < 7; ++k) ah_store<V>(a.g_box + ((size_t)b * a.A_loc * 7 + s * 7 + k) * hw + cell0, gb[k]);
            if (a.dir.p) {
#pragma unroll
                for (int j = 0; j < AH_MAX_BINS; ++j) {
                    if (j >= NB) break;
                    ah_store<V>(a.g_dir + ((size_t)b * a.A_loc * NB + s * NB + j) * hw + cell0, gd[j]);
                }
            }
        }
    }
    red.reduce(acc);
    if (tid < 3) a.partials[((size_t)b * gridDim.x + blockIdx.x) * 3 + tid] = red.total(tid);
}

// one workgroup folds the block partials (FoldSum)
__global__ __launch_bounds__(AH_T) void al_finish_kernel(AlArgs a) {
    __shared__ FoldSum<AH_T, 3> sum;
    const int tid = threadIdx.x;
    sum.fold(a.partials, a.num_partials);
    if (tid < 3) {
        const float weight = tid == 0 ? a.cls_weight : tid == 1 ? a.loc_weight : a.dir_weight;
        a.out[tid] = (float)(sum.total(tid) / (double)(a.B > 0 ? a.B : 1)) * weight;
    }
}

// ---- decode ----------------------------------------------------------------------------------------------------------------
struct AdArgs {
    int B, H, W, A_loc, NB;
    MapRef box, dir;                 // dir.p == nullptr: no direction classifier
    const float *anchors;            // (H W A_loc, 7)
    float dir_offset, dir_limit_offset;
    float *out;                      // (B, H W A_loc, 7)
    int vec4;                        // the table, the output and a sample's piece of it are 16-byte aligned
};

constexpr int AD_T = 64;             // one wave a workgroup: AD_T * V cells x A_loc x 28 bytes of LDS
constexpr int AD_PAIR_SLOTS = 13;    // two cells a thread up to here (46 KB), one beyond (57 KB at AH_MAX_SLOTS)

// A workgroup owns AD_T * V consecutive cells.  Their anchors are one contiguous piece of the table and their boxes one
// contiguous piece of the output, in the same (cell, slot, 7) order: the piece is staged in LDS, decoded in place, and leaves
// in whole lines (a thread's own rows lie A_loc * 28 bytes apart).
template <int V>
__global__ __launch_bounds__(AD_T) void ad_decode_kernel(AdArgs a) {
    extern __shared__ float s_box[];                                // (cells, A_loc, 7)
    const int b = blockIdx.y, tid = threadIdx.x;
    const int Wg = a.W / V;
    const long long t = (long long)blockIdx.x * AD_T + tid, hw = (long long)a.H * a.W, A = hw * a.A_loc;
    const long long first = (long long)blockIdx.x * AD_T * V;       // the first cell: a thread's cell0 = t * V
    const long long left = hw - first;
    const int nfl = (int)(left < AD_T * V ? left : AD_T * V) * a.A_loc * 7;
    const float *src = a.anchors + first * a.A_loc * 7;
    float *dst = a.out + ((size_t)b * A + first * a.A_loc) * 7;
    const int n4 = a.vec4 ? nfl / 4 : 0;
    for (int i = tid; i < n4; i += AD_T) reinterpret_cast<float4 *>(s_box)[i] = reinterpret_cast<const float4 *>(src)[i];
    for (int i = n4 * 4 + tid; i < nfl; i += AD_T) s_box[i] = src[i];
    __syncthreads();
    if (t < (long long)a.H * Wg) {
        const int y = (int)(t / Wg), x = (int)(t - (long long)y * Wg) * V;
        const int NB = a.NB;
        const float period = __fdiv_rn(AH_2PI, (float)(NB > 0 ? NB : 1));
        for (int s = 0; s < a.A_loc; ++s) {
            float pk[7][V];
#pragma unroll
            for (int k = 0; k < 7; ++k)
                ah_load<V>(a.box, b, s * 7 + k, y, x, pk[k]);
            int bin[V];
#pragma unroll
            for (int i = 0; i < V; ++i) bin[i] = 0;
            if (a.dir.p) {
                float top[V];
#pragma unroll
                for (int j = 0; j < AH_MAX_BINS; ++j) {
                    if (j >= NB) break;
                    float lg[V];
                    ah_load<V>(a.dir, b, s * NB + j, y, x, lg);
#pragma unroll
                    for (int i = 0; i < V; ++i)
                        if (j == 0 || lg[i] > top[i]) { top[i] = lg[i]; bin[i] = j; }      // the lower bin on equal logits
                }
            }
#pragma unroll
            for (int i = 0; i < V; ++i) {
                float *o = s_box + ((tid * V + i) * a.A_loc + s) * 7;
                float an[7];
#pragma unroll
                for (int k = 0; k < 7; ++k) an[k] = o[k];
                const float diag = __fsqrt_rn(__fadd_rn(__fmul_rn(an[3], an[3]), __fmul_rn(an[4], an[4])));
                o[0] = __fadd_rn(__fmul_rn(pk[0][i], diag), an[0]);
                o[1] = __fadd_rn(__fmul_rn(pk[1][i], diag), an[1]);
                o[2] = __fadd_rn(__fmul_rn(pk[2][i], an[5]), an[2]);
                o[3] = __fmul_rn(expf(pk[3][i]), an[3]);
                o[4] = __fmul_rn(expf(pk[4][i]), an[4]);
                o[5] = __fmul_rn(expf(pk[5][i]), an[5]);
                float rg = __fadd_rn(pk[6][i], an[6]);
                if (a.dir.p) {
                    const float folded = ah_limit_period(__fsub_rn(rg, a.dir_offset), a.dir_limit_offset, period);
                    rg = __fadd_rn(__fadd_rn(folded, a.dir_offset), __fmul_rn(period, (float)bin[i]));
                }
                o[6] = rg;
            }
        }
    }
    __syncthreads();
    for (int i = tid; i < n4; i += AD_T) reinterpret_cast<float4 *>(dst)[i] = reinterpret_cast<const float4 *>(s_box)[i];
    for (int i = n4 * 4 + tid; i < nfl; i += AD_T) dst[i] = s_box[i];
}

// two neighbours along W in one access: unit stride along W, every other stride even, the first element on a pair boundary
static bool ah_pair_ok(const MapRef &m) {
    if (!m.p) return true;
    const uintptr_t pair = m.bf16 ? 4 : 8;
    return m.sw == 1 && m.sb % 2 == 0 && m.sc % 2 == 0 && m.sh % 2 == 0 && (reinterpret_cast<uintptr_t>(m.p) % pair) == 0;
}

static int ah_loss_blocks(int H, int W, int V) { return divup((long long)H * (W / V), AH_T); }

}  // namespace pdm

using namespace pdm;

extern "C" size_t pdm_anchor_targets_workspace_bytes(int B, int M, int num_sets) {
    if (B <= 0 || M < 0 || num_sets <= 0) return 0;
    return align256(sizeof(int) * (size_t)B * (num_sets + 1)) + align256(sizeof(float) * (size_t)B * M * AH_REC) +
           align256(sizeof(unsigned) * (size_t)B * M) + align256(sizeof(int) * (size_t)B * num_sets);
}

// anchors (A, 7) fp32 on the device, A = cells * A_loc in the order y, x, slot; set_of_slot: HOST array of A_loc anchor sets;
// set_of_class: HOST array of num_class + 1 ints, [g] = the set of global class g (1-based) or -1; matched / unmatched: HOST
// arrays of num_sets thresholds; gt_boxes (B, M, cols >= 8) fp32, class last, NOT modified.  Every output element is written.
extern "C" int pdm_anchor_targets(void *stream, int B, int M, int cols, int A, int A_loc, int num_sets, int num_class,
                                  const float *anchors, const int *set_of_slot, const int *set_of_class, const float *matched,
                                  const float *unmatched, const float *gt_boxes, int norm_by_num_examples, int *box_cls_labels,
                                  float *box_reg_targets, float *reg_weights, int *num_pos, void *workspace, size_t workspace_bytes) {
    PDM_REQUIRE(B >= 0 && B <= 65535 && M >= 0 && cols >= 8 && A >= 1 && A_loc >= 1 && A_loc <= AH_MAX_SLOTS && A % A_loc == 0 &&
                num_sets >= 1 && num_sets <= AH_MAX_SETS && num_class >= 1 && num_class <= AH_MAX_CLASSES, PDM_E_BADARG,
                "anchor_targets: bad size (B %d, M %d, cols %d, A %d, A_loc %d <= %d, sets %d <= %d, classes %d <= %d)", B, M, cols, A, A_loc,
                AH_MAX_SLOTS, num_sets, AH_MAX_SETS, num_class, AH_MAX_CLASSES);
    PDM_REQUIRE(M <= AH_MAX_GT, PDM_E_TOOLARGE, "anchor_targets: M = %d boxes per sample > MAX_GT = %d", M, AH_MAX_GT);
    PDM_REQUIRE((long long)A * 7 + (long long)AH_T * AH_PER_BLOCK <= 0x7fffffffll, PDM_E_TOOLARGE, "anchor_targets: A = %d anchors per sample", A);
    PDM_REQUIRE(set_of_slot && set_of_class && matched && unmatched, PDM_E_BADARG, "anchor_targets: null table");
    AtArgs a{};
    a.B = B; a.M = M; a.cols = cols; a.A = A; a.A_loc = A_loc; a.S = num_sets; a.C = num_class; a.norm = norm_by_num_examples ? 1 : 0;
    for (int s = 0; s < A_loc; ++s) {
        PDM_REQUIRE(set_of_slot[s] >= 0 && set_of_slot[s] < num_sets, PDM_E_BADARG, "anchor_targets: slot %d names set %d", s, set_of_slot[s]);
        a.set_of_slot[s] = set_of_slot[s];
    }
    a.set_of_class[0] = -1;
    for (int g = 1; g <= num_class; ++g) {
        PDM_REQUIRE(set_of_class[g] >= -1 && set_of_class[g] < num_sets, PDM_E_BADARG, "anchor_targets: class %d names set %d", g, set_of_class[g]);
        a.set_of_class[g] = set_of_class[g];
    }
    for (int s = 0; s < num_sets; ++s) { a.matched[s] = matched[s]; a.unmatched[s] = unmatched[s]; }
    if (B == 0) return 0;
    PDM_REQUIRE(anchors && box_cls_labels && box_reg_targets && reg_weights && num_pos && (M == 0 || gt_boxes), PDM_E_BADARG,
                "anchor_targets: null pointer");
    PDM_REQUIRE(workspace && workspace_bytes >= pdm_anchor_targets_workspace_bytes(B, M, num_sets), PDM_E_BADARG,
                "anchor_targets: workspace too small (%zu bytes, need %zu)", workspace_bytes, pdm_anchor_targets_workspace_bytes(B, M, num_sets));
    PDM_WS_ALIGNED("anchor_targets", workspace);
    char *ws = static_cast<char *>(workspace);
    a.starts = reinterpret_cast<int *>(ws);      ws += align256(sizeof(int) * (size_t)B * (num_sets + 1));
    a.rec = reinterpret_cast<float *>(ws);       ws += align256(sizeof(float) * (size_t)B * M * AH_REC);
    a.best = reinterpret_cast<unsigned *>(ws);   ws += align256(sizeof(unsigned) * (size_t)B * M);
    a.examples = reinterpret_cast<int *>(ws);
    a.anchors = anchors; a.gt = gt_boxes;
    a.labels = box_cls_labels; a.targets = box_reg_targets; a.weights = reg_weights; a.num_pos = num_pos;
    if (int rc = zero_fill(stream, "anchor_targets(zero)", box_reg_targets, sizeof(float) * (size_t)B * A * 7)) return rc;
    hipLaunchKernelGGL(at_prepare_kernel, dim3((unsigned)B), dim3(AH_T), 0, as_stream(stream), a);
    if (int rc = check_launch("anchor_targets(prepare)")) return rc;
    const dim3 grid((unsigned)divup(A, (long long)AH_T * AH_PER_BLOCK), (unsigned)B);
    hipLaunchKernelGGL(at_best_kernel, grid, dim3(AH_T), 0, as_stream(stream), a);
    if (int rc = check_launch("anchor_targets(best)")) return rc;
    hipLaunchKernelGGL(at_assign_kernel, grid, dim3(AH_T), 0, as_stream(stream), a);
    if (int rc = check_launch("anchor_targets(assign)")) return rc;
    if (!a.norm) return 0;
    hipLaunchKernelGGL(at_norm_kernel, dim3((unsigned)divup(A, AH_T), (unsigned)B), dim3(AH_T), 0, as_stream(stream), a);
    return check_launch("anchor_targets(norm)");
}

extern "C" size_t pdm_anchor_head_loss_workspace_bytes(int B, int H, int W) {
    if (B <= 0 || H <= 0 || W <= 0) return 0;
    return sizeof(double) * 3 * (size_t)B * ah_loss_blocks(H, W, 1);
}

// maps: HOST array of 3 device pointers [cls (A_loc C), box (A_loc 7), dir (A_loc num_dir_bins) | NULL], (B, channels, H, W)
// with channel = slot * width + column; bf16: HOST array of 3 flags; strides: HOST array of 3 x 4 element strides (b, c, y, x).
// labels (B, A) int32, targets (B, A, 7) fp32, num_pos (B) int32 with A = H W A_loc in the order y, x, slot; anchor_rot: HOST
// array of A_loc rotations; code_weights: HOST array of 7.  out[0..2] = the weighted cls / loc / dir terms (dir 0 without the
// map); grad_* fp32 NCHW = d term / d map, every element written (grad_dir may be NULL without the map).
extern "C" int pdm_anchor_head_loss(void *stream, int B, int H, int W, int A_loc, int num_class, int num_dir_bins, const void *const *maps,
                                    const int *bf16, const long long *strides, const int *labels, const float *targets, const int *num_pos,
                                    const float *anchor_rot, const float *code_weights, float cls_weight, float loc_weight, float dir_weight,
                                    float dir_offset, float beta, float alpha, float gamma, float *out, float *grad_cls, float *grad_box,
                                    float *grad_dir, void *workspace, size_t workspace_bytes) {
    PDM_REQUIRE(B >= 0 && B <= 65535 && H >= 1 && W >= 1 && A_loc >= 1 && A_loc <= AH_MAX_SLOTS && num_class >= 1 && num_class <= AH_MAX_CLASSES &&
                (long long)H * W * A_loc * 7 <= 0x7fffffffll, PDM_E_BADARG,
                "anchor_head_loss: bad size (B %d, H %d, W %d, A_loc %d <= %d, classes %d <= %d)", B, H, W, A_loc, AH_MAX_SLOTS, num_class,
                AH_MAX_CLASSES);
    PDM_REQUIRE(maps && bf16 && strides && anchor_rot && code_weights && out, PDM_E_BADARG, "anchor_head_loss: null pointer");
    PDM_REQUIRE(!maps[2] || (num_dir_bins >= 1 && num_dir_bins <= AH_MAX_BINS), PDM_E_BADARG, "anchor_head_loss: 1 .. %d direction bins",
                AH_MAX_BINS);
    PDM_REQUIRE(gamma > 0.0f && beta >= 0.0f, PDM_E_BADARG, "anchor_head_loss: gamma must be positive and beta non-negative");
    AlArgs a{};
    a.B = B; a.H = H; a.W = W; a.A_loc = A_loc; a.C = num_class; a.NB = maps[2] ? num_dir_bins : 0;
    a.cls = map_ref(maps[0], bf16[0], strides);
    a.box = map_ref(maps[1], bf16[1], strides + 4);
    a.dir = map_ref(maps[2], bf16[2], strides + 8);
    a.labels = labels; a.targets = targets; a.num_pos = num_pos;
    for (int s = 0; s < A_loc; ++s) a.rot[s] = anchor_rot[s];
    for (int k = 0; k < 7; ++k) a.cw[k] = code_weights[k];
    a.cls_weight = cls_weight; a.loc_weight = loc_weight; a.dir_weight = maps[2] ? dir_weight : 0.0f; a.dir_offset = dir_offset;
    a.beta = beta; a.alpha = alpha; a.gamma = gamma;
    a.partials = static_cast<double *>(workspace); a.out = out; a.g_cls = grad_cls; a.g_box = grad_box; a.g_dir = grad_dir;
    if (B > 0) {
        PDM_REQUIRE(maps[0] && maps[1] && labels && targets && num_pos && grad_cls && grad_box && (!maps[2] || grad_dir), PDM_E_BADARG,
                    "anchor_head_loss: null pointer");
        PDM_REQUIRE(workspace && workspace_bytes >= pdm_anchor_head_loss_workspace_bytes(B, H, W), PDM_E_BADARG,
                    "anchor_head_loss: workspace too small (%zu bytes, need %zu)", workspace_bytes, pdm_anchor_head_loss_workspace_bytes(B, H, W));
        PDM_WS_ALIGNED("anchor_head_loss", workspace);
        const uintptr_t outs = reinterpret_cast<uintptr_t>(grad_cls) | reinterpret_cast<uintptr_t>(grad_box) | reinterpret_cast<uintptr_t>(grad_dir);
        const bool pair = W % 2 == 0 && ah_pair_ok(a.cls) && ah_pair_ok(a.box) && ah_pair_ok(a.dir) && outs % 8 == 0;
        const int blocks = ah_loss_blocks(H, W, pair ? 2 : 1);
        a.num_partials = B * blocks;
        const dim3 grid((unsigned)blocks, (unsigned)B);
        if (pair) hipLaunchKernelGGL(al_loss_kernel<2>, grid, dim3(AH_T), 0, as_stream(stream), a);
        else hipLaunchKernelGGL(al_loss_kernel<1>, grid, dim3(AH_T), 0, as_stream(stream), a);
        if (int rc = check_launch("anchor_head_loss(loss)")) return rc;
    }
    hipLaunchKernelGGL(al_finish_kernel, dim3(1), dim3(AH_T), 0, as_stream(stream), a);
    return check_launch("anchor_head_loss(finish)");
}

// maps: HOST array of 2 device pointers [box (A_loc 7), dir (A_loc num_dir_bins) | NULL]; bf16 / strides as above (2 and 2 x 4
// entries); anchors (H W A_loc, 7) fp32 on the device -> batch_box_preds (B, H W A_loc, 7) fp32, every element written.
extern "C" int pdm_anchor_decode(void *stream, int B, int H, int W, int A_loc, int num_dir_bins, const void *const *maps, const int *bf16,
                                 const long long *strides, const float *anchors, float dir_offset, float dir_limit_offset,
                                 float *batch_box_preds) {
    PDM_REQUIRE(B >= 0 && B <= 65535 && H >= 1 && W >= 1 && A_loc >= 1 && A_loc <= AH_MAX_SLOTS && (long long)H * W * A_loc * 7 <= 0x7fffffffll,
                PDM_E_BADARG, "anchor_decode: bad size (B %d, H %d, W %d, A_loc %d <= %d)", B, H, W, A_loc, AH_MAX_SLOTS);
    PDM_REQUIRE(maps && bf16 && strides, PDM_E_BADARG, "anchor_decode: null table");
    PDM_REQUIRE(!maps[1] || (num_dir_bins >= 1 && num_dir_bins <= AH_MAX_BINS), PDM_E_BADARG, "anchor_decode: 1 .. %d direction bins", AH_MAX_BINS);
    if (B == 0) return 0;
    PDM_REQUIRE(maps[0] && anchors && batch_box_preds, PDM_E_BADARG, "anchor_decode: null pointer");
    AdArgs a{};
    a.B = B; a.H = H; a.W = W; a.A_loc = A_loc; a.NB = maps[1] ? num_dir_bins : 0;
    a.box = map_ref(maps[0], bf16[0], strides);
    a.dir = map_ref(maps[1], bf16[1], strides + 4);
    a.anchors = anchors; a.dir_offset = dir_offset; a.dir_limit_offset = dir_limit_offset; a.out = batch_box_preds;
    a.vec4 = (reinterpret_cast<uintptr_t>(anchors) % 16 == 0 && reinterpret_cast<uintptr_t>(batch_box_preds) % 16 == 0 &&
              ((long long)H * W * A_loc * 7) % 4 == 0) ? 1 : 0;
    const bool pair = W % 2 == 0 && A_loc <= AD_PAIR_SLOTS && ah_pair_ok(a.box) && ah_pair_ok(a.dir);
    const int V = pair ? 2 : 1;
    const dim3 grid((unsigned)divup((long long)H * (W / V), AD_T), (unsigned)B);
    const size_t lds = sizeof(float) * (size_t)AD_T * V * A_loc * 7;
    if (pair) hipLaunchKernelGGL(ad_decode_kernel<2>, grid, dim3(AD_T), lds, as_stream(stream), a);
    else hipLaunchKernelGGL(ad_decode_kernel<1>, grid, dim3(AD_T), lds, as_stream(stream), a);
    return check_launch("anchor_decode");
}

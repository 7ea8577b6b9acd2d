// Batched detector post-processing (Detector3DTemplate.post_processing on the device): score threshold, top PRE_MAX
// candidates, rotated / axis-aligned NMS, first POST_MAX survivors, padded per-sample outputs and the recall counts of
// generate_recall_record, for every sample of a batch in five launches and without a host synchronisation.
//
// The work is split into S segments: one per sample (class-agnostic, S = B) or one per (sample, class) pair
// (MULTI_CLASSES_NMS, S = B * C, segment b * C + k).  Stages:
//   select    one workgroup per segment: candidate = score >= thresh (NaN never passes); the first min(PRE_MAX,
//             #candidates) in pdm_topk_sampling's order (score descending, then lower row) by the same radix select +
//             bitonic sort (rank_select.h); gathers their boxes, scores, labels and rows into the workspace.
//   mask      pdm_nms's suppression mask, batched: grid (column blocks, row blocks, S), blocks past the segment's
//             device-side count and blocks below the diagonal exit at once.  For thresh >= 0 a pair whose BEV bounding
//             circles are disjoint (inflated past inside_box's 1e-2 tolerance and the rounding of the corners) has
//             overlap 0, hence IoU 0, and is not evaluated; every other pair runs the same iou_bev / iou_normal as
//             pdm_nms (nms_mask_tile, nms.h), so each segment's keep list is bit-identical to pdm_nms on the same boxes.
//   scan      one wave per segment (the register `removed` walk of pdm_nms: nms_walk, nms.h), stops at POST_MAX keeps.
//   finalize  one workgroup per sample: the sample's class segments one after another (class 0's survivors, then
//             class 1's, ...) as padded rows / boxes / scores / labels and a count; with gt boxes, the 3-D IoU of every
//             kept box against every gt row (trailing all-zero rows trimmed) in the operation order of
//             iou3d_nms_utils._iou3d_from_overlap, and the recall counts [gt, rcnn_t0, ...] summed over the batch.
#include "nms.h"
#include "rank_select.h"

namespace pdm {

constexpr int PP_MAX_PRE = TK_MAXK;   // 16384 candidates per segment: 128 KB of LDS items, 256 mask words per row
constexpr int PP_MAX_C = 64;          // classes per sample in multi-class mode
constexpr int PP_MAX_G = 4096;        // gt rows per sample
constexpr int PP_MAX_T = 8;           // recall thresholds
constexpr int PP_FIN_THREADS = 256;

struct PPArgs {
    int B, C, S, multi, pre, post, postc, cb, P;
    long long rows;
    const float *cls;
    int cls_stride;
    const float *boxes;
    int box_stride;
    const int *offsets;
    const float *batch_index;
    float score_thresh, nms_thresh;
    int normal;
    // workspace
    unsigned long long *mask;
    float *sel_boxes, *sel_scores;
    int *sel_rows, *sel_labels, *seg_n, *keep, *seg_kept;
    // outputs
    long long *out_rows;
    float *out_boxes, *out_scores;
    long long *out_labels;
    int *out_count, *err;
    // recall
    const float *gt;
    int G, gt_dim, nt;
    float t[PP_MAX_T];
    unsigned long long *recall;
};

// the sample's rows [lo, hi), clamped so that a malformed offsets table cannot send a workgroup out of bounds
__device__ __forceinline__ void pp_rows_of(const PPArgs &a, int b, long long &lo, long long &hi) {
    lo = a.offsets[b];
    hi = a.offsets[b + 1];
    lo = lo < 0 ? 0 : lo > a.rows ? a.rows : lo;
    hi = hi < lo ? lo : hi > a.rows ? a.rows : hi;
}

// class-agnostic: torch.max over the classes (NaN propagates, the lowest class wins a tie), label = argmax + 1;
// multi-class: the segment's own column, label = k + 1
__device__ __forceinline__ float pp_score(const PPArgs &a, long long r, int k, int *label) {
    const float *row = a.cls + r * a.cls_stride;
    if (a.multi) {
        *label = k + 1;
        return row[k];
    }
    float best = row[0];
    int arg = 0;
    for (int c = 1; c < a.C; ++c) {
        const float v = row[c];
        if (best == best && (v != v || v > best)) { best = v; arg = c; }
    }
    *label = arg + 1;
    return best;
}

__device__ __forceinline__ unsigned pp_key(const PPArgs &a, long long r, int k) {
    int lab;
    const float v = pp_score(a, r, k, &lab);
    return v >= a.score_thresh ? topk_key(__float_as_uint(v)) : 0xffffffffu;   // a non-candidate ranks below them all
}

__global__ __launch_bounds__(TK_THREADS) void pp_select_kernel(PPArgs a) {
    extern __shared__ unsigned long long s_items[];
    __shared__ alignas(16) RankLds lds;
    __shared__ int s_cnt, s_bad;
    const int s = blockIdx.x, tid = threadIdx.x;
    const int b = a.multi ? s / a.C : s, k = a.multi ? s % a.C : 0;
    long long lo, hi;
    pp_rows_of(a, b, lo, hi);
    const int n = (int)(hi - lo);
    if (tid == 0) { s_cnt = 0; s_bad = 0; }
    __syncthreads();
    int cnt = 0;
    bool bad = false;
    for (int i = tid; i < n; i += TK_THREADS) {
        cnt += pp_key(a, lo + i, k) != 0xffffffffu;
        if (a.batch_index && a.batch_index[lo + i] != (float)b) bad = true;
    }
    // sample-major check: every row lies in exactly one sample's range and carries that sample's index
    if (a.batch_index && s == 0 && tid == 0 && (a.offsets[0] != 0 || (long long)a.offsets[a.B] != a.rows)) bad = true;
    if (cnt) atomicAdd(&s_cnt, cnt);
    if (bad) s_bad = 1;
    __syncthreads();
    if (tid == 0 && s_bad) atomicOr(a.err, 1);
    const int K = min(s_cnt, a.pre);
    if (tid == 0) a.seg_n[s] = K;
    if (K == 0) return;

    // K <= #candidates, so every selected key is a candidate's
    rank_select(n, K, [&](int i) { return pp_key(a, lo + i, k); }, s_items, lds);
    const size_t base = (size_t)s * a.pre;
    for (int r = tid; r < K; r += TK_THREADS) {
        const long long row = lo + (long long)(unsigned)(s_items[r] & 0xffffffffull);
        int lab;
        const float v = pp_score(a, row, k, &lab);
        a.sel_rows[base + r] = (int)row;
        a.sel_scores[base + r] = v;
        a.sel_labels[base + r] = lab;
        const float *bx = a.boxes + row * a.box_stride;
        float *o = a.sel_boxes + (base + r) * 7;
#pragma unroll
        for (int f = 0; f < 7; ++f) o[f] = bx[f];
    }
}

__global__ __launch_bounds__(64) void pp_mask_kernel(PPArgs a) {
    const int s = blockIdx.z, row_start = blockIdx.y, col_start = blockIdx.x;
    const int n = a.seg_n[s];
    if (col_start < row_start || col_start * 64 >= n) return;   // never read by the scan
    const unsigned long long t = nms_mask_tile(n, a.sel_boxes + (size_t)s * a.pre * 7, row_start, col_start, a.nms_thresh,
                                               a.normal != 0, a.nms_thresh >= 0.f);
    const int cur = row_start * 64 + threadIdx.x;
    if (cur < n) a.mask[((size_t)s * a.pre + cur) * a.cb + col_start] = t;
}

// one wave per segment: nms.h's walk, stops at POST_MAX keeps
__global__ __launch_bounds__(64) void pp_scan_kernel(PPArgs a) {
    const int s = blockIdx.x;
    int *keep = a.keep + (size_t)s * a.postc;
    const int kept = nms_walk(a.seg_n[s], a.post, a.mask + (size_t)s * a.pre * a.cb, a.cb, [&](int k, int i) { keep[k] = i; });
    if (threadIdx.x == 0) a.seg_kept[s] = kept;
}

// iou3d_nms_utils._iou3d_from_overlap for one (box, gt) pair, operation for operation (-ffp-contract=off); torch.min /
// torch.max / clamp propagate NaN, so do these
__device__ __forceinline__ float pp_nan_min(float x, float y) { return (x != x || y != y) ? x + y : (x < y ? x : y); }
__device__ __forceinline__ float pp_nan_max(float x, float y) { return (x != x || y != y) ? x + y : (x > y ? x : y); }

__device__ __forceinline__ float pp_iou3d(const float *a, const float *g) {
    const float ov = box_overlap_bev(a, g);
    const float a_max = a[2] + a[5] / 2, a_min = a[2] - a[5] / 2;
    const float b_max = g[2] + g[5] / 2, b_min = g[2] - g[5] / 2;
    float h = pp_nan_min(a_max, b_max) - pp_nan_max(a_min, b_min);
    h = h < 0.f ? 0.f : h;
    const float o3 = ov * h;
    const float vol_a = a[3] * a[4] * a[5], vol_b = g[3] * g[4] * g[5];
    float den = vol_a + vol_b - o3;
    den = den < 1e-6f ? 1e-6f : den;
    return o3 / den;
}

__global__ __launch_bounds__(PP_FIN_THREADS) void pp_finalize_kernel(PPArgs a) {
    __shared__ int s_off[PP_MAX_C + 1];
    __shared__ int s_g;
    __shared__ unsigned s_hit[PP_MAX_G];   // bit t: some kept box has IoU > t[t]; bit 31: some IoU is NaN
    __shared__ int s_cnt[PP_MAX_T];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int segs = a.multi ? a.C : 1, s0 = b * segs;
    long long lo, hi;
    pp_rows_of(a, b, lo, hi);
    if (tid == 0) {
        int acc = 0;
        for (int j = 0; j < segs; ++j) { s_off[j] = acc; acc += a.seg_kept[s0 + j]; }
        s_off[segs] = acc;
    }
    __syncthreads();
    const int total = s_off[segs];
    for (int p = tid; p < a.P; p += PP_FIN_THREADS) {
        const size_t o = (size_t)b * a.P + p;
        if (p < total) {
            int j = 0;
            while (p >= s_off[j + 1]) ++j;
            const size_t src = (size_t)(s0 + j) * a.pre + a.keep[(size_t)(s0 + j) * a.postc + (p - s_off[j])];
            a.out_rows[o] = (long long)a.sel_rows[src] - lo;
            a.out_scores[o] = a.sel_scores[src];
            a.out_labels[o] = a.sel_labels[src];
#pragma unroll
            for (int f = 0; f < 7; ++f) a.out_boxes[o * 7 + f] = a.sel_boxes[src * 7 + f];
        } else {
            a.out_rows[o] = -1;
            a.out_scores[o] = 0.f;
            a.out_labels[o] = 0;
#pragma unroll
            for (int f = 0; f < 7; ++f) a.out_boxes[o * 7 + f] = 0.f;
        }
    }
    if (tid == 0) a.out_count[b] = total;
    if (!a.gt) return;

    // recall: trailing gt rows whose sum is 0 do not count (generate_recall_record)
    const float *gt = a.gt + (size_t)b * a.G * a.gt_dim;
    if (tid == 0) {
        int g = a.G - 1;
        for (; g >= 0; --g) {
            float sum = 0.f;
            for (int f = 0; f < a.gt_dim; ++f) sum += gt[(size_t)g * a.gt_dim + f];
            if (sum != 0.f) break;
        }
        s_g = g + 1;
    }
    for (int g = tid; g < PP_MAX_G; g += PP_FIN_THREADS) s_hit[g] = 0u;
    if (tid < PP_MAX_T) s_cnt[tid] = 0;
    __syncthreads();
    const int ng = s_g;
    // every (kept box, gt) pair: max over boxes > t  <=>  some IoU > t and none is NaN (torch.max propagates NaN)
    for (int e = tid; e < ng * total; e += PP_FIN_THREADS) {
        const int g = e % ng, p = e / ng;
        int j = 0;
        while (p >= s_off[j + 1]) ++j;
        const size_t src = (size_t)(s0 + j) * a.pre + a.keep[(size_t)(s0 + j) * a.postc + (p - s_off[j])];
        float bx[7], gb[7];
#pragma unroll
        for (int f = 0; f < 7; ++f) { bx[f] = a.sel_boxes[src * 7 + f]; gb[f] = gt[(size_t)g * a.gt_dim + f]; }
        const float v = pp_iou3d(bx, gb);
        unsigned bits = v != v ? 0x80000000u : 0u;
#pragma unroll
        for (int t = 0; t < PP_MAX_T; ++t) bits |= (t < a.nt && v > a.t[t]) ? 1u << t : 0u;
        if (bits) atomicOr(&s_hit[g], bits);
    }
    __syncthreads();
    if (total > 0) {
        for (int g = tid; g < ng; g += PP_FIN_THREADS) {
            const unsigned h = s_hit[g];
            if (h & 0x80000000u) continue;
            for (int t = 0; t < PP_MAX_T; ++t)
                if (h & (1u << t)) atomicAdd(&s_cnt[t], 1);
        }
    }
    __syncthreads();
    if (tid == 0 && ng > 0) atomicAdd(&a.recall[0], (unsigned long long)ng);
    if (tid < a.nt && s_cnt[tid] > 0) atomicAdd(&a.recall[1 + tid], (unsigned long long)s_cnt[tid]);
}

struct PPLayout {
    size_t mask, sel_boxes, sel_scores, sel_rows, sel_labels, seg_n, keep, seg_kept, total;
};

static PPLayout pp_layout(int S, int pre, int post) {
    const size_t s = (size_t)S, p = (size_t)pre, cb = (size_t)((pre + 63) / 64), postc = (size_t)(post < pre ? post : pre);
    PPLayout l;
    size_t off = 0;
    l.mask = off;       off += align256(s * p * cb * sizeof(unsigned long long));
    l.sel_boxes = off;  off += align256(s * p * 7 * sizeof(float));
    l.sel_scores = off; off += align256(s * p * sizeof(float));
    l.sel_rows = off;   off += align256(s * p * sizeof(int));
    l.sel_labels = off; off += align256(s * p * sizeof(int));
    l.seg_n = off;      off += align256(s * sizeof(int));
    l.keep = off;       off += align256(s * postc * sizeof(int));
    l.seg_kept = off;   off += align256(s * sizeof(int));
    l.total = off;
    return l;
}

// the error flag and the recall counts start at 0 on every call: two unrelated buffers in one launch, by a kernel for the
// reason told at pdm::zero_fill (api.hip)
__global__ __launch_bounds__(64) void pp_zero_kernel(int *__restrict__ err, unsigned long long *__restrict__ recall, int nr) {
    if (threadIdx.x == 0) *err = 0;
    if (recall && (int)threadIdx.x < nr) recall[threadIdx.x] = 0ull;
}

}  // namespace pdm

using namespace pdm;

extern "C" size_t pdm_post_process_workspace_bytes(int num_segments, int pre_max, int post_max) {
    if (num_segments <= 0 || pre_max <= 0 || post_max <= 0) return 0;
    return pp_layout(num_segments, pre_max, post_max).total;
}

extern "C" int pdm_post_process(void *stream, int B, int C, int multi_class, long long rows, const float *cls, int cls_stride,
                                const float *boxes, int box_stride, const int *offsets, const float *batch_index,
                                float score_thresh, int pre_max, int post_max, float nms_thresh, int nms_normal, int G,
                                int gt_dim, const float *gt, int num_thresh, const float *recall_thresh, void *workspace,
                                size_t workspace_bytes, long long *out_rows, float *out_boxes, float *out_scores,
                                long long *out_labels, int *out_count, int *err_flag, long long *recall) {
    PDM_REQUIRE(B >= 0 && C >= 1 && rows >= 0 && rows <= 0x7fffffffLL, PDM_E_BADARG, "post_process: B=%d C=%d rows=%lld", B, C, rows);
    PDM_REQUIRE(multi_class == 0 || multi_class == 1, PDM_E_BADARG, "post_process: multi_class=%d", multi_class);
    PDM_REQUIRE(!multi_class || C <= PP_MAX_C, PDM_E_TOOLARGE, "post_process: %d classes (multi-class mode: at most %d)", C, PP_MAX_C);
    PDM_REQUIRE(pre_max >= 1 && pre_max <= PP_MAX_PRE, PDM_E_TOOLARGE, "post_process: pre_max=%d (1 .. %d)", pre_max, PP_MAX_PRE);
    PDM_REQUIRE(post_max >= 1, PDM_E_BADARG, "post_process: post_max=%d", post_max);
    const long long S = (long long)B * (multi_class ? C : 1);
    PDM_REQUIRE(S <= 65535, PDM_E_TOOLARGE, "post_process: %lld segments (at most 65535)", S);
    const long long P = (long long)post_max * (multi_class ? C : 1);
    PDM_REQUIRE(P <= 0x7fffffffLL, PDM_E_TOOLARGE, "post_process: %lld output rows per sample", P);
    PDM_REQUIRE(cls_stride >= C && box_stride >= 7, PDM_E_BADARG, "post_process: cls_stride=%d (C=%d) box_stride=%d", cls_stride, C, box_stride);
    PDM_REQUIRE(G >= 0 && G <= PP_MAX_G, PDM_E_TOOLARGE, "post_process: %d gt rows (0 .. %d)", G, PP_MAX_G);
    PDM_REQUIRE(num_thresh >= 0 && num_thresh <= PP_MAX_T, PDM_E_BADARG, "post_process: %d recall thresholds (0 .. %d)", num_thresh, PP_MAX_T);
    PDM_REQUIRE(!gt || (gt_dim >= 7 && recall), PDM_E_BADARG, "post_process: gt needs gt_dim >= 7 (%d) and a recall buffer", gt_dim);
    PDM_REQUIRE(num_thresh == 0 || recall_thresh, PDM_E_BADARG, "post_process: null recall thresholds");
    PDM_REQUIRE(err_flag && offsets && out_rows && out_boxes && out_scores && out_labels && out_count, PDM_E_BADARG,
                "post_process: null pointer");
    PDM_REQUIRE(rows == 0 || (cls && boxes), PDM_E_BADARG, "post_process: null cls or boxes");
    const size_t need = pdm_post_process_workspace_bytes((int)S, pre_max, post_max);
    PDM_REQUIRE(S == 0 || (workspace && workspace_bytes >= need), PDM_E_BADARG,
                "post_process: workspace of %zu bytes, need %zu", workspace ? workspace_bytes : (size_t)0, need);
    PDM_WS_ALIGNED("post_process", workspace);
    hipLaunchKernelGGL(pp_zero_kernel, dim3(1), dim3(64), 0, as_stream(stream), err_flag,
                       reinterpret_cast<unsigned long long *>(recall), 1 + num_thresh);
    int rc = check_launch("post_process(zero)");
    if (rc || B == 0) return rc;

    const PPLayout l = pp_layout((int)S, pre_max, post_max);
    char *ws = static_cast<char *>(workspace);
    PPArgs a = {};
    a.B = B; a.C = C; a.S = (int)S; a.multi = multi_class; a.pre = pre_max; a.post = post_max;
    a.postc = post_max < pre_max ? post_max : pre_max; a.cb = (pre_max + 63) / 64; a.P = (int)P;
    a.rows = rows; a.cls = cls; a.cls_stride = cls_stride; a.boxes = boxes; a.box_stride = box_stride;
    a.offsets = offsets; a.batch_index = batch_index; a.score_thresh = score_thresh; a.nms_thresh = nms_thresh;
    a.normal = nms_normal ? 1 : 0;
    a.mask = reinterpret_cast<unsigned long long *>(ws + l.mask);
    a.sel_boxes = reinterpret_cast<float *>(ws + l.sel_boxes);
    a.sel_scores = reinterpret_cast<float *>(ws + l.sel_scores);
    a.sel_rows = reinterpret_cast<int *>(ws + l.sel_rows);
    a.sel_labels = reinterpret_cast<int *>(ws + l.sel_labels);
    a.seg_n = reinterpret_cast<int *>(ws + l.seg_n);
    a.keep = reinterpret_cast<int *>(ws + l.keep);
    a.seg_kept = reinterpret_cast<int *>(ws + l.seg_kept);
    a.out_rows = out_rows; a.out_boxes = out_boxes; a.out_scores = out_scores; a.out_labels = out_labels;
    a.out_count = out_count; a.err = err_flag;
    a.gt = G > 0 ? gt : nullptr; a.G = G; a.gt_dim = gt_dim; a.nt = num_thresh;
    for (int t = 0; t < num_thresh; ++t) a.t[t] = recall_thresh[t];
    a.recall = reinterpret_cast<unsigned long long *>(recall);

    int k2 = 2;
    while (k2 < pre_max) k2 <<= 1;
    const size_t lds = (size_t)k2 * sizeof(unsigned long long);
    if (lds > 64 * 1024) {   // granted per device (static LDS comes on top: 156 KB, as topk_sampling)
        const int e = grant_lds(reinterpret_cast<const void *>(&pp_select_kernel), 156 * 1024);
        PDM_REQUIRE(e == 0, PDM_E_TOOLARGE, "post_process: cannot obtain %zu bytes of LDS: %s", lds, hipGetErrorString((hipError_t)e));
    }
    hipLaunchKernelGGL(pp_select_kernel, dim3((unsigned)S), dim3(TK_THREADS), lds, as_stream(stream), a);
    rc = check_launch("post_process(select)");
    if (rc) return rc;
    hipLaunchKernelGGL(pp_mask_kernel, dim3(a.cb, a.cb, (unsigned)S), dim3(64), 0, as_stream(stream), a);
    rc = check_launch("post_process(mask)");
    if (rc) return rc;
    hipLaunchKernelGGL(pp_scan_kernel, dim3((unsigned)S), dim3(64), 0, as_stream(stream), a);
    rc = check_launch("post_process(scan)");
    if (rc) return rc;
    hipLaunchKernelGGL(pp_finalize_kernel, dim3(B), dim3(PP_FIN_THREADS), 0, as_stream(stream), a);
    return check_launch("post_process(finalize)");
}

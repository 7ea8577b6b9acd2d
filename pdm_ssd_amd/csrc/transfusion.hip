// TransFusionHead's query initialisation and box decode on the device (the reference's
// pcdet/models/dense_heads/transfusion_head.py:160-203 and :397-479), each one launch chain for the whole batch with no
// host read and no atomics on results.
//
// pdm_tf_proposals   mask (one thread per cell of every class: s = sigmoid(logit) survives if no cell of its k x k window
//                    has a greater s and the window lies inside the map; an exempt class survives everywhere; others
//                    score 0) -> local (one workgroup per slice of TF_SLICE flat (class, y, x) indices of a sample:
//                    rank_select (rank_select.h) of the slice's min(P, length) best, ties by lower index, re-sorted by
//                    index and written as candidates, so that the candidate list of a sample is in flat-index order) ->
//                    select (one workgroup per sample: rank_select of the P best candidates, ties by lower position = lower
//                    flat index; then index, class, position and the masked score of every class at the cell).  A member
//                    of the sample's best P is among its slice's best P under the same tie rule, so the two stages pick
//                    what one rank select over all C * H * W scores picks (the reference sorts them all).
// pdm_tf_decode      one workgroup per sample: a query's score, centre, sizes and angle (rot = [sin, cos]); the survivors
//                    of the score threshold (strict) and the centre range (inclusive) compacted in query order by a
//                    block scan, padding rows zeroed
#include "loss_kit.h"
#include "rank_select.h"
#include "tf_decode.h"

namespace pdm {

constexpr int TF_T = 256;
constexpr int TF_MAX_CLASSES = 32;
constexpr int TF_SLICE = 4096;       // flat indices per workgroup of the local stage (at least P)

struct TfpArgs {
    int B, C, H, W, pad, P, ysize;
    unsigned exempt;                 // bit c: class c survives everywhere
    const float *logits;             // (B, C, H, W)
    float *masked;                   // (B, C, H, W)
    int slice, nslice;               // flat indices per slice, slices per sample
    unsigned *cand_key;              // (B, nslice * P): topk_key of a candidate, 0xffffffff = padding
    int *cand_idx;                   // (B, nslice * P): its flat index
    long long *index, *cls;          // (B, P)
    float *qhs, *pos;                // (B, C, P), (B, P, 2)
};

__global__ __launch_bounds__(TF_T) void tf_mask_kernel(TfpArgs a) {
    const long long hw = (long long)a.H * a.W, total = (long long)a.B * a.C * hw;
    const long long i = (long long)blockIdx.x * TF_T + threadIdx.x;
    if (i >= total) return;
    const int cell = (int)(i % hw), y = cell / a.W, x = cell - y * a.W, c = (int)((i / hw) % a.C);
    const float s = sigmoid_rn(a.logits[i]);
    bool keep = true;
    if (!((a.exempt >> c) & 1u)) {
        keep = y >= a.pad && y < a.H - a.pad && x >= a.pad && x < a.W - a.pad;
        if (keep) {
            const float *plane = a.logits + (i - cell);
            for (int dy = -a.pad; dy <= a.pad; ++dy)
                for (int dx = -a.pad; dx <= a.pad; ++dx)
                    keep = keep && !(sigmoid_rn(plane[(y + dy) * a.W + x + dx]) > s);
        }
    }
    a.masked[i] = keep ? s : 0.0f;
}

__global__ __launch_bounds__(TK_THREADS) void tf_local_kernel(TfpArgs a) {
    extern __shared__ unsigned long long s_items[];
    __shared__ alignas(16) RankLds lds;
    const int b = blockIdx.y, sl = blockIdx.x, tid = threadIdx.x, n = a.C * a.H * a.W, P = a.P;
    const int lo = sl * a.slice, len = min(n, lo + a.slice) - lo, K = min(P, len);      // len >= 1 by the grid
    const float *masked = a.masked + (size_t)b * n + lo;
    rank_select(len, K, [&](int i) { return topk_key(__float_as_uint(masked[i])); }, s_items, lds);
    __syncthreads();
    const int K2 = 1 << (32 - __builtin_clz(max(K, 2) - 1));
    for (int r = tid; r < K; r += TK_THREADS) {                      // (key, index) -> (index, key); the padding stays last
        const unsigned long long it = s_items[r];
        s_items[r] = (it << 32) | (it >> 32);
    }
    __syncthreads();
    bitonic_sort_items(s_items, K2);
    const size_t base = ((size_t)b * a.nslice + sl) * P;
    for (int r = tid; r < P; r += TK_THREADS) {
        const unsigned long long it = r < K ? s_items[r] : 0ull;
        a.cand_key[base + r] = r < K ? (unsigned)(it & 0xffffffffull) : 0xffffffffu;
        a.cand_idx[base + r] = r < K ? lo + (int)(unsigned)(it >> 32) : 0;
    }
}

__global__ __launch_bounds__(TK_THREADS) void tf_select_kernel(TfpArgs a) {
    extern __shared__ unsigned long long s_items[];
    __shared__ alignas(16) RankLds lds;
    const int b = blockIdx.x, tid = threadIdx.x, hw = a.H * a.W, n = a.C * hw, P = a.P, n2 = a.nslice * P;
    const float *masked = a.masked + (size_t)b * n;
    const unsigned *ckey = a.cand_key + (size_t)b * n2;
    const int *cidx = a.cand_idx + (size_t)b * n2;
    // a score is never negative, so a real candidate's key is below the padding's: the P best are real (n >= P)
    rank_select(n2, P, [&](int j) { return ckey[j]; }, s_items, lds);
    __syncthreads();
    for (int r = tid; r < P; r += TK_THREADS) {
        const int i = cidx[(int)(unsigned)(s_items[r] & 0xffffffffull)], c = i / hw, cell = i - c * hw;
        const size_t slot = (size_t)b * P + r;
        a.index[slot] = cell;
        a.cls[slot] = c;
        // the reference's position table runs over (x_size, y_size) in `ij` order and is then flipped
        a.pos[2 * slot] = (float)(cell % a.ysize) + 0.5f;
        a.pos[2 * slot + 1] = (float)(cell / a.ysize) + 0.5f;
    }
    for (int e = tid; e < a.C * P; e += TK_THREADS) {
        const int c = e / P, r = e - c * P;
        const int cell = cidx[(int)(unsigned)(s_items[r] & 0xffffffffull)] % hw;
        a.qhs[(size_t)b * a.C * P + e] = masked[(size_t)c * hw + cell];
    }
}

struct TfdArgs {
    int B, C, P, E;
    const float *heatmap, *center, *height, *dim, *rot, *vel, *qhs;   // (B, c, P) each
    const long long *cls;            // (B, P)
    float score_thresh, lo[3], hi[3];
    float x0, y0, vx, vy, stride;
    float *boxes, *scores;           // (B, P, 7 + E), (B, P)
    long long *labels;               // (B, P)
    int *count;                      // (B)
};

__global__ __launch_bounds__(TF_T) void tf_decode_kernel(TfdArgs a) {
    __shared__ int s_wave[TF_T / 64];
    const int b = blockIdx.x, tid = threadIdx.x, P = a.P, D = 7 + a.E;
    float *boxes = a.boxes + (size_t)b * P * D, *scores = a.scores + (size_t)b * P;
    long long *labels = a.labels + (size_t)b * P;
    int kept = 0;
    for (int p0 = 0; p0 < P; p0 += TF_T) {
        const int p = p0 + tid;
        bool keep = false;
        float box[9], score = 0.0f;
        long long c = 0;
        if (p < P) {
            c = a.cls[(size_t)b * P + p];
            c = c < 0 ? 0 : c >= a.C ? a.C - 1 : c;
            const size_t at = ((size_t)b * a.C + c) * P + p;
            score = __fmul_rn(sigmoid_rn(a.heatmap[at]), a.qhs[at]);
            tf_decode_box(TfBoxMaps{P, a.E, a.center, a.height, a.dim, a.rot, a.vel, a.x0, a.y0, a.vx, a.vy, a.stride}, b, p, box);
            keep = score > a.score_thresh;
#pragma unroll
            for (int d = 0; d < 3; ++d) keep = keep && box[d] >= a.lo[d] && box[d] <= a.hi[d];
        }
        int tot;
        const int pos = kept + block_scan<TF_T>(keep ? 1 : 0, s_wave, &tot);
        kept += tot;
        if (keep) {                                                  // pos <= p: a row is never written before its turn
            for (int d = 0; d < D; ++d) boxes[(size_t)pos * D + d] = box[d];
            scores[pos] = score;
            labels[pos] = c + 1;
        }
    }
    for (int r = kept + tid; r < P; r += TF_T) {
        for (int d = 0; d < D; ++d) boxes[(size_t)r * D + d] = 0.0f;
        scores[r] = 0.0f;
        labels[r] = 0;
    }
    if (tid == 0) a.count[b] = kept;
}

}  // namespace pdm

using namespace pdm;

static int tf_slice(int P) { return P > TF_SLICE ? P : TF_SLICE; }

// the masked scores (B, C, H, W), then the candidates' keys and flat indices (B, slices * P each); 0 for a bad shape
extern "C" size_t pdm_tf_proposals_workspace_bytes(int B, int C, int H, int W, int P) {
    if (B <= 0 || C < 1 || H < 1 || W < 1 || P < 1 || (long long)C * H * W > 0x7fffffffll) return 0;
    const size_t n = (size_t)C * H * W, cand = (size_t)B * divup((long long)n, tf_slice(P)) * P;
    return align256(sizeof(float) * B * n) + align256(sizeof(unsigned) * cand) + sizeof(int) * cand;
}

// exempt: HOST array of num_exempt classes that survive everywhere.  workspace >= pdm_tf_proposals_workspace_bytes(...), 8-byte aligned.
extern "C" int pdm_tf_proposals(void *stream, int B, int C, int H, int W, const float *logits, int nms_kernel, int num_exempt,
                                const int *exempt, int P, int y_size, long long *index, long long *cls,
                                float *query_heatmap_score, float *query_pos, void *workspace, size_t workspace_bytes) {
    PDM_REQUIRE(B >= 0 && C >= 1 && C <= TF_MAX_CLASSES && H >= 1 && W >= 1 && (long long)C * H * W <= 0x7fffffffll &&
                (long long)B * C * H * W <= 0x7fffffffll, PDM_E_BADARG, "tf_proposals: bad size");
    PDM_REQUIRE(nms_kernel >= 1 && (nms_kernel & 1) == 1, PDM_E_BADARG, "tf_proposals: NMS_KERNEL_SIZE = %d must be odd", nms_kernel);
    PDM_REQUIRE(P >= 1 && (long long)P <= (long long)C * H * W, PDM_E_BADARG, "tf_proposals: P = %d out of range (1 .. C * H * W)", P);
    PDM_REQUIRE(P <= TK_MAXK, PDM_E_TOOLARGE, "tf_proposals: P = %d > %d", P, TK_MAXK);
    PDM_REQUIRE(y_size >= 1 && num_exempt >= 0 && (num_exempt == 0 || exempt), PDM_E_BADARG, "tf_proposals: bad table");
    if (B == 0) return 0;
    PDM_REQUIRE(logits && index && cls && query_heatmap_score && query_pos && workspace, PDM_E_BADARG, "tf_proposals: null pointer");
    const size_t need = pdm_tf_proposals_workspace_bytes(B, C, H, W, P);
    PDM_REQUIRE(workspace_bytes >= need && (reinterpret_cast<uintptr_t>(workspace) & 7) == 0, PDM_E_BADARG,
                "tf_proposals: workspace of %zu bytes, need %zu (8-byte aligned)", workspace_bytes, need);
    TfpArgs a{};
    a.B = B; a.C = C; a.H = H; a.W = W; a.pad = nms_kernel / 2; a.P = P; a.ysize = y_size;
    for (int e = 0; e < num_exempt; ++e) {
        PDM_REQUIRE(exempt[e] >= 0 && exempt[e] < C, PDM_E_BADARG, "tf_proposals: exempt class %d of %d classes", exempt[e], C);
        a.exempt |= 1u << exempt[e];
    }
    const size_t n = (size_t)C * H * W;
    a.slice = tf_slice(P); a.nslice = divup((long long)n, a.slice);
    PDM_REQUIRE(a.nslice <= 65535 && B <= 65535 && (long long)a.nslice * P <= 0x7fffffffll, PDM_E_TOOLARGE, "tf_proposals: %d slices", a.nslice);
    const size_t cand = (size_t)B * a.nslice * P;
    char *ws = static_cast<char *>(workspace);
    a.masked = reinterpret_cast<float *>(ws);
    a.cand_key = reinterpret_cast<unsigned *>(ws + align256(sizeof(float) * B * n));
    a.cand_idx = reinterpret_cast<int *>(ws + align256(sizeof(float) * B * n) + align256(sizeof(unsigned) * cand));
    a.logits = logits; a.index = index; a.cls = cls; a.qhs = query_heatmap_score; a.pos = query_pos;
    hipLaunchKernelGGL(tf_mask_kernel, dim3((unsigned)divup((long long)B * C * H * W, TF_T)), dim3(TF_T), 0, as_stream(stream), a);
    if (int rc = check_launch("tf_proposals(mask)")) return rc;
    const int k2 = 1 << (32 - __builtin_clz((P > 2 ? P : 2) - 1));
    const size_t lds = (size_t)k2 * sizeof(unsigned long long);
    if (lds > 48 * 1024) {
        int e = grant_lds(reinterpret_cast<const void *>(&tf_local_kernel), 156 * 1024);
        if (e == 0) e = grant_lds(reinterpret_cast<const void *>(&tf_select_kernel), 156 * 1024);
        PDM_REQUIRE(e == 0, PDM_E_TOOLARGE, "tf_proposals: cannot obtain %zu bytes of LDS: %s", lds, hipGetErrorString((hipError_t)e));
    }
    hipLaunchKernelGGL(tf_local_kernel, dim3((unsigned)a.nslice, (unsigned)B), dim3(TK_THREADS), lds, as_stream(stream), a);
    if (int rc = check_launch("tf_proposals(local)")) return rc;
    hipLaunchKernelGGL(tf_select_kernel, dim3((unsigned)B), dim3(TK_THREADS), lds, as_stream(stream), a);
    return check_launch("tf_proposals(select)");
}

// limit_range: HOST array [x0 y0 z0 x1 y1 z1]; vel may be NULL (boxes then have 7 columns)
extern "C" int pdm_tf_decode(void *stream, int B, int C, int P, const float *heatmap, const float *center, const float *height,
                             const float *dim, const float *rot, const float *vel, const long long *cls,
                             const float *query_heatmap_score, float score_thresh, const float *limit_range, float x0, float y0,
                             float vx, float vy, float stride, float *boxes, float *scores, long long *labels, int *count) {
    PDM_REQUIRE(B >= 0 && C >= 1 && P >= 1 && (long long)B * C * P <= 0x7fffffffll, PDM_E_BADARG, "tf_decode: bad size");
    PDM_REQUIRE(score_thresh >= 0.0f, PDM_E_BADARG, "tf_decode: SCORE_THRESH = %g is negative", (double)score_thresh);
    PDM_REQUIRE(limit_range, PDM_E_BADARG, "tf_decode: null table");
    if (B == 0) return 0;
    PDM_REQUIRE(heatmap && center && height && dim && rot && cls && query_heatmap_score && boxes && scores && labels && count,
                PDM_E_BADARG, "tf_decode: null pointer");
    TfdArgs a{};
    a.B = B; a.C = C; a.P = P; a.E = vel ? 2 : 0;
    a.heatmap = heatmap; a.center = center; a.height = height; a.dim = dim; a.rot = rot; a.vel = vel; a.qhs = query_heatmap_score;
    a.cls = cls; a.score_thresh = score_thresh;
    for (int d = 0; d < 3; ++d) { a.lo[d] = limit_range[d]; a.hi[d] = limit_range[3 + d]; }
    a.x0 = x0; a.y0 = y0; a.vx = vx; a.vy = vy; a.stride = stride;
    a.boxes = boxes; a.scores = scores; a.labels = labels; a.count = count;
    hipLaunchKernelGGL(tf_decode_kernel, dim3((unsigned)B), dim3(TF_T), 0, as_stream(stream), a);
    return check_launch("tf_decode");
}

// RoI point pooling and RoI-aware pooling: the operators of the reference's roipoint_pool3d_cuda and roiaware_pool3d_cuda
// extensions (pcdet/ops/roipoint_pool3d/src/roipoint_pool3d_kernel.cu, pcdet/ops/roiaware_pool3d/src/roiaware_pool3d_kernel.cu)
// that turn a one-stage point detector into a two-stage one.  Same values as the reference, other mechanism:
//   - the reference allocates a (B, N, M) / (K, P) int matrix on every call and has ONE THREAD per box walk its N entries;
//     here a workgroup per box tests the points 256 at a time and compacts the hits in index order with a 64-bit ballot
//     and a prefix popcount.  Nothing of size points x boxes exists, nothing is allocated, no global atomic is used.
//   - RoI-aware backward is a gather (a wave per point walks the boxes in order), so it is deterministic where the
//     reference's atomicAdd is not, and it writes every element of grad_in.
// The in-box test and the voxel of a point are box_geometry.h's point_in_box3d_cs / roiaware_voxel, the test the same
// function points_in_boxes (iou3d_nms.hip) evaluates.  Built with -ffp-contract=off: one rounding per operation.
#include "box_geometry.h"
#include "roiaware.h"

namespace pdm {

constexpr int RP_NT = 256;       // threads per workgroup, one workgroup per (sample, box)
constexpr int RP_LIST = 2048;    // hit indices held in LDS between the search and the row copies

// out[e] = val(e / W, e % W) for e in [e0, e1) by the whole workgroup: a scalar head up to a 16-byte boundary of the
// ADDRESS, float4 stores, a scalar tail (rows of 3 + C floats are 16-byte aligned only when 3 + C is a multiple of 4;
// a box's block of S rows is written as one flat range, so wide stores apply whatever the row length)
template <class F>
__device__ __forceinline__ void emit_flat(float *out, unsigned e0, unsigned e1, unsigned W, F val) {
    const unsigned tid = threadIdx.x;
    unsigned head = (unsigned)(((16u - (unsigned)(reinterpret_cast<uintptr_t>(out + e0) & 15u)) & 15u) >> 2);
    if (head > e1 - e0) head = e1 - e0;
    for (unsigned e = e0 + tid; e < e0 + head; e += RP_NT) out[e] = val(e / W, e % W);
    const unsigned v0 = e0 + head, nv = (e1 - v0) >> 2;
    for (unsigned j = tid; j < nv; j += RP_NT) {
        const unsigned e = v0 + 4u * j;
        unsigned row = e / W, col = e % W;
        float v[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            v[t] = val(row, col);
            if (++col == W) { col = 0; ++row; }
        }
        *reinterpret_cast<float4 *>(out + e) = make_float4(v[0], v[1], v[2], v[3]);
    }
    for (unsigned e = v0 + 4u * nv + tid; e < e1; e += RP_NT) out[e] = val(e / W, e % W);
}

// roipool3dLauncher (roipoint_pool3d_kernel.cu:38-134) in one launch.  boxes: rows of box_stride floats.
// CANON: the PointRCNN head's epilogue (pointrcnn_head.py:121-129) as well — the three sizes enlarged by (ex, ey, ez) first,
// the pooled coordinates relative to the RoI centre and rotated by -heading (the c, s of the in-box test ARE cos / sin of
// -heading), zeros in every row of an empty box.
template <bool CANON>
__global__ __launch_bounds__(RP_NT) void roipoint_pool_kernel(int N, int M, int C, int S, const float *__restrict__ xyz,
                                                              const float *__restrict__ boxes, int box_stride, float ex, float ey,
                                                              float ez, const float *__restrict__ feats, float *pooled,
                                                              int *__restrict__ empty_flag) {
    __shared__ int s_list[RP_LIST];
    __shared__ int s_wave[RP_NT / 64];
    __shared__ int s_resume;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int bm = blockIdx.x, b = bm / M;
    const unsigned W = 3u + (unsigned)C;
    float bx[7];
#pragma unroll
    for (int f = 0; f < 7; ++f) bx[f] = boxes[(size_t)bm * box_stride + f];
    if (CANON) { bx[3] += ex; bx[4] += ey; bx[5] += ez; }   // enlarge_box3d: one fp32 add per size
    float c, s;
    box_cos_sin_f(bx[6], &c, &s);
    const float reach2 = box_reach2_pool(bx);
    const float *px = xyz + (size_t)b * N * 3;
    const float *pf = feats + (size_t)b * N * C;             // never dereferenced when C == 0
    float *out = pooled + (size_t)bm * S * W;

    // element (col) of the output row made from point p
    auto from_point = [&](int p, unsigned col) -> float {
        if (col >= 3u) return pf[(size_t)p * C + (col - 3u)];
        if (!CANON) return px[(size_t)p * 3 + col];
        if (col == 2u) return px[(size_t)p * 3 + 2] - bx[2];
        const float sx = px[(size_t)p * 3] - bx[0], sy = px[(size_t)p * 3 + 1] - bx[1];
        return col == 0u ? sx * c + sy * (-s) : sx * s + sy * c;
    };

    int found = 0, next = 0;   // rows written so far; first point not yet searched (both uniform)
    while (found < S && next < N) {
        const int want = min(RP_LIST, S - found);
        int n = 0;
        while (n < want && next < N) {
            const int p = next + tid;
            bool hit = false;
            if (p < N) {
                const float x = px[(size_t)p * 3], y = px[(size_t)p * 3 + 1], z = px[(size_t)p * 3 + 2];
                const float sx = x - bx[0], sy = y - bx[1];
                float lx, ly;
                if (!(sx * sx + sy * sy > reach2)) hit = point_in_box3d_cs(x, y, z, bx, c, s, &lx, &ly);
            }
            const unsigned long long bal = __ballot(hit);
            if (lane == 0) s_wave[wave] = __popcll(bal);
            __syncthreads();
            int base = n, tot = 0;
#pragma unroll
            for (int w = 0; w < RP_NT / 64; ++w) {
                const int t = s_wave[w];
                if (w < wave) base += t;
                tot += t;
            }
            const int slot = base + lanes_below(bal, lane);
            if (hit && slot < want) s_list[slot] = p;
            if (hit && slot == want) s_resume = p;   // the first hit this round has no room for
            __syncthreads();
            if (n + tot > want) {
                n = want;
                next = s_resume;
            } else {
                n += tot;
                next += RP_NT;
            }
        }
        const int k0 = found;
        emit_flat(out, (unsigned)k0 * W, (unsigned)(k0 + n) * W, W,
                  [&](unsigned row, unsigned col) { return from_point(s_list[row - (unsigned)k0], col); });
        found += n;
        __syncthreads();   // s_list is refilled by the next round
    }
    const int cnt = found;
    if (tid == 0) empty_flag[bm] = cnt == 0 ? 1 : 0;
    if (cnt == 0) {
        if (CANON) emit_flat(out, 0u, (unsigned)S * W, W, [](unsigned, unsigned) { return 0.f; });
        return;   // the reference leaves the rows of an empty box to the caller's zero fill
    }
    if (cnt >= S) return;
    // fewer than S hits: row k >= cnt repeats row k % cnt (get_pooled_idx :92-99)
    if (cnt <= RP_LIST) {   // one round: s_list still holds every hit
        emit_flat(out, (unsigned)cnt * W, (unsigned)S * W, W,
                  [&](unsigned row, unsigned col) { return from_point(s_list[row % (unsigned)cnt], col); });
    } else {                // re-read the rows this workgroup wrote (ordered by the barrier that ended the last round)
        emit_flat(out, (unsigned)cnt * W, (unsigned)S * W, W,
                  [&](unsigned row, unsigned col) { return out[(row % (unsigned)cnt) * W + col]; });
    }
}

// ---- RoI-aware pooling --------------------------------------------------------------------------------------------------
constexpr int RA_LDS_VOX = 8192;   // voxel counters of a box held in LDS (32 KB); larger grids count in the caller's workspace

// roiaware_pool3d_launcher (roiaware_pool3d_kernel.cu:39-233), a workgroup per box: the points are tested 256 at a time in
// ascending order; the first wave then appends the hits of that block to their voxels' lists in index order (lanes of one
// voxel ranked by a ballot), so a list holds the first max_pts - 1 points of its voxel, ascending, as the reference's serial
// walk leaves them.  Then the lists are completed (count in slot 0, zeros behind the entries: every element written) and
// pooled over (voxel, channel) with the channel as the fast axis.
__global__ __launch_bounds__(RA_NT) void roiaware_forward_kernel(int P, int C, int max_pts, int ox, int oy, int oz,
                                                                 const float *__restrict__ rois, const float *__restrict__ pts,
                                                                 const float *__restrict__ feats, int pool_method, int *ws_cnt,
                                                                 int *pts_idx, int *__restrict__ argmax, float *__restrict__ pooled) {
    __shared__ int s_cnt[RA_LDS_VOX];
    __shared__ int s_vox[RA_NT];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int k = blockIdx.x, V = ox * oy * oz, cap = max_pts - 1;
    int *cnt = V <= RA_LDS_VOX ? s_cnt : ws_cnt + (size_t)k * V;
    int *list = pts_idx + (size_t)k * V * max_pts;
    for (int v = tid; v < V; v += RA_NT) cnt[v] = 0;
    float bx[7];
#pragma unroll
    for (int f = 0; f < 7; ++f) bx[f] = rois[(size_t)k * 7 + f];
    float c, s;
    box_cos_sin_f(bx[6], &c, &s);
    const float reach2 = box_reach2_pool(bx);
    __syncthreads();

    for (int p0 = 0; p0 < P; p0 += RA_NT) {
        const int p = p0 + tid;
        const int v = p < P ? roiaware_cell_of(pts, (size_t)p, bx, c, s, reach2, ox, oy, oz) : -1;
        s_vox[tid] = v;
        if (!__syncthreads_or(v >= 0)) continue;   // no hit in this block of points (nobody reads s_vox)
        if (wave == 0)
            roiaware_append_block(s_vox, p0, cnt, [&](int lv, int slot, int pt) {
                if (slot < cap) list[(size_t)lv * max_pts + 1 + slot] = pt;
            });
        __syncthreads();
    }
    __syncthreads();
    // slot 0 = count (capped), zeros behind the entries
    for (int v = wave; v < V; v += RA_NT / 64) {
        const int n = min(cnt[v], cap);
        int *l = list + (size_t)v * max_pts;
        if (lane == 0) l[0] = n;
        for (int q = n + 1 + lane; q < max_pts; q += 64) l[q] = 0;
    }
    __syncthreads();
    const unsigned VC = (unsigned)V * (unsigned)C;
    for (unsigned e = tid; e < VC; e += RA_NT) {
        const unsigned v = e / (unsigned)C, ch = e % (unsigned)C;
        const int n = min(cnt[v], cap);
        const int *l = list + (size_t)v * max_pts + 1;
        const size_t o = (size_t)k * VC + e;
        if (pool_method == 0) {
            int arg;
            const float best = roiaware_list_max(l, n, feats, C, ch, &arg);
            if (arg != -1) pooled[o] = best;
            argmax[o] = arg;
        } else if (n > 0) {
            pooled[o] = roiaware_list_avg(l, n, feats, C, ch);
        }
    }
}

// roiaware_pool3d_backward_launcher (:236-307) as a gather: a wave per point walks the boxes in ascending order, 64 at a
// time; for a box that contains the point it recomputes the point's voxel and adds that voxel's term to the point's row,
// which it alone writes — max: grad_out where argmax names the point; avg: grad_out * (1 / max(count, 1)) if the point is in
// the voxel's list (searched: the list holds only the first max_pts - 1 points).  Terms are added in ascending (box, voxel)
// order (a point has one voxel per box); grad_in is fully written.
__global__ __launch_bounds__(RA_NT) void roiaware_backward_kernel(int K, int P, int C, int max_pts, int ox, int oy, int oz,
                                                                  const float *__restrict__ rois, const float *__restrict__ pts,
                                                                  const int *__restrict__ pts_idx, const int *__restrict__ argmax,
                                                                  const float *__restrict__ grad_out, int pool_method, float *grad_in) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int p = blockIdx.x * (RA_NT / 64) + wave;
    if (p >= P) return;   // (no workgroup barrier below)
    const int V = ox * oy * oz;
    const float x = pts[(size_t)p * 3], y = pts[(size_t)p * 3 + 1], z = pts[(size_t)p * 3 + 2];
    float *g = grad_in + (size_t)p * C;
    for (int ch = lane; ch < C; ch += 64) g[ch] = 0.f;
    for (int k0 = 0; k0 < K; k0 += 64) {
        const int k = k0 + lane;
        int v = -1;
        if (k < K) {
            float bx[7];
#pragma unroll
            for (int f = 0; f < 7; ++f) bx[f] = rois[(size_t)k * 7 + f];
            const float sx = x - bx[0], sy = y - bx[1];
            if (!(sx * sx + sy * sy > box_reach2_pool(bx))) {
                float c, s, lx, ly;
                box_cos_sin_f(bx[6], &c, &s);
                if (point_in_box3d_cs(x, y, z, bx, c, s, &lx, &ly)) v = roiaware_voxel(lx, ly, z, bx, ox, oy, oz);
            }
        }
        unsigned long long hits = __ballot(v >= 0);
        while (hits) {
            const int j = __ffsll((long long)hits) - 1;
            hits &= hits - 1ull;
            const size_t cell = (size_t)(k0 + j) * V + __shfl(v, j, 64);
            if (pool_method == 0) {
                for (int ch = lane; ch < C; ch += 64)
                    if (argmax[cell * C + ch] == p) g[ch] += grad_out[cell * C + ch];
            } else {
                const int *l = pts_idx + cell * max_pts;
                const int n = min(max(l[0], 0), max_pts - 1);
                bool mine = false;
                for (int q = lane; q < n; q += 64) mine |= l[1 + q] == p;
                if (__ballot(mine)) {
                    const float w = 1 / fmaxf((float)n, 1.0f);
                    for (int ch = lane; ch < C; ch += 64) g[ch] += grad_out[cell * C + ch] * w;
                }
            }
        }
    }
}

}  // namespace pdm

using namespace pdm;

static int roipoint_args(const char *who, int B, int N, int M, int C, int S, const void *xyz, const void *boxes, const void *feats,
                         const void *pooled, const void *empty_flag) {
    PDM_REQUIRE(B >= 0 && N >= 0 && M >= 0 && C >= 0 && S >= 0, PDM_E_BADARG, "%s: B=%d N=%d M=%d C=%d S=%d", who, B, N, M, C, S);
    if (B == 0 || N == 0 || M == 0 || S == 0) return 0;
    PDM_REQUIRE(xyz && boxes && pooled && empty_flag && (C == 0 || feats), PDM_E_BADARG, "%s: null pointer", who);
    PDM_REQUIRE((long long)B * M < (1ll << 31) && (long long)S * (3 + (long long)C) < (1ll << 31), PDM_E_TOOLARGE,
                "%s: B * M = %lld boxes or S * (3 + C) = %lld floats per box (each below 2^31)", who, (long long)B * M,
                (long long)S * (3 + (long long)C));
    return 1;   // sizes are non-zero and the arguments fit: launch
}

extern "C" int pdm_roipoint_pool3d(void *stream, int B, int N, int M, int C, int S, const float *xyz, const float *boxes,
                                   const float *feats, float *pooled, int *empty_flag) {
    const int rc = roipoint_args("roipoint_pool3d", B, N, M, C, S, xyz, boxes, feats, pooled, empty_flag);
    if (rc <= 0) return rc;   // an error code, or 0: a zero size, nothing to write
    hipLaunchKernelGGL(roipoint_pool_kernel<false>, dim3(B * M), dim3(RP_NT), 0, as_stream(stream), N, M, C, S, xyz, boxes, 7, 0.f, 0.f,
                       0.f, feats, pooled, empty_flag);
    return check_launch("roipoint_pool3d");
}

extern "C" int pdm_roipoint_pool3d_canonical(void *stream, int B, int N, int M, int C, int S, const float *xyz, const float *rois,
                                             int roi_stride, float extra_x, float extra_y, float extra_z, const float *feats,
                                             float *pooled, int *empty_flag) {
    const int rc = roipoint_args("roipoint_pool3d_canonical", B, N, M, C, S, xyz, rois, feats, pooled, empty_flag);
    if (rc <= 0) return rc;   // an error code, or 0: a zero size, nothing to write
    PDM_REQUIRE(roi_stride >= 7, PDM_E_BADARG, "roipoint_pool3d_canonical: roi_stride=%d (at least 7)", roi_stride);
    hipLaunchKernelGGL(roipoint_pool_kernel<true>, dim3(B * M), dim3(RP_NT), 0, as_stream(stream), N, M, C, S, xyz, rois, roi_stride,
                       extra_x, extra_y, extra_z, feats, pooled, empty_flag);
    return check_launch("roipoint_pool3d_canonical");
}

static int roiaware_args(const char *who, int K, int P, int C, int max_pts, int ox, int oy, int oz) {
    PDM_REQUIRE(K >= 0 && P >= 0 && C >= 0, PDM_E_BADARG, "%s: K=%d P=%d C=%d", who, K, P, C);
    PDM_REQUIRE(ox >= 1 && oy >= 1 && oz >= 1 && ox <= 256 && oy <= 256 && oz <= 256, PDM_E_BADARG,
                "%s: out size (%d, %d, %d): each of 1 .. 256 (voxel indices are 8 bits in the reference)", who, ox, oy, oz);
    PDM_REQUIRE(max_pts >= 2, PDM_E_BADARG, "%s: max_pts=%d (slot 0 is the count: at least 2)", who, max_pts);
    PDM_REQUIRE((long long)ox * oy * oz * (long long)C < (1ll << 31), PDM_E_TOOLARGE, "%s: %lld pooled values per box (below 2^31)", who,
                (long long)ox * oy * oz * (long long)C);
    return 0;
}

extern "C" size_t pdm_roiaware_pool3d_workspace_bytes(int K, int out_x, int out_y, int out_z) {
    if (K <= 0 || out_x <= 0 || out_y <= 0 || out_z <= 0) return 0;
    const size_t V = (size_t)out_x * out_y * out_z;
    return V <= (size_t)RA_LDS_VOX ? 0 : (size_t)K * V * sizeof(int);
}

extern "C" int pdm_roiaware_pool3d_forward(void *stream, int K, int P, int C, int max_pts, int out_x, int out_y, int out_z,
                                           const float *rois, const float *pts, const float *feats, int pool_method, void *workspace,
                                           size_t workspace_bytes, int *pts_idx_of_voxels, int *argmax, float *pooled) {
    const int rc = roiaware_args("roiaware_pool3d_forward", K, P, C, max_pts, out_x, out_y, out_z);
    if (rc) return rc;
    PDM_REQUIRE(pool_method == 0 || pool_method == 1, PDM_E_BADARG, "roiaware_pool3d_forward: pool_method=%d (0 max, 1 avg)", pool_method);
    if (K == 0) return 0;
    PDM_REQUIRE(rois && pts_idx_of_voxels && (P == 0 || pts) && (C == 0 || (pooled && (P == 0 || feats) && (pool_method == 1 || argmax))),
                PDM_E_BADARG, "roiaware_pool3d_forward: null pointer");
    const size_t need = pdm_roiaware_pool3d_workspace_bytes(K, out_x, out_y, out_z);
    PDM_REQUIRE(need == 0 || (workspace && workspace_bytes >= need), PDM_E_BADARG,
                "roiaware_pool3d_forward: workspace of %zu bytes, need %zu", workspace_bytes, need);
    PDM_WS_ALIGNED("roiaware_pool3d_forward", workspace);
    hipLaunchKernelGGL(roiaware_forward_kernel, dim3(K), dim3(RA_NT), 0, as_stream(stream), P, C, max_pts, out_x, out_y, out_z, rois, pts,
                       feats, pool_method, static_cast<int *>(workspace), pts_idx_of_voxels, argmax, pooled);
    return check_launch("roiaware_pool3d_forward");
}

extern "C" int pdm_roiaware_pool3d_backward(void *stream, int K, int P, int C, int max_pts, int out_x, int out_y, int out_z,
                                            const float *rois, const float *pts, const int *pts_idx_of_voxels, const int *argmax,
                                            const float *grad_out, int pool_method, float *grad_in) {
    const int rc = roiaware_args("roiaware_pool3d_backward", K, P, C, max_pts, out_x, out_y, out_z);
    if (rc) return rc;
    PDM_REQUIRE(pool_method == 0 || pool_method == 1, PDM_E_BADARG, "roiaware_pool3d_backward: pool_method=%d (0 max, 1 avg)", pool_method);
    if (P == 0 || C == 0) return 0;
    PDM_REQUIRE(pts && grad_in && (K == 0 || (rois && grad_out && (pool_method == 0 ? (const void *)argmax : (const void *)pts_idx_of_voxels))),
                PDM_E_BADARG, "roiaware_pool3d_backward: null pointer");
    hipLaunchKernelGGL(roiaware_backward_kernel, dim3(divup(P, RA_NT / 64)), dim3(RA_NT), 0, as_stream(stream), K, P, C, max_pts, out_x,
                       out_y, out_z, rois, pts, pts_idx_of_voxels, argmax, grad_out, pool_method, grad_in);
    return check_launch("roiaware_pool3d_backward");
}

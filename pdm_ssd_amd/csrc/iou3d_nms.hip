// Rotated-box BEV overlap / IoU and NMS: the operators of the reference's iou3d_nms
// extension (pcdet/ops/iou3d_nms/src/iou3d_nms_kernel.cu, iou3d_nms.cpp) that detector post-processing calls.
// Boxes are 7 floats [x, y, z, dx, dy, dz, heading].  Same geometry as the reference: rotate the corners, collect
// proper edge intersections and contained corners (1e-2 margin), order them by atan2 about their centroid with the
// same bubble sort, fan area; IoU = overlap / max(sa + sb - overlap, 1e-8); a box is suppressed by an earlier kept
// box iff IoU > thresh (strict).
// MI355X-first difference: the reference copies the N x N/64 suppression mask to the host and reduces it there
// (cudaMemcpy + a CPU loop per call); here a one-wave kernel walks the mask on the device (each lane owns 64-box
// words of the `removed` set), so a call enqueues two kernels and nothing synchronises until the caller reads the count.
#include "nms.h"

namespace pdm {

// out (na, nb): mode 0 overlap area, 1 BEV IoU; 16 x 16 pairs per workgroup, the 16 boxes of each side staged in LDS
__global__ __launch_bounds__(256) void boxes_pairwise_kernel(int mode, int na, const float *__restrict__ boxes_a, int nb,
                                                             const float *__restrict__ boxes_b, float *__restrict__ out) {
    __shared__ float sa[16 * 7], sb[16 * 7];
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    const int a0 = blockIdx.y * 16, b0 = blockIdx.x * 16;
    if (threadIdx.x < 112) {
        const int i = threadIdx.x / 7, f = threadIdx.x % 7;
        sa[threadIdx.x] = a0 + i < na ? boxes_a[(size_t)(a0 + i) * 7 + f] : 0.f;
        sb[threadIdx.x] = b0 + i < nb ? boxes_b[(size_t)(b0 + i) * 7 + f] : 0.f;
    }
    __syncthreads();
    const int ai = a0 + ty, bi = b0 + tx;
    if (ai >= na || bi >= nb) return;
    out[(size_t)ai * nb + bi] = mode == 0 ? box_overlap_bev(sa + ty * 7, sb + tx * 7) : iou_bev(sa + ty * 7, sb + tx * 7);
}

__global__ __launch_bounds__(256) void boxes_aligned_overlap_kernel(int n, const float *__restrict__ boxes_a,
                                                                    const float *__restrict__ boxes_b, float *__restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float a[7], b[7];
#pragma unroll
    for (int f = 0; f < 7; ++f) { a[f] = boxes_a[(size_t)i * 7 + f]; b[f] = boxes_b[(size_t)i * 7 + f]; }
    out[i] = box_overlap_bev(a, b);
}

// mask (n, ceil(n/64)) : bit j of word (i, cb) set iff box 64 cb + j (> i) overlaps box i above the threshold
__global__ __launch_bounds__(64) void nms_mask_kernel(int n, float thresh, int normal, const float *__restrict__ boxes,
                                                      unsigned long long *__restrict__ mask) {
    const int row_start = blockIdx.y, col_start = blockIdx.x;
    const int cur = row_start * 64 + threadIdx.x;
    if (col_start < row_start) {   // earlier columns never matter: only later boxes can be suppressed by this one
        if (cur < n) mask[(size_t)cur * gridDim.x + col_start] = 0ull;
        return;
    }
    const unsigned long long t = nms_mask_tile(n, boxes, row_start, col_start, thresh, normal != 0, false);
    if (cur < n) mask[(size_t)cur * gridDim.x + col_start] = t;
}

// one wave, boxes visited in score order (nms.h's walk without a keep limit)
__global__ __launch_bounds__(64) void nms_scan_kernel(int n, int col_blocks, const unsigned long long *__restrict__ mask,
                                                      long long *__restrict__ keep, int *__restrict__ num_out) {
    const int kept = nms_walk(n, n, mask, col_blocks, [&](int k, int i) { keep[k] = i; });
    if (threadIdx.x == 0) *num_out = kept;
}

// more than 16384 boxes: the same walk with the `removed` words in LDS (col_blocks <= 16384 words = 128 KB)
__global__ __launch_bounds__(64) void nms_scan_lds_kernel(int n, int col_blocks, const unsigned long long *__restrict__ mask,
                                                          long long *__restrict__ keep, int *__restrict__ num_out) {
    extern __shared__ unsigned long long removed[];
    const int lane = threadIdx.x;
    for (int cb = lane; cb < col_blocks; cb += 64) removed[cb] = 0ull;
    __syncthreads();
    int kept = 0;
    for (int i = 0; i < n; ++i) {
        const int nblock = i >> 6, inblock = i & 63;
        if ((removed[nblock] >> inblock) & 1ull) continue;   // wave-uniform (same address in every lane)
        if (lane == 0) keep[kept] = i;
        ++kept;
        const unsigned long long *row = mask + (size_t)i * col_blocks;
        for (int cb = nblock + lane; cb < col_blocks; cb += 64) removed[cb] |= row[cb];
        __syncthreads();   // one wave: orders the LDS writes before the next box's read
    }
    if (lane == 0) *num_out = kept;
}

}  // namespace pdm

using namespace pdm;

extern "C" int pdm_boxes_overlap_bev(void *stream, int na, const float *boxes_a, int nb, const float *boxes_b, float *out) {
    PDM_REQUIRE(na >= 0 && nb >= 0, PDM_E_BADARG, "boxes_overlap_bev: negative size");
    if (na == 0 || nb == 0) return 0;
    PDM_REQUIRE(boxes_a && boxes_b && out, PDM_E_BADARG, "boxes_overlap_bev: null pointer");
    hipLaunchKernelGGL(boxes_pairwise_kernel, dim3(divup(nb, 16), divup(na, 16)), dim3(256), 0, as_stream(stream), 0, na, boxes_a,
                       nb, boxes_b, out);
    return check_launch("boxes_overlap_bev");
}

extern "C" int pdm_boxes_iou_bev(void *stream, int na, const float *boxes_a, int nb, const float *boxes_b, float *out) {
    PDM_REQUIRE(na >= 0 && nb >= 0, PDM_E_BADARG, "boxes_iou_bev: negative size");
    if (na == 0 || nb == 0) return 0;
    PDM_REQUIRE(boxes_a && boxes_b && out, PDM_E_BADARG, "boxes_iou_bev: null pointer");
    hipLaunchKernelGGL(boxes_pairwise_kernel, dim3(divup(nb, 16), divup(na, 16)), dim3(256), 0, as_stream(stream), 1, na, boxes_a,
                       nb, boxes_b, out);
    return check_launch("boxes_iou_bev");
}

extern "C" int pdm_boxes_aligned_overlap_bev(void *stream, int n, const float *boxes_a, const float *boxes_b, float *out) {
    PDM_REQUIRE(n >= 0, PDM_E_BADARG, "boxes_aligned_overlap_bev: negative size");
    if (n == 0) return 0;
    PDM_REQUIRE(boxes_a && boxes_b && out, PDM_E_BADARG, "boxes_aligned_overlap_bev: null pointer");
    hipLaunchKernelGGL(boxes_aligned_overlap_kernel, dim3(divup(n, 256)), dim3(256), 0, as_stream(stream), n, boxes_a, boxes_b, out);
    return check_launch("boxes_aligned_overlap_bev");
}

extern "C" size_t pdm_nms_workspace_bytes(int n) {
    if (n <= 0) return 0;
    return (size_t)n * ((n + 63) / 64) * sizeof(unsigned long long);
}

// boxes (n, 7) sorted by descending score; keep (n) int64 receives the kept positions in order, *num_out (device int)
// their count.  normal != 0: axis-aligned footprints (nms_normal_gpu).  Any n the n x n/64 mask workspace allows
// (n <= 1048576; beyond 16384 boxes the suppression walk keeps its bitmap in LDS instead of registers).
extern "C" int pdm_nms(void *stream, int n, const float *boxes, float thresh, int normal, void *workspace,
                       size_t workspace_bytes, long long *keep, int *num_out) {
    PDM_REQUIRE(n >= 0 && n <= 16384 * 64, PDM_E_TOOLARGE, "nms: n=%d (at most 1048576 boxes)", n);
    PDM_REQUIRE(num_out, PDM_E_BADARG, "nms: null pointer");
    if (n == 0) return zero_fill(stream, "nms(zero)", num_out, sizeof(int));
    PDM_REQUIRE(boxes && keep && workspace && workspace_bytes >= pdm_nms_workspace_bytes(n), PDM_E_BADARG,
                "nms: null pointer or workspace of %zu bytes, need %zu", workspace_bytes, pdm_nms_workspace_bytes(n));
    PDM_WS_ALIGNED("nms", workspace);
    const int cb = (n + 63) / 64;
    unsigned long long *mask = static_cast<unsigned long long *>(workspace);
    hipLaunchKernelGGL(nms_mask_kernel, dim3(cb, cb), dim3(64), 0, as_stream(stream), n, thresh, normal, boxes, mask);
    int rc = check_launch("nms(mask)");
    if (rc) return rc;
    if (n <= 16384) {
        hipLaunchKernelGGL(nms_scan_kernel, dim3(1), dim3(64), 0, as_stream(stream), n, cb, mask, keep, num_out);
    } else {
        const size_t lds = (size_t)cb * sizeof(unsigned long long);
        if (lds > 64 * 1024 - 256) {   // granted per device (common.h)
            const int e = grant_lds(reinterpret_cast<const void *>(&nms_scan_lds_kernel), 160 * 1024);
            PDM_REQUIRE(e == 0, PDM_E_TOOLARGE, "nms: cannot obtain %zu bytes of LDS", lds);
        }
        hipLaunchKernelGGL(nms_scan_lds_kernel, dim3(1), dim3(64), lds, as_stream(stream), n, cb, mask, keep, num_out);
    }
    return check_launch("nms(scan)");
}

// ---- points_in_boxes (pcdet/ops/roiaware_pool3d/src/roiaware_pool3d_kernel.cu:313-336): the first box of the
// sample's list that contains each point, -1 for background.  Boxes staged in LDS in chunks of 128.
namespace pdm {
__global__ __launch_bounds__(256) void points_in_boxes_kernel(int T, int M, const float *__restrict__ boxes,
                                                              const float *__restrict__ pts, int *__restrict__ box_idx) {
    __shared__ float sb[128 * 7];
    const int b = blockIdx.y, p = blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = p < M;
    float x = 0.f, y = 0.f, z = 0.f;
    if (live) {
        const float *pt = pts + ((size_t)b * M + p) * 3;
        x = pt[0]; y = pt[1]; z = pt[2];
    }
    int found = -1;
    for (int k0 = 0; k0 < T; k0 += 128) {
        const int nk = min(128, T - k0);
        __syncthreads();
        for (int e = threadIdx.x; e < nk * 7; e += blockDim.x) sb[e] = boxes[((size_t)b * T + k0) * 7 + e];
        __syncthreads();
        if (!live || found >= 0) continue;
        for (int k = 0; k < nk; ++k) {
            const float *bx = sb + k * 7;
            float lx, ly;
            if (point_in_box3d(x, y, z, bx, &lx, &ly)) {   // box_geometry.h, shared with roi_pool.hip
                found = k0 + k;
                break;
            }
        }
    }
    if (live) box_idx[(size_t)b * M + p] = found;
}
}  // namespace pdm

extern "C" int pdm_points_in_boxes(void *stream, int B, int T, int M, const float *boxes, const float *pts, int *box_idx) {
    PDM_REQUIRE(B >= 0 && T >= 0 && M >= 0 && B <= 65535, PDM_E_BADARG, "points_in_boxes: B=%d T=%d M=%d", B, T, M);
    if (B == 0 || M == 0) return 0;
    PDM_REQUIRE(pts && box_idx && (T == 0 || boxes), PDM_E_BADARG, "points_in_boxes: null pointer");
    hipLaunchKernelGGL(pdm::points_in_boxes_kernel, dim3(pdm::divup(M, 256), B), dim3(256), 0, pdm::as_stream(stream), T, M, boxes, pts,
                       box_idx);
    return pdm::check_launch("points_in_boxes");
}

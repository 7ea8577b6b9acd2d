// Batched training augmentation on the device: the reference's DataAugmentor.forward
// (pcdet/datasets/augmentor/data_augmentor.py:290-318) with the KITTI recipe's gt_sampling, random_world_flip,
// random_world_rotation and random_world_scaling, followed by DataProcessor.mask_points_and_boxes_outside_range
// (pcdet/datasets/processor/data_processor.py:79-93) and the class column of Dataset.prepare_data (dataset.py:158-215),
// for a whole batch of raw ragged clouds resident in HBM.  Per scene, in this order:
//   gt_sampling (database_sampler.py:445-502, :365-443, :130-147): per sample group (config order) the drawn database
//     entries; a candidate is accepted iff its BEV overlap is exactly 0 with every existing box (the scene's boxes,
//     non-target ones included, plus the boxes accepted for earlier groups) and with every other candidate of its own
//     draw (both members of a colliding pair are dropped).  box_overlap_bev (box_geometry.h) is iou3d_cpu.cpp's
//     arithmetic with its 1e-2 margin; IoU = 0 <=> overlap = 0.  Scene points inside an accepted box enlarged by
//     REMOVE_EXTRA_WIDTH are removed with points_in_boxes_cpu's test (roiaware_pool3d.cpp:121-140: margin 1e-2, the
//     comparisons in double, cos(-rz) / sin(-rz)).  Rows = [object points of the accepted entries, acceptance order,
//     each shifted by its box centre] + [surviving scene points, in order]; boxes = [target boxes] + [accepted boxes].
//   world transforms in AUG_CONFIG_LIST order (augmentor_utils.py:8-92), then limit_period(heading, 0.5, 2 pi).
//   range mask: points by x / y range, boxes by centre in range on all three axes (box_utils.py:93-115).
//
// Draws (the reference's numpy global RNG cannot be replayed; these are build-defined, as N1's):
//   fmix32 = the murmur3 finaliser;  u24(k) = (k >> 8) * 2^-24;  uniform(lo, hi, k) = lo + u24(k) * (hi - lo) in fp32
//   scene key  K(s, b) = draw_key (draws.h) = fmix32(fmix32(seed ^ step * 0x85EBCA6B) ^ b * 0x9E3779B1 ^ s * 0x7F4A7C15), step = state[0]
//     flip bit x = K(1, b) & 1, flip bit y = K(2, b) & 1, angle = uniform(rot, K(3, b)), scale = uniform(scale, K(4, b))
//   class permutation of epoch e for group g over [0, n): feistel_perm (draws.h), a 4-round balanced Feistel network on 2w bits
//     (2^(2w) >= n, w >= 1) keyed by kp = fmix32(fmix32(seed ^ 0x5BD1E995 ^ g * 0x9E3779B1) + e * 0x85EBCA6B), round r:
//     (L, R) -> (R, L ^ (fmix32(kp ^ R * 0x9E3779B1 ^ (r + 1) * 0x7F4A7C15) & (2^w - 1))), cycle-walked into [0, n).
//   pointer rule (sample_with_fixed_number): per group, the scenes in order; num = SAMPLE_NUM (minus the scene's boxes
//     of the class with LIMIT_WHOLE_SCENE; skipped when <= 0); if pointer >= n: epoch += 1, pointer = 0; the slice is
//     perm[pointer, min(pointer + num, n)) (short at an epoch end); pointer += num.
//
// Floating-point order (this file is built with -ffp-contract=off; nothing is fused):
//   rotation  x' = (x*c + y*(-s)) + z*0,  y' = (x*s + y*c) + z*0,  z' = (x*0 + y*0) + z  (rotate_points_along_z's fp32
//             matmul, summed left to right), c = fp32(cos(double(angle))), s = fp32(sin(double(angle))), heading += angle
//   flip y    heading = -(heading + fp32(pi));  scaling  x, y, z, dx, dy, dz *= scale
//   limit_period  h - floor(h / fp32(2 pi) + 0.5) * fp32(2 pi)
//   object point  x_rel + box_x (fp32);  enlarged box  dims + extra (fp32)
//   point in box  |z - cz| > dz / 2.0 (double) -> out; lx = sx*c' + sy*(-s'), ly = sx*s' + sy*c' (fp32, c' / s' of -rz as
//             above); in iff |lx| < dx / 2.0 + 1e-2f and |ly| < dy / 2.0 + 1e-2f, compared in double.
// Every output entry is written by a kernel (no memset, no atomics): the results are deterministic and a captured
// graph replays them exactly.
#include "box_geometry.h"
#include "draws.h"

namespace pdm {

constexpr int AG_MAXB = 1024;      // scenes per call
constexpr int AG_MAXG = 8;         // sample groups
constexpr int AG_MAXK = 256;       // candidate slots per scene (sum of the groups' SAMPLE_NUM)
constexpr int AG_MAXM = 256;       // input boxes per scene
constexpr int AG_THREADS = 256;
constexpr float AG_PI = 3.14159265358979323846f;
constexpr float AG_2PI = 6.28318530717958647692f;

struct AGGroups {
    int n;
    int cls[AG_MAXG];     // class index (0-based) of the group
    int num[AG_MAXG];     // SAMPLE_NUM
    int len[AG_MAXG];     // database entries of the class
    int first[AG_MAXG];   // database index of the class's first entry
    int slot[AG_MAXG];    // first candidate slot of the group
};

struct AGWorld {          // the per-scene transform: ops = up to 4 nibbles (1 flip x, 2 flip y, 3 rotation, 4 scaling)
    unsigned ops;
    float range[6];
    float extra[3];
};

__device__ __forceinline__ float ag_uniform(float lo, float hi, unsigned k) {
    const float u = (float)(k >> 8) * 0x1p-24f;
    return __fadd_rn(lo, __fmul_rn(u, __fsub_rn(hi, lo)));
}
// (x, y, z) through the scene's transform list (points: h == nullptr, dims == nullptr)
__device__ __forceinline__ void ag_world(unsigned ops, int flip, float c, float s, float angle, float scale, float &x,
                                         float &y, float &z, float *h, float *dims) {
    for (int k = 0; k < 4; ++k) {
        const unsigned op = (ops >> (4 * k)) & 15u;
        if (op == 1u && (flip & 1)) {
            y = -y;
            if (h) *h = -*h;
        } else if (op == 2u && (flip & 2)) {
            x = -x;
            if (h) *h = -__fadd_rn(*h, AG_PI);
        } else if (op == 3u) {
            const float nx = __fadd_rn(__fadd_rn(__fmul_rn(x, c), __fmul_rn(y, -s)), __fmul_rn(z, 0.f));
            const float ny = __fadd_rn(__fadd_rn(__fmul_rn(x, s), __fmul_rn(y, c)), __fmul_rn(z, 0.f));
            const float nz = __fadd_rn(__fadd_rn(__fmul_rn(x, 0.f), __fmul_rn(y, 0.f)), z);
            x = nx; y = ny; z = nz;
            if (h) *h = __fadd_rn(*h, angle);
        } else if (op == 4u) {
            x = __fmul_rn(x, scale); y = __fmul_rn(y, scale); z = __fmul_rn(z, scale);
            if (dims) { dims[0] = __fmul_rn(dims[0], scale); dims[1] = __fmul_rn(dims[1], scale); dims[2] = __fmul_rn(dims[2], scale); }
        }
    }
}

__device__ __forceinline__ bool ag_in_range_xy(const float *r, float x, float y) {
    return x >= r[0] && x <= r[3] && y >= r[1] && y <= r[4];
}

// ---- draw: state + seed -> sampled database indices (-1 padded), flip bits, angle, scale ------------------------------
__global__ __launch_bounds__(1024) void ag_draw_kernel(int B, AGGroups g, int limit, int M, const float *__restrict__ gt,
                                                       unsigned seed, int *__restrict__ state, int flip_axes, int use_rot,
                                                       float rlo, float rhi, int use_scale, float slo, float shi, int K,
                                                       int *__restrict__ sampled, int *__restrict__ flip,
                                                       float *__restrict__ angle, float *__restrict__ scale,
                                                       int *__restrict__ walk) {
    const int tid = threadIdx.x;
    const unsigned step = (unsigned)state[0];
    for (int b = tid; b < B; b += blockDim.x) {
        int f = 0;
        if (flip_axes & 1) f |= (int)(draw_key(seed, step, b, 1) & 1u);
        if (flip_axes & 2) f |= (int)(draw_key(seed, step, b, 2) & 1u) << 1;
        flip[b] = f;
        angle[b] = use_rot ? ag_uniform(rlo, rhi, draw_key(seed, step, b, 3)) : 0.f;
        scale[b] = use_scale ? ag_uniform(slo, shi, draw_key(seed, step, b, 4)) : 1.f;
    }
    if (tid < g.n) {   // the pointer rule: one lane per group walks the scenes in order
        int epoch = state[1 + 2 * tid], ptr = state[2 + 2 * tid];
        const int n = g.len[tid];
        for (int b = 0; b < B; ++b) {
            int num = g.num[tid];
            if (limit) {
                const float want = (float)(g.cls[tid] + 1);
                for (int m = 0; m < M; ++m) num -= gt[((size_t)b * M + m) * 8 + 7] == want ? 1 : 0;
            }
            int *w = walk + ((size_t)b * AG_MAXG + tid) * 3;
            if (num > 0) {
                if (ptr >= n) { ++epoch; ptr = 0; }
                w[0] = epoch; w[1] = ptr; w[2] = min(num, n - ptr);
                ptr += num;
            } else {
                w[0] = 0; w[1] = 0; w[2] = 0;
            }
        }
        state[1 + 2 * tid] = epoch;
        state[2 + 2 * tid] = ptr;
    }
    __syncthreads();   // the walk table (global, written by this workgroup) is read below
    for (int e = tid; e < B * K; e += blockDim.x) {
        const int b = e / K, slot = e - b * K;
        int out = -1;
        for (int t = 0; t < g.n; ++t) {
            const int j = slot - g.slot[t];
            if (j < 0 || j >= g.num[t]) continue;
            const int *w = walk + ((size_t)b * AG_MAXG + t) * 3;
            if (j < w[2]) {
                const unsigned kp = fmix32(fmix32(seed ^ 0x5BD1E995u ^ (unsigned)t * 0x9E3779B1u) + (unsigned)w[0] * 0x85EBCA6Bu);
                out = g.first[t] + (int)feistel_perm((unsigned)(w[1] + j), (unsigned)g.len[t], kp);
            }
        }
        sampled[e] = out;
    }
    if (tid == 0) state[0] = (int)(step + 1u);
}

// ---- collision select + box outputs: one workgroup per scene -----------------------------------------------------------
struct AGSelect {
    int B, M, K, M_out, remove_outside;
    long long db_entries;
    const float *gt, *db_boxes;
    const long long *db_off;
    const int *sampled, *flip;
    const float *angle, *scale;
    float *out_boxes;
    int *out_nbox, *accepted, *num_accepted, *obj_off;
};

__global__ __launch_bounds__(AG_THREADS) void ag_select_kernel(AGSelect a, AGGroups g, AGWorld wd) {
    __shared__ float ex[(AG_MAXM + AG_MAXK) * 7];
    __shared__ float exr[AG_MAXM + AG_MAXK];
    __shared__ float exc[AG_MAXM + AG_MAXK];     // class column of the existing boxes (> 0 target, < 0 other)
    __shared__ float cand[AG_MAXK * 7];
    __shared__ float crad[AG_MAXK];
    __shared__ int s_idx[AG_MAXK];
    __shared__ int s_acc[AG_MAXK];
    __shared__ int s_wave[AG_THREADS / 64];
    const int b = blockIdx.x, tid = threadIdx.x;
    int tot;

    // existing boxes: the scene's present rows (class != 0), in order
    int n_exist = 0;
    for (int m0 = 0; m0 < a.M; m0 += AG_THREADS) {
        const int m = m0 + tid;
        const float *src = a.gt + ((size_t)b * a.M + m) * 8;
        const bool present = m < a.M && src[7] != 0.f;
        const int pos = n_exist + block_scan<AG_THREADS>(present ? 1 : 0, s_wave, &tot);
        if (present) {
            for (int f = 0; f < 7; ++f) ex[pos * 7 + f] = src[f];
            exc[pos] = src[7];
            exr[pos] = bev_radius(src);
        }
        n_exist += tot;
    }
    int n_acc = 0;
    __syncthreads();
    for (int t = 0; t < g.n; ++t) {
        const int num = g.num[t];
        int idx = -1;
        if (tid < num) {
            idx = a.sampled[(size_t)b * a.K + g.slot[t] + tid];
            if (idx >= a.db_entries) idx = -1;   // outside the database: padding
            s_idx[tid] = idx;
            if (idx >= 0) {
                for (int f = 0; f < 7; ++f) cand[tid * 7 + f] = a.db_boxes[(size_t)idx * 7 + f];
                crad[tid] = bev_radius(cand + tid * 7);
            }
        }
        __syncthreads();
        bool valid = idx >= 0;
        if (valid) {
            const float *me = cand + tid * 7;
            const float mr = crad[tid];
            for (int e = 0; e < n_exist && valid; ++e) {
                if (bev_circles_disjoint(me[0], me[1], mr, ex[e * 7], ex[e * 7 + 1], exr[e])) continue;
                if (!(box_overlap_bev(me, ex + e * 7) == 0.f)) valid = false;
            }
            for (int c = 0; c < num && valid; ++c) {
                if (c == tid || s_idx[c] < 0) continue;
                if (bev_circles_disjoint(me[0], me[1], mr, cand[c * 7], cand[c * 7 + 1], crad[c])) continue;
                if (!(box_overlap_bev(me, cand + c * 7) == 0.f)) valid = false;
            }
        }
        const int r = block_scan<AG_THREADS>(valid ? 1 : 0, s_wave, &tot);
        if (valid) {
            const int pos = n_exist + r;
            for (int f = 0; f < 7; ++f) ex[pos * 7 + f] = cand[tid * 7 + f];
            exr[pos] = crad[tid];
            exc[pos] = (float)(g.cls[t] + 1);
            s_acc[n_acc + r] = idx;
        }
        n_exist += tot;
        n_acc += tot;
        __syncthreads();
    }
    for (int k = tid; k < a.K; k += AG_THREADS) a.accepted[(size_t)b * a.K + k] = k < n_acc ? s_acc[k] : -1;
    if (tid == 0) {
        a.num_accepted[b] = n_acc;
        int acc = 0;
        int *oo = a.obj_off + (size_t)b * (a.K + 1);
        for (int k = 0; k < n_acc; ++k) {
            oo[k] = acc;
            acc += (int)(a.db_off[s_acc[k] + 1] - a.db_off[s_acc[k]]);
        }
        oo[n_acc] = acc;
    }

    // box outputs: [target scene boxes] + [accepted], transformed, heading wrapped, range-masked, compacted, zero-padded
    float c = 1.f, s = 0.f;
    box_cos_sin(a.angle[b], &c, &s);
    const int fl = a.flip[b];
    const float ang = a.angle[b], sc = a.scale[b];
    int n_out = 0;
    for (int e0 = 0; e0 < n_exist; e0 += AG_THREADS) {
        const int e = e0 + tid;
        bool keep = false;
        float bx[8];
        if (e < n_exist && exc[e] > 0.f) {
            for (int f = 0; f < 7; ++f) bx[f] = ex[e * 7 + f];
            bx[7] = exc[e];
            ag_world(wd.ops, fl, c, s, ang, sc, bx[0], bx[1], bx[2], &bx[6], &bx[3]);
            bx[6] = __fsub_rn(bx[6], __fmul_rn(floorf(__fadd_rn(__fdiv_rn(bx[6], AG_2PI), 0.5f)), AG_2PI));
            keep = !a.remove_outside ||
                   (bx[0] >= wd.range[0] && bx[0] <= wd.range[3] && bx[1] >= wd.range[1] && bx[1] <= wd.range[4] &&
                    bx[2] >= wd.range[2] && bx[2] <= wd.range[5]);
        }
        const int pos = n_out + block_scan<AG_THREADS>(keep ? 1 : 0, s_wave, &tot);
        if (keep && pos < a.M_out)
            for (int f = 0; f < 8; ++f) a.out_boxes[((size_t)b * a.M_out + pos) * 8 + f] = bx[f];
        n_out += tot;
    }
    for (int k = n_out * 8 + tid; k < a.M_out * 8; k += AG_THREADS) a.out_boxes[(size_t)b * a.M_out * 8 + k] = 0.f;
    if (tid == 0) a.out_nbox[b] = n_out;
}

// ---- scene edit: count (per segment) -> scan -> fill; W workgroups per scene, each owns one contiguous segment --------
struct AGScene {
    int B, C, K, W;
    long long capacity;
    const float *raw;
    const int *counts;
    const float *db_pts, *db_boxes;
    const long long *db_off;
    const int *accepted, *num_accepted, *obj_off, *flip;
    const float *angle, *scale;
    int *seg_count, *seg_base;
    long long *scene_off;
    int *out_counts, *overflow;
    float *out;
};

struct AGSceneLds {
    float box[AG_MAXK * 7];     // accepted boxes, enlarged
    float cs[AG_MAXK * 2];      // cos(-rz), sin(-rz)
    float lim2[AG_MAXK];        // squared bounding-circle reject radius
    int off[AG_MAXK + 1];       // object-row prefix
    int src[AG_MAXK];           // database index
    int s_wave[AG_THREADS / 64];
};

struct AGRowCtx {
    int nacc, obj_total, n_scene;
    long long start;
    float c, s, angle, scale;
    int flip;
};

__device__ __forceinline__ AGRowCtx ag_scene_setup(const AGScene &a, const AGWorld &wd, AGSceneLds &L, int b) {
    AGRowCtx x;
    long long start = 0;
    for (int k = 0; k < b; ++k) start += a.counts[k];
    x.start = start;
    x.n_scene = a.counts[b];
    x.nacc = a.num_accepted[b];
    const int *oo = a.obj_off + (size_t)b * (a.K + 1);
    for (int k = threadIdx.x; k <= x.nacc; k += AG_THREADS) L.off[k] = oo[k];
    for (int k = threadIdx.x; k < x.nacc; k += AG_THREADS) {
        const int idx = a.accepted[(size_t)b * a.K + k];
        L.src[k] = idx;
        float *bx = L.box + k * 7;
        for (int f = 0; f < 7; ++f) bx[f] = a.db_boxes[(size_t)idx * 7 + f];
        bx[3] = __fadd_rn(bx[3], wd.extra[0]);
        bx[4] = __fadd_rn(bx[4], wd.extra[1]);
        bx[5] = __fadd_rn(bx[5], wd.extra[2]);
        float c, s;
        box_cos_sin(-bx[6], &c, &s);
        L.cs[2 * k] = c;
        L.cs[2 * k + 1] = s;
        L.lim2[k] = box_reach2(bx);   // bounding-circle reject radius (box_geometry.h)
    }
    x.obj_total = oo[x.nacc];
    box_cos_sin(a.angle[b], &x.c, &x.s);
    x.angle = a.angle[b];
    x.scale = a.scale[b];
    x.flip = a.flip[b];
    __syncthreads();
    return x;
}

// row r of the scene's virtual list -> kept?, transformed xyz, source row pointer
__device__ __forceinline__ bool ag_row(const AGScene &a, const AGWorld &wd, const AGSceneLds &L, const AGRowCtx &x, int r,
                                       float &px, float &py, float &pz, const float *&src) {
    if (r < x.obj_total) {
        int lo = 0, hi = x.nacc - 1;            // last entry with off <= r
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (L.off[mid] <= r) lo = mid; else hi = mid - 1;
        }
        const int idx = L.src[lo];
        src = a.db_pts + (size_t)(a.db_off[idx] + (r - L.off[lo])) * a.C;
        const float *bx = L.box + lo * 7;
        px = __fadd_rn(src[0], bx[0]);
        py = __fadd_rn(src[1], bx[1]);
        pz = __fadd_rn(src[2], bx[2]);
    } else {
        src = a.raw + (size_t)(x.start + (r - x.obj_total)) * a.C;
        px = src[0]; py = src[1]; pz = src[2];
        for (int k = 0; k < x.nacc; ++k) {
            const float *bx = L.box + k * 7;
            const float dx = px - bx[0], dy = py - bx[1];
            if (dx * dx + dy * dy > L.lim2[k]) continue;
            if (point_in_box_margin(dx, dy, pz, bx, L.cs[2 * k], L.cs[2 * k + 1])) return false;
        }
    }
    ag_world(wd.ops, x.flip, x.c, x.s, x.angle, x.scale, px, py, pz, nullptr, nullptr);
    return ag_in_range_xy(wd.range, px, py);
}

__device__ __forceinline__ void ag_segment(int total, int W, int w, int *r0, int *r1) {
    const int per = (total + W - 1) / W;
    *r0 = min(total, w * per);
    *r1 = min(total, *r0 + per);
}

__global__ __launch_bounds__(AG_THREADS) void ag_count_kernel(AGScene a, AGWorld wd) {
    __shared__ AGSceneLds L;
    const int b = blockIdx.y, w = blockIdx.x;
    const AGRowCtx x = ag_scene_setup(a, wd, L, b);
    int r0, r1;
    ag_segment(x.obj_total + x.n_scene, a.W, w, &r0, &r1);
    int n = 0;
    for (int r = r0 + threadIdx.x; r < r1; r += AG_THREADS) {
        float px, py, pz;
        const float *src;
        n += ag_row(a, wd, L, x, r, px, py, pz, src) ? 1 : 0;
    }
    for (int off = 32; off > 0; off >>= 1) n += __shfl_down(n, off, 64);
    if ((threadIdx.x & 63) == 0) L.s_wave[threadIdx.x >> 6] = n;
    __syncthreads();
    if (threadIdx.x == 0) {
        int t = 0;
        for (int k = 0; k < AG_THREADS / 64; ++k) t += L.s_wave[k];
        a.seg_count[(size_t)b * a.W + w] = t;
    }
}

// seg_count (B, W) -> seg_base, out_counts, offsets (B + 1), overflow: see common.h.  One workgroup, thread b = frame b.
__global__ __launch_bounds__(1024) void segment_scan_kernel(int B, int W, const int *__restrict__ seg_count,
                                                            int *__restrict__ seg_base, int *__restrict__ out_counts,
                                                            long long *__restrict__ offsets, int *__restrict__ overflow,
                                                            long long capacity) {
    __shared__ long long s[1024];
    const int b = threadIdx.x;
    long long tot = 0;
    if (b < B) {
        for (int w = 0; w < W; ++w) {
            seg_base[(size_t)b * W + w] = (int)tot;
            tot += seg_count[(size_t)b * W + w];
        }
        out_counts[b] = (int)tot;
    }
    s[b] = tot;
    __syncthreads();
    for (int off = 1; off < 1024; off <<= 1) {   // Hillis-Steele inclusive scan
        const long long v = b >= off ? s[b - off] : 0;
        __syncthreads();
        s[b] += v;
        __syncthreads();
    }
    if (b < B) offsets[b] = s[b] - tot;
    if (b == 0) {
        offsets[B] = s[1023];
        overflow[0] = s[1023] > capacity ? 1 : 0;
    }
}

int segment_scan_launch(void *stream, const char *what, int B, int W, const int *seg_count, int *seg_base, int *out_counts,
                        long long *offsets, int *overflow, long long capacity) {
    hipLaunchKernelGGL(segment_scan_kernel, dim3(1), dim3(1024), 0, as_stream(stream), B, W, seg_count, seg_base, out_counts,
                       offsets, overflow, capacity);
    return check_launch(what);
}

__global__ __launch_bounds__(AG_THREADS) void ag_fill_kernel(AGScene a, AGWorld wd) {
    __shared__ AGSceneLds L;
    const int b = blockIdx.y, w = blockIdx.x;
    const AGRowCtx x = ag_scene_setup(a, wd, L, b);
    int r0, r1;
    ag_segment(x.obj_total + x.n_scene, a.W, w, &r0, &r1);
    long long pos = a.scene_off[b] + a.seg_base[(size_t)b * a.W + w];
    for (int c0 = r0; c0 < r1; c0 += AG_THREADS) {
        const int r = c0 + threadIdx.x;
        float px = 0.f, py = 0.f, pz = 0.f;
        const float *src = nullptr;
        const bool keep = r < r1 && ag_row(a, wd, L, x, r, px, py, pz, src);
        int tot;
        const long long p = pos + block_scan<AG_THREADS>(keep ? 1 : 0, L.s_wave, &tot);
        if (keep && p < a.capacity) {
            float *o = a.out + (size_t)p * a.C;
            o[0] = px; o[1] = py; o[2] = pz;
            for (int f = 3; f < a.C; ++f) o[f] = src[f];
        }
        pos += tot;
    }
}

static int ag_segments(int B) { return max(1, min(64, 2048 / max(B, 1))); }

struct AGLayout {
    size_t walk, obj_off, seg_count, seg_base, scene_off, total;
};

static AGLayout ag_layout(int B, int K) {
    AGLayout l;
    const int W = ag_segments(B);
    size_t o = 0;
    l.walk = o; o += align256((size_t)B * AG_MAXG * 3 * sizeof(int));
    l.obj_off = o; o += align256((size_t)B * (K + 1) * sizeof(int));
    l.seg_count = o; o += align256((size_t)B * W * sizeof(int));
    l.seg_base = o; o += align256((size_t)B * W * sizeof(int));
    l.scene_off = o; o += align256((size_t)(B + 1) * sizeof(long long));
    l.total = o;
    return l;
}

static int ag_groups(const char *who, int G, const int *cls, const int *num, const int *len, const int *first, int K,
                     AGGroups *g) {
    PDM_REQUIRE(G >= 0 && G <= AG_MAXG, PDM_E_TOOLARGE, "%s: %d sample groups (at most %d)", who, G, AG_MAXG);
    PDM_REQUIRE(G == 0 || (cls && num), PDM_E_BADARG, "%s: null group array", who);
    *g = AGGroups{};
    g->n = G;
    int slot = 0;
    for (int t = 0; t < G; ++t) {
        PDM_REQUIRE(cls[t] >= 0 && num[t] >= 1, PDM_E_BADARG, "%s: group %d: class %d, sample_num %d", who, t, cls[t], num[t]);
        g->cls[t] = cls[t];
        g->num[t] = num[t];
        g->len[t] = len ? len[t] : 0;
        g->first[t] = first ? first[t] : 0;
        PDM_REQUIRE(!len || (len[t] >= 1 && len[t] <= (1 << 30)), PDM_E_BADARG, "%s: group %d has %d database entries", who, t,
                    len ? len[t] : 0);
        PDM_REQUIRE(!first || first[t] >= 0, PDM_E_BADARG, "%s: group %d: first entry %d", who, t, first ? first[t] : 0);
        g->slot[t] = slot;
        slot += num[t];
    }
    PDM_REQUIRE(slot == K, PDM_E_BADARG, "%s: K=%d but the groups' sample numbers sum to %d", who, K, slot);
    return 0;
}

static int ag_world_args(const char *who, unsigned ops, const float *range, const float *extra, AGWorld *wd) {
    PDM_REQUIRE(range, PDM_E_BADARG, "%s: null point_cloud_range", who);
    for (int k = 0; k < 8; ++k) {
        const unsigned op = (ops >> (4 * k)) & 15u;
        PDM_REQUIRE(op <= 4u && (k < 4 || op == 0u), PDM_E_BADARG, "%s: bad transform list 0x%x", who, ops);
    }
    wd->ops = ops;
    for (int k = 0; k < 6; ++k) wd->range[k] = range[k];
    for (int k = 0; k < 3; ++k) wd->extra[k] = extra ? extra[k] : 0.f;
    return 0;
}

}  // namespace pdm

using namespace pdm;

extern "C" size_t pdm_augment_workspace_bytes(int B, int K) {
    if (B < 0 || B > AG_MAXB || K < 0 || K > AG_MAXK) return 0;
    return ag_layout(B, K).total;
}

extern "C" int pdm_augment_draw(void *stream, int B, int G, const int *group_class, const int *group_num,
                                const int *group_len, const int *group_first, int limit_whole_scene, int M,
                                const float *gt_boxes, unsigned seed, int *state, int flip_axes, int use_rot, float rot_lo,
                                float rot_hi, int use_scale, float scale_lo, float scale_hi, int K, int *sampled, int *flip,
                                float *angle, float *scale, void *workspace, size_t workspace_bytes) {
    PDM_REQUIRE(B >= 0 && M >= 0 && K >= 0 && flip_axes >= 0 && flip_axes <= 3, PDM_E_BADARG,
                "augment_draw: B=%d M=%d K=%d flip_axes=%d", B, M, K, flip_axes);
    PDM_REQUIRE(B <= AG_MAXB && M <= AG_MAXM && K <= AG_MAXK, PDM_E_TOOLARGE, "augment_draw: B=%d M=%d K=%d (limits %d, %d, %d)",
                B, M, K, AG_MAXB, AG_MAXM, AG_MAXK);
    AGGroups g;
    int rc = ag_groups("augment_draw", G, group_class, group_num, group_len, group_first, K, &g);
    if (rc) return rc;
    PDM_REQUIRE(G == 0 || (group_len && group_first), PDM_E_BADARG, "augment_draw: null group array");
    if (B == 0) return 0;
    PDM_REQUIRE(state && flip && angle && scale && (K == 0 || sampled) && (M == 0 || gt_boxes) && workspace, PDM_E_BADARG,
                "augment_draw: null pointer");
    const AGLayout l = ag_layout(B, K);
    PDM_REQUIRE(workspace_bytes >= l.total, PDM_E_BADARG, "augment_draw: workspace %zu < %zu bytes", workspace_bytes, l.total);
    PDM_WS_ALIGNED("augment_draw", workspace);
    int *walk = reinterpret_cast<int *>(static_cast<char *>(workspace) + l.walk);
    hipLaunchKernelGGL(ag_draw_kernel, dim3(1), dim3(1024), 0, as_stream(stream), B, g, limit_whole_scene ? 1 : 0, M, gt_boxes,
                       seed, state, flip_axes, use_rot ? 1 : 0, rot_lo, rot_hi, use_scale ? 1 : 0, scale_lo, scale_hi, K,
                       sampled, flip, angle, scale, walk);
    return check_launch("augment_draw");
}

extern "C" int pdm_augment_select(void *stream, int B, int M, const float *gt_boxes, int G, const int *group_class,
                                  const int *group_num, long long db_entries, const float *db_boxes,
                                  const long long *db_offsets, int K, const int *sampled, const int *flip,
                                  const float *angle, const float *scale, unsigned ops, const float *point_cloud_range,
                                  int remove_outside, int M_out, float *out_boxes, int *out_num_boxes, int *accepted,
                                  int *num_accepted, void *workspace, size_t workspace_bytes) {
    PDM_REQUIRE(B >= 0 && M >= 0 && K >= 0 && M_out >= 0 && db_entries >= 0, PDM_E_BADARG,
                "augment_select: B=%d M=%d K=%d M_out=%d entries=%lld", B, M, K, M_out, db_entries);
    PDM_REQUIRE(B <= AG_MAXB && M <= AG_MAXM && K <= AG_MAXK && M_out <= AG_MAXM + AG_MAXK, PDM_E_TOOLARGE,
                "augment_select: B=%d M=%d K=%d M_out=%d (limits %d, %d, %d, %d)", B, M, K, M_out, AG_MAXB, AG_MAXM, AG_MAXK,
                AG_MAXM + AG_MAXK);
    AGGroups g;
    int rc = ag_groups("augment_select", G, group_class, group_num, nullptr, nullptr, K, &g);
    if (rc) return rc;
    AGWorld wd;
    rc = ag_world_args("augment_select", ops, point_cloud_range, nullptr, &wd);
    if (rc) return rc;
    if (B == 0) return 0;
    PDM_REQUIRE(flip && angle && scale && out_num_boxes && num_accepted && workspace && (M == 0 || gt_boxes) &&
                (M_out == 0 || out_boxes) && (K == 0 || (sampled && accepted && db_boxes && db_offsets)),
                PDM_E_BADARG, "augment_select: null pointer");
    const AGLayout l = ag_layout(B, K);
    PDM_REQUIRE(workspace_bytes >= l.total, PDM_E_BADARG, "augment_select: workspace %zu < %zu bytes", workspace_bytes, l.total);
    PDM_WS_ALIGNED("augment_select", workspace);
    AGSelect a;
    a.B = B; a.M = M; a.K = K; a.M_out = M_out; a.remove_outside = remove_outside ? 1 : 0;
    a.db_entries = db_entries;
    a.gt = gt_boxes; a.db_boxes = db_boxes; a.db_off = db_offsets;
    a.sampled = sampled; a.flip = flip; a.angle = angle; a.scale = scale;
    a.out_boxes = out_boxes; a.out_nbox = out_num_boxes; a.accepted = accepted; a.num_accepted = num_accepted;
    a.obj_off = reinterpret_cast<int *>(static_cast<char *>(workspace) + l.obj_off);
    hipLaunchKernelGGL(ag_select_kernel, dim3(B), dim3(AG_THREADS), 0, as_stream(stream), a, g, wd);
    return check_launch("augment_select");
}

static int ag_scene_args(const char *who, int B, int C, const float *raw, const int *counts, const float *db_points,
                         const long long *db_offsets, const float *db_boxes, int K, const int *accepted,
                         const int *num_accepted, const int *flip, const float *angle, const float *scale, unsigned ops,
                         const float *point_cloud_range, const float *extra_width, long long capacity, int *out_counts,
                         int *overflow, float *out_rows, void *workspace, size_t workspace_bytes, AGScene *a, AGWorld *wd) {
    PDM_REQUIRE(B >= 0 && K >= 0 && C >= 3 && C <= 16 && capacity >= 0, PDM_E_BADARG, "%s: B=%d K=%d C=%d capacity=%lld", who, B,
                K, C, capacity);
    PDM_REQUIRE(B <= AG_MAXB && K <= AG_MAXK, PDM_E_TOOLARGE, "%s: B=%d K=%d (limits %d, %d)", who, B, K, AG_MAXB, AG_MAXK);
    int rc = ag_world_args(who, ops, point_cloud_range, extra_width, wd);
    if (rc) return rc;
    PDM_REQUIRE(extra_width, PDM_E_BADARG, "%s: null extra width", who);
    if (B == 0) return 0;
    PDM_REQUIRE(raw && counts && flip && angle && scale && num_accepted && out_counts && overflow && workspace &&
                (K == 0 || (accepted && db_points && db_offsets && db_boxes)),
                PDM_E_BADARG, "%s: null pointer", who);
    const AGLayout l = ag_layout(B, K);
    PDM_REQUIRE(workspace_bytes >= l.total, PDM_E_BADARG, "%s: workspace %zu < %zu bytes", who, workspace_bytes, l.total);
    PDM_WS_ALIGNED(who, workspace);
    char *ws = static_cast<char *>(workspace);
    a->B = B; a->C = C; a->K = K; a->W = ag_segments(B); a->capacity = capacity;
    a->raw = raw; a->counts = counts; a->db_pts = db_points; a->db_boxes = db_boxes; a->db_off = db_offsets;
    a->accepted = accepted; a->num_accepted = num_accepted; a->flip = flip; a->angle = angle; a->scale = scale;
    a->obj_off = reinterpret_cast<int *>(ws + l.obj_off);
    a->seg_count = reinterpret_cast<int *>(ws + l.seg_count);
    a->seg_base = reinterpret_cast<int *>(ws + l.seg_base);
    a->scene_off = reinterpret_cast<long long *>(ws + l.scene_off);
    a->out_counts = out_counts; a->overflow = overflow; a->out = out_rows;
    return 0;
}

extern "C" int pdm_augment_scene_count(void *stream, int B, int C, const float *raw, const int *counts,
                                       const float *db_points, const long long *db_offsets, const float *db_boxes, int K,
                                       const int *accepted, const int *num_accepted, const int *flip, const float *angle,
                                       const float *scale, unsigned ops, const float *point_cloud_range,
                                       const float *extra_width, long long capacity, int *out_counts, int *overflow,
                                       float *out_rows, void *workspace, size_t workspace_bytes) {
    AGScene a;
    AGWorld wd;
    const int rc = ag_scene_args("augment_scene_count", B, C, raw, counts, db_points, db_offsets, db_boxes, K, accepted,
                                 num_accepted, flip, angle, scale, ops, point_cloud_range, extra_width, capacity, out_counts,
                                 overflow, out_rows, workspace, workspace_bytes, &a, &wd);
    if (rc || B == 0) return rc;
    hipLaunchKernelGGL(ag_count_kernel, dim3(a.W, B), dim3(AG_THREADS), 0, as_stream(stream), a, wd);
    int e = check_launch("augment_scene_count(count)");
    if (e) return e;
    return segment_scan_launch(stream, "augment_scene_count(scan)", B, a.W, a.seg_count, a.seg_base, a.out_counts, a.scene_off,
                               a.overflow, a.capacity);
}

extern "C" int pdm_augment_scene_fill(void *stream, int B, int C, const float *raw, const int *counts,
                                      const float *db_points, const long long *db_offsets, const float *db_boxes, int K,
                                      const int *accepted, const int *num_accepted, const int *flip, const float *angle,
                                      const float *scale, unsigned ops, const float *point_cloud_range,
                                      const float *extra_width, long long capacity, int *out_counts, int *overflow,
                                      float *out_rows, void *workspace, size_t workspace_bytes) {
    AGScene a;
    AGWorld wd;
    const int rc = ag_scene_args("augment_scene_fill", B, C, raw, counts, db_points, db_offsets, db_boxes, K, accepted,
                                 num_accepted, flip, angle, scale, ops, point_cloud_range, extra_width, capacity, out_counts,
                                 overflow, out_rows, workspace, workspace_bytes, &a, &wd);
    if (rc || B == 0) return rc;
    PDM_REQUIRE(capacity == 0 || out_rows, PDM_E_BADARG, "augment_scene_fill: null output rows");
    hipLaunchKernelGGL(ag_fill_kernel, dim3(a.W, B), dim3(AG_THREADS), 0, as_stream(stream), a, wd);
    return check_launch("augment_scene_fill");
}

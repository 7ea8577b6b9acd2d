// KITTI dataset front end on the device: the per-point work of the reference's
// KittiDataset.get_infos / create_groundtruth_database / __getitem__ (pcdet/datasets/kitti/kitti_dataset.py:124-139,
// :150-275, :371-428) for a whole batch of ragged frames resident in HBM.
//
// Frames are packed as the augmentor takes them: raw (sum N_i, C) fp32 rows, counts (B) int32; frame b starts at row
// counts[0] + ... + counts[b - 1].  Calibration is per frame: V2C (B, 3, 4), R0 (B, 3, 3), P2 (B, 3, 4) fp32,
// image_shape (B, 2) int32 [height, width].
//
// FOV flag (get_fov_flag o rect_to_img o lidar_to_rect, calibration_kitti.py:65-84).  The reference does this in fp32
// through BLAS, whose summation order is not defined; here it is done in double from the fp32 inputs, every product and
// sum rounded once (__dmul_rn / __dadd_rn, nothing fused), in this order:
//   cam_j  = ((V2C[j][0] x + V2C[j][1] y) + V2C[j][2] z) + V2C[j][3]              j = 0, 1, 2
//   rect_i = (R0[i][0] cam_0 + R0[i][1] cam_1) + R0[i][2] cam_2                   i = 0, 1, 2
//   hom_k  = ((P2[k][0] rect_0 + P2[k][1] rect_1) + P2[k][2] rect_2) + P2[k][3]   k = 0, 1, 2
//   u = hom_0 / rect_2,  v = hom_1 / rect_2,  depth = hom_2 - P2[2][3]
//   keep  <=>  u >= 0 and u < width and v >= 0 and v < height and depth >= 0      (a NaN compares false)
//
// Box membership, two rules (DESIGN.md says why there are two):
//   hull   (num_points_in_gt of the infos; box_utils.in_hull on boxes_to_corners_3d): the exact oriented box without a
//          margin, in double on the fp32 box: X = x - cx, Y = y - cy, Z = z - cz; c = cos(h), s = sin(h) in double;
//          lx = X c + Y s, ly = Y c - X s; inside <=> |lx| <= dx / 2 and |ly| <= dy / 2 and |Z| <= dz / 2.  Counted over the
//          points inside the FOV only.
//   margin (the database; points_in_boxes_cpu, roiaware_pool3d.cpp:121-140): box_geometry.h's point_in_box_margin, the
//          very function the augmentation's point removal calls.  Counted and gathered over all points.
// Object points are written relative to the float64 box centre: fp32(double(x) - centre_x), rounded once.
//
// Every pass is count -> scan -> fill.  The unit of work is one wave (64 lanes) over one contiguous segment of a frame:
// the in-wave prefix is a ballot and a popcount, the per-(frame, segment[, box]) counts go to fixed workspace slots and are
// folded in slot order.  No atomics, no memset: every output entry is written by a kernel, two runs give the same bits
// and a captured graph replays them exactly.
#include "box_geometry.h"

namespace pdm {

constexpr int KD_MAXB = 1024;      // frames per call
constexpr int KD_MAXM = 256;       // boxes per frame (augment.py's MAX_BOXES)
constexpr int KD_THREADS = 256;
constexpr int KD_WAVES = KD_THREADS / 64;

struct KDCalib {
    double V[12], R[9], P[12];
    double w, h;
};

struct KDFrames {
    int B, C, S;                 // S wave segments per frame
    long long total_rows;        // rows of raw: nothing is read at or past it
    const float *raw;
    const int *counts;
    const float *V2C, *R0, *P2;
    const int *shape;
};

__device__ __forceinline__ KDCalib kd_calib(const KDFrames &f, int b) {
    KDCalib c;
    for (int k = 0; k < 12; ++k) c.V[k] = (double)f.V2C[(size_t)b * 12 + k];
    for (int k = 0; k < 9; ++k) c.R[k] = (double)f.R0[(size_t)b * 9 + k];
    for (int k = 0; k < 12; ++k) c.P[k] = (double)f.P2[(size_t)b * 12 + k];
    c.h = (double)f.shape[2 * b];
    c.w = (double)f.shape[2 * b + 1];
    return c;
}

__device__ __forceinline__ double kd_dot3(const double *m, double a, double b, double c) {
    return __dadd_rn(__dadd_rn(__dmul_rn(m[0], a), __dmul_rn(m[1], b)), __dmul_rn(m[2], c));
}

__device__ __forceinline__ bool kd_in_fov(const KDCalib &c, float xf, float yf, float zf) {
    const double x = (double)xf, y = (double)yf, z = (double)zf;
    double cam[3], rect[3], hom[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) cam[j] = __dadd_rn(kd_dot3(c.V + 4 * j, x, y, z), c.V[4 * j + 3]);
#pragma unroll
    for (int i = 0; i < 3; ++i) rect[i] = kd_dot3(c.R + 3 * i, cam[0], cam[1], cam[2]);
#pragma unroll
    for (int k = 0; k < 3; ++k) hom[k] = __dadd_rn(kd_dot3(c.P + 4 * k, rect[0], rect[1], rect[2]), c.P[4 * k + 3]);
    const double u = __ddiv_rn(hom[0], rect[2]), v = __ddiv_rn(hom[1], rect[2]);
    const double depth = __dsub_rn(hom[2], c.P[11]);
    return u >= 0.0 && u < c.w && v >= 0.0 && v < c.h && depth >= 0.0;
}

__device__ __forceinline__ bool kd_in_hull(float px, float py, float pz, const float *bx, double c, double s) {
    const double X = (double)px - (double)bx[0], Y = (double)py - (double)bx[1], Z = (double)pz - (double)bx[2];
    const double lx = __dadd_rn(__dmul_rn(X, c), __dmul_rn(Y, s));
    const double ly = __dsub_rn(__dmul_rn(Y, c), __dmul_rn(X, s));
    return fabs(lx) <= (double)bx[3] / 2.0 && fabs(ly) <= (double)bx[4] / 2.0 && fabs(Z) <= (double)bx[5] / 2.0;
}

// first row and number of rows of frame b, clipped so that no row at or past total_rows is ever touched
__device__ __forceinline__ void kd_frame(const KDFrames &f, int b, long long *start, int *n) {
    long long s = 0;
    for (int k = 0; k < b; ++k) s += max(f.counts[k], 0);
    long long c = max(f.counts[b], 0);
    if (s > f.total_rows) s = f.total_rows;
    if (s + c > f.total_rows) c = f.total_rows - s;
    *start = s;
    *n = (int)c;
}

// segment `seg` of S over n rows: whole chunks of 64 rows, so that a wave's loads stay aligned
__device__ __forceinline__ void kd_segment(int n, int S, int seg, int *r0, int *r1) {
    const int per = ((n + S - 1) / S + 63) & ~63;
    *r0 = (int)min((long long)n, (long long)seg * per);
    *r1 = (int)min((long long)n, (long long)*r0 + per);
}

__device__ __forceinline__ void kd_xyz(const float *row, int C, float &x, float &y, float &z, float &w) {
    if (C == 4) {
        const float4 v = *reinterpret_cast<const float4 *>(row);   // one 16 B load per point
        x = v.x; y = v.y; z = v.z; w = v.w;
    } else {
        x = row[0]; y = row[1]; z = row[2]; w = 0.f;
    }
}

// ---- FOV crop ----------------------------------------------------------------------------------------------------------
struct KDFov {
    KDFrames f;
    long long capacity;
    int *seg_count, *seg_base;      // (B, S)
    long long *frame_off;           // (B + 1)
    int *out_counts, *overflow;
    unsigned char *flags;           // (total_rows) or null
    float *out;
};

__global__ __launch_bounds__(KD_THREADS) void kd_fov_count_kernel(KDFov a) {
    const int b = blockIdx.y, lane = threadIdx.x & 63, seg = blockIdx.x * KD_WAVES + (threadIdx.x >> 6);
    const KDCalib cal = kd_calib(a.f, b);
    long long start;
    int n, r0, r1;
    kd_frame(a.f, b, &start, &n);
    kd_segment(n, a.f.S, seg, &r0, &r1);
    int cnt = 0;
    for (int c0 = r0; c0 < r1; c0 += 64) {
        const int r = c0 + lane;
        bool keep = false;
        if (r < r1) {
            float x, y, z, w;
            kd_xyz(a.f.raw + (size_t)(start + r) * a.f.C, a.f.C, x, y, z, w);
            keep = kd_in_fov(cal, x, y, z);
            if (a.flags) a.flags[start + r] = keep ? 1 : 0;
        }
        cnt += __popcll(__ballot(keep));
    }
    if (lane == 0) a.seg_count[(size_t)b * a.f.S + seg] = cnt;
}

__global__ __launch_bounds__(KD_THREADS) void kd_fov_fill_kernel(KDFov a) {
    const int b = blockIdx.y, lane = threadIdx.x & 63, seg = blockIdx.x * KD_WAVES + (threadIdx.x >> 6);
    const KDCalib cal = kd_calib(a.f, b);
    long long start;
    int n, r0, r1;
    kd_frame(a.f, b, &start, &n);
    kd_segment(n, a.f.S, seg, &r0, &r1);
    const int C = a.f.C;
    long long pos = a.frame_off[b] + a.seg_base[(size_t)b * a.f.S + seg];
    for (int c0 = r0; c0 < r1; c0 += 64) {
        const int r = c0 + lane;
        bool keep = false;
        float x = 0.f, y = 0.f, z = 0.f, w = 0.f;
        const float *src = a.f.raw + (size_t)(start + min(r, r1 - 1)) * C;
        if (r < r1) {
            kd_xyz(src, C, x, y, z, w);
            keep = kd_in_fov(cal, x, y, z);
        }
        const unsigned long long mask = __ballot(keep);
        const long long p = pos + lanes_below(mask, lane);
        if (keep && p < a.capacity) {
            float *o = a.out + (size_t)p * C;
            if (C == 4) {
                *reinterpret_cast<float4 *>(o) = make_float4(x, y, z, w);
            } else {
                o[0] = x; o[1] = y; o[2] = z;
                for (int k = 3; k < C; ++k) o[k] = src[k];
            }
        }
        pos += __popcll(mask);
    }
}

// ---- box membership: num_points_in_gt and the ground-truth database ------------------------------------------------------
struct KDBoxes {
    KDFrames f;
    int M;
    const float *boxes;             // (B, M, 7) fp32
    const int *box_count;           // (B)
    const double *centres;          // (B, M, 3) float64 (fill only)
    int *seg_hull, *seg_db;         // (B, S, M) per-segment counts
    int *seg_base;                  // (B, S, M) exclusive prefix of seg_db over the segments
    int *within;                    // (B, M) exclusive prefix of the database counts over the frame's boxes
    long long *frame_tot;           // (B) database points of the frame
    long long *frame_off;           // (B) first database point of the frame
    int *entry_start;               // (B) first database entry of the frame
    int *num_in_gt, *db_count;      // (B, M) outputs
    long long *totals;              // [points P, entries N]
    long long cap_points, cap_entries;
    float *out_points;              // (P, C)
    long long *out_offsets;         // (N + 1)
    float *out_boxes;               // (N, 7)
};

struct KDBoxLds {
    float box[KD_MAXM * 7];
    float cs[KD_MAXM * 2];          // box_cos_sin(-heading): the margin rule's rotation
    float lim2[KD_MAXM];
    double dcs[KD_MAXM * 2];        // cos / sin of the heading in double: the hull rule's rotation
};

__device__ __forceinline__ int kd_stage_boxes(const KDBoxes &a, KDBoxLds &L, int b) {
    const int nb = min(max(a.box_count[b], 0), a.M);
    for (int k = threadIdx.x; k < nb; k += KD_THREADS) {
        float *bx = L.box + k * 7;
        for (int f = 0; f < 7; ++f) bx[f] = a.boxes[((size_t)b * a.M + k) * 7 + f];
        float c, s;
        box_cos_sin(-bx[6], &c, &s);
        L.cs[2 * k] = c;
        L.cs[2 * k + 1] = s;
        L.lim2[k] = box_reach2(bx);
        L.dcs[2 * k] = cos((double)bx[6]);
        L.dcs[2 * k + 1] = sin((double)bx[6]);
    }
    __syncthreads();
    return nb;
}

__global__ __launch_bounds__(KD_THREADS) void kd_box_count_kernel(KDBoxes a) {
    __shared__ KDBoxLds L;
    const int b = blockIdx.y, lane = threadIdx.x & 63, seg = blockIdx.x * KD_WAVES + (threadIdx.x >> 6);
    const int nb = kd_stage_boxes(a, L, b);
    const KDCalib cal = kd_calib(a.f, b);
    long long start;
    int n, r0, r1;
    kd_frame(a.f, b, &start, &n);
    kd_segment(n, a.f.S, seg, &r0, &r1);
    int ch[KD_MAXM / 64] = {0, 0, 0, 0}, cd[KD_MAXM / 64] = {0, 0, 0, 0};   // lane l holds boxes l, l + 64, ...
    for (int c0 = r0; c0 < r1; c0 += 64) {
        const int r = c0 + lane;
        const bool valid = r < r1;
        float x = 0.f, y = 0.f, z = 0.f, w = 0.f;
        bool fov = false;
        if (valid) {
            kd_xyz(a.f.raw + (size_t)(start + r) * a.f.C, a.f.C, x, y, z, w);
            fov = kd_in_fov(cal, x, y, z);
        }
#pragma unroll
        for (int j = 0; j < KD_MAXM / 64; ++j) {
            for (int kk = 0; kk < 64 && j * 64 + kk < nb; ++kk) {
                const int k = j * 64 + kk;
                const float *bx = L.box + k * 7;       // the same address in every lane: an LDS broadcast
                const float dx = x - bx[0], dy = y - bx[1];
                const bool near = valid && !(dx * dx + dy * dy > L.lim2[k]);
                if (__ballot(near) == 0ull) continue;
                const bool in_db = near && point_in_box_margin(dx, dy, z, bx, L.cs[2 * k], L.cs[2 * k + 1]);
                const bool in_hull = near && fov && kd_in_hull(x, y, z, bx, L.dcs[2 * k], L.dcs[2 * k + 1]);
                const int nd = __popcll(__ballot(in_db)), nh = __popcll(__ballot(in_hull));
                if (lane == kk) { cd[j] += nd; ch[j] += nh; }
            }
        }
    }
#pragma unroll
    for (int j = 0; j < KD_MAXM / 64; ++j) {
        const int k = j * 64 + lane;
        if (k < a.M) {
            const size_t slot = ((size_t)b * a.f.S + seg) * a.M + k;
            a.seg_hull[slot] = ch[j];
            a.seg_db[slot] = cd[j];
        }
    }
}

// per frame: fold the segments' counts in segment order, then the exclusive prefix over the frame's boxes
__global__ __launch_bounds__(KD_THREADS) void kd_box_fold_kernel(KDBoxes a) {
    __shared__ int s[KD_THREADS];
    const int b = blockIdx.x, k = threadIdx.x;
    const int nb = min(max(a.box_count[b], 0), a.M);
    int h = 0, d = 0;
    if (k < a.M) {
        for (int w = 0; w < a.f.S; ++w) {
            const size_t slot = ((size_t)b * a.f.S + w) * a.M + k;
            a.seg_base[slot] = d;
            d += a.seg_db[slot];
            h += a.seg_hull[slot];
        }
        if (k >= nb) { h = 0; d = 0; }
        a.num_in_gt[(size_t)b * a.M + k] = h;
        a.db_count[(size_t)b * a.M + k] = d;
    }
    s[k] = d;
    __syncthreads();
    for (int off = 1; off < KD_THREADS; off <<= 1) {
        const int v = k >= off ? s[k - off] : 0;
        __syncthreads();
        s[k] += v;
        __syncthreads();
    }
    if (k < a.M) a.within[(size_t)b * a.M + k] = s[k] - d;
    if (k == 0) a.frame_tot[b] = s[KD_THREADS - 1];
}

__global__ __launch_bounds__(1024) void kd_box_scan_kernel(KDBoxes a) {
    __shared__ long long sp[1024];
    __shared__ int se[1024];
    const int b = threadIdx.x;
    const long long tot = b < a.f.B ? a.frame_tot[b] : 0;
    const int nb = b < a.f.B ? min(max(a.box_count[b], 0), a.M) : 0;
    sp[b] = tot;
    se[b] = nb;
    __syncthreads();
    for (int off = 1; off < 1024; off <<= 1) {
        const long long v = b >= off ? sp[b - off] : 0;
        const int e = b >= off ? se[b - off] : 0;
        __syncthreads();
        sp[b] += v;
        se[b] += e;
        __syncthreads();
    }
    if (b < a.f.B) {
        a.frame_off[b] = sp[b] - tot;
        a.entry_start[b] = se[b] - nb;
    }
    if (b == 0) {
        a.totals[0] = sp[1023];
        a.totals[1] = se[1023];
    }
}

__global__ __launch_bounds__(KD_THREADS) void kd_box_fill_kernel(KDBoxes a) {
    __shared__ KDBoxLds L;
    const int b = blockIdx.y, lane = threadIdx.x & 63, seg = blockIdx.x * KD_WAVES + (threadIdx.x >> 6);
    const int nb = kd_stage_boxes(a, L, b);
    long long start;
    int n, r0, r1;
    kd_frame(a.f, b, &start, &n);
    kd_segment(n, a.f.S, seg, &r0, &r1);
    const int C = a.f.C;
    const long long foff = a.frame_off[b];
    const int e0 = a.entry_start[b];
    if (blockIdx.x == 0) {            // the frame's rows of offsets / boxes
        for (int k = threadIdx.x; k < nb; k += KD_THREADS) {
            const long long e = (long long)e0 + k;
            if (e < a.cap_entries) {
                a.out_offsets[e] = foff + a.within[(size_t)b * a.M + k];
                for (int f = 0; f < 7; ++f) a.out_boxes[e * 7 + f] = L.box[k * 7 + f];
            }
        }
        if (b == a.f.B - 1 && threadIdx.x == 0 && (long long)e0 + nb <= a.cap_entries)
            a.out_offsets[(long long)e0 + nb] = foff + a.frame_tot[b];
    }
    long long run[KD_MAXM / 64];      // lane l: next output row of boxes l, l + 64, ...
#pragma unroll
    for (int j = 0; j < KD_MAXM / 64; ++j) {
        const int k = j * 64 + lane;
        run[j] = k < nb ? foff + a.within[(size_t)b * a.M + k] + a.seg_base[((size_t)b * a.f.S + seg) * a.M + k] : 0;
    }
    for (int c0 = r0; c0 < r1; c0 += 64) {
        const int r = c0 + lane;
        const bool valid = r < r1;
        float x = 0.f, y = 0.f, z = 0.f, w = 0.f;
        const float *src = a.f.raw + (size_t)(start + min(r, r1 - 1)) * C;
        if (valid) kd_xyz(src, C, x, y, z, w);
#pragma unroll
        for (int j = 0; j < KD_MAXM / 64; ++j) {
            for (int kk = 0; kk < 64 && j * 64 + kk < nb; ++kk) {
                const int k = j * 64 + kk;
                const float *bx = L.box + k * 7;
                const float dx = x - bx[0], dy = y - bx[1];
                const bool near = valid && !(dx * dx + dy * dy > L.lim2[k]);
                if (__ballot(near) == 0ull) continue;
                const bool in_db = near && point_in_box_margin(dx, dy, z, bx, L.cs[2 * k], L.cs[2 * k + 1]);
                const unsigned long long mask = __ballot(in_db);
                if (mask == 0ull) continue;
                const long long p = __shfl(run[j], kk, 64) + lanes_below(mask, lane);
                if (in_db && p < a.cap_points) {
                    const double *ctr = a.centres + ((size_t)b * a.M + k) * 3;
                    float *o = a.out_points + (size_t)p * C;
                    const float ox = (float)__dsub_rn((double)x, ctr[0]);
                    const float oy = (float)__dsub_rn((double)y, ctr[1]);
                    const float oz = (float)__dsub_rn((double)z, ctr[2]);
                    if (C == 4) {
                        *reinterpret_cast<float4 *>(o) = make_float4(ox, oy, oz, w);
                    } else {
                        o[0] = ox; o[1] = oy; o[2] = oz;
                        for (int f = 3; f < C; ++f) o[f] = src[f];
                    }
                }
                if (lane == kk) run[j] += __popcll(mask);
            }
        }
    }
}

static int kd_segments(int B) { return KD_WAVES * max(1, min(64, 2048 / max(B, 1))); }

struct KDFovLayout { size_t seg_count, seg_base, frame_off, total; };

static KDFovLayout kd_fov_layout(int B) {
    KDFovLayout l;
    const size_t S = kd_segments(B);
    size_t o = 0;
    l.seg_count = o; o += align256((size_t)B * S * sizeof(int));
    l.seg_base = o; o += align256((size_t)B * S * sizeof(int));
    l.frame_off = o; o += align256((size_t)(B + 1) * sizeof(long long));
    l.total = o;
    return l;
}

struct KDBoxLayout { size_t seg_hull, seg_db, seg_base, within, frame_tot, frame_off, entry_start, total; };

static KDBoxLayout kd_box_layout(int B, int M) {
    KDBoxLayout l;
    const size_t S = kd_segments(B), slots = (size_t)B * S * M * sizeof(int);
    size_t o = 0;
    l.seg_hull = o; o += align256(slots);
    l.seg_db = o; o += align256(slots);
    l.seg_base = o; o += align256(slots);
    l.within = o; o += align256((size_t)B * M * sizeof(int));
    l.frame_tot = o; o += align256((size_t)B * sizeof(long long));
    l.frame_off = o; o += align256((size_t)B * sizeof(long long));
    l.entry_start = o; o += align256((size_t)B * sizeof(int));
    l.total = o;
    return l;
}

static int kd_frames_args(const char *who, int B, int C, long long total_rows, const float *raw, const int *counts,
                          const float *V2C, const float *R0, const float *P2, const int *image_shape, KDFrames *f) {
    PDM_REQUIRE(B >= 0 && C >= 3 && C <= 16 && total_rows >= 0, PDM_E_BADARG, "%s: B=%d C=%d rows=%lld", who, B, C, total_rows);
    PDM_REQUIRE(B <= KD_MAXB, PDM_E_TOOLARGE, "%s: B=%d (at most %d frames)", who, B, KD_MAXB);
    if (B == 0) return 0;
    PDM_REQUIRE(counts && V2C && R0 && P2 && image_shape && (total_rows == 0 || raw), PDM_E_BADARG, "%s: null pointer", who);
    PDM_REQUIRE(C != 4 || (reinterpret_cast<uintptr_t>(raw) & 15) == 0, PDM_E_BADARG, "%s: rows of 4 floats must be 16 B aligned",
                who);
    f->B = B; f->C = C; f->S = kd_segments(B); f->total_rows = total_rows;
    f->raw = raw; f->counts = counts; f->V2C = V2C; f->R0 = R0; f->P2 = P2; f->shape = image_shape;
    return 0;
}

static int kd_fov_args(const char *who, int B, int C, long long total_rows, const float *raw, const int *counts,
                       const float *V2C, const float *R0, const float *P2, const int *image_shape, long long capacity,
                       int *out_counts, int *overflow, void *workspace, size_t workspace_bytes, KDFov *a) {
    const int rc = kd_frames_args(who, B, C, total_rows, raw, counts, V2C, R0, P2, image_shape, &a->f);
    if (rc || B == 0) return rc;
    PDM_REQUIRE(capacity >= 0, PDM_E_BADARG, "%s: capacity=%lld", who, capacity);
    PDM_REQUIRE(out_counts && overflow && workspace, PDM_E_BADARG, "%s: null pointer", who);
    const KDFovLayout l = kd_fov_layout(B);
    PDM_REQUIRE(workspace_bytes >= l.total, PDM_E_BADARG, "%s: workspace %zu < %zu bytes", who, workspace_bytes, l.total);
    PDM_WS_ALIGNED(who, workspace);
    char *ws = static_cast<char *>(workspace);
    a->capacity = capacity;
    a->seg_count = reinterpret_cast<int *>(ws + l.seg_count);
    a->seg_base = reinterpret_cast<int *>(ws + l.seg_base);
    a->frame_off = reinterpret_cast<long long *>(ws + l.frame_off);
    a->out_counts = out_counts; a->overflow = overflow;
    a->flags = nullptr; a->out = nullptr;
    return 0;
}

static int kd_box_args(const char *who, int B, int C, long long total_rows, const float *raw, const int *counts,
                       const float *V2C, const float *R0, const float *P2, const int *image_shape, int M, const float *boxes,
                       const int *box_count, int *num_points_in_gt, int *db_count, long long *totals, void *workspace,
                       size_t workspace_bytes, KDBoxes *a) {
    PDM_REQUIRE(M >= 0, PDM_E_BADARG, "%s: M=%d", who, M);
    PDM_REQUIRE(M <= KD_MAXM, PDM_E_TOOLARGE, "%s: M=%d (at most %d boxes per frame)", who, M, KD_MAXM);
    const int rc = kd_frames_args(who, B, C, total_rows, raw, counts, V2C, R0, P2, image_shape, &a->f);
    if (rc || B == 0) return rc;
    PDM_REQUIRE(box_count && totals && workspace && (M == 0 || (boxes && num_points_in_gt && db_count)), PDM_E_BADARG,
                "%s: null pointer", who);
    const KDBoxLayout l = kd_box_layout(B, M);
    PDM_REQUIRE(workspace_bytes >= l.total, PDM_E_BADARG, "%s: workspace %zu < %zu bytes", who, workspace_bytes, l.total);
    PDM_WS_ALIGNED(who, workspace);
    char *ws = static_cast<char *>(workspace);
    a->M = M; a->boxes = boxes; a->box_count = box_count; a->centres = nullptr;
    a->seg_hull = reinterpret_cast<int *>(ws + l.seg_hull);
    a->seg_db = reinterpret_cast<int *>(ws + l.seg_db);
    a->seg_base = reinterpret_cast<int *>(ws + l.seg_base);
    a->within = reinterpret_cast<int *>(ws + l.within);
    a->frame_tot = reinterpret_cast<long long *>(ws + l.frame_tot);
    a->frame_off = reinterpret_cast<long long *>(ws + l.frame_off);
    a->entry_start = reinterpret_cast<int *>(ws + l.entry_start);
    a->num_in_gt = num_points_in_gt; a->db_count = db_count; a->totals = totals;
    a->cap_points = 0; a->cap_entries = 0;
    a->out_points = nullptr; a->out_offsets = nullptr; a->out_boxes = nullptr;
    return 0;
}

}  // namespace pdm

using namespace pdm;

extern "C" size_t pdm_kitti_data_fov_workspace_bytes(int B) {
    if (B < 0 || B > KD_MAXB) return 0;
    return kd_fov_layout(B).total;
}

extern "C" size_t pdm_kitti_data_boxes_workspace_bytes(int B, int M) {
    if (B < 0 || B > KD_MAXB || M < 0 || M > KD_MAXM) return 0;
    return kd_box_layout(B, M).total;
}

extern "C" int pdm_kitti_data_fov_count(void *stream, int B, int C, long long total_rows, const float *raw, const int *counts,
                                        const float *V2C, const float *R0, const float *P2, const int *image_shape,
                                        long long capacity, int *out_counts, int *overflow, unsigned char *flags,
                                        void *workspace, size_t workspace_bytes) {
    KDFov a;
    const int rc = kd_fov_args("kitti_data_fov_count", B, C, total_rows, raw, counts, V2C, R0, P2, image_shape, capacity,
                               out_counts, overflow, workspace, workspace_bytes, &a);
    if (rc || B == 0) return rc;
    a.flags = flags;
    hipLaunchKernelGGL(kd_fov_count_kernel, dim3(a.f.S / KD_WAVES, B), dim3(KD_THREADS), 0, as_stream(stream), a);
    const int e = check_launch("kitti_data_fov_count(count)");
    if (e) return e;
    return segment_scan_launch(stream, "kitti_data_fov_count(scan)", B, a.f.S, a.seg_count, a.seg_base, a.out_counts, a.frame_off,
                               a.overflow, a.capacity);
}

extern "C" int pdm_kitti_data_fov_fill(void *stream, int B, int C, long long total_rows, const float *raw, const int *counts,
                                       const float *V2C, const float *R0, const float *P2, const int *image_shape,
                                       long long capacity, int *out_counts, int *overflow, float *out_rows, void *workspace,
                                       size_t workspace_bytes) {
    KDFov a;
    const int rc = kd_fov_args("kitti_data_fov_fill", B, C, total_rows, raw, counts, V2C, R0, P2, image_shape, capacity,
                               out_counts, overflow, workspace, workspace_bytes, &a);
    if (rc || B == 0) return rc;
    PDM_REQUIRE(capacity == 0 || out_rows, PDM_E_BADARG, "kitti_data_fov_fill: null output rows");
    PDM_REQUIRE(C != 4 || (reinterpret_cast<uintptr_t>(out_rows) & 15) == 0, PDM_E_BADARG,
                "kitti_data_fov_fill: rows of 4 floats must be 16 B aligned");
    a.out = out_rows;
    hipLaunchKernelGGL(kd_fov_fill_kernel, dim3(a.f.S / KD_WAVES, B), dim3(KD_THREADS), 0, as_stream(stream), a);
    return check_launch("kitti_data_fov_fill");
}

extern "C" int pdm_kitti_data_boxes_count(void *stream, int B, int C, long long total_rows, const float *raw,
                                          const int *counts, const float *V2C, const float *R0, const float *P2,
                                          const int *image_shape, int M, const float *boxes, const int *box_count,
                                          int *num_points_in_gt, int *db_count, long long *totals, void *workspace,
                                          size_t workspace_bytes) {
    KDBoxes a;
    const int rc = kd_box_args("kitti_data_boxes_count", B, C, total_rows, raw, counts, V2C, R0, P2, image_shape, M, boxes,
                               box_count, num_points_in_gt, db_count, totals, workspace, workspace_bytes, &a);
    if (rc || B == 0) return rc;
    hipLaunchKernelGGL(kd_box_count_kernel, dim3(a.f.S / KD_WAVES, B), dim3(KD_THREADS), 0, as_stream(stream), a);
    int e = check_launch("kitti_data_boxes_count(count)");
    if (e) return e;
    hipLaunchKernelGGL(kd_box_fold_kernel, dim3(B), dim3(KD_THREADS), 0, as_stream(stream), a);
    e = check_launch("kitti_data_boxes_count(fold)");
    if (e) return e;
    hipLaunchKernelGGL(kd_box_scan_kernel, dim3(1), dim3(1024), 0, as_stream(stream), a);
    return check_launch("kitti_data_boxes_count(scan)");
}

extern "C" int pdm_kitti_data_boxes_fill(void *stream, int B, int C, long long total_rows, const float *raw, const int *counts,
                                         const float *V2C, const float *R0, const float *P2, const int *image_shape, int M,
                                         const float *boxes, const int *box_count, const double *centres,
                                         int *num_points_in_gt, int *db_count, long long *totals, long long capacity_points,
                                         long long capacity_entries, float *out_points, long long *out_offsets,
                                         float *out_boxes, void *workspace, size_t workspace_bytes) {
    KDBoxes a;
    const int rc = kd_box_args("kitti_data_boxes_fill", B, C, total_rows, raw, counts, V2C, R0, P2, image_shape, M, boxes,
                               box_count, num_points_in_gt, db_count, totals, workspace, workspace_bytes, &a);
    if (rc || B == 0) return rc;
    PDM_REQUIRE(capacity_points >= 0 && capacity_entries >= 0, PDM_E_BADARG, "kitti_data_boxes_fill: capacity %lld points, %lld entries",
                capacity_points, capacity_entries);
    PDM_REQUIRE(out_offsets && (M == 0 || centres) && (capacity_points == 0 || out_points) && (capacity_entries == 0 || out_boxes),
                PDM_E_BADARG, "kitti_data_boxes_fill: null pointer");
    PDM_REQUIRE(C != 4 || (reinterpret_cast<uintptr_t>(out_points) & 15) == 0, PDM_E_BADARG,
                "kitti_data_boxes_fill: rows of 4 floats must be 16 B aligned");
    a.centres = centres;
    a.cap_points = capacity_points; a.cap_entries = capacity_entries;
    a.out_points = out_points; a.out_offsets = out_offsets; a.out_boxes = out_boxes;
    hipLaunchKernelGGL(kd_box_fill_kernel, dim3(a.f.S / KD_WAVES, B), dim3(KD_THREADS), 0, as_stream(stream), a);
    return check_launch("kitti_data_boxes_fill");
}

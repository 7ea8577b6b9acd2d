// KITTI object evaluation on the device: detections -> camera annotations -> overlaps -> the two
// statistics passes of kitti_object_eval_python/eval.py, for a whole set of frames per launch.
//
//   pdm_kitti_boxes_to_camera   lidar boxes of a padded batch -> camera box, image box, alpha (fp32, the reference's dtypes)
//   pdm_kitti_eval_overlaps     bbox / BEV / 3D overlaps of every (detection, ground truth) pair WITHIN a frame
//   pdm_kitti_eval_dt_flags     clean_data's detection flags for every (class, difficulty)
//   pdm_kitti_eval_pass1        compute_statistics_jit(compute_fp=False): true-positive scores into fixed slots
//   pdm_kitti_eval_pass2        compute_statistics_jit(compute_fp=True) for every threshold + the sums over frames
//
// A "combination" is (metric, class, difficulty, overlap set), index ((mi * nC + c) * nD + d) * K + k.  Frames are
// ragged: gt_off / dt_off (F + 1) give the box ranges, ov_off (F + 1) the start of the frame's (ndt x ngt) overlap
// block, detection-major as eval.py indexes it (overlaps[j, i]).  Nothing here uses atomics: every output element has
// one writer and the sums over frames are taken in a fixed order, so two runs give the same bits.
#include <math.h>

#include "common.h"

namespace pdm {

constexpr int KE_MAXC = 8;          // classes per call
constexpr int KE_MAXM = 3;          // metrics per call
constexpr int KE_PTS = 41;          // N_SAMPLE_PTS
constexpr int KE_MAXCOMBO = 1024;   // one thread per combination in pass 1
constexpr int KE_MAXDT = 4096;      // detections per frame (one assignment bit each, per lane, in LDS)
constexpr int KE_CHUNKS = 128;      // frame chunks of pass 2 (partial sums, folded in chunk order)
constexpr int KE_LDS = 65536;

struct KEFrames {
    int F;
    const int *gt_off, *dt_off, *ov_off;
};

struct KECombos {
    int nM, nC, nD, K;
    int metric[KE_MAXM];
};

// ---- conversion ----------------------------------------------------------------------------------------------------

__global__ void ke_to_camera_kernel(int B, int P, const float *__restrict__ boxes, const int *__restrict__ count,
                                    const float *__restrict__ V2C, const float *__restrict__ R0, const float *__restrict__ P2m,
                                    const int *__restrict__ image_shape, float *__restrict__ cam, float *__restrict__ img,
                                    float *__restrict__ alpha) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (long long)B * P) return;
    const int b = (int)(t / P), s = (int)(t % P);
    float *oc = cam + t * 7, *oi = img + t * 4;
    if (s >= count[b]) {
        for (int k = 0; k < 7; ++k) oc[k] = 0.f;
        for (int k = 0; k < 4; ++k) oi[k] = 0.f;
        alpha[t] = 0.f;
        return;
    }
    const float *bx = boxes + t * 7;
    const float *v = V2C + b * 12, *r0 = R0 + b * 9, *p2 = P2m + b * 12;
    // lidar_to_rect: [x y z 1] . (V2C^T . R0^T), with z lowered to the box bottom
    const float pl[4] = {bx[0], bx[1], bx[2] - bx[5] / 2, 1.f};
    float loc[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        float acc = 0.f;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            float m = 0.f;
#pragma unroll
            for (int k = 0; k < 3; ++k) m += v[k * 4 + i] * r0[j * 3 + k];
            acc += pl[i] * m;
        }
        loc[j] = acc;
    }
    const float l = bx[3], w = bx[4], h = bx[5];
    const float ry = -bx[6] - 1.57079632679489661923f;
    oc[0] = loc[0]; oc[1] = loc[1]; oc[2] = loc[2]; oc[3] = l; oc[4] = h; oc[5] = w; oc[6] = ry;
    const float c = cosf(ry), s_ = sinf(ry);
    const float xs[4] = {l / 2, l / 2, -l / 2, -l / 2}, zs[4] = {w / 2, -w / 2, -w / 2, w / 2};
    float u0 = INFINITY, v0 = INFINITY, u1 = -INFINITY, v1 = -INFINITY;
    for (int k = 0; k < 8; ++k) {
        const float xc = xs[k & 3], zc = zs[k & 3], yc = k < 4 ? 0.f : -h;
        const float px = loc[0] + (xc * c + zc * s_), py = loc[1] + yc, pz = loc[2] + (-xc * s_ + zc * c);
        const float uu = (px * p2[0] + py * p2[1] + pz * p2[2] + p2[3]) / pz;
        const float vv = (px * p2[4] + py * p2[5] + pz * p2[6] + p2[7]) / pz;
        u0 = fminf(u0, uu); u1 = fmaxf(u1, uu); v0 = fminf(v0, vv); v1 = fmaxf(v1, vv);
    }
    if (image_shape) {
        const float wm = (float)(image_shape[b * 2 + 1] - 1), hm = (float)(image_shape[b * 2] - 1);
        u0 = fminf(fmaxf(u0, 0.f), wm); u1 = fminf(fmaxf(u1, 0.f), wm);
        v0 = fminf(fmaxf(v0, 0.f), hm); v1 = fminf(fmaxf(v1, 0.f), hm);
    }
    oi[0] = u0; oi[1] = v0; oi[2] = u1; oi[3] = v1;
    alpha[t] = -atan2f(-bx[1], bx[0]) + ry;
}

// ---- overlaps ------------------------------------------------------------------------------------------------------

// frame of pair p: the last f with ov_off[f] <= p (empty frames share an offset with their successor)
__device__ __forceinline__ int ke_frame_of(const int *__restrict__ ov_off, int F, int p) {
    int lo = 0, hi = F;   // ov_off[lo] <= p < ov_off[hi]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (ov_off[mid] <= p) lo = mid; else hi = mid;
    }
    return lo;
}

// Intersection area of two rotated rectangles [x, y, dx, dy, angle] in fp32, the way rotate_iou.py's inter() builds it:
// corners turned by -angle about the centre, the corners of either box inside the other plus the crossings of the 4 x 4
// sides, ordered around their centroid, summed as a triangle fan.  Every operation is a single fp32 rounding in the
// reference's order (the translation unit is built with -ffp-contract=off; cos / sin / sqrt are correctly rounded via
// fp64), because the reference's own rounding error reaches some 1e-4 of IoU for small boxes far from the sensor: a
// more accurate clip would agree with it less well than this one does.
__device__ __forceinline__ void ke_corners(const float *r, float *c) {
    const float ac = (float)cos((double)r[4]), as = (float)sin((double)r[4]);
    const float hx = r[2] / 2, hy = r[3] / 2;
    const float cx[4] = {-hx, -hx, hx, hx}, cy[4] = {-hy, hy, hy, -hy};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        c[2 * i] = ac * cx[i] + as * cy[i] + r[0];
        c[2 * i + 1] = -as * cx[i] + ac * cy[i] + r[1];
    }
}

__device__ __forceinline__ bool ke_in_quad(float px, float py, const float *c) {
    const float ab0 = c[2] - c[0], ab1 = c[3] - c[1], ad0 = c[6] - c[0], ad1 = c[7] - c[1];
    const float ap0 = px - c[0], ap1 = py - c[1];
    const float abab = ab0 * ab0 + ab1 * ab1, abap = ab0 * ap0 + ab1 * ap1;
    const float adad = ad0 * ad0 + ad1 * ad1, adap = ad0 * ap0 + ad1 * ap1;
    return abab >= abap && abap >= 0 && adad >= adap && adap >= 0;
}

__device__ __forceinline__ bool ke_cross(const float *p1, const float *p2, int i, int j, float *out) {
    const float a0 = p1[2 * i], a1 = p1[2 * i + 1], b0 = p1[2 * ((i + 1) & 3)], b1 = p1[2 * ((i + 1) & 3) + 1];
    const float c0 = p2[2 * j], c1 = p2[2 * j + 1], d0 = p2[2 * ((j + 1) & 3)], d1 = p2[2 * ((j + 1) & 3) + 1];
    const float ba0 = b0 - a0, ba1 = b1 - a1, da0 = d0 - a0, ca0 = c0 - a0, da1 = d1 - a1, ca1 = c1 - a1;
    const bool acd = da1 * ca0 > ca1 * da0;
    const bool bcd = (d1 - b1) * (c0 - b0) > (c1 - b1) * (d0 - b0);
    if (acd == bcd) return false;
    const bool abc = ca1 * ba0 > ba1 * ca0, abd = da1 * ba0 > ba1 * da0;
    if (abc == abd) return false;
    const float dc0 = d0 - c0, dc1 = d1 - c1;
    const float abba = a0 * b1 - b0 * a1, cddc = c0 * d1 - d0 * c1;
    const float dh = ba1 * dc0 - ba0 * dc1;
    out[0] = (abba * dc0 - ba0 * cddc) / dh;
    out[1] = (abba * dc1 - ba1 * cddc) / dh;
    return true;
}

// r1 = the ground truth, r2 = the detection (the order rotate_iou_kernel_eval hands them over)
__device__ float ke_rotated_inter(const float *r1, const float *r2) {
    float c1[8], c2[8], pts[16], vs[8];
    ke_corners(r1, c1);
    ke_corners(r2, c2);
    int n = 0;
    for (int i = 0; i < 4; ++i) {
        if (ke_in_quad(c1[2 * i], c1[2 * i + 1], c2) && n < 8) { pts[2 * n] = c1[2 * i]; pts[2 * n + 1] = c1[2 * i + 1]; ++n; }
        if (ke_in_quad(c2[2 * i], c2[2 * i + 1], c1) && n < 8) { pts[2 * n] = c2[2 * i]; pts[2 * n + 1] = c2[2 * i + 1]; ++n; }
    }
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) {
            float x[2];
            if (ke_cross(c1, c2, i, j, x) && n < 8) { pts[2 * n] = x[0]; pts[2 * n + 1] = x[1]; ++n; }
        }
    if (n < 3) return 0.f;
    float m0 = 0.f, m1 = 0.f;
    for (int i = 0; i < n; ++i) { m0 += pts[2 * i]; m1 += pts[2 * i + 1]; }
    m0 /= (float)n; m1 /= (float)n;
    for (int i = 0; i < n; ++i) {
        float v0 = pts[2 * i] - m0, v1 = pts[2 * i + 1] - m1;
        const float d = (float)sqrt((double)(v0 * v0 + v1 * v1));
        v0 = v0 / d; v1 = v1 / d;
        if (v1 < 0) v0 = -2 - v0;
        vs[i] = v0;
    }
    for (int i = 1; i < n; ++i) {
        if (vs[i - 1] > vs[i]) {
            const float t = vs[i], tx = pts[2 * i], ty = pts[2 * i + 1];
            int j = i;
            while (j > 0 && vs[j - 1] > t) {
                vs[j] = vs[j - 1]; pts[2 * j] = pts[2 * j - 2]; pts[2 * j + 1] = pts[2 * j - 1];
                --j;
            }
            vs[j] = t; pts[2 * j] = tx; pts[2 * j + 1] = ty;
        }
    }
    float area = 0.f;
    for (int i = 0; i + 2 < n; ++i)
        area += fabsf(((pts[0] - pts[2 * i + 4]) * (pts[2 * i + 3] - pts[2 * i + 5]) -
                       (pts[1] - pts[2 * i + 5]) * (pts[2 * i + 2] - pts[2 * i + 4])) / 2.0f);
    return area;
}

// boxes are doubles: bbox (n, 4), cam (n, 7) = [x, y, z, l, h, w, ry]
__global__ void ke_overlap_kernel(KEFrames fr, int metric, const double *__restrict__ gt_bbox, const double *__restrict__ dt_bbox,
                                  const double *__restrict__ gt_cam, const double *__restrict__ dt_cam, int NP,
                                  double *__restrict__ out) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= NP) return;
    const int f = ke_frame_of(fr.ov_off, fr.F, p);
    const int ngt = fr.gt_off[f + 1] - fr.gt_off[f];
    const int local = p - fr.ov_off[f];
    const int j = fr.dt_off[f] + local / ngt, i = fr.gt_off[f] + local % ngt;
    double r = 0.0;
    if (metric == 0) {
        const double *b = dt_bbox + (long long)j * 4, *q = gt_bbox + (long long)i * 4;
        const double qarea = (q[2] - q[0]) * (q[3] - q[1]);
        const double iw = fmin(b[2], q[2]) - fmax(b[0], q[0]);
        if (iw > 0) {
            const double ih = fmin(b[3], q[3]) - fmax(b[1], q[1]);
            if (ih > 0) {
                const double ua = (b[2] - b[0]) * (b[3] - b[1]) + qarea - iw * ih;
                r = iw * ih / ua;
            }
        }
    } else {
        const double *b = dt_cam + (long long)j * 7, *q = gt_cam + (long long)i * 7;
        const float fb[5] = {(float)b[0], (float)b[2], (float)b[3], (float)b[5], (float)b[6]};
        const float fq[5] = {(float)q[0], (float)q[2], (float)q[3], (float)q[5], (float)q[6]};
        const float ai = ke_rotated_inter(fq, fb);
        if (metric == 1) {
            const float a1 = fb[2] * fb[3], a2 = fq[2] * fq[3];
            r = (double)(ai / (a1 + a2 - ai));
        } else if (ai > 0) {
            const double rinc = (double)ai;
            const double iw = fmin(b[1], q[1]) - fmax(b[1] - b[4], q[1] - q[4]);
            if (iw > 0) {
                const double a1 = b[3] * b[4] * b[5], a2 = q[3] * q[4] * q[5];
                const double inc = iw * rinc;
                r = inc / (a1 + a2 - inc);
            }
        }
    }
    out[p] = r;
}

// ---- clean_data, detection side ------------------------------------------------------------------------------------

struct KEClasses {
    int nC, nD;
    int cls[KE_MAXC];
    int diff[3];
};

__global__ void ke_dt_flags_kernel(int ND, const double *__restrict__ dt_bbox, const int *__restrict__ dt_name, KEClasses kc,
                                   signed char *__restrict__ ign) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= ND) return;
    const double height = fabs(dt_bbox[(long long)j * 4 + 3] - dt_bbox[(long long)j * 4 + 1]);
    const int name = dt_name[j];
    for (int c = 0; c < kc.nC; ++c)
        for (int d = 0; d < kc.nD; ++d) {
            const double min_h = kc.diff[d] == 0 ? 40.0 : 25.0;
            signed char v;
            if (height < min_h) v = 1;
            else if (name == kc.cls[c]) v = 0;
            else v = -1;
            ign[(long long)(c * kc.nD + d) * ND + j] = v;
        }
}

// ---- statistics ----------------------------------------------------------------------------------------------------

struct KEData {
    const double *ov;            // (nM, NP)
    long long NP;
    const signed char *ign_gt;   // (nC * nD, NG)
    const signed char *ign_dt;   // (nC * nD, ND)
    long long NG, ND;
    const double *dt_score, *gt_alpha, *dt_alpha, *gt_bbox, *dt_bbox;
    const int *gt_name;
    const double *min_overlap;   // (combinations)
};

__device__ __forceinline__ bool ke_bit(const unsigned *mask, int stride, int j) { return (mask[(j >> 5) * stride] >> (j & 31)) & 1u; }
__device__ __forceinline__ void ke_set(unsigned *mask, int stride, int j) { mask[(j >> 5) * stride] |= 1u << (j & 31); }

// one workgroup per frame, one thread per combination; slab slot of (mi, k, cd, frame) =
// (mi * K + k) * SV + voff[cd * (F + 1) + f] .. voff[cd * (F + 1) + f + 1]: true-positive scores first, NaN after them
__global__ void ke_pass1_kernel(KEFrames fr, KECombos cb, KEData d, const int *__restrict__ voff, long long SV,
                                double *__restrict__ slab) {
    extern __shared__ unsigned ke_lds[];
    const int f = blockIdx.x, t = threadIdx.x;
    const int ncombo = cb.nM * cb.nC * cb.nD * cb.K;
    if (t >= ncombo) return;
    const int k = t % cb.K, cd = (t / cb.K) % (cb.nC * cb.nD), mi = t / (cb.K * cb.nC * cb.nD);
    const int g0 = fr.gt_off[f], ngt = fr.gt_off[f + 1] - g0, d0 = fr.dt_off[f], ndt = fr.dt_off[f + 1] - d0;
    const int stride = blockDim.x;
    unsigned *mask = ke_lds + t;
    for (int w = 0; w < (ndt + 31) >> 5; ++w) mask[w * stride] = 0u;
    const double *ov = d.ov + (long long)mi * d.NP + fr.ov_off[f];
    const signed char *ig = d.ign_gt + (long long)cd * d.NG + g0, *id = d.ign_dt + (long long)cd * d.ND + d0;
    const double *score = d.dt_score + d0;
    const double mo = d.min_overlap[t];
    const int s0 = voff[cd * (fr.F + 1) + f], s1 = voff[cd * (fr.F + 1) + f + 1];
    double *out = slab + (long long)(mi * cb.K + k) * SV;
    int ntp = s0;
    for (int i = 0; i < ngt; ++i) {
        if (ig[i] == -1) continue;
        int det = -1;
        double best = -10000000.0;
        for (int j = 0; j < ndt; ++j) {
            if (id[j] == -1 || ke_bit(mask, stride, j)) continue;
            if (ov[(long long)j * ngt + i] > mo && score[j] > best) { det = j; best = score[j]; }
        }
        if (det < 0) continue;
        if (!(ig[i] == 1 || id[det] == 1) && ntp < s1) out[ntp++] = score[det];
        ke_set(mask, stride, det);
    }
    for (; ntp < s1; ++ntp) out[ntp] = __longlong_as_double(0x7ff8000000000000LL);
}

// one wave per (frame chunk, combination); lane = threshold.  The frame's flags, scores and overlaps are read at
// wave-uniform addresses (one request per wave); a lane's own state is its assignment bits in LDS and four counters.
__global__ void ke_pass2_kernel(KEFrames fr, KECombos cb, KEData d, const double *__restrict__ thresholds,
                                const int *__restrict__ nthr, int compute_aos, int per_chunk, long long *__restrict__ part) {
    extern __shared__ unsigned ke_lds[];
    const int chunk = blockIdx.x, t = blockIdx.y, lane = threadIdx.x;
    const int ncombo = cb.nM * cb.nC * cb.nD * cb.K;
    const int cd = (t / cb.K) % (cb.nC * cb.nD), mi = t / (cb.K * cb.nC * cb.nD);
    const int metric = cb.metric[mi];
    const bool active = lane < nthr[t];
    const double thresh = active ? thresholds[t * KE_PTS + lane] : 0.0;
    const double mo = d.min_overlap[t];
    unsigned *mask = ke_lds + lane;
    long long tp = 0, fp = 0, fn = 0;
    double sim = 0.0;
    const int f_end = min(fr.F, (chunk + 1) * per_chunk);
    if (active)
        for (int f = chunk * per_chunk; f < f_end; ++f) {
            const int g0 = fr.gt_off[f], ngt = fr.gt_off[f + 1] - g0, d0 = fr.dt_off[f], ndt = fr.dt_off[f + 1] - d0;
            for (int w = 0; w < (ndt + 31) >> 5; ++w) mask[w * 64] = 0u;
            const double *ov = d.ov + (long long)mi * d.NP + fr.ov_off[f];
            const signed char *ig = d.ign_gt + (long long)cd * d.NG + g0, *id = d.ign_dt + (long long)cd * d.ND + d0;
            const double *score = d.dt_score + d0;
            for (int i = 0; i < ngt; ++i) {
                const int gi = ig[i];
                if (gi == -1) continue;
                int det = -1;
                bool ign_pick = false;
                double max_ov = 0.0;
                for (int j = 0; j < ndt; ++j) {
                    const int dj = id[j];
                    if (dj == -1 || ke_bit(mask, 64, j) || score[j] < thresh) continue;
                    const double o = ov[(long long)j * ngt + i];
                    if (!(o > mo)) continue;
                    if ((o > max_ov || ign_pick) && dj == 0) { max_ov = o; det = j; ign_pick = false; }
                    else if (det < 0 && dj == 1) { det = j; ign_pick = true; }
                }
                if (det < 0) { if (gi == 0) ++fn; continue; }
                if (!(gi == 1 || id[det] == 1)) {
                    ++tp;
                    if (compute_aos) sim += (1.0 + cos(d.gt_alpha[g0 + i] - d.dt_alpha[d0 + det])) / 2.0;
                }
                ke_set(mask, 64, det);
            }
            for (int j = 0; j < ndt; ++j)
                if (!(ke_bit(mask, 64, j) || id[j] != 0 || score[j] < thresh)) ++fp;
            if (metric == 0) {
                // detections inside a DontCare region are no false positives (criterion 0: share of the detection's area)
                for (int i = 0; i < ngt; ++i) {
                    if (d.gt_name[g0 + i] != 6) continue;
                    const double *q = d.gt_bbox + (long long)(g0 + i) * 4;
                    for (int j = 0; j < ndt; ++j) {
                        if (ke_bit(mask, 64, j) || id[j] != 0 || score[j] < thresh) continue;
                        const double *b = d.dt_bbox + (long long)(d0 + j) * 4;
                        double o = 0.0;
                        const double iw = fmin(b[2], q[2]) - fmax(b[0], q[0]);
                        if (iw > 0) {
                            const double ih = fmin(b[3], q[3]) - fmax(b[1], q[1]);
                            if (ih > 0) o = iw * ih / ((b[2] - b[0]) * (b[3] - b[1]));
                        }
                        if (o > mo) { ke_set(mask, 64, j); --fp; }
                    }
                }
            }
        }
    long long *o = part + ((long long)(chunk * ncombo + t) * 64 + lane) * 4;
    o[0] = tp; o[1] = fp; o[2] = fn; o[3] = __double_as_longlong(sim);
}

// sums over the chunks in chunk order: (combination, threshold) -> [tp, fp, fn, similarity bits]
__global__ void ke_fold_kernel(int ncombo, int nchunks, const long long *__restrict__ part, long long *__restrict__ sums) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= ncombo * KE_PTS) return;
    const int t = e / KE_PTS, lane = e % KE_PTS;
    long long tp = 0, fp = 0, fn = 0;
    double sim = 0.0;
    for (int c = 0; c < nchunks; ++c) {
        const long long *p = part + ((long long)(c * ncombo + t) * 64 + lane) * 4;
        tp += p[0]; fp += p[1]; fn += p[2]; sim += __longlong_as_double(p[3]);
    }
    long long *o = sums + (long long)e * 4;
    o[0] = tp; o[1] = fp; o[2] = fn; o[3] = __double_as_longlong(sim);
}

static int ke_chunks(int F) { return F < KE_CHUNKS ? (F > 0 ? F : 1) : KE_CHUNKS; }

static int ke_check_combos(const char *who, int nM, const int *metrics, int nC, int nD, int K, KECombos *cb) {
    PDM_REQUIRE(nM >= 1 && nM <= KE_MAXM && metrics && nC >= 1 && nC <= KE_MAXC && nD >= 1 && nD <= 3 && K >= 1, PDM_E_BADARG,
                "%s: metrics=%d classes=%d difficulties=%d overlap sets=%d", who, nM, nC, nD, K);
    PDM_REQUIRE((long long)nM * nC * nD * K <= KE_MAXCOMBO, PDM_E_TOOLARGE, "%s: %lld combinations (limit %d)", who,
                (long long)nM * nC * nD * K, KE_MAXCOMBO);
    cb->nM = nM; cb->nC = nC; cb->nD = nD; cb->K = K;
    for (int m = 0; m < KE_MAXM; ++m) cb->metric[m] = 0;
    for (int m = 0; m < nM; ++m) {
        PDM_REQUIRE(metrics[m] >= 0 && metrics[m] <= 2, PDM_E_BADARG, "%s: metric %d", who, metrics[m]);
        cb->metric[m] = metrics[m];
    }
    return 0;
}

}  // namespace pdm

using namespace pdm;

extern "C" int pdm_kitti_boxes_to_camera(void *stream, int B, int P, const float *boxes, const int *count, const float *V2C,
                                         const float *R0, const float *P2, const int *image_shape, float *cam, float *img,
                                         float *alpha) {
    PDM_REQUIRE(B >= 0 && P >= 0, PDM_E_BADARG, "kitti_boxes_to_camera: B=%d P=%d", B, P);
    PDM_REQUIRE((long long)B * P <= (1LL << 30), PDM_E_TOOLARGE, "kitti_boxes_to_camera: B * P = %lld", (long long)B * P);
    if ((long long)B * P == 0) return 0;
    PDM_REQUIRE(boxes && count && V2C && R0 && P2 && cam && img && alpha, PDM_E_BADARG, "kitti_boxes_to_camera: null pointer");
    hipLaunchKernelGGL(ke_to_camera_kernel, dim3(divup((long long)B * P, 256)), dim3(256), 0, as_stream(stream), B, P, boxes,
                       count, V2C, R0, P2, image_shape, cam, img, alpha);
    return check_launch("kitti_boxes_to_camera");
}

extern "C" int pdm_kitti_eval_overlaps(void *stream, int F, const int *gt_off, const int *dt_off, const int *ov_off,
                                       long long NP, int nM, const int *metrics, const double *gt_bbox, const double *dt_bbox,
                                       const double *gt_cam, const double *dt_cam, double *overlaps) {
    PDM_REQUIRE(F >= 0 && NP >= 0 && nM >= 1 && nM <= KE_MAXM && metrics, PDM_E_BADARG, "kitti_eval_overlaps: F=%d NP=%lld nM=%d", F,
                NP, nM);
    PDM_REQUIRE(NP < (1LL << 31) - 256, PDM_E_TOOLARGE, "kitti_eval_overlaps: %lld pairs", NP);
    for (int m = 0; m < nM; ++m)
        PDM_REQUIRE(metrics[m] >= 0 && metrics[m] <= 2, PDM_E_BADARG, "kitti_eval_overlaps: metric %d", metrics[m]);
    if (F == 0 || NP == 0) return 0;
    PDM_REQUIRE(gt_off && dt_off && ov_off && gt_bbox && dt_bbox && gt_cam && dt_cam && overlaps, PDM_E_BADARG,
                "kitti_eval_overlaps: null pointer");
    const KEFrames fr{F, gt_off, dt_off, ov_off};
    for (int m = 0; m < nM; ++m) {
        hipLaunchKernelGGL(ke_overlap_kernel, dim3(divup(NP, 256)), dim3(256), 0, as_stream(stream), fr, metrics[m], gt_bbox,
                           dt_bbox, gt_cam, dt_cam, (int)NP, overlaps + (long long)m * NP);
        const int rc = check_launch("kitti_eval_overlaps");
        if (rc) return rc;
    }
    return 0;
}

extern "C" int pdm_kitti_eval_dt_flags(void *stream, long long ND, const double *dt_bbox, const int *dt_name, int nC,
                                       const int *classes, int nD, const int *difficulties, signed char *ign_dt) {
    PDM_REQUIRE(ND >= 0 && nC >= 1 && nC <= KE_MAXC && nD >= 1 && nD <= 3 && classes && difficulties, PDM_E_BADARG,
                "kitti_eval_dt_flags: ND=%lld classes=%d difficulties=%d", ND, nC, nD);
    PDM_REQUIRE(ND < (1LL << 31) - 256, PDM_E_TOOLARGE, "kitti_eval_dt_flags: %lld detections", ND);
    KEClasses kc;
    kc.nC = nC; kc.nD = nD;
    for (int c = 0; c < KE_MAXC; ++c) kc.cls[c] = c < nC ? classes[c] : -1;
    for (int d = 0; d < 3; ++d) kc.diff[d] = 0;
    for (int d = 0; d < nD; ++d) {
        PDM_REQUIRE(difficulties[d] >= 0 && difficulties[d] <= 2, PDM_E_BADARG, "kitti_eval_dt_flags: difficulty %d", difficulties[d]);
        kc.diff[d] = difficulties[d];
    }
    if (ND == 0) return 0;
    PDM_REQUIRE(dt_bbox && dt_name && ign_dt, PDM_E_BADARG, "kitti_eval_dt_flags: null pointer");
    hipLaunchKernelGGL(ke_dt_flags_kernel, dim3(divup(ND, 256)), dim3(256), 0, as_stream(stream), (int)ND, dt_bbox, dt_name, kc,
                       ign_dt);
    return check_launch("kitti_eval_dt_flags");
}

extern "C" size_t pdm_kitti_eval_workspace_bytes(int F, int combinations) {
    if (F < 0 || combinations < 0 || combinations > KE_MAXCOMBO) return 0;
    return (size_t)ke_chunks(F) * combinations * 64 * 4 * sizeof(long long);
}

extern "C" int pdm_kitti_eval_pass1(void *stream, int F, const int *gt_off, const int *dt_off, const int *ov_off, int max_dt,
                                    int nM, const int *metrics, int nC, int nD, int K, const double *overlaps, long long NP,
                                    const signed char *ign_gt, long long NG, const signed char *ign_dt, long long ND,
                                    const double *dt_score, const double *min_overlap, const int *slot_off, long long SV,
                                    double *slab) {
    KECombos cb;
    int rc = ke_check_combos("kitti_eval_pass1", nM, metrics, nC, nD, K, &cb);
    if (rc) return rc;
    PDM_REQUIRE(F >= 0 && max_dt >= 0 && NP >= 0 && NG >= 0 && ND >= 0 && SV >= 0, PDM_E_BADARG,
                "kitti_eval_pass1: F=%d max_dt=%d NP=%lld NG=%lld ND=%lld SV=%lld", F, max_dt, NP, NG, ND, SV);
    const int ncombo = nM * nC * nD * K, threads = (ncombo + 63) / 64 * 64, words = (max_dt + 31) / 32;
    PDM_REQUIRE(max_dt <= KE_MAXDT && (long long)words * threads * 4 <= KE_LDS, PDM_E_TOOLARGE,
                "kitti_eval_pass1: %d detections in a frame x %d combinations (limits %d, %d bytes of LDS)", max_dt, ncombo, KE_MAXDT,
                KE_LDS);
    if (F == 0) return 0;
    PDM_REQUIRE(gt_off && dt_off && ov_off && min_overlap && slot_off && (SV == 0 || slab) && (NP == 0 || overlaps) &&
                    (NG == 0 || ign_gt) && (ND == 0 || (ign_dt && dt_score)), PDM_E_BADARG, "kitti_eval_pass1: null pointer");
    const KEFrames fr{F, gt_off, dt_off, ov_off};
    KEData d{};
    d.ov = overlaps; d.NP = NP; d.ign_gt = ign_gt; d.ign_dt = ign_dt; d.NG = NG; d.ND = ND; d.dt_score = dt_score;
    d.min_overlap = min_overlap;
    hipLaunchKernelGGL(ke_pass1_kernel, dim3(F), dim3(threads), (size_t)words * threads * 4, as_stream(stream), fr, cb, d, slot_off,
                       SV, slab);
    return check_launch("kitti_eval_pass1");
}

extern "C" int pdm_kitti_eval_pass2(void *stream, int F, const int *gt_off, const int *dt_off, const int *ov_off, int max_dt,
                                    int nM, const int *metrics, int nC, int nD, int K, const double *overlaps, long long NP,
                                    const signed char *ign_gt, long long NG, const signed char *ign_dt, long long ND,
                                    const double *dt_score, const double *gt_alpha, const double *dt_alpha, const double *gt_bbox,
                                    const double *dt_bbox, const int *gt_name, const double *min_overlap, const double *thresholds,
                                    const int *num_thresholds, int compute_aos, void *workspace, size_t workspace_bytes,
                                    long long *sums) {
    KECombos cb;
    int rc = ke_check_combos("kitti_eval_pass2", nM, metrics, nC, nD, K, &cb);
    if (rc) return rc;
    PDM_REQUIRE(F >= 0 && max_dt >= 0 && NP >= 0 && NG >= 0 && ND >= 0, PDM_E_BADARG,
                "kitti_eval_pass2: F=%d max_dt=%d NP=%lld NG=%lld ND=%lld", F, max_dt, NP, NG, ND);
    PDM_REQUIRE(max_dt <= KE_MAXDT, PDM_E_TOOLARGE, "kitti_eval_pass2: %d detections in a frame (limit %d)", max_dt, KE_MAXDT);
    const int ncombo = nM * nC * nD * K;
    PDM_REQUIRE(min_overlap && thresholds && num_thresholds && sums && workspace, PDM_E_BADARG, "kitti_eval_pass2: null pointer");
    const size_t need = pdm_kitti_eval_workspace_bytes(F, ncombo);
    PDM_REQUIRE(workspace_bytes >= need, PDM_E_BADARG, "kitti_eval_pass2: workspace %zu < %zu bytes", workspace_bytes, need);
    PDM_WS_ALIGNED("kitti_eval_pass2", workspace);
    PDM_REQUIRE(F == 0 || (gt_off && dt_off && ov_off && (NP == 0 || overlaps) && (NG == 0 || (ign_gt && gt_alpha && gt_bbox && gt_name)) &&
                           (ND == 0 || (ign_dt && dt_score && dt_alpha && dt_bbox))), PDM_E_BADARG, "kitti_eval_pass2: null pointer");
    const KEFrames fr{F, gt_off, dt_off, ov_off};
    KEData d{};
    d.ov = overlaps; d.NP = NP; d.ign_gt = ign_gt; d.ign_dt = ign_dt; d.NG = NG; d.ND = ND; d.dt_score = dt_score;
    d.gt_alpha = gt_alpha; d.dt_alpha = dt_alpha; d.gt_bbox = gt_bbox; d.dt_bbox = dt_bbox; d.gt_name = gt_name;
    d.min_overlap = min_overlap;
    const int nchunks = ke_chunks(F), per_chunk = F == 0 ? 1 : (F + nchunks - 1) / nchunks;
    const int words = (max_dt + 31) / 32;
    long long *part = static_cast<long long *>(workspace);
    hipLaunchKernelGGL(ke_pass2_kernel, dim3(nchunks, ncombo), dim3(64), (size_t)(words > 0 ? words : 1) * 64 * 4, as_stream(stream),
                       fr, cb, d, thresholds, num_thresholds, compute_aos ? 1 : 0, per_chunk, part);
    rc = check_launch("kitti_eval_pass2");
    if (rc) return rc;
    hipLaunchKernelGGL(ke_fold_kernel, dim3(divup((long long)ncombo * KE_PTS, 256)), dim3(256), 0, as_stream(stream), ncombo, nchunks,
                       part, sums);
    return check_launch("kitti_eval_pass2 (fold)");
}

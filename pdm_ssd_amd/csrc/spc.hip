// PV-RCNN++'s proposal-centric partition: sample_points_with_roi and the front half of sector_fps of the
// reference's voxel_set_abstraction.py for the whole batch, on the device, without the (points x rois) matrix.
//
// A TILE is SPC_TILE consecutive rows of ONE sample (sample b owns ceil(cnt[b] / SPC_TILE) tiles; the tile table is a scan of
// the counts made once, by spc_plan_kernel, so a workgroup finds its sample by a bisection and never straddles two).  Five
// launches, none of which reads anything on the host:
//   plan    row and tile starts of every sample (one workgroup)
//   count   a workgroup per tile stages its sample's rois in LDS as (cx, cy, cz, ||dims / 2|| + radius) and walks them once for
//           four rows per lane at a time (lane l of chunk c owns row 64 c + l: the loads of a wave are one run of 768 bytes; the
//           roi words are broadcast reads).  Per row: the verdict and the sector as one byte in the workspace, and the tile's
//           count per sector (an LDS integer histogram)
//   sample  a workgroup per sample turns its tiles' counts into their exclusive prefix per sector, in place; the totals are
//           seg_cnt, their sum kept_cnt; the empty-mask fallback and the take counts (in double) are decided here
//   scan    scan_totals over the B max(S, 1) segment counts: where every segment starts in the output
//   fill    a workgroup per tile again: rank of a row among the rows of its sector inside its 64-row chunk from ballots, chunk
//           and tile prefixes on top, so a segment holds its rows in source order.  No atomic cursor anywhere: two runs and a
//           graph replay give the same bits.
//
// Arithmetic (nothing contracted): d = sqrt_rn(sqdist(p - c)) per roi, rois walked in ascending index with a strict < on d
// (a candidate is looked at only when its SQUARED distance is below the best one's, which d < best implies: sqrt_rn is
// monotone); kept when d_min < fl(sqrt_rn(sqdist(dims / 2)) + radius) of the roi that gave d_min.  Sector
// floor(fl(fl(atan2f(y, x) + PI_F) / SIZE_F)), clamped to [0, S]: S means "no sector" (dropped, but counted in kept_cnt).
#include "common.h"

namespace pdm {

constexpr int SPC_T = 256;                          // 4 waves
constexpr int SPC_CHUNKS = 16;                      // 64-row chunks of a tile, SPC_CHUNKS / 4 per wave
constexpr int SPC_PER = SPC_CHUNKS / (SPC_T / 64);  // rows per lane
constexpr int SPC_TILE = 64 * SPC_CHUNKS;
constexpr int SPC_MAXN = 1024;                      // rois of a sample held in LDS: 16 KiB
constexpr int SPC_MAXS = 64;                        // sectors
constexpr int SPC_CODES = SPC_MAXS + 1;             // + "no sector"
constexpr unsigned char SPC_OUT = 0xff;             // the byte of a row that is not kept

struct SpcArgs {
    int N, B, n, roi_stride, S, K, fallback;
    int ncodes;                         // S + 1 (sector S = dropped), or 1 when S = 0
    int nseg;                           // max(S, 1)
    int ntiles;                         // tiles the launches cover: ceil(N / TILE) + B at most
    float radius;
    const float *xyz, *rois;
    const int *cnt;
    float *seg_xyz;
    int *seg_row, *seg_cnt, *seg_take, *kept_cnt;
    unsigned char *mask;                // may be null
    // workspace
    unsigned char *code;                // (N)
    int *row_start, *tile_start;        // (B + 1) each
    int *tile_cnt;                      // (ntiles, ncodes): counts, then exclusive prefixes inside the sample
    int *seg_base;                      // (B nseg + 1)
    int *fb_code;                       // (B): the code of the fallback row, -1 without one
};

__device__ __forceinline__ int spc_sector(float x, float y, int S) {
    const float PI_F = 3.14159265358979323846f;
    const float size = (float)(2.0 * 3.14159265358979323846 / (double)S);
    const float q = floorf(__fdiv_rn(__fadd_rn(atan2f(y, x), PI_F), size));
    if (q >= 0.0f) return q < (float)S ? (int)q : S;
    return q < 0.0f ? 0 : S;           // NaN: no sector
}

// rows of sample b never leave [0, N): counts are clamped at 0 and at what is left of the N rows
__global__ __launch_bounds__(1024) void spc_plan_kernel(SpcArgs a) {
    __shared__ int s_wave[1024 / 64];
    int rows = 0, tiles = 0;
    for (int base = 0; base < a.B; base += 1024) {
        const int b = base + threadIdx.x;
        const int c = b < a.B ? max(a.cnt[b], 0) : 0;
        int total;
        const int excl = block_scan<1024>(c, s_wave, &total);
        const int start = min(rows + excl, a.N), live = min(c, a.N - start);
        const int t = (live + SPC_TILE - 1) / SPC_TILE;
        int ttotal;
        const int texcl = block_scan<1024>(t, s_wave, &ttotal);
        if (b < a.B) {
            a.row_start[b] = start;
            a.tile_start[b] = min(tiles + texcl, a.ntiles);
        }
        rows = min(rows + total, a.N);
        tiles += ttotal;
    }
    if (threadIdx.x == 0) {
        a.row_start[a.B] = rows;
        a.tile_start[a.B] = min(tiles, a.ntiles);
    }
}

// the sample that owns `tile`: the last b with tile_start[b] <= tile (empty samples own no tile); -1 past the last tile
__device__ __forceinline__ int spc_sample_of_tile(const SpcArgs &a, int tile) {
    if (tile >= a.tile_start[a.B]) return -1;
    int lo = 0, hi = a.B;               // tile_start[lo] <= tile < tile_start[hi]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (a.tile_start[mid] <= tile) lo = mid; else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(SPC_T) void spc_count_kernel(SpcArgs a) {
    __shared__ float4 s_roi[SPC_MAXN];
    __shared__ int s_hist[SPC_CODES];
    __shared__ int s_b;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid == 0) s_b = spc_sample_of_tile(a, blockIdx.x);
    if (tid < SPC_CODES) s_hist[tid] = 0;
    __syncthreads();
    const int b = s_b;
    if (b < 0) return;
    for (int j = tid; j < a.n; j += SPC_T) {
        const float *r = a.rois + ((size_t)b * a.n + j) * a.roi_stride;
        const float hx = __fdiv_rn(r[3], 2.0f), hy = __fdiv_rn(r[4], 2.0f), hz = __fdiv_rn(r[5], 2.0f);
        s_roi[j] = make_float4(r[0], r[1], r[2], __fadd_rn(__fsqrt_rn(sqdist(hx, hy, hz)), a.radius));
    }
    __syncthreads();
    const int row0 = a.row_start[b] + (blockIdx.x - a.tile_start[b]) * SPC_TILE, row_end = a.row_start[b + 1];

    float px[SPC_PER], py[SPC_PER], pz[SPC_PER], best[SPC_PER], best2[SPC_PER], thr[SPC_PER];
    int row[SPC_PER];
#pragma unroll
    for (int i = 0; i < SPC_PER; ++i) {
        row[i] = row0 + (wave + i * (SPC_T / 64)) * 64 + lane;
        const bool live = row[i] < row_end;
        const float *p = a.xyz + (size_t)(live ? row[i] : row0) * 3;
        px[i] = p[0]; py[i] = p[1]; pz[i] = p[2];
        best[i] = best2[i] = __builtin_inff();
        thr[i] = 0.0f;
    }
    for (int j = 0; j < a.n; ++j) {
        const float4 r = s_roi[j];
#pragma unroll
        for (int i = 0; i < SPC_PER; ++i) {
            const float d2 = sqdist(__fsub_rn(px[i], r.x), __fsub_rn(py[i], r.y), __fsub_rn(pz[i], r.z));
            if (d2 < best2[i]) {
                const float d = __fsqrt_rn(d2);
                if (d < best[i]) { best[i] = d; best2[i] = d2; thr[i] = r.w; }
            }
        }
    }
#pragma unroll
    for (int i = 0; i < SPC_PER; ++i) {
        if (row[i] >= row_end) continue;
        const bool keep = best[i] < thr[i];
        unsigned char code = SPC_OUT;
        if (keep) code = a.S > 0 ? (unsigned char)spc_sector(px[i], py[i], a.S) : 0;
        a.code[row[i]] = code;
        if (a.mask) a.mask[row[i]] = keep ? 1 : 0;
        if (keep) atomicAdd(&s_hist[code], 1);     // LDS integer counts: the sum does not depend on the order
    }
    __syncthreads();
    if (tid < a.ncodes) a.tile_cnt[(size_t)blockIdx.x * a.ncodes + tid] = s_hist[tid];
}

__global__ __launch_bounds__(SPC_T) void spc_sample_kernel(SpcArgs a) {
    __shared__ int s_tot[SPC_CODES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.x;
    const int t0 = a.tile_start[b], t1 = a.tile_start[b + 1];
    for (int s = wave; s < a.ncodes; s += SPC_T / 64) {     // a wave scans the tiles of one sector, 64 at a time
        int carry = 0;
        for (int base = t0; base < t1; base += 64) {
            const int t = base + lane;
            int *w = a.tile_cnt + (size_t)t * a.ncodes + s;
            const int v = t < t1 ? *w : 0;
            const int incl = wave_scan_incl(v);
            if (t < t1) *w = carry + incl - v;
            carry += __shfl(incl, 63, 64);
        }
        if (lane == 0) s_tot[s] = carry;
    }
    __syncthreads();
    if (tid != 0) return;
    int kept = 0;
    for (int s = 0; s < a.ncodes; ++s) kept += s_tot[s];
    int fb = -1;
    const int r0 = a.row_start[b];
    if (kept == 0 && a.fallback && a.row_start[b + 1] > r0) {      // points[:1] of a sample whose mask is empty
        fb = a.S > 0 ? spc_sector(a.xyz[(size_t)r0 * 3], a.xyz[(size_t)r0 * 3 + 1], a.S) : 0;
        s_tot[fb] = 1;
        kept = 1;
    }
    a.fb_code[b] = fb;
    a.kept_cnt[b] = kept;
    for (int s = 0; s < a.nseg; ++s) {
        const int c = s_tot[s];
        a.seg_cnt[(size_t)b * a.nseg + s] = c;
        a.seg_base[(size_t)b * a.nseg + s] = c;
        if (a.S > 0) {
            // min(c, ceil(c / N' * K)) as python evaluates it: a double division, a double product, the ceiling
            int take = 0;
            if (c > 0) {
                const double want = ceil(__dmul_rn(__ddiv_rn((double)c, (double)kept), (double)a.K));
                take = want < (double)c ? (int)want : c;
            }
            a.seg_take[(size_t)b * a.nseg + s] = take;
        }
    }
}

__global__ __launch_bounds__(SPC_T) void spc_fill_kernel(SpcArgs a) {
    __shared__ int s_chunk[SPC_CHUNKS][SPC_CODES];
    __shared__ int s_b;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid == 0) s_b = spc_sample_of_tile(a, blockIdx.x);
    for (int k = tid; k < SPC_CHUNKS * SPC_CODES; k += SPC_T) (&s_chunk[0][0])[k] = 0;
    __syncthreads();
    const int b = s_b;
    if (b < 0) return;
    const int first = a.row_start[b], row_end = a.row_start[b + 1];
    const int row0 = first + (blockIdx.x - a.tile_start[b]) * SPC_TILE;
    const int fb = a.fb_code[b];

    int code[SPC_PER], rank[SPC_PER];
#pragma unroll
    for (int i = 0; i < SPC_PER; ++i) {
        const int chunk = wave + i * (SPC_T / 64), row = row0 + chunk * 64 + lane;
        int c = row < row_end ? (int)a.code[row] : (int)SPC_OUT;
        if (fb >= 0 && row == first) c = fb;
        if (c >= a.nseg) c = -1;                    // not kept, or kept in no sector: no output row
        code[i] = c;
        rank[i] = 0;
        unsigned long long todo = __ballot(c >= 0);
        while (todo) {                              // one round per sector present in the chunk
            const int leader = __ffsll((long long)todo) - 1;
            const int cs = __shfl(c, leader, 64);
            const unsigned long long m = __ballot(c == cs);
            if (c == cs) rank[i] = lanes_below(m, lane);
            if (lane == leader) s_chunk[chunk][cs] = __popcll(m);
            todo &= ~m;
        }
    }
    __syncthreads();
    if (tid < a.nseg) {                             // counts of the chunks -> where each starts inside the segment
        int run = a.seg_base[(size_t)b * a.nseg + tid] + a.tile_cnt[(size_t)blockIdx.x * a.ncodes + tid];
        for (int k = 0; k < SPC_CHUNKS; ++k) {
            const int c = s_chunk[k][tid];
            s_chunk[k][tid] = run;
            run += c;
        }
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < SPC_PER; ++i) {
        if (code[i] < 0) continue;
        const int chunk = wave + i * (SPC_T / 64), row = row0 + chunk * 64 + lane;
        const int pos = s_chunk[chunk][code[i]] + rank[i];
        if (pos >= a.N) continue;                   // (cannot happen: a segment's rows are rows of xyz)
        const float *p = a.xyz + (size_t)row * 3;
        float *o = a.seg_xyz + (size_t)pos * 3;
        o[0] = p[0]; o[1] = p[1]; o[2] = p[2];
        a.seg_row[pos] = row;
    }
}

static size_t spc_layout(int N, int B, int S, SpcArgs *a, unsigned char *ws) {
    const int ncodes = S > 0 ? S + 1 : 1, nseg = S > 0 ? S : 1;
    const long long ntiles = ((long long)N + SPC_TILE - 1) / SPC_TILE + B;
    size_t off = 0;
    auto take = [&](size_t bytes) { const size_t at = off; off += align256(bytes); return ws ? ws + at : nullptr; };
    unsigned char *code = take((size_t)N);
    int *row_start = (int *)take(sizeof(int) * ((size_t)B + 1));
    int *tile_start = (int *)take(sizeof(int) * ((size_t)B + 1));
    int *tile_cnt = (int *)take(sizeof(int) * (size_t)ntiles * ncodes);
    int *seg_base = (int *)take(sizeof(int) * ((size_t)B * nseg + 1));
    int *fb_code = (int *)take(sizeof(int) * (size_t)B);
    if (a) {
        a->ncodes = ncodes; a->nseg = nseg; a->ntiles = (int)ntiles;
        a->code = code; a->row_start = row_start; a->tile_start = tile_start; a->tile_cnt = tile_cnt; a->seg_base = seg_base;
        a->fb_code = fb_code;
    }
    return off;
}

static int spc_check_sizes(int N, int B, int n, int roi_stride, int S, int K) {
    PDM_REQUIRE(N >= 0 && B >= 0 && B <= ST_MAXB, PDM_E_BADARG, "spc_partition: bad size (N=%d B=%d, at most %d samples)", N, B, ST_MAXB);
    PDM_REQUIRE(roi_stride >= 7, PDM_E_BADARG, "spc_partition: rois of %d columns (7 + C)", roi_stride);
    PDM_REQUIRE(n >= 1, PDM_E_BADARG, "spc_partition: %d rois a sample (the nearest of none is not defined)", n);
    PDM_REQUIRE(n <= SPC_MAXN, PDM_E_TOOLARGE, "spc_partition: %d rois a sample exceed the cap of %d the workgroup stages in LDS", n, SPC_MAXN);
    PDM_REQUIRE(S >= 0 && S <= SPC_MAXS, PDM_E_BADARG, "spc_partition: %d sectors (0 = filter only, up to %d)", S, SPC_MAXS);
    PDM_REQUIRE(S == 0 || K >= 1, PDM_E_BADARG, "spc_partition: num_keypoints %d (at least 1)", K);
    PDM_REQUIRE((long long)N * 3 <= 0x7fffffffll && (long long)B * n * roi_stride <= 0x7fffffffll, PDM_E_TOOLARGE,
                "spc_partition: point or roi elements exceed int32");
    return 0;
}

}  // namespace pdm

using namespace pdm;

extern "C" int pdm_spc_partition_max_rois(void) { return SPC_MAXN; }
extern "C" int pdm_spc_partition_max_sectors(void) { return SPC_MAXS; }

extern "C" size_t pdm_spc_partition_ws_bytes(int N, int B, int num_sectors) {
    if (N < 0 || B < 0 || B > ST_MAXB || num_sectors < 0 || num_sectors > SPC_MAXS) return 0;
    return spc_layout(N, B, num_sectors, nullptr, nullptr);
}

extern "C" int pdm_spc_partition(void *stream, int N, const float *xyz, int B, const int *xyz_batch_cnt, int n, int roi_stride,
                                 const float *rois, float radius, int num_sectors, int num_keypoints, int fallback, float *seg_xyz,
                                 int *seg_row, int *seg_cnt, int *seg_take, int *kept_cnt, unsigned char *mask, void *workspace,
                                 size_t workspace_bytes) {
    if (int rc = spc_check_sizes(N, B, n, roi_stride, num_sectors, num_keypoints)) return rc;
    PDM_REQUIRE(radius == radius, PDM_E_BADARG, "spc_partition: the radius is NaN");
    if (B == 0) return 0;
    PDM_REQUIRE(xyz_batch_cnt && rois && seg_cnt && kept_cnt && (num_sectors == 0 || seg_take), PDM_E_BADARG, "spc_partition: null pointer");
    PDM_REQUIRE(N == 0 || (xyz && seg_xyz && seg_row), PDM_E_BADARG, "spc_partition: null pointer");
    PDM_REQUIRE(workspace, PDM_E_BADARG, "spc_partition: null workspace");
    PDM_WS_ALIGNED("spc_partition", workspace);
    SpcArgs a{};
    const size_t need = spc_layout(N, B, num_sectors, &a, (unsigned char *)workspace);
    PDM_REQUIRE(workspace_bytes >= need, PDM_E_BADARG, "spc_partition: workspace of %zu bytes, %zu needed", workspace_bytes, need);
    a.N = N; a.B = B; a.n = n; a.roi_stride = roi_stride; a.S = num_sectors; a.K = num_keypoints; a.fallback = fallback != 0;
    a.radius = radius; a.xyz = xyz; a.rois = rois; a.cnt = xyz_batch_cnt;
    a.seg_xyz = seg_xyz; a.seg_row = seg_row; a.seg_cnt = seg_cnt; a.seg_take = seg_take; a.kept_cnt = kept_cnt; a.mask = mask;
    hipStream_t st = as_stream(stream);
    hipLaunchKernelGGL(spc_plan_kernel, dim3(1), dim3(1024), 0, st, a);
    if (int rc = check_launch("spc_partition(plan)")) return rc;
    hipLaunchKernelGGL(spc_count_kernel, dim3(a.ntiles), dim3(SPC_T), 0, st, a);
    if (int rc = check_launch("spc_partition(count)")) return rc;
    hipLaunchKernelGGL(spc_sample_kernel, dim3(B), dim3(SPC_T), 0, st, a);
    if (int rc = check_launch("spc_partition(sample)")) return rc;
    hipLaunchKernelGGL(scan_totals_kernel<1024>, dim3(1), dim3(1024), 0, st, B * a.nseg, a.seg_base, (int *)nullptr, 0, -1);
    if (int rc = check_launch("spc_partition(scan)")) return rc;
    hipLaunchKernelGGL(spc_fill_kernel, dim3(a.ntiles), dim3(SPC_T), 0, st, a);
    return check_launch("spc_partition(fill)");
}

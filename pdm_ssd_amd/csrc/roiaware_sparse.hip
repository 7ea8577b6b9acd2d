// Part-A2's RoI-aware pooling for the whole batch, straight to sparse rows: what PartA2FCHead.roiaware_pool and
// the `sum(-1).nonzero()` + gather behind it compute (reference partA2_head.py:104-197), without the dense
// (B N, S, S, S, 4 + C) tensor, the (N, S, S, S, max_pts) point lists, the per-sample loop or the nonzero.
//
// count -> scan -> fill, a workgroup per box in every box-wise launch:
//   count   the box's points per cell in an LDS histogram -> hits[r] = sum over its cells of min(count, cap)
//   scan    one workgroup: hits -> the boxes' list offsets (scan_totals)
//   fill    the histogram again, capped, scanned into the cells' starts (hist_to_cursors); the points then appended to their
//           cells' segments in ascending index order (roiaware_append_block, the composed kernel's own append), so a segment
//           IS the composed kernel's list; then the activity of every occupied cell: the fp32 sum, in ascending channel order,
//           of its four averaged part channels is non-zero.  One record (cell, segment start, length) per ACTIVE cell, in
//           ascending cell order -> nact[r]
//   scan    nact -> the boxes' row offsets; record = {Q, overflow}: the caller's one host read
//   emit    rows q0[r] .. : coords (r, x, y, z), part = the average, rpn = the maximum, over the segment (roiaware_list_avg /
//           roiaware_list_max: the composed kernel's arithmetic, so the same bits)
// The in-box test, the cell of a point, the cap (the first max_pts - 1 points of a cell in ascending index) and the summation
// order are roiaware.h's.  No float atomics (the histogram's are LDS integer counts); every result is a function of the input
// alone.  The point lists live in a workspace of list_capacity entries chosen by the caller: a box whose segment would end past
// it sets record[1] and takes no rows (the caller refuses the result).
#include <algorithm>

#include "roiaware.h"

namespace pdm {

constexpr int RS_MAX_CELLS = 4096;   // cells of a box: two LDS tables of ints (counts / cursors, and the starts)
constexpr int RS_SCAN_NT = 1024;

struct RsSpace {
    int *hits;       // (R + 1): capped hits of a box, then their exclusive prefix with the total behind
    int *nact;       // (R + 1): active cells of a box, then the prefix
    int *list;       // (L): the cells' segments, box after box, cell after cell
    int *rec_cell;   // (min(L, R V)) per active cell, from rs_rec_base(r): its cell, its segment's start in list, its length
    int *rec_start;
    int *rec_n;
};

static size_t rs_rec_capacity(long long R, int V, long long L) { return (size_t)(L < R * V ? L : R * V); }

static size_t rs_bytes(long long R, int V, long long L) {
    return 2 * align256((size_t)(R + 1) * sizeof(int)) + align256((size_t)L * sizeof(int)) + 3 * align256(rs_rec_capacity(R, V, L) * sizeof(int));
}

static RsSpace rs_carve(void *workspace, long long R, int V, long long L) {
    char *p = static_cast<char *>(workspace);
    RsSpace s;
    s.hits = reinterpret_cast<int *>(p); p += align256((size_t)(R + 1) * sizeof(int));
    s.nact = reinterpret_cast<int *>(p); p += align256((size_t)(R + 1) * sizeof(int));
    s.list = reinterpret_cast<int *>(p); p += align256((size_t)L * sizeof(int));
    const size_t rc = align256(rs_rec_capacity(R, V, L) * sizeof(int));
    s.rec_cell = reinterpret_cast<int *>(p); p += rc;
    s.rec_start = reinterpret_cast<int *>(p); p += rc;
    s.rec_n = reinterpret_cast<int *>(p);
    return s;
}

// first record of box r: at most min(hits, V) cells of a box are active, so both prefixes bound the records in front of it
__device__ __forceinline__ long long rs_rec_base(int r, int V, int off) { return min((long long)off, (long long)r * V); }

// the box, and the rows [*p0, *p0 + *np) of its sample (rows are batch-major, counts per sample), clamped into [0, P)
__device__ __forceinline__ void rs_box(int r, int N, int P, const float *__restrict__ rois, const int *__restrict__ counts, float *bx, int *p0,
                                       int *np) {
#pragma unroll
    for (int f = 0; f < 7; ++f) bx[f] = rois[(size_t)r * 7 + f];
    const int b = r / N;
    int start = 0;
    for (int k = 0; k < b; ++k) start = min(start + max(counts[k], 0), P);
    *p0 = start;
    *np = max(min(counts[b], P - start), 0);
}

// cnt[v] += 1 for every point of the sample inside the box (LDS integer atomics: counts do not depend on the order)
__device__ __forceinline__ void rs_histogram(int *cnt, int V, const float *__restrict__ pts, int p0, int np, const float *bx, float c, float s,
                                             float reach2, int ox, int oy, int oz) {
    for (int v = threadIdx.x; v < V; v += RA_NT) cnt[v] = 0;
    __syncthreads();
    for (int i = threadIdx.x; i < np; i += RA_NT) {
        const int v = roiaware_cell_of(pts, (size_t)p0 + i, bx, c, s, reach2, ox, oy, oz);
        if (v >= 0) atomicAdd(&cnt[v], 1);
    }
    __syncthreads();
}

__global__ __launch_bounds__(RA_NT) void rs_count_kernel(int N, int P, int cap, int ox, int oy, int oz, const float *__restrict__ rois,
                                                         const float *__restrict__ pts, const int *__restrict__ counts, int *__restrict__ hits) {
    __shared__ int s_cnt[RS_MAX_CELLS];
    __shared__ int s_wave[RA_NT / 64];
    const int r = blockIdx.x, V = ox * oy * oz;
    float bx[7], c, s;
    int p0, np;
    rs_box(r, N, P, rois, counts, bx, &p0, &np);
    box_cos_sin_f(bx[6], &c, &s);
    rs_histogram(s_cnt, V, pts, p0, np, bx, c, s, box_reach2_pool(bx), ox, oy, oz);
    int local = 0;
    for (int v = threadIdx.x; v < V; v += RA_NT) local += min(s_cnt[v], cap);
    int total;
    block_scan<RA_NT>(local, s_wave, &total);
    if (threadIdx.x == 0) hits[r] = total;
}

__global__ __launch_bounds__(RA_NT) void rs_fill_kernel(int N, int P, int cap, int ox, int oy, int oz, const float *__restrict__ rois,
                                                        const float *__restrict__ pts, const int *__restrict__ counts,
                                                        const float *__restrict__ part, long long L, RsSpace ws, int *record) {
    __shared__ int s_cnt[RS_MAX_CELLS];
    __shared__ int s_start[RS_MAX_CELLS + 1];
    __shared__ int s_vox[RA_NT];
    __shared__ int s_wave[RA_NT / 64];
    const int tid = threadIdx.x, wave = tid >> 6;
    const int r = blockIdx.x, V = ox * oy * oz;
    const int off = ws.hits[r], h = ws.hits[r + 1] - off;   // (uniform)
    if (h <= 0 || off < 0 || (long long)off + h > L) {
        if (tid == 0) {
            ws.nact[r] = 0;
            if (h != 0) record[1] = 1;   // the list has no room for this box's segment: every writer stores the same 1
        }
        return;
    }
    float bx[7], c, s;
    int p0, np;
    rs_box(r, N, P, rois, counts, bx, &p0, &np);
    box_cos_sin_f(bx[6], &c, &s);
    const float reach2 = box_reach2_pool(bx);
    rs_histogram(s_cnt, V, pts, p0, np, bx, c, s, reach2, ox, oy, oz);
    for (int v = tid; v < V; v += RA_NT) s_cnt[v] = min(s_cnt[v], cap);
    __syncthreads();
    hist_to_cursors<RA_NT>(s_cnt, V, s_wave, s_start);       // s_start[0 .. V]: the capped segments; s_start[V] == h
    if (s_start[V] != h) {                                   // (uniform; the count launch saw the same inputs, so it never differs)
        if (tid == 0) { ws.nact[r] = 0; record[1] = 1; }
        return;
    }
    for (int v = tid; v < V; v += RA_NT) s_cnt[v] = 0;       // now the points appended to a cell so far
    __syncthreads();

    int *list = ws.list + off;
    for (int i0 = 0; i0 < np; i0 += RA_NT) {
        const int i = i0 + tid;
        const int v = i < np ? roiaware_cell_of(pts, (size_t)p0 + i, bx, c, s, reach2, ox, oy, oz) : -1;
        s_vox[tid] = v;
        if (!__syncthreads_or(v >= 0)) continue;   // no hit in this block of points (nobody reads s_vox)
        if (wave == 0)
            roiaware_append_block(s_vox, p0 + i0, s_cnt, [&](int lv, int slot, int pt) {
                if (slot < cap) list[s_start[lv] + slot] = pt;   // s_start[lv] + slot < s_start[lv + 1] <= h
            });
        __syncthreads();
    }
    __syncthreads();   // the segments, written by the first wave, are read by every wave below

    // activity and the records of the active cells, in ascending cell order
    const long long rbase = rs_rec_base(r, V, off);
    int seen = 0;
    for (int v0 = 0; v0 < V; v0 += RA_NT) {
        const int v = v0 + tid;
        int n = 0, st = 0;
        bool active = false;
        if (v < V) {
            st = s_start[v];
            n = s_start[v + 1] - st;
            if (n > 0) {
                float sum = roiaware_list_avg(list + st, n, part, 4, 0);
#pragma unroll
                for (unsigned ch = 1; ch < 4; ++ch) sum += roiaware_list_avg(list + st, n, part, 4, ch);
                active = sum != 0.f;
            }
        }
        int total;
        const int rank = block_scan<RA_NT>(active ? 1 : 0, s_wave, &total);
        if (active) {
            const long long at = rbase + seen + rank;
            ws.rec_cell[at] = v;
            ws.rec_start[at] = off + st;
            ws.rec_n[at] = n;
        }
        seen += total;
    }
    if (tid == 0) ws.nact[r] = seen;
}

__global__ __launch_bounds__(RA_NT) void rs_emit_kernel(int C, int Q, int ox, int oy, int oz, const float *__restrict__ part,
                                                        const float *__restrict__ rpn, RsSpace ws, int *__restrict__ coords,
                                                        float *__restrict__ out_part, float *__restrict__ out_rpn) {
    const int r = blockIdx.x, V = ox * oy * oz, tid = threadIdx.x;
    const int q0 = ws.nact[r], na = ws.nact[r + 1] - q0;
    if (na <= 0 || q0 < 0 || q0 + na > Q) return;   // (Q is the caller's copy of the total: rows past it have no memory)
    const long long rbase = rs_rec_base(r, V, ws.hits[r]);
    for (int j = tid; j < na; j += RA_NT) {
        const int v = ws.rec_cell[rbase + j];
        int *o = coords + (size_t)(q0 + j) * 4;
        o[0] = r;
        o[1] = v / (oy * oz);
        o[2] = (v / oz) % oy;
        o[3] = v % oz;
    }
    for (unsigned e = tid; e < (unsigned)na * 4u; e += RA_NT) {
        const unsigned j = e >> 2, ch = e & 3u;
        out_part[(size_t)q0 * 4 + e] = roiaware_list_avg(ws.list + ws.rec_start[rbase + j], ws.rec_n[rbase + j], part, 4, ch);
    }
    const unsigned NC = (unsigned)na * (unsigned)C;
    for (unsigned e = tid; e < NC; e += RA_NT) {
        const unsigned j = e / (unsigned)C, ch = e % (unsigned)C;
        int arg;
        const float best = roiaware_list_max(ws.list + ws.rec_start[rbase + j], ws.rec_n[rbase + j], rpn, C, ch, &arg);
        out_rpn[(size_t)q0 * C + e] = arg != -1 ? best : 0.f;   // the composed form leaves its zero fill where nothing wins
    }
}

}  // namespace pdm

using namespace pdm;

static int rs_args(const char *who, int B, int N, int P, int C, int max_pts, int ox, int oy, int oz, long long L) {
    PDM_REQUIRE(B >= 0 && N >= 0 && P >= 0 && C >= 1 && L >= 0, PDM_E_BADARG, "%s: B=%d N=%d P=%d C=%d list_capacity=%lld", who, B, N, P, C, L);
    PDM_REQUIRE(B <= ST_MAXB, PDM_E_BADARG, "%s: B=%d samples (at most %d)", who, B, ST_MAXB);
    PDM_REQUIRE(ox >= 1 && oy >= 1 && oz >= 1 && (long long)ox * oy * oz <= RS_MAX_CELLS, PDM_E_BADARG,
                "%s: pool size (%d, %d, %d): at least 1 each and at most %d cells a box", who, ox, oy, oz, RS_MAX_CELLS);
    PDM_REQUIRE(max_pts >= 2, PDM_E_BADARG, "%s: max_pts=%d (slot 0 of the composed list is the count: at least 2)", who, max_pts);
    PDM_REQUIRE((long long)B * N < (1ll << 31) / RS_MAX_CELLS && L < (1ll << 31) && (long long)P * C < (1ll << 31), PDM_E_TOOLARGE,
                "%s: B * N = %lld boxes, list_capacity %lld or P * C = %lld", who, (long long)B * N, L, (long long)P * C);
    const long long per_box = std::min((long long)P, (long long)ox * oy * oz * (max_pts - 1));
    PDM_REQUIRE((long long)B * N * per_box < (1ll << 31), PDM_E_TOOLARGE, "%s: %lld boxes of up to %lld listed points (the product below 2^31)",
                who, (long long)B * N, per_box);
    return 0;
}

extern "C" size_t pdm_roiaware_pool_sparse_workspace_bytes(int B, int N, int out_x, int out_y, int out_z, long long list_capacity) {
    if (B <= 0 || N <= 0 || out_x <= 0 || out_y <= 0 || out_z <= 0 || list_capacity < 0) return 0;
    return rs_bytes((long long)B * N, out_x * out_y * out_z, list_capacity);
}

extern "C" int pdm_roiaware_pool_sparse_index(void *stream, int B, int N, int P, int max_pts, int out_x, int out_y, int out_z,
                                              const float *rois, const float *pts, const int *counts, const float *part,
                                              long long list_capacity, int *record, void *workspace, size_t workspace_bytes) {
    const int rc = rs_args("roiaware_pool_sparse_index", B, N, P, 1, max_pts, out_x, out_y, out_z, list_capacity);
    if (rc) return rc;
    PDM_REQUIRE(record, PDM_E_BADARG, "roiaware_pool_sparse_index: null record");
    const long long R = (long long)B * N;
    if (R == 0) {   // nothing to pool: record = {0, 0}
        return zero_fill(stream, "roiaware_pool_sparse_index", record, 2 * sizeof(int));
    }
    PDM_REQUIRE(rois && counts && (P == 0 || (pts && part)), PDM_E_BADARG, "roiaware_pool_sparse_index: null pointer");
    const size_t need = rs_bytes(R, out_x * out_y * out_z, list_capacity);
    PDM_REQUIRE(workspace && workspace_bytes >= need, PDM_E_BADARG, "roiaware_pool_sparse_index: workspace of %zu bytes, need %zu",
                workspace_bytes, need);
    PDM_WS_ALIGNED("roiaware_pool_sparse_index", workspace);
    const RsSpace ws = rs_carve(workspace, R, out_x * out_y * out_z, list_capacity);
    hipStream_t st = as_stream(stream);
    hipLaunchKernelGGL(rs_count_kernel, dim3((unsigned)R), dim3(RA_NT), 0, st, N, P, max_pts - 1, out_x, out_y, out_z, rois, pts, counts, ws.hits);
    hipLaunchKernelGGL(scan_totals_kernel<RS_SCAN_NT>, dim3(1), dim3(RS_SCAN_NT), 0, st, (int)R, ws.hits, record, 0, 1);
    hipLaunchKernelGGL(rs_fill_kernel, dim3((unsigned)R), dim3(RA_NT), 0, st, N, P, max_pts - 1, out_x, out_y, out_z, rois, pts, counts, part,
                       list_capacity, ws, record);
    hipLaunchKernelGGL(scan_totals_kernel<RS_SCAN_NT>, dim3(1), dim3(RS_SCAN_NT), 0, st, (int)R, ws.nact, record, 0, -1);
    return check_launch("roiaware_pool_sparse_index");
}

extern "C" int pdm_roiaware_pool_sparse_emit(void *stream, int B, int N, int P, int C, int out_x, int out_y, int out_z, const float *part,
                                             const float *rpn, long long list_capacity, int Q, const void *workspace,
                                             size_t workspace_bytes, int *coords, float *out_part, float *out_rpn) {
    const int rc = rs_args("roiaware_pool_sparse_emit", B, N, P, C, 2, out_x, out_y, out_z, list_capacity);
    if (rc) return rc;
    PDM_REQUIRE(Q >= 0, PDM_E_BADARG, "roiaware_pool_sparse_emit: Q=%d", Q);
    const long long R = (long long)B * N;
    if (Q == 0 || R == 0) return 0;   // no active cell: nothing to write, nothing launched
    PDM_REQUIRE(part && rpn && coords && out_part && out_rpn, PDM_E_BADARG, "roiaware_pool_sparse_emit: null pointer");
    PDM_REQUIRE((long long)Q * C < (1ll << 31), PDM_E_TOOLARGE, "roiaware_pool_sparse_emit: Q * C = %lld (below 2^31)", (long long)Q * C);
    const size_t need = rs_bytes(R, out_x * out_y * out_z, list_capacity);
    PDM_REQUIRE(workspace && workspace_bytes >= need, PDM_E_BADARG, "roiaware_pool_sparse_emit: workspace of %zu bytes, need %zu",
                workspace_bytes, need);
    PDM_WS_ALIGNED("roiaware_pool_sparse_emit", workspace);
    const RsSpace ws = rs_carve(const_cast<void *>(workspace), R, out_x * out_y * out_z, list_capacity);
    hipLaunchKernelGGL(rs_emit_kernel, dim3((unsigned)R), dim3(RA_NT), 0, as_stream(stream), C, Q, out_x, out_y, out_z, part, rpn, ws, coords,
                       out_part, out_rpn);
    return check_launch("roiaware_pool_sparse_emit");
}

// pdm_sparse_fc: SparseConvTensor.dense() of the RoI grids followed by the first shared FC of Part-A2's head, without the dense
// (R, C S^3) tensor.  out[r] = epilogue(sum over the rows q of box r of W[:, :, cell(q)] x[q]), with the Conv1d
// weight's column c * cells + cell (dense() is channels-first) repacked cell-major into the A fragments of mfma_f32_16x16x4f32.
//
// Rows arrive sorted by (box, cell), one row per (box, cell) at most.  A cell's rows therefore belong to DISTINCT boxes: they
// go through that cell's (C x Cout) weight block as one small GEMM, 16 rows a tile, and no two rows of a cell add into the same
// output.  What has to be ordered is the sum of a box over its cells:
//   index   box_start (lower bounds in the sorted rows); per cell, count -> scan -> fill of its rows in ascending box order (a
//           workgroup per cell searches every box's segment for the cell: no atomics, no sort, the same lists every run)
//   main    a workgroup owns (a tile of TR boxes) x (a chunk of cells) and walks the chunk's cells in ascending order; the
//           tile's boxes' rows of a cell are a contiguous piece of its list; products are added into an LDS accumulator
//           (TR x Cout) by the one wave that owns the output channels, so every element sees its terms in ascending cell order.
//           The tile is written whole, zeros included, to partial[chunk]
//   reduce  out = epilogue(partial[0] + partial[1] + ...), ascending (fc_reduce.h, shared with bev_roi_crop.hip)
// Fixed-order partials rather than 64-bit fixed-point atomics: the chunk boundaries are a function of (R, cells, Cout) alone, so
// two runs give the same bits, the result keeps fp32's relative error bound with no quantisation term, no scale has to be taken
// from the data first, and the partials (chunks x R x Cout floats) are small beside the weight.
#include <algorithm>

#include "fc_reduce.h"
#include "mfma_f32.h"

namespace pdm {

constexpr int FC_NT = 256;
constexpr int FC_ACC_FLOATS = 16384;   // the LDS accumulator: TR = min(128, 16384 / Cout) boxes

struct FcPlan {
    int TR, tiles, chunk_cells, nchunk;
};

static FcPlan fc_plan(int R, int cells, int Cout) {
    FcPlan p;
    p.TR = std::min(128, FC_ACC_FLOATS / Cout);
    p.tiles = divup(std::max(R, 1), p.TR);
    const SplitK k = split_k_plan(cells, p.tiles);
    p.chunk_cells = k.chunk;
    p.nchunk = k.nchunk;
    return p;
}

struct FcSpace {
    int *box_start;    // (R + 1)
    int *cell_start;   // (cells + 1): counts, then their prefix
    int *cell_rows;    // (Q): the rows of a cell, ascending
    float *partial;    // (nchunk, R, Cout)
};

static size_t fc_bytes(long long Q, int R, int cells, int Cout) {
    const FcPlan p = fc_plan(R, cells, Cout);
    return align256((size_t)(R + 1) * sizeof(int)) + align256((size_t)(cells + 1) * sizeof(int)) + align256((size_t)std::max(Q, 1ll) * sizeof(int)) +
           align256((size_t)p.nchunk * R * Cout * sizeof(float));
}

static FcSpace fc_carve(void *workspace, long long Q, int R, int cells) {
    char *p = static_cast<char *>(workspace);
    FcSpace s;
    s.box_start = reinterpret_cast<int *>(p); p += align256((size_t)(R + 1) * sizeof(int));
    s.cell_start = reinterpret_cast<int *>(p); p += align256((size_t)(cells + 1) * sizeof(int));
    s.cell_rows = reinterpret_cast<int *>(p); p += align256((size_t)std::max(Q, 1ll) * sizeof(int));
    s.partial = reinterpret_cast<float *>(p);
    return s;
}

// first row in [lo, hi) whose box is >= target (the rows' boxes ascend)
__device__ __forceinline__ int fc_lower_box(const int *__restrict__ coords, int lo, int hi, int target) {
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (coords[(size_t)mid * 4] < target) lo = mid + 1; else hi = mid;
    }
    return lo;
}

__device__ __forceinline__ int fc_cell(const int *__restrict__ coords, int q, int sy, int sz) {
    const int *c = coords + (size_t)q * 4;
    return (c[1] * sy + c[2]) * sz + c[3];
}

__global__ __launch_bounds__(FC_NT) void fc_box_start_kernel(int Q, int R, const int *__restrict__ coords, int *__restrict__ box_start) {
    const int r = blockIdx.x * FC_NT + threadIdx.x;
    if (r <= R) box_start[r] = fc_lower_box(coords, 0, Q, r);
}

// a workgroup per cell: the row of every box at this cell (a binary search in the box's segment, whose cells ascend), counted
// (FILL = false: cell_start[cell] = count) or written in ascending box order (FILL = true)
template <bool FILL>
__global__ __launch_bounds__(FC_NT) void fc_cell_rows_kernel(int R, int sy, int sz, const int *__restrict__ coords,
                                                             const int *__restrict__ box_start, int *cell_start, int *__restrict__ cell_rows) {
    __shared__ int s_wave[FC_NT / 64];
    const int cell = blockIdx.x;
    const int base = FILL ? cell_start[cell] : 0, room = FILL ? cell_start[cell + 1] - base : 0;
    int seen = 0;
    for (int r0 = 0; r0 < R; r0 += FC_NT) {
        const int r = r0 + threadIdx.x;
        int q = -1;
        if (r < R) {
            int lo = box_start[r];
            const int end = box_start[r + 1];
            int hi = end;
            while (lo < hi) {
                const int mid = lo + ((hi - lo) >> 1);
                if (fc_cell(coords, mid, sy, sz) < cell) lo = mid + 1; else hi = mid;
            }
            if (lo < end && fc_cell(coords, lo, sy, sz) == cell) q = lo;
        }
        int total;
        const int rank = block_scan<FC_NT>(q >= 0 ? 1 : 0, s_wave, &total);
        if (FILL && q >= 0 && seen + rank < room) cell_rows[base + seen + rank] = q;
        seen += total;
    }
    if (!FILL && threadIdx.x == 0) cell_start[cell] = seen;
}

struct FcArgs {
    int R, TR, cells, chunk_cells, Ca, Cb, Cout;
    const int *coords;
    const float *xa, *xb, *wpack;
    const int *cell_start, *cell_rows;
    float *partial;
};

__global__ __launch_bounds__(FC_NT) void fc_main_kernel(FcArgs a) {
    extern __shared__ __align__(16) float fc_smem[];
    const int C = a.Ca + a.Cb, XS = C + 4, KB = C / 16, NB = a.Cout / 16;
    float *acc = fc_smem;                        // (TR, Cout)
    float *xs = fc_smem + a.TR * a.Cout;         // (16, C + 4): the staged rows, the B operand
    int *s_box = reinterpret_cast<int *>(xs + 16 * XS);   // (16): the staged rows' boxes, relative to the tile
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, pos = lane & 15, g = lane >> 4;
    const int r_lo = blockIdx.x * a.TR, r_hi = min(a.R, r_lo + a.TR);
    const int c_lo = blockIdx.y * a.chunk_cells, c_hi = min(a.cells, c_lo + a.chunk_cells);
    for (int e = tid; e < a.TR * a.Cout; e += FC_NT) acc[e] = 0.f;

    for (int cell = c_lo; cell < c_hi; ++cell) {
        const int ls = a.cell_start[cell], le = a.cell_start[cell + 1];
        // the tile's piece of the cell's list (uniform: every thread finds the same bounds)
        int lo = ls, hi = le;
        while (lo < hi) {
            const int mid = lo + ((hi - lo) >> 1);
            if (a.coords[(size_t)a.cell_rows[mid] * 4] < r_lo) lo = mid + 1; else hi = mid;
        }
        const int first = lo;
        hi = le;
        while (lo < hi) {
            const int mid = lo + ((hi - lo) >> 1);
            if (a.coords[(size_t)a.cell_rows[mid] * 4] < r_hi) lo = mid + 1; else hi = mid;
        }
        const int last = lo;
        for (int g0 = first; g0 < last; g0 += 16) {
            const int m = min(16, last - g0);
            __syncthreads();   // the accumulator's zero fill; the previous tile's reads of xs and s_box
            for (int e = tid; e < 16 * (C / 4); e += FC_NT) {
                const int row = e / (C / 4), c4 = 4 * (e % (C / 4));
                f4 v = {0.f, 0.f, 0.f, 0.f};
                if (row < m) {
                    const size_t q = (size_t)a.cell_rows[g0 + row];
                    v = c4 < a.Ca ? *reinterpret_cast<const f4 *>(a.xa + q * a.Ca + c4)
                                  : *reinterpret_cast<const f4 *>(a.xb + q * a.Cb + (c4 - a.Ca));
                }
                *reinterpret_cast<f4 *>(xs + row * XS + c4) = v;
            }
            if (tid < 16) s_box[tid] = tid < m ? a.coords[(size_t)a.cell_rows[g0 + tid] * 4] - r_lo : -1;
            __syncthreads();
            const int box = s_box[pos];
            for (int nb = wave; nb < NB; nb += FC_NT / 64) {
                f4 d = {0.f, 0.f, 0.f, 0.f};
                for (int kb = 0; kb < KB; ++kb)
                    d = mfma4(d, a_frag(a.wpack, ((size_t)cell * KB + kb) * NB + nb, lane), b_frag(xs, pos, XS, kb, g));
                // D layout of mfma_f32.h, row pos.  A wave owns its channel blocks for the whole walk and the rows of a cell
                // are distinct boxes: every accumulator element is one wave's, in program order
                if ((unsigned)box < (unsigned)a.TR) {
                    f4 *o = reinterpret_cast<f4 *>(acc + box * a.Cout + 16 * nb + 4 * g);
                    *o = *o + d;
                }
            }
        }
    }
    __syncthreads();
    float *out = a.partial + ((size_t)blockIdx.y * a.R + r_lo) * a.Cout;
    for (int e = tid; e < (r_hi - r_lo) * a.Cout; e += FC_NT) out[e] = acc[e];
}

}  // namespace pdm

using namespace pdm;

static int fc_args(const char *who, long long Q, int R, int sx, int sy, int sz, int Ca, int Cb, int Cout) {
    PDM_REQUIRE(Q >= 0 && R >= 0 && sx >= 1 && sy >= 1 && sz >= 1, PDM_E_BADARG, "%s: Q=%lld R=%d grid (%d, %d, %d)", who, Q, R, sx, sy, sz);
    PDM_REQUIRE((long long)sx * sy * sz <= 32768, PDM_E_BADARG, "%s: %lld cells a box (at most 32768)", who, (long long)sx * sy * sz);
    PDM_REQUIRE(Ca >= 4 && Cb >= 0 && Ca % 4 == 0 && Cb % 4 == 0 && (Ca + Cb) % 16 == 0 && Ca + Cb <= 512, PDM_E_BADARG,
                "%s: C_a=%d C_b=%d (multiples of 4, the sum a multiple of 16 up to 512)", who, Ca, Cb);
    PDM_REQUIRE(Cout >= 16 && Cout % 16 == 0 && Cout <= 1024, PDM_E_BADARG, "%s: Cout=%d (a multiple of 16 up to 1024)", who, Cout);
    PDM_REQUIRE(Q < (1ll << 29) && (long long)R * Cout < (1ll << 31), PDM_E_TOOLARGE, "%s: Q=%lld rows or R * Cout = %lld", who, Q,
                (long long)R * Cout);
    return 0;
}

extern "C" size_t pdm_sparse_fc_packed_floats(int cells, int C, int Cout) {
    if (cells <= 0 || C <= 0 || Cout <= 0 || C % 16 || Cout % 16) return 0;
    return (size_t)cells * C * Cout;
}

extern "C" int pdm_sparse_fc_chunks(int R, int cells, int Cout) {
    if (R < 0 || cells <= 0 || Cout < 16 || Cout > 1024 || Cout % 16) return 0;
    return fc_plan(R, cells, Cout).nchunk;
}

extern "C" size_t pdm_sparse_fc_workspace_bytes(long long Q, int R, int cells, int Cout) {
    if (Q < 0 || R <= 0 || cells <= 0 || Cout < 16 || Cout > 1024 || Cout % 16) return 0;
    return fc_bytes(Q, R, cells, Cout);
}

extern "C" int pdm_sparse_fc(void *stream, long long Q, int R, int sx, int sy, int sz, int Ca, int Cb, int Cout, const int *coords,
                             const float *xa, const float *xb, const float *wpack, const float *scale, const float *shift, int relu,
                             float *out, void *workspace, size_t workspace_bytes) {
    const int rc = fc_args("sparse_fc", Q, R, sx, sy, sz, Ca, Cb, Cout);
    if (rc) return rc;
    if (R == 0) return 0;
    PDM_REQUIRE(out && (scale == nullptr) == (shift == nullptr), PDM_E_BADARG, "sparse_fc: null out, or one of scale and shift without the other");
    PDM_REQUIRE(Q == 0 || (coords && xa && wpack && (Cb == 0 || xb)), PDM_E_BADARG, "sparse_fc: null pointer");
    PDM_REQUIRE(Q == 0 || (((reinterpret_cast<uintptr_t>(xa) | reinterpret_cast<uintptr_t>(xb) | reinterpret_cast<uintptr_t>(wpack)) & 15) == 0),
                PDM_E_BADARG, "sparse_fc: the features and the packed weight are read 16 bytes at a time: 16-byte aligned");
    const int cells = sx * sy * sz;
    const size_t need = fc_bytes(Q, R, cells, Cout);
    PDM_REQUIRE(workspace && workspace_bytes >= need, PDM_E_BADARG, "sparse_fc: workspace of %zu bytes, need %zu", workspace_bytes, need);
    PDM_WS_ALIGNED("sparse_fc", workspace);
    const FcSpace ws = fc_carve(workspace, Q, R, cells);
    const FcPlan plan = fc_plan(R, cells, Cout);
    hipStream_t st = as_stream(stream);
    int nchunk = 0;
    if (Q > 0) {
        nchunk = plan.nchunk;
        hipLaunchKernelGGL(fc_box_start_kernel, dim3(divup(R + 1, FC_NT)), dim3(FC_NT), 0, st, (int)Q, R, coords, ws.box_start);
        hipLaunchKernelGGL(fc_cell_rows_kernel<false>, dim3(cells), dim3(FC_NT), 0, st, R, sy, sz, coords, ws.box_start, ws.cell_start, ws.cell_rows);
        hipLaunchKernelGGL(scan_totals_kernel<1024>, dim3(1), dim3(1024), 0, st, cells, ws.cell_start, (int *)nullptr, 0, -1);
        hipLaunchKernelGGL(fc_cell_rows_kernel<true>, dim3(cells), dim3(FC_NT), 0, st, R, sy, sz, coords, ws.box_start, ws.cell_start, ws.cell_rows);
        const size_t lds = ((size_t)plan.TR * Cout + 16 * (size_t)(Ca + Cb + 4)) * sizeof(float) + 16 * sizeof(int);
        if (lds > 64 * 1024) {
            const int e = grant_lds(reinterpret_cast<const void *>(&fc_main_kernel), 128 * 1024);
            PDM_REQUIRE(e == 0, PDM_E_TOOLARGE, "sparse_fc: cannot obtain %zu bytes of LDS: %s", lds, hipGetErrorString((hipError_t)e));
        }
        FcArgs a{R, plan.TR, cells, plan.chunk_cells, Ca, Cb, Cout, coords, xa, xb, wpack, ws.cell_start, ws.cell_rows, ws.partial};
        hipLaunchKernelGGL(fc_main_kernel, dim3(plan.tiles, plan.nchunk), dim3(FC_NT), lds, st, a);
    }
    hipLaunchKernelGGL(fc_reduce_kernel, dim3(divup((long long)R * Cout, FC_NT)), dim3(FC_NT), 0, st, R, Cout, nchunk, ws.partial, scale, shift,
                       relu, out);
    return check_launch("sparse_fc");
}

// Weight gradient of the sparse 3-D convolution, on the exact f32 MFMA with the ROWS as the contraction:
//     dW[co][k][ci] = sum over output rows i of dy[i][co] * x[nbr[i][k]][ci].
// Two phases, no float atomics:
//   1. a workgroup owns (row chunk, offset k).  It walks its chunk in tiles of 64 rows (32 at 128 x 128 channels); a tile in
//      which no row has offset k is skipped (the forward's tile mask, one offset of it).  The dy tile (A operand) and the
//      gathered x rows (B operand, zeros for -1) are staged in LDS row-major; mfma_f32_16x16x4f32 contracts 4 rows a step.  The
//      Cout/16 x Cin/16 accumulator blocks are split over the four waves.  The chunk's partial (Cout, Cin padded) block goes
//      to the workspace.
//   2. one launch sums the chunks in ascending order and writes (Cout, kvol, Cin) fp32, the layout of weight.grad.
// The chunk boundaries are a function of (P_out, kvol, Cin, Cout) alone (scw_chunk_rows), never of the device: two runs and
// a graph replay give the same bits.
// WIDE (pdm_sparse_conv_wide_wgrad): Cin or Cout = 256 does not fit the one-workgroup-holds-all-blocks layout (the
// 128 x 128 tile already fills LDS).  The (Cout, Cin) block runs as sub-blocks of at most 128 x 128 on a third grid dimension,
// z = (Cout sub-block) * (Cin sub-blocks) + (Cin sub-block): a sub-block reads its 128 columns of dy and of x at a column offset
// with the full row strides and writes its corner of the same [chunk][k][Cout][Cin] partial.  Every partial element has one
// writer and the same chain over the rows as a narrow run on those columns; phase two is unchanged.
#include "mfma_f32.h"

namespace pdm {

constexpr int SCW_T = 256;                          // 4 waves
constexpr int SCW_MAXK = 27;
constexpr int SCW_MIN_CHUNK = 1024;                 // rows of a chunk at least: 16 tiles
constexpr int SCW_MAX_CHUNKS = 1024;
constexpr size_t SCW_WS_CAP = (size_t)64 << 20;     // bytes of partials at most (one chunk is always allowed)

struct ScwArgs {
    int P_out, P_in, kvol, cin, cout, chunk_rows;
    const float *dy;        // (P_out, cout)
    const float *x;         // (P_in, cin)
    const int *nbr;         // (P_out, kvol)
    float *part;            // [chunk][k][cout][cin padded]
};

static int scw_cin_pad(int cin) { return cin < 16 ? 16 : cin; }
static bool scw_widths_ok(int cin, int cout) {
    return ((cin >= 3 && cin <= 8) || cin == 16 || cin == 32 || cin == 64 || cin == 128) && (cout == 16 || cout == 32 || cout == 64 || cout == 128);
}
static bool scw_widths_ok_wide(int cin, int cout) {
    return (cin == 256 || cout == 256) ? scw_widths_ok(cin == 256 ? 128 : cin, cout == 256 ? 128 : cout) : scw_widths_ok(cin, cout);
}
static size_t scw_partial_bytes(int kvol, int cin, int cout) { return sizeof(float) * (size_t)kvol * (size_t)cout * (size_t)scw_cin_pad(cin); }
// rows of a chunk: a multiple of 64, at least SCW_MIN_CHUNK, and large enough that the partials stay under both caps
static int scw_chunk_rows(int P_out, int kvol, int cin, int cout) {
    long long most = (long long)(SCW_WS_CAP / scw_partial_bytes(kvol, cin, cout));
    most = most < 1 ? 1 : (most > SCW_MAX_CHUNKS ? SCW_MAX_CHUNKS : most);
    long long rows = ((long long)P_out + most - 1) / most;
    rows = (rows + 63) / 64 * 64;
    return (int)(rows < SCW_MIN_CHUNK ? SCW_MIN_CHUNK : rows);
}

// LDS row stride in floats of a tile row of c = 16 n channels: = 16 mod 32, so that the two rows a 32-lane half reads in one
// ds_read_b32 (16 lanes each) fall on disjoint banks
constexpr int scw_stride(int c) { return c % 32 == 0 ? c + 16 : c; }

template <int CB, int IB, bool WIDE>
__global__ __launch_bounds__(SCW_T) void sparse_conv_wgrad_kernel(ScwArgs a) {
    constexpr int ROWS = (CB + IB == 16) ? 32 : 64;         // 128 x 128: two 64-row tiles would not fit 64 KB
    constexpr int SD = scw_stride(16 * CB), SX = scw_stride(16 * IB);
    constexpr int WC0 = CB >= 2 ? 2 : 1;
    constexpr int WI = IB < 4 / WC0 ? IB : 4 / WC0;         // waves across the Cin blocks
    constexpr int WC = CB < 4 / WI ? CB : 4 / WI;           // waves across the Cout blocks
    constexpr int NCB = CB / WC, NIB = IB / WI;             // blocks of one wave
    __shared__ int s_nbr[ROWS];
    __shared__ __attribute__((aligned(16))) float s_dy[ROWS * SD];
    __shared__ __attribute__((aligned(16))) float s_x[ROWS * SX];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int pos = lane & 15, g = lane >> 4;
    const int chunk = blockIdx.x, k = blockIdx.y;
    // WIDE: this workgroup's sub-block of (16 CB, 16 IB) channels and the partial's row stride (the whole padded Cin)
    const int nsub_i = WIDE && a.cin > 16 * IB ? a.cin / (16 * IB) : 1;
    const int co0 = WIDE ? ((int)blockIdx.z / nsub_i) * (16 * CB) : 0, ci0 = WIDE ? ((int)blockIdx.z % nsub_i) * (16 * IB) : 0;
    const int pstride = WIDE ? nsub_i * (16 * IB) : 16 * IB;
    const long long c0 = (long long)chunk * a.chunk_rows;
    const long long c1 = min(c0 + (long long)a.chunk_rows, (long long)a.P_out);
    const bool active = wave < WC * WI;
    const int cb0 = active ? (wave / WI) * NCB : 0, ib0 = active ? (wave % WI) * NIB : 0;
    const bool vec_dy = (reinterpret_cast<uintptr_t>(a.dy) & 15) == 0;
    const bool vec_x = (a.cin & 3) == 0 && (reinterpret_cast<uintptr_t>(a.x) & 15) == 0;

    f4 acc[NCB][NIB];
#pragma unroll
    for (int c = 0; c < NCB; ++c)
#pragma unroll
        for (int i = 0; i < NIB; ++i) acc[c][i] = f4{0.f, 0.f, 0.f, 0.f};

    for (long long r0 = c0; r0 < c1; r0 += ROWS) {
        const int live = (int)min((long long)ROWS, c1 - r0);
        int r = -1;
        if (tid < live) {
            r = a.nbr[(size_t)(r0 + tid) * a.kvol + k];
            if (r < 0 || r >= a.P_in) r = -1;
        }
        if (tid < ROWS) s_nbr[tid] = r;
        // the barrier also ends the previous tile's reads of s_dy and s_x
        if (!__syncthreads_or(r >= 0)) continue;
        for (int q = tid; q < ROWS * CB * 4; q += SCW_T) {
            const int row = q / (4 * CB), c = 4 * (q % (4 * CB));
            f4 v = {0.f, 0.f, 0.f, 0.f};
            if (row < live) v = load_quad(a.dy + (size_t)(r0 + row) * a.cout + co0 + c, vec_dy);
            *reinterpret_cast<f4 *>(&s_dy[row * SD + c]) = v;
        }
        for (int q = tid; q < ROWS * IB * 4; q += SCW_T) {
            const int row = q / (4 * IB), c = 4 * (q % (4 * IB));
            f4 v = {0.f, 0.f, 0.f, 0.f};
            const int rr = s_nbr[row];
            if (rr >= 0) v = load_quad_ragged(a.x + (size_t)rr * a.cin + ci0 + c, ci0 + c, a.cin, vec_x);
            *reinterpret_cast<f4 *>(&s_x[row * SX + c]) = v;
        }
        __syncthreads();
        if (active) {
#pragma unroll 4
            for (int s = 0; s < ROWS / 4; ++s) {
                // lane (pos, g): A[co = pos][row = g] and B[row = g][ci = pos] of the step's four rows
                float fa[NCB], fb[NIB];
#pragma unroll
                for (int c = 0; c < NCB; ++c) fa[c] = s_dy[(4 * s + g) * SD + 16 * (cb0 + c) + pos];
#pragma unroll
                for (int i = 0; i < NIB; ++i) fb[i] = s_x[(4 * s + g) * SX + 16 * (ib0 + i) + pos];
#pragma unroll
                for (int c = 0; c < NCB; ++c)
#pragma unroll
                    for (int i = 0; i < NIB; ++i) acc[c][i] = __builtin_amdgcn_mfma_f32_16x16x4f32(fa[c], fb[i], acc[c][i], 0, 0, 0);
            }
        }
    }

    // lane (pos, g), register j of block (c, i) = dW[co = 16 (cb0 + c) + 4 g + j][ci = 16 (ib0 + i) + pos]; written even when every
    // tile was skipped: phase two reads every partial
    if (!active) return;
    float *dst = a.part + (((size_t)chunk * a.kvol + k) * (size_t)a.cout + co0) * pstride + ci0;
#pragma unroll
    for (int c = 0; c < NCB; ++c)
#pragma unroll
        for (int i = 0; i < NIB; ++i) {
            const float v[4] = {acc[c][i].x, acc[c][i].y, acc[c][i].z, acc[c][i].w};
#pragma unroll
            for (int j = 0; j < 4; ++j) dst[(size_t)(16 * (cb0 + c) + 4 * g + j) * pstride + 16 * (ib0 + i) + pos] = v[j];
        }
}

// dW[co][k][ci] = the chunks' partials added in ascending chunk order; the columns past cin are dropped
__global__ __launch_bounds__(SCW_T) void sparse_conv_wgrad_reduce_kernel(int nchunks, int kvol, int cin, int cin_pad, int cout,
                                                                         const float *__restrict__ part, float *__restrict__ dw) {
    const int t = blockIdx.x * SCW_T + threadIdx.x;
    if (t >= cout * kvol * cin) return;
    const int ci = t % cin, k = (t / cin) % kvol, co = t / (cin * kvol);
    float s = 0.0f;
    for (int ch = 0; ch < nchunks; ++ch) s += part[(((size_t)ch * kvol + k) * cout + co) * cin_pad + ci];
    dw[t] = s;
}

template <int CB>
static void scw_launch(int ib, dim3 grid, hipStream_t s, const ScwArgs &a) {
    switch (ib) {
        case 1: hipLaunchKernelGGL((sparse_conv_wgrad_kernel<CB, 1, false>), grid, dim3(SCW_T), 0, s, a); break;
        case 2: hipLaunchKernelGGL((sparse_conv_wgrad_kernel<CB, 2, false>), grid, dim3(SCW_T), 0, s, a); break;
        case 4: hipLaunchKernelGGL((sparse_conv_wgrad_kernel<CB, 4, false>), grid, dim3(SCW_T), 0, s, a); break;
        default: hipLaunchKernelGGL((sparse_conv_wgrad_kernel<CB, 8, false>), grid, dim3(SCW_T), 0, s, a); break;
    }
}

// a 256-wide side runs as two sub-blocks of 8 blocks; the other side keeps its own block count
template <int CB>
static void scw_launch_wide(int ib, dim3 grid, hipStream_t s, const ScwArgs &a) {
    switch (ib) {
        case 1: hipLaunchKernelGGL((sparse_conv_wgrad_kernel<CB, 1, true>), grid, dim3(SCW_T), 0, s, a); break;
        case 2: hipLaunchKernelGGL((sparse_conv_wgrad_kernel<CB, 2, true>), grid, dim3(SCW_T), 0, s, a); break;
        case 4: hipLaunchKernelGGL((sparse_conv_wgrad_kernel<CB, 4, true>), grid, dim3(SCW_T), 0, s, a); break;
        default: hipLaunchKernelGGL((sparse_conv_wgrad_kernel<CB, 8, true>), grid, dim3(SCW_T), 0, s, a); break;
    }
}

}  // namespace pdm

using namespace pdm;

// rows of one chunk of pdm_sparse_conv_wgrad, a pure function of its arguments; 0 for sizes the operator rejects
extern "C" int pdm_sparse_conv_wgrad_chunk_rows(int P_out, int kvol, int Cin, int Cout) {
    if (P_out < 0 || kvol < 1 || kvol > SCW_MAXK || !scw_widths_ok(Cin, Cout)) return 0;
    return scw_chunk_rows(P_out, kvol, Cin, Cout);
}

// bytes of the partials (at least one chunk's); 0 for sizes the operator rejects
extern "C" size_t pdm_sparse_conv_wgrad_workspace_bytes(int P_out, int kvol, int Cin, int Cout) {
    if (P_out < 0 || kvol < 1 || kvol > SCW_MAXK || !scw_widths_ok(Cin, Cout)) return 0;
    const int nchunks = divup(P_out, scw_chunk_rows(P_out, kvol, Cin, Cout));
    return align256(scw_partial_bytes(kvol, Cin, Cout) * (size_t)(nchunks < 1 ? 1 : nchunks));
}

// dy (P_out, Cout), x (P_in, Cin), nbr (P_out, kvol) input rows or -1 (an entry outside [0, P_in) counts as -1) ->
// dw (Cout, kvol, Cin) fp32, every element written (zeros for P_out == 0).
static int scw_run(bool wide, void *stream, int P_out, int P_in, int kvol, int Cin, int Cout, const float *dy, const float *x, const int *nbr,
                   float *dw, void *workspace, size_t workspace_bytes) {
    PDM_REQUIRE(P_out >= 0 && P_in >= 0, PDM_E_BADARG, "sparse_conv_wgrad: bad size");
    PDM_REQUIRE(kvol >= 1 && kvol <= SCW_MAXK, PDM_E_BADARG, "sparse_conv_wgrad: %d offsets, at most %d", kvol, SCW_MAXK);
    if (wide) {
        PDM_REQUIRE((Cin >= 3 && Cin <= 8) || Cin == 16 || Cin == 32 || Cin == 64 || Cin == 128 || Cin == 256, PDM_E_BADARG,
                    "sparse_conv_wide_wgrad: %d input channels (3 to 8, 16, 32, 64, 128 or 256)", Cin);
        PDM_REQUIRE(Cout == 16 || Cout == 32 || Cout == 64 || Cout == 128 || Cout == 256, PDM_E_BADARG,
                    "sparse_conv_wide_wgrad: %d output channels (16, 32, 64, 128 or 256)", Cout);
    } else {
        PDM_REQUIRE((Cin >= 3 && Cin <= 8) || Cin == 16 || Cin == 32 || Cin == 64 || Cin == 128, PDM_E_BADARG,
                    "sparse_conv_wgrad: %d input channels (3 to 8, 16, 32, 64 or 128)", Cin);
        PDM_REQUIRE(Cout == 16 || Cout == 32 || Cout == 64 || Cout == 128, PDM_E_BADARG, "sparse_conv_wgrad: %d output channels (16, 32, 64 or 128)",
                    Cout);
    }
    PDM_REQUIRE((long long)P_out * kvol <= 0x7fffffffll, PDM_E_TOOLARGE, "sparse_conv_wgrad: %d rows x %d offsets exceed int32", P_out, kvol);
    PDM_REQUIRE(dw && workspace && (P_out == 0 || (dy && nbr)) && (P_out == 0 || P_in == 0 || x), PDM_E_BADARG, "sparse_conv_wgrad: null pointer");
    PDM_WS_ALIGNED("sparse_conv_wgrad", workspace);
    const int chunk_rows = scw_chunk_rows(P_out, kvol, Cin, Cout), nchunks = divup(P_out, chunk_rows);
    const size_t need = scw_partial_bytes(kvol, Cin, Cout) * (size_t)nchunks;
    PDM_REQUIRE(workspace_bytes >= need, PDM_E_BADARG, "sparse_conv_wgrad: workspace too small (%zu bytes, need %zu)", workspace_bytes, need);
    float *part = static_cast<float *>(workspace);
    hipStream_t s = as_stream(stream);
    const int cin_pad = scw_cin_pad(Cin);
    if (nchunks) {
        const ScwArgs a{P_out, P_in, kvol, Cin, Cout, chunk_rows, dy, x, nbr, part};
        if (Cin <= 128 && Cout <= 128) {        // the narrow launch, also under the wide entry: the same bits
            const dim3 grid((unsigned)nchunks, (unsigned)kvol);
            switch (Cout / 16) {
                case 1: scw_launch<1>(cin_pad / 16, grid, s, a); break;
                case 2: scw_launch<2>(cin_pad / 16, grid, s, a); break;
                case 4: scw_launch<4>(cin_pad / 16, grid, s, a); break;
                default: scw_launch<8>(cin_pad / 16, grid, s, a); break;
            }
        } else {
            const int cb = (Cout > 128 ? 128 : Cout) / 16, ib = (cin_pad > 128 ? 128 : cin_pad) / 16;
            const dim3 grid((unsigned)nchunks, (unsigned)kvol, (unsigned)((Cout / (16 * cb)) * (cin_pad / (16 * ib))));
            switch (cb) {
                case 1: scw_launch_wide<1>(ib, grid, s, a); break;
                case 2: scw_launch_wide<2>(ib, grid, s, a); break;
                case 4: scw_launch_wide<4>(ib, grid, s, a); break;
                default: scw_launch_wide<8>(ib, grid, s, a); break;
            }
        }
        if (int rc = check_launch("sparse_conv_wgrad(partials)")) return rc;
    }
    hipLaunchKernelGGL(sparse_conv_wgrad_reduce_kernel, dim3((unsigned)divup((long long)Cout * kvol * Cin, SCW_T)), dim3(SCW_T), 0, s, nchunks, kvol, Cin,
                       cin_pad, Cout, part, dw);
    return check_launch("sparse_conv_wgrad(sum)");
}

extern "C" int pdm_sparse_conv_wgrad(void *stream, int P_out, int P_in, int kvol, int Cin, int Cout, const float *dy, const float *x,
                                     const int *nbr, float *dw, void *workspace, size_t workspace_bytes) {
    return scw_run(false, stream, P_out, P_in, kvol, Cin, Cout, dy, x, nbr, dw, workspace, workspace_bytes);
}

// pdm_sparse_conv_wgrad and its two queries with Cin and Cout up to 256 (the WIDE note above).  The chunk rule is the narrow
// one, so for Cin, Cout <= 128 the launches and the bits are the narrow entry's.
extern "C" int pdm_sparse_conv_wide_wgrad_chunk_rows(int P_out, int kvol, int Cin, int Cout) {
    if (P_out < 0 || kvol < 1 || kvol > SCW_MAXK || !scw_widths_ok_wide(Cin, Cout)) return 0;
    return scw_chunk_rows(P_out, kvol, Cin, Cout);
}

extern "C" size_t pdm_sparse_conv_wide_wgrad_workspace_bytes(int P_out, int kvol, int Cin, int Cout) {
    if (P_out < 0 || kvol < 1 || kvol > SCW_MAXK || !scw_widths_ok_wide(Cin, Cout)) return 0;
    const int nchunks = divup(P_out, scw_chunk_rows(P_out, kvol, Cin, Cout));
    return align256(scw_partial_bytes(kvol, Cin, Cout) * (size_t)(nchunks < 1 ? 1 : nchunks));
}

extern "C" int pdm_sparse_conv_wide_wgrad(void *stream, int P_out, int P_in, int kvol, int Cin, int Cout, const float *dy, const float *x,
                                          const int *nbr, float *dw, void *workspace, size_t workspace_bytes) {
    return scw_run(true, stream, P_out, P_in, kvol, Cin, Cout, dy, x, nbr, dw, workspace, workspace_bytes);
}

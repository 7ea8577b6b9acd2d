// Sparse 3-D convolution over a rulebook (DESIGN.md "Voxel path"), output-stationary on the exact f32 MFMA:
//     out[i][:] = epilogue(sum_k W[k] x[nbr[i][k]][:]),      epilogue = (* scale + shift) -> (+ residual[i]) -> ReLU.
// A workgroup owns 64 output rows (a wave 16 of them, all output channels) and walks the offsets k in ascending order; an
// offset that none of the 64 rows has is skipped (a mask over the tile, a function of the input).  Per offset and per 16
// input channels the gathered rows (zeros for -1) and that slice of W[k] go through LDS: rows as the B operand, weights as
// the A operand of mfma_f32_16x16x4f32 in the packed fragment order of rows_gemm.hip, so that a lane's accumulator holds 4
// consecutive channels of one row.  No atomics and no split over k: two runs and a graph replay give the same bits.
// Two LDS stages; the global loads of step s + 2 are in flight while step s computes.
// SPLIT (pdm_sparse_conv_split, the training path's forward and data gradient): every offset's products are added
// in an accumulator of their own, which is then added to the running sum: the order of `per offset mm, then add`, whose rounding
// error is about a third of one long chain's.  The same operands, the same skip, no atomics; other bits than the plain form.
// WIDE (pdm_sparse_conv_wide, pdm_sparse_conv_wide_split): the same kernel with 256 channels admitted.  Cin = 256 is
// 16 blocks kb instead of 8; Cout = 256 is the NB = 16 instantiation, 16 accumulator blocks a lane over ONE gather of the rows
// (48 KB of weight and row stages instead of 32).  An output element's chain (k ascending, kb ascending, four MFMA steps a block)
// does not depend on how the output columns are blocked, so for Cin, Cout <= 128 the wide entries run the narrow instantiations
// and give the narrow entries' bits.
#include "mfma_f32.h"

namespace pdm {

constexpr int SCV_ROWS = 64;    // output rows per workgroup
constexpr int SCV_T = 256;      // 4 waves
constexpr int SCV_MAXK = 27;    // offsets at most (3 x 3 x 3): the tile's mask is one 32-bit word

struct ScvArgs {
    int P_out, P_in, kvol, cin, nkb, cout, relu;
    const float *x;         // (P_in, cin)
    const int *nbr;         // (P_out, kvol)
    const float *wpack;     // [k][kb][nb][lane][4]: W[k][cin = 16 kb + 4 (lane >> 4) + j][cout = 16 nb + (lane & 15)], zero past cin
    const float *scale, *shift, *residual;      // null or (cout), (cout), (P_out, cout)
    float *out;             // (P_out, cout)
};

template <int NB, bool SPLIT>
__global__ __launch_bounds__(SCV_T) void sparse_conv_kernel(ScvArgs a) {
    __shared__ int s_nbr[SCV_ROWS * SCV_MAXK];
    __shared__ unsigned s_mask;
    __shared__ __attribute__((aligned(16))) float s_x[2][SCV_ROWS * MFMA_ROW_STRIDE];
    __shared__ __attribute__((aligned(16))) float s_w[2][NB * 64 * 4];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int pos = lane & 15, g = lane >> 4;
    const long long r0 = (long long)blockIdx.x * SCV_ROWS;
    const int live = (int)min((long long)SCV_ROWS, a.P_out - r0);     // rows of this tile

    // the tile's neighbour table, and which offsets any of its rows has
    if (tid == 0) s_mask = 0;
    __syncthreads();
    unsigned mine = 0;
    for (int q = tid; q < SCV_ROWS * a.kvol; q += SCV_T) {
        int r = -1;
        if (q < live * a.kvol) r = a.nbr[(size_t)r0 * a.kvol + q];
        if (r < 0 || r >= a.P_in) r = -1;
        s_nbr[q] = r;
        if (r >= 0) mine |= 1u << (q % a.kvol);
    }
    if (mine) atomicOr(&s_mask, mine);
    __syncthreads();
    const unsigned mask = s_mask;
    const int steps = __popc(mask) * a.nkb;

    // staging roles: channels [4 part, +4) of the 16-channel slice of row hrow; float4 tid (and tid + 256) of the weight slice
    const int hrow = tid >> 2, part = tid & 3;
    const bool vec_x = (a.cin & 3) == 0 && (reinterpret_cast<uintptr_t>(a.x) & 15) == 0;
    auto load_x = [&](int k, int kb) {
        const int r = s_nbr[hrow * a.kvol + k];
        if (r < 0) return f4{0.f, 0.f, 0.f, 0.f};
        const int c = 16 * kb + 4 * part;
        return load_quad_ragged(a.x + (size_t)r * a.cin + c, c, a.cin, vec_x);
    };
    constexpr int WQ = (NB * 64 + SCV_T - 1) / SCV_T;      // float4s of a weight slice per thread
    struct Regs { f4 x, w[WQ]; };
    auto load = [&](int k, int kb) {
        Regs r;
        r.x = load_x(k, kb);
        const f4 *src = reinterpret_cast<const f4 *>(a.wpack) + ((size_t)k * a.nkb + kb) * (NB * 64);
#pragma unroll
        for (int q = 0; q < WQ; ++q) {
            r.w[q] = f4{0.f, 0.f, 0.f, 0.f};
            if (tid + q * SCV_T < NB * 64) r.w[q] = src[tid + q * SCV_T];
        }
        return r;
    };
    auto stage = [&](int buf, const Regs &r) {
        *reinterpret_cast<f4 *>(&s_x[buf][hrow * MFMA_ROW_STRIDE + 4 * part]) = r.x;
#pragma unroll
        for (int q = 0; q < WQ; ++q)
            if (tid + q * SCV_T < NB * 64) reinterpret_cast<f4 *>(s_w[buf])[tid + q * SCV_T] = r.w[q];
    };
    // the loads run ahead of the MFMAs: a cursor over (present offset, 16-channel block) in ascending order
    unsigned rem = mask;
    int lk = rem ? __ffs((int)rem) - 1 : 0, lkb = 0;
    auto advance = [&]() {
        if (++lkb == a.nkb) {
            lkb = 0;
            rem &= rem - 1;
            lk = rem ? __ffs((int)rem) - 1 : 0;
        }
    };

    f4 acc[NB], sum[SPLIT ? NB : 1];       // SPLIT: acc holds the current offset's products, sum the offsets before it
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) acc[nb] = f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int nb = 0; nb < (SPLIT ? NB : 1); ++nb) sum[nb] = f4{0.f, 0.f, 0.f, 0.f};
    int kb_of_step = 0;

    Regs regs{};
    if (steps > 0) {
        regs = load(lk, lkb); advance();
        stage(0, regs);
    }
    __syncthreads();
    if (steps > 1) { regs = load(lk, lkb); advance(); }
    for (int s = 0; s < steps; ++s) {
        const int cur = s & 1;
        if (SPLIT) {        // a new offset begins every nkb steps
            if (kb_of_step == a.nkb) {
                kb_of_step = 0;
#pragma unroll
                for (int nb = 0; nb < NB; ++nb) {
                    sum[nb] += acc[nb];
                    acc[nb] = f4{0.f, 0.f, 0.f, 0.f};
                }
            }
            ++kb_of_step;
        }
        const f4 fb = b_frag(s_x[cur], 16 * wave + pos, MFMA_ROW_STRIDE, 0, g);
        f4 fa[NB];
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) fa[nb] = a_frag(s_w[cur], nb, lane);
        if (s + 1 < steps) stage(cur ^ 1, regs);        // that stage was last read in step s - 1, behind the barrier
        if (s + 2 < steps) { regs = load(lk, lkb); advance(); }
        mfma4_grid(acc, fa, fb);
        __syncthreads();
    }

    if (SPLIT) {
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) acc[nb] = sum[nb] + acc[nb];
    }
    // D layout of mfma_f32.h: row r0 + 16 wave + pos
    const int lrow = 16 * wave + pos;
    if (lrow >= live) return;
    const size_t row = (size_t)(r0 + lrow);
    const bool vec_o = (reinterpret_cast<uintptr_t>(a.out) & 15) == 0;
    const bool vec_r = a.residual && (reinterpret_cast<uintptr_t>(a.residual) & 15) == 0;
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) {
        const int c0 = 16 * nb + 4 * g;
        f4 v = scale_shift_relu4(acc[nb], a.scale, a.shift, c0, false);
        if (a.residual) v += load_quad(a.residual + row * a.cout + c0, vec_r);
        store_quad(a.out + row * a.cout + c0, scale_shift_relu4(v, nullptr, nullptr, c0, a.relu), vec_o);
    }
}

}  // namespace pdm

using namespace pdm;

// floats of the packed weights of one convolution: kvol x ceil(Cin / 16) x (Cout / 16) blocks of 64 lanes x 4
extern "C" size_t pdm_sparse_conv_packed_floats(int kvol, int Cin, int Cout) {
    if (kvol < 1 || Cin < 1 || Cout < 16 || (Cout & 15)) return 0;
    return (size_t)kvol * (size_t)((Cin + 15) / 16) * (size_t)(Cout / 16) * 256;
}

// x (P_in, Cin), nbr (P_out, kvol) input rows or -1 (an entry outside [0, P_in) counts as -1), wpack as above (16-byte
// aligned) -> out (P_out, Cout).  scale and shift come together or not at all; residual (P_out, Cout) or null.
template <bool SPLIT>
static int scv_run(bool wide, void *stream, int P_out, int P_in, int kvol, int Cin, int Cout, const float *x, const int *nbr, const float *wpack,
                   const float *scale, const float *shift, const float *residual, int relu, float *out) {
    PDM_REQUIRE(P_out >= 0 && P_in >= 0, PDM_E_BADARG, "sparse_conv: bad size");
    PDM_REQUIRE(kvol >= 1 && kvol <= SCV_MAXK, PDM_E_BADARG, "sparse_conv: %d offsets, at most %d", kvol, SCV_MAXK);
    if (wide) {
        PDM_REQUIRE((Cin >= 3 && Cin <= 8) || Cin == 16 || Cin == 32 || Cin == 64 || Cin == 128 || Cin == 256, PDM_E_BADARG,
                    "sparse_conv_wide: %d input channels (3 to 8, 16, 32, 64, 128 or 256)", Cin);
        PDM_REQUIRE(Cout == 16 || Cout == 32 || Cout == 64 || Cout == 128 || Cout == 256, PDM_E_BADARG,
                    "sparse_conv_wide: %d output channels (16, 32, 64, 128 or 256)", Cout);
    } else {
        PDM_REQUIRE((Cin >= 3 && Cin <= 8) || Cin == 16 || Cin == 32 || Cin == 64 || Cin == 128, PDM_E_BADARG,
                    "sparse_conv: %d input channels (3 to 8, 16, 32, 64 or 128)", Cin);
        PDM_REQUIRE(Cout == 16 || Cout == 32 || Cout == 64 || Cout == 128, PDM_E_BADARG, "sparse_conv: %d output channels (16, 32, 64 or 128)", Cout);
    }
    PDM_REQUIRE((long long)P_out * kvol <= 0x7fffffffll, PDM_E_TOOLARGE, "sparse_conv: %d rows x %d offsets exceed int32", P_out, kvol);
    PDM_REQUIRE((scale == nullptr) == (shift == nullptr), PDM_E_BADARG, "sparse_conv: scale and shift come together");
    if (P_out == 0) return 0;
    PDM_REQUIRE(nbr && wpack && out && (P_in == 0 || x), PDM_E_BADARG, "sparse_conv: null pointer");
    PDM_REQUIRE((reinterpret_cast<uintptr_t>(wpack) & 15) == 0, PDM_E_BADARG, "sparse_conv: packed weights must be 16-byte aligned");
    ScvArgs a{P_out, P_in, kvol, Cin, (Cin + 15) / 16, Cout, relu != 0, x, nbr, wpack, scale, shift, residual, out};
    const dim3 grid((unsigned)divup(P_out, SCV_ROWS)), block(SCV_T);
    hipStream_t s = as_stream(stream);
    switch (Cout / 16) {
        case 1: hipLaunchKernelGGL((sparse_conv_kernel<1, SPLIT>), grid, block, 0, s, a); break;
        case 2: hipLaunchKernelGGL((sparse_conv_kernel<2, SPLIT>), grid, block, 0, s, a); break;
        case 4: hipLaunchKernelGGL((sparse_conv_kernel<4, SPLIT>), grid, block, 0, s, a); break;
        case 8: hipLaunchKernelGGL((sparse_conv_kernel<8, SPLIT>), grid, block, 0, s, a); break;
        default: hipLaunchKernelGGL((sparse_conv_kernel<16, SPLIT>), grid, block, 0, s, a); break;
    }
    return check_launch("sparse_conv");
}

extern "C" int pdm_sparse_conv(void *stream, int P_out, int P_in, int kvol, int Cin, int Cout, const float *x, const int *nbr, const float *wpack,
                               const float *scale, const float *shift, const float *residual, int relu, float *out) {
    return scv_run<false>(false, stream, P_out, P_in, kvol, Cin, Cout, x, nbr, wpack, scale, shift, residual, relu, out);
}

// pdm_sparse_conv with one accumulator per offset added to a running sum (the SPLIT form above): what the training path runs in
// its forward and its data gradient.  Same arguments, same checks, as deterministic; not the same bits as pdm_sparse_conv.
extern "C" int pdm_sparse_conv_split(void *stream, int P_out, int P_in, int kvol, int Cin, int Cout, const float *x, const int *nbr,
                                     const float *wpack, const float *scale, const float *shift, const float *residual, int relu, float *out) {
    return scv_run<true>(false, stream, P_out, P_in, kvol, Cin, Cout, x, nbr, wpack, scale, shift, residual, relu, out);
}

// pdm_sparse_conv and pdm_sparse_conv_split with Cin and Cout up to 256 (the WIDE note above): the same arguments, checks, chain and
// epilogue; for Cin, Cout <= 128 the same launches, so the same bits.
extern "C" int pdm_sparse_conv_wide(void *stream, int P_out, int P_in, int kvol, int Cin, int Cout, const float *x, const int *nbr,
                                    const float *wpack, const float *scale, const float *shift, const float *residual, int relu, float *out) {
    return scv_run<false>(true, stream, P_out, P_in, kvol, Cin, Cout, x, nbr, wpack, scale, shift, residual, relu, out);
}

extern "C" int pdm_sparse_conv_wide_split(void *stream, int P_out, int P_in, int kvol, int Cin, int Cout, const float *x, const int *nbr,
                                          const float *wpack, const float *scale, const float *shift, const float *residual, int relu,
                                          float *out) {
    return scv_run<true>(true, stream, P_out, P_in, kvol, Cin, Cout, x, nbr, wpack, scale, shift, residual, relu, out);
}

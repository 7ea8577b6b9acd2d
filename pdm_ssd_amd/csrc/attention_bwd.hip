// Backward of the fused multi-head attention (attention.hip, pdm_mha_forward_train) in fp32: the P x N matrix is never
// stored; P_ij is recomputed from the saved (raw maximum, sum) of its query and the dropout mask M_ij from the draws.
//   D_i   = dO_i . O_i
//   dP_ij = r M_ij (dO_i . V_j)                 r = 1 / (1 - p)
//   dS_ij = P_ij (dP_ij - D_i)
//   dV_j  = sum_i r M_ij P_ij dO_i,   dK_j = scale sum_i dS_ij Q_i,   dQ_i = scale sum_j dS_ij K_j
//
// mha_bwd_delta_kernel  D_i per (sample, head, query), channels summed in order.
// mha_bwd_kernel        key-stationary: a workgroup of NW waves owns 16 NW keys of one (sample, head), a wave 16 of them,
//                       held in registers, and walks all query tiles of 16 in ascending order.  All five products run on
//                       v_mfma_f32_16x16x4_f32.  Per tile a lane holds, of S^T = K Q^T and dP^T = V dO^T, the keys
//                       4 (lane >> 4) + r of ONE query (lane & 15), so the query's maximum, sum and D are lane scalars.
//                         dQ^T = K^T dS^T  contracts over keys: B = the lane's own dS[r], A = K read at [key 4 grp + r]
//                                [channel col] -- no value changes lanes (the forward's P V)
//                         dV^T = dO^T Pd   and   dK^T = Q^T dS   contract over queries: the B operand is the tile
//                                transposed, [query 4 grp + r][key col]; it goes through 1 KB of LDS per tile and wave
//                       The wave's dQ^T tile goes to LDS, the workgroup sums the NW tiles in wave order and writes the
//                       block's partial.  dk and dv have one writer per element and one summation order.
// mha_bwd_fold_kernel   dq = scale * the partials summed in ascending block order.
//
// The block size depends on (N, keys_per_chunk) alone, there is no atomic: two runs give the same bits.  Queries >= P and
// keys >= N are read from the last real row and enter with P_ij = 0, so they contribute exactly 0.
#include "attention.h"
#include "draws.h"

namespace pdm {

constexpr int MHAB_T = 256;   // threads of the two small kernels

struct MhaBwdArgs {
    int B, P, N, C, H, nblk, vec, drop;
    const float *q, *k, *v, *out, *dout, *stats;
    long long qs, ks, vs, dqs, dks, dvs;   // row strides in elements
    float c, scale, rinv;                  // log2(e) / sqrt(d), 1 / sqrt(d), 1 / (1 - p)
    unsigned thresh, seed;
    const unsigned *used_step;
    float *delta;                          // (B, H, P)
    float *dqp;                            // (B, H, nblk, P, d)
    float *dq, *dk, *dv;
};

__global__ __launch_bounds__(MHAB_T) void mha_bwd_delta_kernel(MhaBwdArgs a, int D) {
    const long long i = (long long)blockIdx.x * MHAB_T + threadIdx.x;
    if (i >= (long long)a.B * a.H * a.P) return;
    const int p = (int)(i % a.P);
    const long long bh = i / a.P;
    const int h = (int)(bh % a.H), b = (int)(bh / a.H);
    const size_t row = ((size_t)b * a.P + p) * a.C + h * D;
    float acc = 0.0f;
    for (int dd = 0; dd < D; ++dd) acc += a.dout[row + dd] * a.out[row + dd];
    a.delta[i] = acc;
}

template <int D, int NW>
__global__ __launch_bounds__(NW * 64) void mha_bwd_kernel(MhaBwdArgs a) {
    constexpr int DT = D / 16;
    __shared__ __attribute__((aligned(16))) float s_pd[NW][16 * 16];    // [query][key], the wave's own
    __shared__ __attribute__((aligned(16))) float s_ds[NW][16 * 16];
    __shared__ __attribute__((aligned(16))) float s_dq[NW][16 * D];     // [query][channel]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, col = lane & 15, grp = lane >> 4;
    const int blk = blockIdx.x, b = blockIdx.y / a.H, h = blockIdx.y - b * a.H;
    const int k0 = (blk * NW + wave) * 16;                             // may be >= N: the wave then only adds zeros
    const int krow_c = min(k0 + col, a.N - 1);
    const float *kb = a.k + (size_t)b * a.N * a.ks + h * D;
    const float *vb = a.v + (size_t)b * a.N * a.vs + h * D;
    f4 kA[DT], vA[DT];                                              // [key col][channels 16 t + 4 grp ..]
    float kS[DT][4];                                                   // [key 4 grp + r][channel 16 t + col]
#pragma unroll
    for (int t = 0; t < DT; ++t) {
        kA[t] = load_quad(kb + (size_t)krow_c * a.ks + 16 * t + 4 * grp, a.vec);
        vA[t] = load_quad(vb + (size_t)krow_c * a.vs + 16 * t + 4 * grp, a.vec);
#pragma unroll
        for (int r = 0; r < 4; ++r) kS[t][r] = kb[(size_t)min(k0 + 4 * grp + r, a.N - 1) * a.ks + 16 * t + col];
    }
    f4 dk[DT], dv[DT];                                              // ^T: [channel 16 t + 4 grp + r][key col]
#pragma unroll
    for (int t = 0; t < DT; ++t) { dk[t] = f4{0, 0, 0, 0}; dv[t] = f4{0, 0, 0, 0}; }
    const unsigned step = a.drop ? a.used_step[0] : 0u;
    const size_t bh = (size_t)b * a.H + h;
    const float *qb = a.q + (size_t)b * a.P * a.qs + h * D;
    const float *dob = a.dout + (size_t)b * a.P * a.C + h * D;
    float *dqp = a.dqp + (bh * a.nblk + blk) * (size_t)a.P * D;

    for (int q0 = 0; q0 < a.P; q0 += 16) {
        const int qrow = min(q0 + col, a.P - 1);
        f4 qB[DT], doB[DT];                                         // [query col][channels 16 t + 4 grp ..]
        float qS[DT][4], doS[DT][4];                                   // [query 4 grp + r][channel 16 t + col]
#pragma unroll
        for (int t = 0; t < DT; ++t) {
            qB[t] = load_quad(qb + (size_t)qrow * a.qs + 16 * t + 4 * grp, a.vec);
            doB[t] = load_quad(dob + (size_t)qrow * a.C + 16 * t + 4 * grp, a.vec);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int qr = min(q0 + 4 * grp + r, a.P - 1);
                qS[t][r] = qb[(size_t)qr * a.qs + 16 * t + col];
                doS[t][r] = dob[(size_t)qr * a.C + 16 * t + col];
            }
        }
        const float M = a.stats[2 * (bh * a.P + qrow)], rden = 1.0f / a.stats[2 * (bh * a.P + qrow) + 1];
        const float delta = a.delta[bh * a.P + qrow];
        const bool qlive = q0 + col < a.P;
        unsigned dkey = 0;
        if (a.drop) dkey = draw_key(a.seed, step, (unsigned)blockIdx.y, (unsigned)(q0 + col));

        f4 s = f4{0, 0, 0, 0}, dp = f4{0, 0, 0, 0};          // [key 4 grp + r][query col]
#pragma unroll
        for (int t = 0; t < DT; ++t)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                s = __builtin_amdgcn_mfma_f32_16x16x4f32(kA[t][i], qB[t][i], s, 0, 0, 0);
                dp = __builtin_amdgcn_mfma_f32_16x16x4f32(vA[t][i], doB[t][i], dp, 0, 0, 0);
            }
        f4 pd, ds;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int key = k0 + 4 * grp + r;
            float p = exp2f((s[r] - M) * a.c) * rden;
            if (!qlive || key >= a.N) p = 0.0f;
            float w = 1.0f;                                            // r M_ij
            if (a.drop) w = attn_keep(dkey, (unsigned)key, a.thresh) ? a.rinv : 0.0f;
            pd[r] = p * w;
            ds[r] = p * (dp[r] * w - delta);
        }
        // the tiles transposed: written [query col][keys 4 grp ..], read [query 4 grp + r][key col]
        *reinterpret_cast<f4 *>(&s_pd[wave][col * 16 + 4 * grp]) = pd;
        *reinterpret_cast<f4 *>(&s_ds[wave][col * 16 + 4 * grp]) = ds;
        f4 dq[DT];
#pragma unroll
        for (int t = 0; t < DT; ++t) {
            dq[t] = f4{0, 0, 0, 0};
#pragma unroll
            for (int r = 0; r < 4; ++r) dq[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(kS[t][r], ds[r], dq[t], 0, 0, 0);
            *reinterpret_cast<f4 *>(&s_dq[wave][col * D + 16 * t + 4 * grp]) = dq[t];   // [channel 16 t + 4 grp + r][query col]
        }
        __syncthreads();
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float pt = s_pd[wave][(4 * grp + r) * 16 + col], dt = s_ds[wave][(4 * grp + r) * 16 + col];
#pragma unroll
            for (int t = 0; t < DT; ++t) {
                dv[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(doS[t][r], pt, dv[t], 0, 0, 0);
                dk[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(qS[t][r], dt, dk[t], 0, 0, 0);
            }
        }
        for (int e = threadIdx.x; e < 16 * D; e += NW * 64) {          // the block's dQ partial: the waves in order
            float acc = s_dq[0][e];
#pragma unroll
            for (int w = 1; w < NW; ++w) acc += s_dq[w][e];
            const int qq = q0 + e / D;
            if (qq < a.P) dqp[(size_t)qq * D + (e % D)] = acc;
        }
        __syncthreads();
    }
    if (k0 + col >= a.N) return;
    float *dkp = a.dk + ((size_t)b * a.N + k0 + col) * a.dks + h * D + 4 * grp;
    float *dvp = a.dv + ((size_t)b * a.N + k0 + col) * a.dvs + h * D + 4 * grp;
#pragma unroll
    for (int t = 0; t < DT; ++t) {
        store_quad(dkp + 16 * t, dk[t] * a.scale, a.vec);
        store_quad(dvp + 16 * t, dv[t], a.vec);
    }
}

__global__ __launch_bounds__(MHAB_T) void mha_bwd_fold_kernel(MhaBwdArgs a, int D) {
    const long long i = (long long)blockIdx.x * MHAB_T + threadIdx.x;
    if (i >= (long long)a.B * a.P * a.C) return;
    const int ch = (int)(i % a.C), h = ch / D, dd = ch - h * D;
    const long long bp = i / a.C;
    const int p = (int)(bp % a.P), b = (int)(bp / a.P);
    const float *src = a.dqp + (((size_t)b * a.H + h) * a.nblk * a.P + p) * D + dd;
    float acc = 0.0f;
    for (int blk = 0; blk < a.nblk; ++blk) acc += src[(size_t)blk * a.P * D];   // block order
    a.dq[((size_t)b * a.P + p) * a.dqs + ch] = acc * a.scale;
}

// waves per workgroup = keys per block / 16: a function of (N, keys_per_chunk) alone
static int mha_bwd_waves(int N, int keys_per_chunk) {
    const int want = keys_per_chunk > 0 ? keys_per_chunk : (N >= 2048 ? 256 : (N >= 512 ? 64 : 16));
    return want >= 256 ? 16 : (want >= 64 ? 4 : 1);
}

template <int D>
static void mha_bwd_launch(int nw, dim3 grid, hipStream_t s, const MhaBwdArgs &a) {
    if (nw == 16) hipLaunchKernelGGL((mha_bwd_kernel<D, 16>), grid, dim3(1024), 0, s, a);
    else if (nw == 4) hipLaunchKernelGGL((mha_bwd_kernel<D, 4>), grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL((mha_bwd_kernel<D, 1>), grid, dim3(64), 0, s, a);
}

}  // namespace pdm

using namespace pdm;

extern "C" int pdm_mha_backward_keys_per_block(int N, int keys_per_chunk) { return 16 * mha_bwd_waves(N, keys_per_chunk); }

// 0 for a shape pdm_mha_backward rejects
extern "C" size_t pdm_mha_backward_workspace_bytes(int B, int P, int N, int C, int nheads, int keys_per_chunk) {
    if (!mha_supported(B, P, N, C, nheads, keys_per_chunk) || B == 0) return 0;
    const size_t nblk = (size_t)divup(N, 16 * mha_bwd_waves(N, keys_per_chunk));
    return align256((size_t)B * nheads * P * sizeof(float)) + (size_t)B * nblk * P * C * sizeof(float);
}

extern "C" int pdm_mha_backward(void *stream, int B, int P, int N, int C, int nheads, const float *q, long long q_stride,
                                const float *k, long long k_stride, const float *v, long long v_stride, const float *out,
                                const float *dout, const float *stats, double dropout_p, unsigned seed,
                                const unsigned *used_step, int keys_per_chunk, float *dq, long long dq_stride, float *dk,
                                long long dk_stride, float *dv, long long dv_stride, void *workspace, size_t workspace_bytes) {
    PDM_REQUIRE(mha_supported(B, P, N, C, nheads, keys_per_chunk), PDM_E_BADARG,
                "mha_backward: B = %d, P = %d, N = %d, C = %d, heads = %d, keys_per_chunk = %d: needs P, N >= 1, C <= 256 and "
                "C / heads in {16, 32}", B, P, N, C, nheads, keys_per_chunk);
    PDM_REQUIRE(mha_dropout_ok(dropout_p), PDM_E_BADARG, "mha_backward: dropout_p = %g outside [0, 1)", dropout_p);
    PDM_REQUIRE(q_stride >= C && k_stride >= C && v_stride >= C && dq_stride >= C && dk_stride >= C && dv_stride >= C,
                PDM_E_BADARG, "mha_backward: a row stride below C = %d", C);
    if (B == 0) return 0;
    const bool drop = dropout_p > 0.0;
    PDM_REQUIRE(q && k && v && out && dout && stats && dq && dk && dv && workspace && (!drop || used_step), PDM_E_BADARG,
                "mha_backward: null pointer");
    const int nw = mha_bwd_waves(N, keys_per_chunk), nblk = divup(N, 16 * nw), d = C / nheads;
    PDM_REQUIRE((long long)B * nheads <= 65535 && (long long)B * P * C <= 0x7fffffffll, PDM_E_TOOLARGE,
                "mha_backward: %lld sample-heads exceed the grid", (long long)B * nheads);
    const size_t need = pdm_mha_backward_workspace_bytes(B, P, N, C, nheads, keys_per_chunk);
    PDM_REQUIRE(workspace_bytes >= need && (reinterpret_cast<uintptr_t>(workspace) & 7) == 0, PDM_E_BADARG,
                "mha_backward: workspace of %zu bytes, need %zu (8-byte aligned)", workspace_bytes, need);
    MhaBwdArgs a{};
    a.B = B; a.P = P; a.N = N; a.C = C; a.H = nheads; a.nblk = nblk; a.drop = drop;
    a.q = q; a.k = k; a.v = v; a.out = out; a.dout = dout; a.stats = stats;
    a.qs = q_stride; a.ks = k_stride; a.vs = v_stride; a.dqs = dq_stride; a.dks = dk_stride; a.dvs = dv_stride;
    // the forward's condition, extended to every buffer of this call (C % 4 == 0 by d in {16, 32}: dout rows stay aligned)
    a.vec = mha_aligned16(q) && mha_aligned16(k) && mha_aligned16(v) && mha_aligned16(out) && mha_aligned16(dout) &&
            mha_aligned16(dq) && mha_aligned16(dk) && mha_aligned16(dv) && q_stride % 4 == 0 && k_stride % 4 == 0 &&
            v_stride % 4 == 0 && dq_stride % 4 == 0 && dk_stride % 4 == 0 && dv_stride % 4 == 0;
    a.c = (float)(1.4426950408889634 / sqrt((double)d));
    a.scale = (float)(1.0 / sqrt((double)d));
    a.rinv = mha_dropout_rinv(dropout_p); a.thresh = mha_dropout_thresh(dropout_p); a.seed = seed; a.used_step = used_step;
    a.delta = static_cast<float *>(workspace);
    a.dqp = reinterpret_cast<float *>(static_cast<char *>(workspace) + align256((size_t)B * nheads * P * sizeof(float)));
    a.dq = dq; a.dk = dk; a.dv = dv;
    hipStream_t s = as_stream(stream);
    hipLaunchKernelGGL(mha_bwd_delta_kernel, dim3((unsigned)divup((long long)B * nheads * P, MHAB_T)), dim3(MHAB_T), 0, s, a, d);
    if (int rc = check_launch("mha_backward(delta)")) return rc;
    const dim3 grid((unsigned)nblk, (unsigned)(B * nheads));
    if (d == 16) mha_bwd_launch<16>(nw, grid, s, a);
    else mha_bwd_launch<32>(nw, grid, s, a);
    if (int rc = check_launch("mha_backward(keys)")) return rc;
    hipLaunchKernelGGL(mha_bwd_fold_kernel, dim3((unsigned)divup((long long)B * P * C, MHAB_T)), dim3(MHAB_T), 0, s, a, d);
    return check_launch("mha_backward(fold)");
}

// Fused multi-head attention forward in fp32: out = softmax(q_h k_h^T / sqrt(d)) v_h per head, heads concatenated -- what
// sits between nn.MultiheadAttention's in-projection and out-projection with no mask and no dropout.
//
// The transformer head's cross-attention has few queries (200) and many keys (H * W = 32 400): a grid over (sample,
// head, query tile) alone is a few dozen workgroups.  So the keys are split into chunks of keys_per_chunk:
//
// mha_partial_kernel   one workgroup of 4 waves per (sample x head, key chunk, 64 queries); a wave owns 16 queries and
//                      walks its chunk 64 keys at a time with an online softmax.  Both products run on
//                      v_mfma_f32_16x16x4_f32 and are oriented so that no value changes lanes between them:
//                        S^T = K Q^T   A = K tile, B = Q: a lane ends with 4 scores of ONE query (column lane & 15) and the
//                                      keys 4 (lane >> 4) + r of the tile: a query's row is spread over 4 lanes x 4 registers,
//                                      its maximum is 15 fmax and two __shfl_xor (16, 32)
//                        O^T = V^T P^T A = V read at [key 4 (lane >> 4) + r][channel lane & 15], B = the lane's own p[r]:
//                                      the MFMA's k index is a key, and a sum over keys does not care in which order the
//                                      four k slots name them, as long as A and B name them alike
//                      Every step rescales (no deferred maximum): alpha = exp2((m_old - m_new) c) multiplies the running
//                      sum and the accumulator before the tile's P V is added, so a jump of the maximum at any tile is the
//                      ordinary path.  The maximum is kept in raw score units and the difference (s - m) is formed BEFORE
//                      the multiplication by c = log2(e) / sqrt(d): a large common offset of the scores costs no digits.
//                      Writes the chunk's (raw maximum, sum, unnormalised accumulator).
// mha_combine_kernel   one thread per output element: the partials of its query folded in chunk order.
//
// The chunking depends on (N, keys_per_chunk) alone, there is no atomic and no LDS: two runs give the same bits.  A
// single key gives out = its v row bit for bit (p = exp2(0) = 1, fma(v, 1, 0) = v, v / 1 = v).
//
// The training forward (pdm_mha_forward_train) is the same device code with TRAIN = true: the attention dropout multiplies
// the weights that enter the P V product (draws.h: attn_keep), the softmax sum stays the sum before dropout, and the combine
// kernel also writes the query's (raw maximum, sum) for the backward (attention_bwd.hip) and advances the step counter.
#include "attention.h"
#include "draws.h"

namespace pdm {

constexpr int MHA_T = 256;          // 4 waves
constexpr int MHA_QW = 16;          // queries per wave
constexpr int MHA_QB = 64;          // queries per workgroup
constexpr int MHA_KT = 64;          // keys per step of a wave: 4 tiles of 16

struct MhaArgs {
    int B, P, N, C, H, kpc, nchunk, vec;
    const float *q, *k, *v;
    long long qs, ks, vs;            // row strides in elements; a sample is `rows` rows on
    float c;                         // log2(e) / sqrt(d)
    float *ml;                       // (B, H, nchunk, P, 2): raw maximum, sum
    float *acc;                      // (B, H, nchunk, P, d)
    float *out;                      // (B, P, C)
    // TRAIN only
    int drop;                        // dropout_p > 0
    unsigned thresh, seed;           // floor(p 2^32); the draws' seed
    float rinv;                      // 1 / (1 - p)
    unsigned *step, *used_step;      // the device step counter and the copy of the value this call used
    float *stats;                    // (B, H, P, 2): raw maximum over all keys, softmax sum
};

template <int D, bool TRAIN>
__global__ __launch_bounds__(MHA_T) void mha_partial_kernel(MhaArgs a) {
    constexpr int DT = D / 16;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, col = lane & 15, grp = lane >> 4;
    const int q0 = (blockIdx.x * (MHA_QB / MHA_QW) + wave) * MHA_QW;
    if (q0 >= a.P) return;                                           // the whole wave; nothing below synchronises waves
    const int chunk = blockIdx.y, b = blockIdx.z / a.H, h = blockIdx.z - b * a.H;
    const int k_lo = chunk * a.kpc, k_hi = min(a.N, k_lo + a.kpc);   // k_lo < N by the grid
    const int qrow = min(q0 + col, a.P - 1);
    const float *qp = a.q + ((size_t)b * a.P + qrow) * a.qs + h * D + 4 * grp;
    const float *kb = a.k + (size_t)b * a.N * a.ks + h * D + 4 * grp;
    const float *vb = a.v + (size_t)b * a.N * a.vs + h * D + col;
    f4 qv[DT];
#pragma unroll
    for (int t = 0; t < DT; ++t) qv[t] = load_quad(qp + 16 * t, a.vec);

    f4 acc[DT][2];
#pragma unroll
    for (int t = 0; t < DT; ++t) { acc[t][0] = f4{0, 0, 0, 0}; acc[t][1] = f4{0, 0, 0, 0}; }
    float m = -INFINITY, lsum = 0.0f;
    unsigned dkey = 0;
    if constexpr (TRAIN) {
        if (a.drop) dkey = draw_key(a.seed, a.step[0], (unsigned)blockIdx.z, (unsigned)(q0 + col));
    }

    for (int kt = k_lo; kt < k_hi; kt += MHA_KT) {
        f4 s[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int krow = min(kt + 16 * j + col, k_hi - 1);
            const float *kp = kb + (size_t)krow * a.ks;
            s[j] = f4{0, 0, 0, 0};
#pragma unroll
            for (int t = 0; t < DT; ++t) {
                const f4 kv = load_quad(kp + 16 * t, a.vec);
#pragma unroll
                for (int i = 0; i < 4; ++i) s[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(kv[i], qv[t][i], s[j], 0, 0, 0);
            }
        }
        float tmax = -INFINITY;
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                if (kt + 16 * j + 4 * grp + r >= k_hi) s[j][r] = -INFINITY;
                tmax = fmaxf(tmax, s[j][r]);
            }
        tmax = fmaxf(tmax, __shfl_xor(tmax, 16, 64));
        tmax = fmaxf(tmax, __shfl_xor(tmax, 32, 64));                // finite: key kt itself is inside the chunk
        const float m_new = fmaxf(m, tmax);
        const float alpha = exp2f((m - m_new) * a.c);               // 0 on the first step (m = -inf)
        float psum = 0.0f;
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                s[j][r] = exp2f((s[j][r] - m_new) * a.c);
                psum += s[j][r];
            }
        lsum = lsum * alpha + psum;
        m = m_new;
        if constexpr (TRAIN) {
            if (a.drop) {                                            // the sum above is the one before dropout
#pragma unroll
                for (int j = 0; j < 4; ++j)
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        s[j][r] = attn_keep(dkey, (unsigned)(kt + 16 * j + 4 * grp + r), a.thresh) ? s[j][r] * a.rinv : 0.0f;
            }
        }
#pragma unroll
        for (int t = 0; t < DT; ++t) { acc[t][0] *= alpha; acc[t][1] *= alpha; }
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int vrow = min(kt + 16 * j + 4 * grp + r, k_hi - 1);   // a masked key has p = 0 and reads a real row
                const float *vp = vb + (size_t)vrow * a.vs;
#pragma unroll
                for (int t = 0; t < DT; ++t)
                    acc[t][j & 1] = __builtin_amdgcn_mfma_f32_16x16x4f32(vp[16 * t], s[j][r], acc[t][j & 1], 0, 0, 0);
            }
    }
    lsum += __shfl_xor(lsum, 16, 64);
    lsum += __shfl_xor(lsum, 32, 64);
    if (q0 + col >= a.P) return;
    const size_t row = (((size_t)b * a.H + h) * a.nchunk + chunk) * a.P + q0 + col;
    if (grp == 0) { a.ml[2 * row] = m; a.ml[2 * row + 1] = lsum; }
    float *o = a.acc + row * D + 4 * grp;                            // O^T: row = channel 4 grp + r, column = the query
#pragma unroll
    for (int t = 0; t < DT; ++t) {
        const f4 x = acc[t][0] + acc[t][1];
#pragma unroll
        for (int r = 0; r < 4; ++r) o[16 * t + r] = x[r];
    }
}

template <bool TRAIN>
__global__ __launch_bounds__(MHA_T) void mha_combine_kernel(MhaArgs a, int D) {
    const long long i = (long long)blockIdx.x * MHA_T + threadIdx.x;
    if constexpr (TRAIN) {
        if (a.drop && i == 0) {                                      // the partial launch has read the counter: advance it
            const unsigned s = a.step[0];
            a.used_step[0] = s;
            a.step[0] = s + 1u;
        }
    }
    if (i >= (long long)a.B * a.P * a.C) return;
    const int ch = (int)(i % a.C), h = ch / D, dd = ch - h * D;
    const long long bp = i / a.C;
    const int p = (int)(bp % a.P), b = (int)(bp / a.P);
    const size_t row0 = ((size_t)b * a.H + h) * a.nchunk * a.P + p;
    float M = -INFINITY;
    for (int c = 0; c < a.nchunk; ++c) M = fmaxf(M, a.ml[2 * (row0 + (size_t)c * a.P)]);
    float num = 0.0f, den = 0.0f;
    for (int c = 0; c < a.nchunk; ++c) {                             // chunk order
        const size_t row = row0 + (size_t)c * a.P;
        const float w = exp2f((a.ml[2 * row] - M) * a.c);
        num += w * a.acc[row * D + dd];
        den += w * a.ml[2 * row + 1];
    }
    a.out[i] = num / den;
    if constexpr (TRAIN) {
        if (dd == 0) {
            float *st = a.stats + 2 * (((size_t)b * a.H + h) * a.P + p);
            st[0] = M;
            st[1] = den;
        }
    }
}

__global__ __launch_bounds__(MHA_T) void mha_keep_kernel(int H, int P, int N, long long total, unsigned thresh, unsigned seed,
                                                         const unsigned *step, unsigned char *keep) {
    const long long i = (long long)blockIdx.x * MHA_T + threadIdx.x;
    if (i >= total) return;
    const unsigned j = (unsigned)(i % N);
    const long long r = i / N;
    keep[i] = attn_keep(draw_key(seed, step[0], (unsigned)(r / P), (unsigned)(r % P)), j, thresh) ? 1 : 0;
}

}  // namespace pdm

using namespace pdm;

extern "C" int pdm_mha_default_keys_per_chunk(void) { return MHA_DEFAULT_CHUNK; }

// 0 for a shape pdm_mha_forward rejects
extern "C" size_t pdm_mha_forward_workspace_bytes(int B, int P, int N, int C, int nheads, int keys_per_chunk) {
    if (!mha_supported(B, P, N, C, nheads, keys_per_chunk) || B == 0) return 0;
    const size_t nchunk = (size_t)divup(N, mha_chunk(keys_per_chunk));
    return align256((size_t)B * nheads * nchunk * P * 2 * sizeof(float)) + (size_t)B * nchunk * P * C * sizeof(float);
}

extern "C" size_t pdm_mha_forward_train_workspace_bytes(int B, int P, int N, int C, int nheads, int keys_per_chunk) {
    return pdm_mha_forward_workspace_bytes(B, P, N, C, nheads, keys_per_chunk);
}

// the two launches of the forward; train: the dropout parameters and stats of `a` are set
static int mha_forward_launch(const char *who, void *stream, bool train, MhaArgs a, int B, int P, int N, int C, int nheads,
                              const float *q, long long q_stride, const float *k, long long k_stride, const float *v,
                              long long v_stride, int keys_per_chunk, float *out, void *workspace, size_t workspace_bytes) {
    PDM_REQUIRE(mha_supported(B, P, N, C, nheads, keys_per_chunk), PDM_E_BADARG,
                "%s: B = %d, P = %d, N = %d, C = %d, heads = %d, keys_per_chunk = %d: needs P, N >= 1, C <= 256 and "
                "C / heads in {16, 32}", who, B, P, N, C, nheads, keys_per_chunk);
    PDM_REQUIRE(q_stride >= C && k_stride >= C && v_stride >= C, PDM_E_BADARG, "%s: a row stride below C = %d", who, C);
    if (B == 0) return 0;
    PDM_REQUIRE(q && k && v && out && workspace, PDM_E_BADARG, "%s: null pointer", who);
    const int kpc = mha_chunk(keys_per_chunk), nchunk = divup(N, kpc), d = C / nheads;
    PDM_REQUIRE(nchunk <= 65535 && (long long)B * nheads <= 65535 && (long long)B * P * C <= 0x7fffffffll, PDM_E_TOOLARGE,
                "%s: %d key chunks x %lld sample-heads exceed the grid", who, nchunk, (long long)B * nheads);
    const size_t need = pdm_mha_forward_workspace_bytes(B, P, N, C, nheads, keys_per_chunk);
    PDM_REQUIRE(workspace_bytes >= need && (reinterpret_cast<uintptr_t>(workspace) & 7) == 0, PDM_E_BADARG,
                "%s: workspace of %zu bytes, need %zu (8-byte aligned)", who, workspace_bytes, need);
    a.B = B; a.P = P; a.N = N; a.C = C; a.H = nheads; a.kpc = kpc; a.nchunk = nchunk;
    a.q = q; a.k = k; a.v = v; a.qs = q_stride; a.ks = k_stride; a.vs = v_stride;
    a.vec = mha_aligned16(q) && mha_aligned16(k) && q_stride % 4 == 0 && k_stride % 4 == 0;
    a.c = (float)(1.4426950408889634 / sqrt((double)d));
    a.ml = static_cast<float *>(workspace);
    a.acc = reinterpret_cast<float *>(static_cast<char *>(workspace) + align256((size_t)B * nheads * nchunk * P * 2 * sizeof(float)));
    a.out = out;
    const dim3 grid((unsigned)divup(P, MHA_QB), (unsigned)nchunk, (unsigned)(B * nheads));
    const dim3 cgrid((unsigned)divup((long long)B * P * C, MHA_T));
    hipStream_t s = as_stream(stream);
    if (train) {
        if (d == 16) hipLaunchKernelGGL((mha_partial_kernel<16, true>), grid, dim3(MHA_T), 0, s, a);
        else hipLaunchKernelGGL((mha_partial_kernel<32, true>), grid, dim3(MHA_T), 0, s, a);
    } else {
        if (d == 16) hipLaunchKernelGGL((mha_partial_kernel<16, false>), grid, dim3(MHA_T), 0, s, a);
        else hipLaunchKernelGGL((mha_partial_kernel<32, false>), grid, dim3(MHA_T), 0, s, a);
    }
    if (int rc = check_launch(who)) return rc;
    if (train) hipLaunchKernelGGL(mha_combine_kernel<true>, cgrid, dim3(MHA_T), 0, s, a, d);
    else hipLaunchKernelGGL(mha_combine_kernel<false>, cgrid, dim3(MHA_T), 0, s, a, d);
    return check_launch(who);
}

extern "C" int pdm_mha_forward(void *stream, int B, int P, int N, int C, int nheads, const float *q, long long q_stride,
                               const float *k, long long k_stride, const float *v, long long v_stride, int keys_per_chunk,
                               float *out, void *workspace, size_t workspace_bytes) {
    return mha_forward_launch("mha_forward", stream, false, MhaArgs{}, B, P, N, C, nheads, q, q_stride, k, k_stride, v, v_stride,
                              keys_per_chunk, out, workspace, workspace_bytes);
}

extern "C" int pdm_mha_forward_train(void *stream, int B, int P, int N, int C, int nheads, const float *q, long long q_stride,
                                     const float *k, long long k_stride, const float *v, long long v_stride, int keys_per_chunk,
                                     double dropout_p, unsigned seed, unsigned *step, unsigned *used_step, float *stats,
                                     float *out, void *workspace, size_t workspace_bytes) {
    PDM_REQUIRE(mha_dropout_ok(dropout_p), PDM_E_BADARG, "mha_forward_train: dropout_p = %g outside [0, 1)", dropout_p);
    MhaArgs a{};
    a.drop = dropout_p > 0.0;
    PDM_REQUIRE(B == 0 || stats, PDM_E_BADARG, "mha_forward_train: null stats");
    PDM_REQUIRE(B == 0 || !a.drop || (step && used_step), PDM_E_BADARG, "mha_forward_train: dropout_p > 0 needs step and used_step");
    a.thresh = mha_dropout_thresh(dropout_p); a.rinv = mha_dropout_rinv(dropout_p); a.seed = seed;
    a.step = step; a.used_step = used_step; a.stats = stats;
    return mha_forward_launch("mha_forward_train", stream, true, a, B, P, N, C, nheads, q, q_stride, k, k_stride, v, v_stride,
                              keys_per_chunk, out, workspace, workspace_bytes);
}

extern "C" int pdm_mha_dropout_keep(void *stream, int B, int nheads, int P, int N, double dropout_p, unsigned seed,
                                    const unsigned *step, unsigned char *keep) {
    PDM_REQUIRE(B >= 0 && nheads >= 1 && P >= 1 && N >= 1 && mha_dropout_ok(dropout_p), PDM_E_BADARG,
                "mha_dropout_keep: B = %d, heads = %d, P = %d, N = %d, dropout_p = %g", B, nheads, P, N, dropout_p);
    const long long total = (long long)B * nheads * P * N;
    if (total == 0) return 0;
    PDM_REQUIRE(step && keep, PDM_E_BADARG, "mha_dropout_keep: null pointer");
    PDM_REQUIRE(divup(total, MHA_T) > 0 && total / MHA_T < 0x7fffffffll, PDM_E_TOOLARGE, "mha_dropout_keep: %lld weights", total);
    hipLaunchKernelGGL(mha_keep_kernel, dim3((unsigned)divup(total, MHA_T)), dim3(MHA_T), 0, as_stream(stream), nheads, P, N, total,
                       mha_dropout_thresh(dropout_p), seed, step, keep);
    return check_launch("mha_dropout_keep");
}

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
#include "common.h"

namespace pdm {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int MHA_T = 256;          // 4 waves
constexpr int MHA_QW = 16;          // queries per wave
constexpr int MHA_QB = 64;          // queries per workgroup
constexpr int MHA_KT = 64;          // keys per step of a wave: 4 tiles of 16
constexpr int MHA_DEFAULT_CHUNK = 1024;

struct MhaArgs {
    int B, P, N, C, H, kpc, nchunk, vec;
    const float *q, *k, *v;
    long long qs, ks, vs;            // row strides in elements; a sample is `rows` rows on
    float c;                         // log2(e) / sqrt(d)
    float *ml;                       // (B, H, nchunk, P, 2): raw maximum, sum
    float *acc;                      // (B, H, nchunk, P, d)
    float *out;                      // (B, P, C)
};

__device__ __forceinline__ f32x4 mha_load4(const float *p, int vec) {
    if (vec) return *reinterpret_cast<const f32x4 *>(p);
    f32x4 r;
    r[0] = p[0]; r[1] = p[1]; r[2] = p[2]; r[3] = p[3];
    return r;
}

template <int D>
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
    f32x4 qv[DT];
#pragma unroll
    for (int t = 0; t < DT; ++t) qv[t] = mha_load4(qp + 16 * t, a.vec);

    f32x4 acc[DT][2];
#pragma unroll
    for (int t = 0; t < DT; ++t) { acc[t][0] = f32x4{0, 0, 0, 0}; acc[t][1] = f32x4{0, 0, 0, 0}; }
    float m = -INFINITY, lsum = 0.0f;

    for (int kt = k_lo; kt < k_hi; kt += MHA_KT) {
        f32x4 s[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int krow = min(kt + 16 * j + col, k_hi - 1);
            const float *kp = kb + (size_t)krow * a.ks;
            s[j] = f32x4{0, 0, 0, 0};
#pragma unroll
            for (int t = 0; t < DT; ++t) {
                const f32x4 kv = mha_load4(kp + 16 * t, a.vec);
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
        const f32x4 x = acc[t][0] + acc[t][1];
#pragma unroll
        for (int r = 0; r < 4; ++r) o[16 * t + r] = x[r];
    }
}

__global__ __launch_bounds__(MHA_T) void mha_combine_kernel(MhaArgs a, int D) {
    const long long i = (long long)blockIdx.x * MHA_T + threadIdx.x;
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
}

static int mha_chunk(int keys_per_chunk) { return keys_per_chunk > 0 ? keys_per_chunk : MHA_DEFAULT_CHUNK; }

static bool mha_supported(int B, int P, int N, int C, int nheads, int keys_per_chunk) {
    if (B < 0 || P < 1 || N < 1 || C < 1 || C > 256 || nheads < 1 || keys_per_chunk < 0 || C % nheads != 0) return false;
    const int d = C / nheads;
    return d == 16 || d == 32;
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

extern "C" int pdm_mha_forward(void *stream, int B, int P, int N, int C, int nheads, const float *q, long long q_stride,
                               const float *k, long long k_stride, const float *v, long long v_stride, int keys_per_chunk,
                               float *out, void *workspace, size_t workspace_bytes) {
    PDM_REQUIRE(mha_supported(B, P, N, C, nheads, keys_per_chunk), PDM_E_BADARG,
                "mha_forward: B = %d, P = %d, N = %d, C = %d, heads = %d, keys_per_chunk = %d: needs P, N >= 1, C <= 256 and "
                "C / heads in {16, 32}", B, P, N, C, nheads, keys_per_chunk);
    PDM_REQUIRE(q_stride >= C && k_stride >= C && v_stride >= C, PDM_E_BADARG, "mha_forward: a row stride below C = %d", C);
    if (B == 0) return 0;
    PDM_REQUIRE(q && k && v && out && workspace, PDM_E_BADARG, "mha_forward: null pointer");
    const int kpc = mha_chunk(keys_per_chunk), nchunk = divup(N, kpc), d = C / nheads;
    PDM_REQUIRE(nchunk <= 65535 && (long long)B * nheads <= 65535 && (long long)B * P * C <= 0x7fffffffll, PDM_E_TOOLARGE,
                "mha_forward: %d key chunks x %lld sample-heads exceed the grid", nchunk, (long long)B * nheads);
    const size_t need = pdm_mha_forward_workspace_bytes(B, P, N, C, nheads, keys_per_chunk);
    PDM_REQUIRE(workspace_bytes >= need && (reinterpret_cast<uintptr_t>(workspace) & 7) == 0, PDM_E_BADARG,
                "mha_forward: workspace of %zu bytes, need %zu (8-byte aligned)", workspace_bytes, need);
    MhaArgs a{};
    a.B = B; a.P = P; a.N = N; a.C = C; a.H = nheads; a.kpc = kpc; a.nchunk = nchunk;
    a.q = q; a.k = k; a.v = v; a.qs = q_stride; a.ks = k_stride; a.vs = v_stride;
    a.vec = ((reinterpret_cast<uintptr_t>(q) | reinterpret_cast<uintptr_t>(k)) & 15) == 0 && q_stride % 4 == 0 && k_stride % 4 == 0;
    a.c = (float)(1.4426950408889634 / sqrt((double)d));
    a.ml = static_cast<float *>(workspace);
    a.acc = reinterpret_cast<float *>(static_cast<char *>(workspace) + align256((size_t)B * nheads * nchunk * P * 2 * sizeof(float)));
    a.out = out;
    const dim3 grid((unsigned)divup(P, MHA_QB), (unsigned)nchunk, (unsigned)(B * nheads));
    if (d == 16) hipLaunchKernelGGL(mha_partial_kernel<16>, grid, dim3(MHA_T), 0, as_stream(stream), a);
    else hipLaunchKernelGGL(mha_partial_kernel<32>, grid, dim3(MHA_T), 0, as_stream(stream), a);
    if (int rc = check_launch("mha_forward(partial)")) return rc;
    hipLaunchKernelGGL(mha_combine_kernel, dim3((unsigned)divup((long long)B * P * C, MHA_T)), dim3(MHA_T), 0, as_stream(stream), a, d);
    return check_launch("mha_forward(combine)");
}

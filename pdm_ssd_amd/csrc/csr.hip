// The inverted index of csr.h: one builder for every payload, and the channel-major scatter-add backward through it.
//
// LDS float atomics turned out to be the limit of the LDS-accumulating backward of three_interpolate: ~270 GB/s of
// grad_out for every shape, i.e. one ds_add_f32 lane every three cycles per CU.  The scatter is inverted once per
// (idx, weight) pair instead: per cloud a table "target k <- its (source row, weight) contributions" (counting sort, one
// workgroup per cloud), then
//   grad_points[b, c, k] += sum_{(j, w) in list(k)} w * grad_out[b, c, j]
// with the grad_out rows of a few channels staged in LDS (coalesced global reads, random LDS READS) and one thread per
// target.  Needs m <= 16384 (LDS histogram) and row_len <= 65535 (16-bit j).
#include "csr.h"

namespace pdm {

constexpr int CSR_THREADS = 1024;

template <CsrPayload P>
__global__ __launch_bounds__(CSR_THREADS) void csr_build_kernel(int ne, int per, int m, const int *__restrict__ idx,
                                                                const float *__restrict__ weight, CsrLists L) {
    extern __shared__ int s_cnt[];   // m counters, then fill cursors
    __shared__ int s_wave[CSR_THREADS / 64];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int *__restrict__ id = idx + (size_t)b * ne;
    for (int k = tid; k < m; k += CSR_THREADS) s_cnt[k] = 0;
    __syncthreads();
    for (int e = tid; e < ne; e += CSR_THREADS) {
        const int k = id[e];
        if (k >= 0 && k < m) atomicAdd(&s_cnt[k], 1);
    }
    __syncthreads();
    hist_to_cursors<CSR_THREADS>(s_cnt, m, s_wave, L.start + (size_t)b * (m + 1));
    for (int e = tid; e < ne; e += CSR_THREADS) {
        const int k = id[e];
        if (k < 0 || k >= m) continue;
        const size_t pos = (size_t)b * ne + atomicAdd(&s_cnt[k], 1);
        if constexpr (P == CSR_ROW_WEIGHT) {
            L.row[pos] = (unsigned short)(e / per);
            L.weight[pos] = weight ? weight[(size_t)b * ne + e] : 1.0f;
        } else {
            L.elem[pos] = e;
        }
    }
}

template <int TC>
__global__ __launch_bounds__(CSR_THREADS) void interp_grad_csr_kernel(int c, int n, int ne, int m,
                                                                      const float *__restrict__ grad_out,
                                                                      const int *__restrict__ start_all,
                                                                      const unsigned short *__restrict__ ej_all,
                                                                      const float *__restrict__ ew_all,
                                                                      float *__restrict__ grad_points) {
    extern __shared__ float s_g[];   // TC x n
    const int b = blockIdx.y, c0 = blockIdx.x * TC, tid = threadIdx.x;
    const int nc = min(TC, c - c0);
    const float *__restrict__ g = grad_out + ((size_t)b * c + c0) * n;
    for (int e = tid; e < nc * n; e += CSR_THREADS) s_g[e] = g[e];   // nc consecutive rows are one contiguous block
    __syncthreads();
    const int *__restrict__ start = start_all + (size_t)b * (m + 1);
    const unsigned short *__restrict__ ej = ej_all + (size_t)b * ne;
    const float *__restrict__ ew = ew_all + (size_t)b * ne;
    for (int k = tid; k < m; k += CSR_THREADS) {
        const int s = start[k], e = start[k + 1];
        float acc[TC];
#pragma unroll
        for (int ci = 0; ci < TC; ++ci) acc[ci] = 0.0f;
        for (int p = s; p < e; ++p) {
            const int j = ej[p];
            const float w = ew[p];
#pragma unroll
            for (int ci = 0; ci < TC; ++ci)
                if (ci < nc) acc[ci] += s_g[ci * n + j] * w;
        }
#pragma unroll
        for (int ci = 0; ci < TC; ++ci)
            if (ci < nc) grad_points[((size_t)b * c + c0 + ci) * m + k] += acc[ci];   // rows are exclusive to this workgroup
    }
}

static size_t round16(size_t x) { return (x + 15) / 16 * 16; }

size_t csr_workspace_bytes(CsrPayload payload, int b, long long ne, int m) {
    if (b <= 0 || ne <= 0 || m <= 0) return 0;
    if (payload == CSR_ELEMENT) return (size_t)b * ((size_t)(m + 1) + (size_t)ne) * sizeof(int) + 64;
    return round16((size_t)b * (m + 1) * sizeof(int)) + round16((size_t)b * ne * sizeof(unsigned short)) +
           (size_t)b * ne * sizeof(float) + 64;
}

CsrLists csr_carve(void *workspace, CsrPayload payload, int b, long long ne, int m) {
    CsrLists L = {nullptr, nullptr, nullptr, nullptr};
    uintptr_t p = (reinterpret_cast<uintptr_t>(workspace) + 15) & ~(uintptr_t)15;
    L.start = reinterpret_cast<int *>(p);
    if (payload == CSR_ELEMENT) {
        L.elem = L.start + (size_t)b * (m + 1);
        return L;
    }
    p += round16((size_t)b * (m + 1) * sizeof(int));
    L.row = reinterpret_cast<unsigned short *>(p);
    p += round16((size_t)b * ne * sizeof(unsigned short));
    L.weight = reinterpret_cast<float *>(p);
    return L;
}

template <CsrPayload P>
static int csr_build_launch_as(void *stream, const char *who, int b, int ne, int per, int m, const int *idx, const float *weight,
                               const CsrLists &lists) {
    const size_t lds = (size_t)m * sizeof(int);
    if (lds + 1024 > 64 * 1024) {   // dynamic + static LDS above the default 64 KB (m near 16384)
        // (the kernel also holds a small static block: dynamic + static must stay within the 160 KB of a CU)
        const int e = grant_lds(reinterpret_cast<const void *>(&csr_build_kernel<P>), 128 * 1024);
        PDM_REQUIRE(e == 0, PDM_E_TOOLARGE, "%s: cannot obtain %zu bytes of LDS", who, lds);
    }
    hipLaunchKernelGGL(csr_build_kernel<P>, dim3(b), dim3(CSR_THREADS), lds, as_stream(stream), ne, per, m, idx, weight, lists);
    return check_launch(who);
}

int csr_build_launch(void *stream, const char *who, CsrPayload payload, int b, int ne, int per, int m, const int *idx,
                     const float *weight, const CsrLists &lists) {
    return payload == CSR_ELEMENT ? csr_build_launch_as<CSR_ELEMENT>(stream, who, b, ne, per, m, idx, weight, lists)
                                  : csr_build_launch_as<CSR_ROW_WEIGHT>(stream, who, b, ne, per, m, idx, weight, lists);
}

bool csr_form_applies(int b, int row_len, long long ne, int m) {
    return m >= 1 && m <= CSR_MAX_TARGETS && row_len >= 1 && row_len <= 32768 && ne <= 0x7fffffffll / 4 && b <= 65535;
}

int csr_scatter_grad_launch(void *stream, const char *who, int b, int c, int row_len, int per, int m, const float *grad_out,
                            const int *idx, const float *weight, float *grad_points, void *workspace) {
    const int ne = row_len * per;
    const CsrLists L = csr_carve(workspace, CSR_ROW_WEIGHT, b, ne, m);
    int rc = csr_build_launch(stream, who, CSR_ROW_WEIGHT, b, ne, per, m, idx, weight, L);
    if (rc) return rc;
    // channel rows staged per workgroup: as many as fit 128 KB of LDS, at most 8
    const int tc = row_len <= 4096 ? 8 : row_len <= 8192 ? 4 : row_len <= 16384 ? 2 : 1;
#define PDM_TIC_LAUNCH(TCV)                                                                                            \
    do {                                                                                                               \
        const size_t lds = (size_t)TCV * row_len * sizeof(float);                                                      \
        if (lds > 64 * 1024) {   /* granted per function and per device (common.h) */                                  \
            const int e = grant_lds(reinterpret_cast<const void *>(&interp_grad_csr_kernel<TCV>), 160 * 1024);         \
            PDM_REQUIRE(e == 0, PDM_E_TOOLARGE, "%s: cannot obtain %zu bytes of LDS", who, lds);                       \
        }                                                                                                              \
        hipLaunchKernelGGL(interp_grad_csr_kernel<TCV>, dim3(divup(c, TCV), b), dim3(CSR_THREADS), lds, as_stream(stream), \
                           c, row_len, ne, m, grad_out, L.start, L.row, L.weight, grad_points);                        \
    } while (0)
    if (tc == 8) PDM_TIC_LAUNCH(8);
    else if (tc == 4) PDM_TIC_LAUNCH(4);
    else if (tc == 2) PDM_TIC_LAUNCH(2);
    else PDM_TIC_LAUNCH(1);
#undef PDM_TIC_LAUNCH
    return check_launch(who);
}

}  // namespace pdm

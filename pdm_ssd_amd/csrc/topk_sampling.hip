// Score-ranked sampling: instance-aware down-sampling keeps the npoint points with the
// highest predicted foreground / centre score instead of running FPS (IA-SSD lineage; the sampling code itself is
// absent from the reference snapshot, where the analogous call is torch.topk over per-point scores).  Build-defined,
// total order so that the result is unique and the CPU oracle can match it exactly:
//   rank by score descending on the order-preserving integer image of the float (so -0.0 < +0.0, -inf lowest,
//   NaN of either sign ranks ABOVE +inf, as torch.topk treats it); equal images -> lower index first.
//   idx[b, r] = index of the r-th ranked point, r = 0 .. k-1.
// One workgroup per cloud: 4 rounds of 8-bit radix select find the k-th key, the chosen points are emitted in index
// order (ties with the k-th key by lowest index) and bitonic-sorted in LDS as 8-byte (key, index) items: rank_select
// (rank_select.h), which post_process.hip calls for its candidates as well.
#include "rank_select.h"

namespace pdm {

__global__ __launch_bounds__(TK_THREADS) void topk_sampling_kernel(int N, int K, const float *__restrict__ scores,
                                                                  int *__restrict__ idx_out) {
    extern __shared__ unsigned long long s_items[];
    __shared__ alignas(16) RankLds lds;
    const int cloud = blockIdx.x, tid = threadIdx.x;
    const unsigned *__restrict__ sc = reinterpret_cast<const unsigned *>(scores) + (size_t)cloud * N;
    rank_select(N, K, [&](int i) { return topk_key(sc[i]); }, s_items, lds);
    for (int r = tid; r < K; r += TK_THREADS) idx_out[(size_t)cloud * K + r] = (int)(unsigned)(s_items[r] & 0xffffffffull);
}

}  // namespace pdm

using namespace pdm;

extern "C" int pdm_topk_sampling(void *stream, int b, int n, int k, const float *scores, int *idx) {
    PDM_REQUIRE(b >= 0 && n >= 0 && k >= 0, PDM_E_BADARG, "topk_sampling: negative size b=%d n=%d k=%d", b, n, k);
    PDM_REQUIRE(k <= n, PDM_E_BADARG, "topk_sampling: k=%d exceeds n=%d", k, n);   // torch.topk raises as well
    PDM_REQUIRE(k <= TK_MAXK, PDM_E_TOOLARGE, "topk_sampling: k=%d exceeds %d", k, TK_MAXK);
    if (b == 0 || k == 0) return 0;
    PDM_REQUIRE(scores && idx, PDM_E_BADARG, "topk_sampling: null pointer");
    int k2 = 2;
    while (k2 < k) k2 <<= 1;
    const size_t lds = (size_t)k2 * sizeof(unsigned long long);
    if (lds > 64 * 1024) {   // > 64 KB of dynamic LDS has to be granted, per device (static LDS comes on top: 156 KB)
        const int e = grant_lds(reinterpret_cast<const void *>(&topk_sampling_kernel), 156 * 1024);
        PDM_REQUIRE(e == 0, PDM_E_TOOLARGE, "topk_sampling: cannot obtain %zu bytes of LDS: %s", lds, hipGetErrorString((hipError_t)e));
    }
    hipLaunchKernelGGL(topk_sampling_kernel, dim3(b), dim3(TK_THREADS), lds, as_stream(stream), n, k, scores, idx);
    return check_launch("topk_sampling");
}

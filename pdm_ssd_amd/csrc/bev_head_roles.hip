// Heat-map head in one launch, role-split form (gfx950): the depthwise 3x3 prologue and the fp32 MFMA chain of
// rows_chain_kernel<8,4,4,1,true> (rows_chain.hip) live in DIFFERENT waves of one workgroup.
//
//   out[cell] = W3 relu(W2 relu(W1 relu(dw3x3(map)[cell] + shift) + b1) + b2) + b3      map (B, H, W, 128) channels-last
//
// In the one-role kernel every wave runs the prologue (LDS and latency bound, no MFMA) and then the chain, and the two
// resident workgroups of a CU take turns: the matrix pipe is busy half the time.  Here ONE workgroup per CU
// of 12 waves walks the 4 x 16 patches:
//   * waves 0-3, one per SIMD, are CONSUMERS: wave r owns patch row r (16 cells) and all channels, activations in registers
//     from layer to layer as in rc_layer.  Their B fragments of layer 1 come from the input tile the producers left in LDS
//     and every A fragment comes from the three layers' packed weights, which stay in LDS for the life of the workgroup
//     (52 KB): no weight stream, no chunk barriers, nothing but ds_read_b128 and MFMAs.
//   * waves 4-11 are PRODUCERS: wave p holds k-block p of the chain's input, lane = (column of 16, quad of 4).  A lane
//     requests its own column of the 6 halo rows from global memory a tile ahead and takes the columns either side from the
//     neighbouring lanes (DPP row shifts), so every byte of the halo is requested once; it runs the 4 x 9 fmas and writes
//     four quads of the chain's input tile.  No halo in LDS and no barrier between producers.
//   * hand-over: two input tiles in LDS; while the consumers run the chain on tile i from buffer i & 1 the producers write
//     tile i + 1 into the other.  ONE workgroup barrier per tile, executed by all twelve waves (gfx950 has no other kind).
// LDS bytes per tile: 32 KB tile write + 32 KB tile read + 4 x 52 KB fragment reads + 80 KB of taps = 352 KB (the one-role
// form: ~620 KB).  Measurements and what was dropped: DESIGN.md 7zg.
//
// Results are bit-equal to rows_chain_kernel<8,4,4,1,true>: per channel the depthwise is shift, then nine IEEE fmas row by
// row, left to right, then max(., 0); per output of a layer the accumulator starts as the bias, k-blocks ascend, the four
// 16x16x4 MFMAs of a k-block run in order, the floor is the same fmed3 and the stores are store_quad_ragged.
#include "mfma_f32.h"

namespace pdm {

#ifndef BR_DIAG
#define BR_DIAG 0   // timing build (make diag-rc, results wrong): 1 = cycle stamps of both roles instead of results (tools/diag/bev_head_phase.py)
#endif
#ifndef BR_PRIO
#define BR_PRIO 1   // consumers run at s_setprio 1: their ds_reads and MFMAs win the issue arbitration against the producer waves of their SIMD
#endif

#ifndef BR_DEPTH
#define BR_DEPTH 1  // producers: tiles whose halo is in flight (7 x 4 VGPRs each); 2 and 3 compile to 16 / 184 bytes of scratch in the 168 VGPRs of a 12-wave workgroup
#endif

template <int S> struct br_slot { static constexpr int value = S; };
typedef const __attribute__((address_space(1))) f4 *br_gf4c;  // a pointer the compiler must treat as global (no flat loads)

struct BevRolesArgs {
    int B, H, W, by_xcd;
    const float *map;                 // (B, H, W, 128)
    const float *dw_w, *dw_shift;     // (9, 128) tap-major with the BatchNorm scale folded in, (128)
    const float *wpack, *bias;        // 128 -> 64 -> 64 -> 16 packed as fused.py::pack_layer, layers back to back
    float *out;
    int out_stride, cout, relu_last;
};

constexpr int BR_CONS = 4, BR_PROD = 8;
constexpr int BR_THREADS = 64 * (BR_CONS + BR_PROD);
// f4 slots per cell of the input tile: 32 quads + 2 of padding.  A consumer lane (pos, g) reads slot 34 pos + 4 kb + g; the
// 16 lanes a ds_read_b128 serves together (mfma_f32.h, MFMA_ROW_STRIDE) hold eight values of pos at g and eight at g + 1,
// and 2 pos + g mod 16 is different for all of them.  A producer wave writes the 32 quads of two cells, 512 contiguous bytes each.
constexpr int BR_ROW = 34;
constexpr int BR_TILE_F4 = 64 * BR_ROW;
constexpr int BR_W2 = 8 * 4 * 64, BR_W3 = BR_W2 + 4 * 4 * 64, BR_W_F4 = BR_W3 + 4 * 64;   // fragment offsets of layers 2, 3; all of them
constexpr int BR_DW = BR_W_F4 + 2 * BR_TILE_F4;                                            // nine depthwise taps and the shift, 32 quads each
constexpr int BR_LDS_BYTES = (BR_DW + 10 * 32) * 16;                                       // 128 000

// One layer on a consumer wave: in[NKB] -> acc[NMB], arithmetic as rc_layer.  A fragments from LDS (wl = the layer's
// fragments + lane, [mb][kb] as packed).  A consumer wave is alone on its SIMD's matrix pipe, so no other wave covers a wait
// of its own: every fragment is requested a whole k-block (16 MFMAs, 512 cycles) ahead of its use, pinned IN FRONT of the
// MFMAs that run meanwhile (left to the scheduler the reads sit behind the 14th MFMA of a k-block and the next k-block
// opens with a wait for them).  an[]: on entry the fragments of this layer's k-block 0 (NMB == 1: of all four k-blocks); on
// exit an[i] = next[i * next_stride], the same for the layer that follows, requested under this layer's last k-block.
template <int NKB, int NMB>
__device__ __forceinline__ void br_layer(const f4 (&in)[NKB], f4 (&acc)[NMB], const f4 *wl, const f4 (&bias)[NMB], float floor, f4 (&an)[4],
                                         const f4 *next, int next_stride) {
#pragma unroll
    for (int mb = 0; mb < NMB; ++mb) acc[mb] = bias[mb];
    if constexpr (NMB == 1) {
        static_assert(NKB == 4, "br_layer: the one-block layer has four k-blocks");
        f4 a[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) a[i] = an[i];
#pragma unroll
        for (int i = 0; i < 4; ++i) an[i] = next[i * next_stride];
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int kb = 0; kb < 4; ++kb) acc[0] = mfma4(acc[0], a[kb], in[kb]);
        __builtin_amdgcn_sched_barrier(0);
    } else {
        static_assert(NMB == 4, "br_layer: four output blocks");
#pragma unroll
        for (int kb = 0; kb < NKB; ++kb) {
            f4 a[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) a[i] = an[i];
#pragma unroll
            for (int i = 0; i < 4; ++i) an[i] = kb + 1 < NKB ? wl[(i * NKB + kb + 1) * 64] : next[i * next_stride];
            __builtin_amdgcn_sched_barrier(0);
            mfma4_grid(&acc[0], a, in[kb]);
            __builtin_amdgcn_sched_barrier(0);
        }
    }
#pragma unroll
    for (int mb = 0; mb < NMB; ++mb) {   // (written out as in rc_layer: floor4's med3 folds differently for a constant floor)
        acc[mb].x = __builtin_amdgcn_fmed3f(acc[mb].x, floor, __builtin_inff());
        acc[mb].y = __builtin_amdgcn_fmed3f(acc[mb].y, floor, __builtin_inff());
        acc[mb].z = __builtin_amdgcn_fmed3f(acc[mb].z, floor, __builtin_inff());
        acc[mb].w = __builtin_amdgcn_fmed3f(acc[mb].w, floor, __builtin_inff());
    }
}

#if BR_DIAG & 1
#define BR_STAMP(arr, i) do { __builtin_amdgcn_s_waitcnt(0xc07f); (arr)[i] = __builtin_amdgcn_s_memtime(); } while (0)   /* lgkmcnt(0) first */
#else
#define BR_STAMP(arr, i)
#endif

__global__ __launch_bounds__(BR_THREADS, 1) void bev_head_roles_kernel(BevRolesArgs a) {
    extern __shared__ __attribute__((aligned(16))) f4 br_lds[];
    f4 *const wl = br_lds, *const tiles = br_lds + BR_W_F4;
    const int t = threadIdx.x, lane = t & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const bool consumer = wave < BR_CONS;
    const int ntx = (a.W + 15) / 16, nty = (a.H + 3) / 4;
    const long long ntiles = (long long)a.B * nty * ntx;
    // the walk of rows_chain_kernel's depthwise form: XCD x takes the contiguous range [x per_xcd, (x + 1) per_xcd) of patches,
    // so the patches that share a halo meet in one L2
    const bool by_xcd = a.by_xcd && (gridDim.x & 7) == 0;
    const long long per_xcd = (ntiles + 7) >> 3, nsteps = by_xcd ? per_xcd * 8 : ntiles;
    // patch of step `step` of this workgroup's walk; false past its last one (a workgroup's patch numbers ascend, so the
    // steps that have a patch are a prefix of its walk)
    auto tile_of = [&](long long step, int &b, int &y0, int &x0) -> bool {
        if (step >= nsteps) return false;
        const long long tl = by_xcd ? (step & 7) * per_xcd + (step >> 3) : step;
        if (tl >= ntiles) return false;
        const unsigned tu = (unsigned)tl, pp = (unsigned)(ntx * nty);
        const unsigned bb = tu / pp, rem = tu - bb * pp, ty = rem / (unsigned)ntx;
        b = (int)bb;
        y0 = (int)ty * 4; x0 = (int)(rem - ty * (unsigned)ntx) * 16;
        return true;
    };
    long long step = blockIdx.x;
    int cb = 0, cy0 = 0, cx0 = 0;   // the patch of this iteration
    if (!tile_of(step, cb, cy0, cx0)) return;   // (uniform over the workgroup, in front of every barrier)
    const long long stride = gridDim.x;
#if BR_DIAG & 1
    long long ds[8] = {};
    int nt = 0;
    long long *const dst = reinterpret_cast<long long *>(a.out) + (size_t)blockIdx.x * 16;
#endif

    // The two roles are two loops (one loop with a branch inside would keep the producers' halo and taps alive through the
    // consumers' chain: the sum of both register sets instead of the larger).  Both execute 1 + (patches of the workgroup) barriers.
    if (!consumer) {
        // ---- producer: wave pw holds k-block pw of the input; lane (ppos, pqq) = quad pq = 4 pw + pqq of column ppos ---------
        // Each lane requests its OWN column of the 6 halo rows; the columns either side come from the neighbouring lanes of
        // its row of 16 (DPP row shifts), and columns -1 and 16 from one more load in which lane 8 ry + 4 side + q holds quad
        // q of halo row ry on that side (handed to lanes 0 / 15 of a row through ds_bpermute).  So every byte of the halo is
        // requested once (7 loads a lane and tile; three loads per row, one per tap column, asked for every cell three times and
        // the tile arrived 10 k cycles after its request began), and 7 registers of 16 bytes hold a tile in flight: BR_DEPTH
        // tiles are on their way at any time.
        const int pw = wave - BR_CONS, ppos = lane & 15, pqq = lane >> 4, pq = 4 * pw + pqq;
        const int e_row = (lane >> 3) < 6 ? (lane >> 3) : 5, e_right = (lane >> 2) & 1, e_q = 4 * pw + (lane & 3);
        const int e_src = 4 * (4 * (ppos >> 3) + pqq);   // ds_bpermute byte index of this lane's edge donor for halo row 0 (+ 32 per row)
        f4 hv[BR_DEPTH][6], he[BR_DEPTH];
        unsigned hin[BR_DEPTH];   // bits 0-5: hv[ry] is inside the map, bit 6: he is (the others count as zero, applied when used)
        // (a cell outside the map: the nearest cell inside is read and dropped, so the loads are issued back to back with no
        //  branch around any of them; for the same reason a fetch past the workgroup's last patch re-reads its first one)
        auto fetch = [&](f4 (&v)[6], f4 &e, unsigned &in, long long s) {
            int b = cb, y0 = cy0, x0 = cx0;
            (void)tile_of(s, b, y0, x0);
            const f4 *__restrict__ img = reinterpret_cast<const f4 *>(a.map) + (size_t)b * a.H * a.W * 32;
            in = 0;
            const int gx = x0 + ppos, sx = gx >= a.W ? a.W - 1 : gx;
#pragma unroll
            for (int ry = 0; ry < 6; ++ry) {
                const int gy = y0 - 1 + ry, sy = gy < 0 ? 0 : gy >= a.H ? a.H - 1 : gy;
#if BR_DIAG & 4   // timing build: no halo loads
                v[ry] = f4{1.f, 2.f, 3.f, (float)sx};
#else
                v[ry] = ((br_gf4c)img)[(unsigned)((sy * a.W + sx) * 32 + pq)];   // (uniform base + a 32-bit lane offset: H W 512 < 2^31, checked at the launch)
#endif
                in |= (unsigned)(gy >= 0 && gy < a.H && gx < a.W) << ry;
            }
            const int gy = y0 - 1 + e_row, ex = e_right ? x0 + 16 : x0 - 1;
            const int sy = gy < 0 ? 0 : gy >= a.H ? a.H - 1 : gy, sxe = ex < 0 ? 0 : ex >= a.W ? a.W - 1 : ex;
#if BR_DIAG & 4
            e = f4{1.f, 2.f, 3.f, (float)sxe};
#else
            e = ((br_gf4c)img)[(unsigned)((sy * a.W + sxe) * 32 + e_q)];
#endif
            in |= (unsigned)(lane < 48 && gy >= 0 && gy < a.H && ex >= 0 && ex < a.W) << 6;
        };
#pragma unroll
        for (int s = 0; s < BR_DEPTH; ++s) fetch(hv[s], he[s], hin[s], step + s * stride);
        // the nine taps and the shift of quad pq: in LDS (slot k of 10, quad pq), read dy row by dy row when used — in registers
        // they took 40 VGPRs beside the halo slots and the kernel spilled.  A wave writes and reads only its own four quads, and
        // a wave's LDS accesses complete in order: no barrier
        f4 *const dwl = br_lds + BR_DW;
        if (ppos < 9) dwl[ppos * 32 + pq] = *reinterpret_cast<const f4 *>(a.dw_w + ppos * 128 + 4 * pq);
        if (ppos == 9) dwl[9 * 32 + pq] = *reinterpret_cast<const f4 *>(a.dw_shift + 4 * pq);
        __builtin_amdgcn_wave_barrier();
        // depthwise 3x3 + shift + ReLU -> quad pq of cells (0..3, ppos) of the input tile.  Tap rows in order, and inside a tap
        // row the four output rows: every output still sees shift, then its nine taps row by row, left to right.
        auto produce = [&](const f4 (&v)[6], f4 e, unsigned in, f4 *tile) {
            const f4 zero = {0.f, 0.f, 0.f, 0.f};
            const f4 shift = dwl[9 * 32 + pq];
            f4 acc[4] = {shift, shift, shift, shift};
            if (!((in >> 6) & 1)) e = zero;
#pragma unroll
            for (int dy = 0; dy < 3; ++dy) {
                const f4 k0 = dwl[(dy * 3 + 0) * 32 + pq], k1 = dwl[(dy * 3 + 1) * 32 + pq], k2 = dwl[(dy * 3 + 2) * 32 + pq];
#pragma unroll
                for (int o = 0; o < 4; ++o) {
                    const int ry = o + dy;
                    const f4 c = (in >> ry) & 1 ? v[ry] : zero;
                    f4 l, r;
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const int ev = __builtin_amdgcn_ds_bpermute(e_src + 32 * ry, __float_as_int(e[j]));   // lanes 0 / 15 of a row: column -1 / 16
                        l[j] = __int_as_float(__builtin_amdgcn_update_dpp(ev, __float_as_int(c[j]), 0x111, 0xf, 0xf, false));   // row_shr:1: column - 1
                        r[j] = __int_as_float(__builtin_amdgcn_update_dpp(ev, __float_as_int(c[j]), 0x101, 0xf, 0xf, false));   // row_shl:1: column + 1
                    }
                    acc[o] = __builtin_elementwise_fma(k0, l, acc[o]);   // the same IEEE fma per channel
                    acc[o] = __builtin_elementwise_fma(k1, c, acc[o]);
                    acc[o] = __builtin_elementwise_fma(k2, r, acc[o]);
                }
                __builtin_amdgcn_sched_barrier(0);   // one tap row at a time
            }
#pragma unroll
            for (int o = 0; o < 4; ++o) {
                const f4 y = f4{fmaxf(acc[o].x, 0.f), fmaxf(acc[o].y, 0.f), fmaxf(acc[o].z, 0.f), fmaxf(acc[o].w, 0.f)};
                tile[(o * 16 + ppos) * BR_ROW + pq] = y;
            }
        };
        produce(hv[0], he[0], hin[0], tiles);   // the first patch into buffer 0
        fetch(hv[0], he[0], hin[0], step + BR_DEPTH * stride);
        __syncthreads();   // weights and first tile written
        int buf = 0;
        // one iteration with the slot of patch i + 1, (i + 1) % BR_DEPTH, as a constant; false behind the workgroup's last patch
        auto iter = [&](auto slot) -> bool {
            constexpr int s = decltype(slot)::value;
            BR_STAMP(ds, 0);
            int nb, ny0, nx0;
            const bool have_next = tile_of(step + stride, nb, ny0, nx0);
            // while the consumers run patch i from buffer buf: patch i + 1 into the other one
            if (have_next) produce(hv[s], he[s], hin[s], tiles + (buf ^ 1) * BR_TILE_F4);
            BR_STAMP(ds, 1);
            fetch(hv[s], he[s], hin[s], step + (1 + BR_DEPTH) * stride);   // its slot takes the halo of patch i + 1 + BR_DEPTH
            BR_STAMP(ds, 2);
            __syncthreads();   // patch i + 1 written, patch i read: the buffers change roles
#if BR_DIAG & 1
            BR_STAMP(ds, 3);
            if (++nt == 3 && t == 64 * BR_CONS)   // the workgroup's third patch: the pipeline is full
                for (int i = 0; i < 4; ++i) dst[8 + i] = ds[i];
#endif
            step += stride;
            buf ^= 1;
            return have_next;
        };
        static_assert(BR_DEPTH >= 1 && BR_DEPTH <= 4, "bev_head_roles: halo slots");
        for (;;) {
            if (!iter(br_slot<1 % BR_DEPTH>{})) return;
            if constexpr (BR_DEPTH > 1) { if (!iter(br_slot<2 % BR_DEPTH>{})) return; }
            if constexpr (BR_DEPTH > 2) { if (!iter(br_slot<3 % BR_DEPTH>{})) return; }
            if constexpr (BR_DEPTH > 3) { if (!iter(br_slot<0>{})) return; }
        }
    } else {
        // ---- consumer: lane (pos, g) of wave r = channels 16 kb + 4 g .. + 3 of cell (r, pos) ------------------------------
#if BR_PRIO
        __builtin_amdgcn_s_setprio(1);
#endif
        const int pos = lane & 15, g = lane >> 4;
        {   // the three layers' fragments into LDS: by the consumers alone, which have nothing else to do until the first tile is there
            const f4 *__restrict__ wsrc = reinterpret_cast<const f4 *>(a.wpack);
            for (int i = t; i < BR_W_F4; i += 64 * BR_CONS) wl[i] = *(br_gf4c)(wsrc + i);
        }
        f4 b1[4], b2[4], b3[1];
#pragma unroll
        for (int mb = 0; mb < 4; ++mb) {
            b1[mb] = *reinterpret_cast<const f4 *>(a.bias + 16 * mb + 4 * g);
            b2[mb] = *reinterpret_cast<const f4 *>(a.bias + 64 + 16 * mb + 4 * g);
        }
        b3[0] = *reinterpret_cast<const f4 *>(a.bias + 128 + 4 * g);
        const float last_floor = a.relu_last ? 0.0f : -__builtin_inff();
        __syncthreads();   // weights and first tile written
        const f4 *const w1 = wl + lane, *const w2 = wl + BR_W2 + lane, *const w3 = wl + BR_W3 + lane;
        f4 an[4];          // the next fragments of the weight walk, carried from layer to layer and from tile to tile
#pragma unroll
        for (int i = 0; i < 4; ++i) an[i] = w1[i * 8 * 64];
        int buf = 0;
        for (;;) {
            BR_STAMP(ds, 0);
            const f4 *tile = tiles + buf * BR_TILE_F4 + (wave * 16 + pos) * BR_ROW + g;
            f4 x0[8], x1[4], x2[4], x3[1];
#pragma unroll
            for (int kb = 0; kb < 8; ++kb) x0[kb] = tile[4 * kb];
            BR_STAMP(ds, 1);
            br_layer<8, 4>(x0, x1, w1, b1, 0.0f, an, w2, 4 * 64);
            BR_STAMP(ds, 2);
            br_layer<4, 4>(x1, x2, w2, b2, 0.0f, an, w3, 64);
            BR_STAMP(ds, 3);
            br_layer<4, 1>(x2, x3, w3, b3, last_floor, an, w1, 8 * 64);
            BR_STAMP(ds, 4);
            const bool live = cy0 + wave < a.H && cx0 + pos < a.W;
#if !(BR_DIAG & 1)
            if (live) {
                const long long row = ((long long)cb * a.H + cy0 + wave) * a.W + cx0 + pos;
                store_quad_ragged(a.out + (size_t)row * a.out_stride, 4 * g, a.cout, x3[0]);
            }
#else
            asm volatile("" :: "v"(x3[0]), "v"((int)live));
#endif
            BR_STAMP(ds, 5);
            int nb = 0, ny0 = 0, nx0 = 0;
            const bool have_next = tile_of(step + stride, nb, ny0, nx0);
            __syncthreads();   // patch i + 1 written, patch i read: the buffers change roles
#if BR_DIAG & 1
            BR_STAMP(ds, 6);
            if (++nt == 3 && t == 0)
                for (int i = 0; i < 7; ++i) dst[i] = ds[i];
#endif
            if (!have_next) break;
            step += stride;
            cb = nb; cy0 = ny0; cx0 = nx0;
            buf ^= 1;
        }
    }
}

static int g_bev_head_form = 1;   // pdm_bev_head_fused: 0 = rows_chain_kernel<8,4,4,1,true>, 1 = the role-split kernel above (default)

// Returns 1 in *launched when form 1 is selected and the shapes are the ones the kernel is written for (the caller takes the
// one-role kernel otherwise).  grid_cap = workgroups per CU as pdm_tune_rows_chain_dw_wg_per_cu sets it (one is resident).
int bev_head_roles_launch(void *stream, int B, int H, int W, int C, const float *map, const float *dw_w, const float *dw_shift,
                          int nlayers, const int *dims, const float *wpack, const float *bias, int relu_last, float *out_pm,
                          int out_stride, int cout, int grid_cap, int by_xcd, int *launched) {
    *launched = 0;
    if (g_bev_head_form != 1) return 0;
    const long long rows = (long long)B * H * W;
    if (rows < 8192 || rows >= (1ll << 31) || C != 128 || nlayers != 3 || dims[0] != 128 || dims[1] != 64 || dims[2] != 64 || dims[3] != 16 ||
        cout > 16 || (long long)H * W * 512 >= (1ll << 31))
        return 0;
    BevRolesArgs a{};
    a.B = B; a.H = H; a.W = W; a.by_xcd = by_xcd;
    a.map = map; a.dw_w = dw_w; a.dw_shift = dw_shift; a.wpack = wpack; a.bias = bias;
    a.out = out_pm; a.out_stride = out_stride; a.cout = cout; a.relu_last = relu_last;
    const long long tiles = (long long)B * ((H + 3) / 4) * ((W + 15) / 16);
    const int grid = (int)(tiles < 256 * grid_cap ? tiles : 256 * grid_cap);
    const int rc = grant_lds(reinterpret_cast<const void *>(&bev_head_roles_kernel), BR_LDS_BYTES);
    if (rc) { set_error("bev_head_fused: %d bytes of LDS refused (%d)", BR_LDS_BYTES, rc); return rc; }
    hipLaunchKernelGGL(bev_head_roles_kernel, dim3(grid), dim3(BR_THREADS), BR_LDS_BYTES, as_stream(stream), a);
    *launched = 1;
    return check_launch("bev_head_fused(roles)");
}

}  // namespace pdm

extern "C" int pdm_tune_bev_head_form(int form) {
    const int old = pdm::g_bev_head_form;
    if (form == 0 || form == 1) pdm::g_bev_head_form = form;
    return old;
}

// The voxel path's index side (DESIGN.md "Voxel path"): points -> dynamic voxels with means, the rulebook of a sparse 3-D
// convolution, and the dense canvas of a sparse tensor.  The convolution itself is sparse_conv_mfma.hip.
//
// One structure serves all of it (sc_index.h): an occupancy BITMAP of the grid, one bit per cell in key order
//     key = ((b * nx + x) * ny + y) * nz + z                      (64-bit; z innermost, x-major: torch.unique's order)
// with the number of set bits in front of every group of 256 cells (a multi-launch scan of the groups' popcounts).  The
// rank of a cell, prefix[group] + popcount(bits below it), is its number in ascending key order: no sort, no hash, no
// race (bits are set with integer atomicOr, which commutes), so every result is a function of the input alone.
//   * voxels of pdm_voxel_assign and output sites of a strided convolution are the set bits, numbered by rank;
//   * the rows of a sparse tensor arrive in any order: row_of_rank[rank(key)] = row turns the bitmap into a lookup.
// The grid, the cell key of a point row and the fixed-point feature sums are voxel_grid.h's, shared with the other front ends.
#include "sc_index.h"
#include "voxel_grid.h"

namespace pdm {

// every set cell -> its coordinates (b, z, y, x) at row rank(cell); rows at or past `cap` are not written
__global__ __launch_bounds__(SC_T) void sc_sites_kernel(int nwords, int nx, int ny, int nz, const unsigned *__restrict__ bits,
                                                        const int *__restrict__ gprefix, int cap, int *__restrict__ coords) {
    const long long w = (long long)blockIdx.x * SC_T + threadIdx.x;
    if (w >= nwords) return;
    unsigned word = bits[w];
    if (!word) return;
    const int g = (int)(w / SC_GW);
    int id = gprefix[g];
    for (int q = g * SC_GW; q < w; ++q) id += __popc(bits[q]);
    for (; word; word &= word - 1, ++id) {
        if (id >= cap) return;
        voxel_key_coords(w * 32 + (__ffs((int)word) - 1), nx, ny, nz, coords + (size_t)id * 4);
    }
}

// ---- a. points -> voxels --------------------------------------------------------------------------------------------
// rows -> keys, occupancy bits and the kept rows of every tile of rows
__global__ __launch_bounds__(SC_T) void va_key_kernel(int N, int C1, const float *__restrict__ points, VoxelGrid g, long long *__restrict__ point_key,
                                                      unsigned *__restrict__ bits, int *__restrict__ ptile) {
    tile_reduce<SC_T, SCAN_ITEMS>(N, {ptile}, [&](long long i, int *kept) {
        const long long key = voxel_key<true>(points + (size_t)i * C1, g);
        point_key[i] = key;
        if (key >= 0) {
            sc_set(bits, key);
            ++kept[0];
        }
    });
}

// every kept row: its place in input order, its voxel, and its columns added to the voxel's fixed-point sums
__global__ __launch_bounds__(SC_T) void va_point_kernel(int N, int C1, const float *__restrict__ points, const long long *__restrict__ point_key,
                                                        const int *__restrict__ ptile, const unsigned *__restrict__ bits,
                                                        const int *__restrict__ gprefix, int *__restrict__ kept_idx, int *__restrict__ unq_inv,
                                                        int *__restrict__ voxel_count, unsigned long long *__restrict__ sums) {
    const int C = C1 - 1;
    long long key;
    tile_scan<SC_T, SCAN_ITEMS>(N, {ptile[blockIdx.x]}, [&](long long i, int *v) { key = point_key[i]; v[0] = key >= 0; },
                                [&](long long i, const int *at) {
        if (key < 0) return;
        const int row = at[0], vid = sc_rank(bits, gprefix, key);
        kept_idx[row] = (int)i;
        unq_inv[row] = vid;
        atomicAdd(&voxel_count[vid], 1);
        const float *p = points + (size_t)i * C1 + 1;
        for (int c = 0; c < C; ++c) fixed20_add(&sums[(size_t)vid * C + c], p[c]);
    });
}

struct VaWorkspace {
    size_t point_key, ptile, index, sums, total;
    ScIndexSize isz;
};
static long long va_capacity(long long N, long long ncell) { return N < ncell ? N : ncell; }
static VaWorkspace va_workspace(long long N, int C, long long ncell) {
    VaWorkspace w{};
    w.isz = sc_index_size(ncell);
    size_t at = 0;
    w.point_key = at; at += align256(sizeof(long long) * (size_t)N);
    w.ptile = at; at += align256(sizeof(int) * (size_t)divup(N, SCAN_TILE));
    w.index = at; at += w.isz.bits + w.isz.gprefix + w.isz.tiles;
    w.sums = at; at += align256(sizeof(long long) * (size_t)C * (size_t)va_capacity(N, ncell));
    w.total = at;
    return w;
}

// ---- b. rulebook ------------------------------------------------------------------------------------------------------
struct ScConv {
    int B, D, H, W;         // the input grid; indices are (b, z, y, x)
    int k[3], s[3], p[3];   // kernel, stride, padding on (z, y, x)
    int o[3];               // the output grid
    int subm, kvol;
};

// input rows -> occupancy bits of the input grid; rows outside the grid take no part
__global__ __launch_bounds__(SC_T) void rb_in_set_kernel(int P, const int *__restrict__ idx, ScConv a, unsigned *__restrict__ bits) {
    const long long i = (long long)blockIdx.x * SC_T + threadIdx.x;
    if (i >= P) return;
    const int *c = idx + (size_t)i * 4;
    if (rb_inside(c, a.B, a.D, a.H, a.W)) sc_set(bits, rb_key(c[0], c[1], c[2], c[3], a.D, a.H, a.W));
}
__global__ __launch_bounds__(SC_T) void rb_in_rows_kernel(int P, const int *__restrict__ idx, ScConv a, const unsigned *__restrict__ bits,
                                                          const int *__restrict__ gprefix, int *__restrict__ row_of_rank) {
    const long long i = (long long)blockIdx.x * SC_T + threadIdx.x;
    if (i >= P) return;
    const int *c = idx + (size_t)i * 4;
    if (rb_inside(c, a.B, a.D, a.H, a.W)) row_of_rank[sc_rank(bits, gprefix, rb_key(c[0], c[1], c[2], c[3], a.D, a.H, a.W))] = (int)i;
}
// (input row, offset) -> the output site that reads it there, if any: o s - p + k = in
__global__ __launch_bounds__(SC_T) void rb_out_set_kernel(long long total, const int *__restrict__ idx, ScConv a, unsigned *__restrict__ bits) {
    const long long t = (long long)blockIdx.x * SC_T + threadIdx.x;
    if (t >= total) return;
    const int i = (int)(t / a.kvol), k = (int)(t % a.kvol);
    const int *c = idx + (size_t)i * 4;
    if (!rb_inside(c, a.B, a.D, a.H, a.W)) return;
    const int kk[3] = {k / (a.k[1] * a.k[2]), (k / a.k[2]) % a.k[1], k % a.k[2]};
    int o[3];
    for (int d = 0; d < 3; ++d) {
        const int v = c[1 + d] + a.p[d] - kk[d];
        if (v < 0 || v % a.s[d] != 0 || v / a.s[d] >= a.o[d]) return;
        o[d] = v / a.s[d];
    }
    sc_set(bits, rb_key(c[0], o[0], o[1], o[2], a.o[0], a.o[1], a.o[2]));
}
// (output site, offset) -> the input row there or -1.  Every axis is tested against its own extent, so a neighbour never
// wraps into the next grid row, and the sample index is part of the key, so it never crosses a sample.
__global__ __launch_bounds__(SC_T) void rb_nbr_kernel(long long total, const int *__restrict__ out_idx, ScConv a, const unsigned *__restrict__ bits,
                                                      const int *__restrict__ gprefix, const int *__restrict__ row_of_rank, int *__restrict__ nbr) {
    const long long t = (long long)blockIdx.x * SC_T + threadIdx.x;
    if (t >= total) return;
    const int i = (int)(t / a.kvol), k = (int)(t % a.kvol);
    const int *c = out_idx + (size_t)i * 4;
    const int kk[3] = {k / (a.k[1] * a.k[2]), (k / a.k[2]) % a.k[1], k % a.k[2]};
    int in[4] = {c[0], 0, 0, 0};
    for (int d = 0; d < 3; ++d) in[1 + d] = a.subm ? c[1 + d] + kk[d] - a.k[d] / 2 : c[1 + d] * a.s[d] - a.p[d] + kk[d];
    int row = -1;
    if (rb_inside(in, a.B, a.D, a.H, a.W)) {
        const long long key = rb_key(in[0], in[1], in[2], in[3], a.D, a.H, a.W);
        if (sc_test(bits, key)) row = row_of_rank[sc_rank(bits, gprefix, key)];
    }
    nbr[t] = row;
}

struct RbWorkspace {
    size_t in_index, out_index, row_of_rank, slots, total;
    ScIndexSize in_sz, out_sz;
};
static int rb_conv(const char *who, ScConv *a, int B, int D, int H, int W, int kd, int kh, int kw, int sd, int sh, int sw, int pd, int ph, int pw,
                   int subm) {
    PDM_REQUIRE(B >= 0 && D >= 1 && H >= 1 && W >= 1, PDM_E_BADARG, "%s: bad grid", who);
    PDM_REQUIRE(kd >= 1 && kh >= 1 && kw >= 1 && kd * kh * kw <= 27, PDM_E_BADARG, "%s: kernel %d x %d x %d: at most 27 offsets", who, kd, kh, kw);
    PDM_REQUIRE(sd >= 1 && sh >= 1 && sw >= 1 && pd >= 0 && ph >= 0 && pw >= 0, PDM_E_BADARG, "%s: bad stride or padding", who);
    PDM_REQUIRE(!subm || (sd == 1 && sh == 1 && sw == 1), PDM_E_BADARG, "%s: a submanifold convolution has stride 1", who);
    *a = ScConv{B, D, H, W, {kd, kh, kw}, {sd, sh, sw}, {pd, ph, pw}, {0, 0, 0}, subm != 0, kd * kh * kw};
    const int in[3] = {D, H, W};
    for (int d = 0; d < 3; ++d) {
        a->o[d] = subm ? in[d] : (in[d] + 2 * a->p[d] - a->k[d]) / a->s[d] + 1;
        PDM_REQUIRE(subm || (in[d] + 2 * a->p[d] >= a->k[d] && a->o[d] >= 1), PDM_E_BADARG, "%s: the kernel does not fit the grid", who);
    }
    PDM_REQUIRE((long long)H * W <= 0x7fffffffll && (long long)D * H * W <= SC_MAXCELL && (long long)B * D * H * W <= SC_MAXCELL, PDM_E_TOOLARGE,
                "%s: more than 2^35 cells", who);
    return 0;
}
static RbWorkspace rb_workspace(long long P_in, const ScConv &a) {
    RbWorkspace w{};
    w.in_sz = sc_index_size((long long)a.B * a.D * a.H * a.W);
    w.out_sz = a.subm ? ScIndexSize{} : sc_index_size((long long)a.B * a.o[0] * a.o[1] * a.o[2]);
    size_t at = 0;
    w.in_index = at; at += w.in_sz.bits + w.in_sz.gprefix + w.in_sz.tiles;
    w.out_index = at; at += w.out_sz.bits + w.out_sz.gprefix + w.out_sz.tiles;
    w.row_of_rank = at; at += align256(sizeof(int) * (size_t)P_in);
    w.slots = at; at += 256;
    w.total = at;
    return w;
}

// ---- d. dense ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(SC_T) void sd_fill_kernel(long long n, int *__restrict__ table) {
    const long long c = (long long)blockIdx.x * SC_T + threadIdx.x;
    if (c < n) table[c] = -1;
}
// the table is in the canvas's own order (b, z, y, x): the scatter below reads it and stores the canvas along x alike
__global__ __launch_bounds__(SC_T) void sd_set_kernel(int P, const int *__restrict__ idx, int B, int D, int H, int W, int *__restrict__ table) {
    const long long p = (long long)blockIdx.x * SC_T + threadIdx.x;
    if (p >= P) return;
    const int *c = idx + (size_t)p * 4;
    if (rb_inside(c, B, D, H, W)) table[(((size_t)c[0] * D + c[1]) * H + c[2]) * W + c[3]] = (int)p;
}
// the transposed rulebook: nbr_t[nbr[i][k]][k] = i.  For a fixed input row and offset at most one output site exists, so
// every entry has at most one writer: plain stores, no atomics.  An entry outside [0, P_in) counts as -1, as in the forward.
__global__ __launch_bounds__(SC_T) void rb_transpose_kernel(long long total, int P_in, int kvol, const int *__restrict__ nbr, int *__restrict__ nbr_t) {
    const long long t = (long long)blockIdx.x * SC_T + threadIdx.x;
    if (t >= total) return;
    const int j = nbr[t];
    if (j >= 0 && j < P_in) nbr_t[(size_t)j * kvol + (int)(t % kvol)] = (int)(t / kvol);
}
// thread = cell of one sample (blockIdx.y): every channel of the cell, zeros included
__global__ __launch_bounds__(SC_T) void sd_scatter_kernel(int C, long long plane, const float *__restrict__ feat, const int *__restrict__ table,
                                                          float *__restrict__ out) {
    const long long cell = (long long)blockIdx.x * SC_T + threadIdx.x;
    if (cell >= plane) return;
    const int b = blockIdx.y;
    const int pid = table[(size_t)b * plane + cell];
    const float *f = feat + (size_t)(pid < 0 ? 0 : pid) * C;
    float *o = out + (size_t)b * C * plane + cell;
    for (int c = 0; c < C; ++c) o[(size_t)c * plane] = pid >= 0 ? f[c] : 0.0f;
}

}  // namespace pdm

using namespace pdm;

extern "C" size_t pdm_voxel_assign_workspace_bytes(int N, int C1, int B, int nx, int ny, int nz) {
    if (N < 0 || C1 < 4 || !voxel_grid_cells_ok(B, nx, ny, nz, SC_MAXCELL)) return 0;
    return va_workspace(N, C1 - 1, (long long)B * nx * ny * nz).total;
}

// points (N, C1) fp32 rows (batch_idx, x, y, z, ...), any row order, any 4-byte alignment.  Outputs at capacity: kept_idx,
// unq_inv (N); voxel_coords (cap, 4) = (b, cz, cy, cx), voxel_count (cap), voxel_mean (cap, C1 - 1) with cap = min(N, cells);
// record (2) = {N', P}.  Only the first N' / P entries are meaningful.
extern "C" int pdm_voxel_assign(void *stream, int N, int C1, const float *points, int B, int nx, int ny, int nz, float x0, float y0, float z0,
                                float vx, float vy, float vz, int *kept_idx, int *unq_inv, int *voxel_coords, int *voxel_count,
                                float *voxel_mean, int *record, void *workspace, size_t workspace_bytes) {
    if (int rc = voxel_grid_check("voxel_assign", N, C1, B, nx, ny, nz, SC_MAXCELL, "more than 2^35 cells")) return rc;
    PDM_REQUIRE(vx > 0.0f && vy > 0.0f && vz > 0.0f, PDM_E_BADARG, "voxel_assign: voxel size must be positive");
    PDM_REQUIRE(record, PDM_E_BADARG, "voxel_assign: null pointer");
    const long long ncell = (long long)B * nx * ny * nz, cap = va_capacity(N, ncell);
    PDM_REQUIRE(N == 0 || (points && kept_idx && unq_inv), PDM_E_BADARG, "voxel_assign: null pointer");
    PDM_REQUIRE(cap == 0 || (voxel_coords && voxel_count && voxel_mean), PDM_E_BADARG, "voxel_assign: null pointer");
    const int C = C1 - 1;
    const VaWorkspace w = va_workspace(N, C, ncell);
    PDM_REQUIRE(w.total == 0 || workspace, PDM_E_BADARG, "voxel_assign: null pointer");
    PDM_WS_ALIGNED("voxel_assign", workspace);
    PDM_REQUIRE(workspace_bytes >= w.total, PDM_E_BADARG, "voxel_assign: workspace too small (%zu bytes, need %zu)", workspace_bytes, w.total);
    char *ws = static_cast<char *>(workspace);
    long long *point_key = reinterpret_cast<long long *>(ws + w.point_key);
    int *ptile = reinterpret_cast<int *>(ws + w.ptile);
    const ScIndex ix = sc_index_at(ws + w.index, w.isz);
    long long *sums = reinterpret_cast<long long *>(ws + w.sums);
    const VoxelGrid g{B, nx, ny, nz, x0, y0, z0, vx, vy, vz};
    const int ntp = divup(N, SCAN_TILE);
    hipStream_t s = as_stream(stream);
    if (int rc = zero_fill(stream, "voxel_assign(zero)", ix.bits, w.isz.bits)) return rc;
    if (int rc = zero_fill(stream, "voxel_assign(zero)", sums, sizeof(long long) * (size_t)C * (size_t)cap)) return rc;
    if (int rc = zero_fill(stream, "voxel_assign(zero)", voxel_count, sizeof(int) * (size_t)cap)) return rc;
    if (ntp && ncell) {
        hipLaunchKernelGGL(va_key_kernel, dim3((unsigned)ntp), dim3(SC_T), 0, s, N, C1, points, g, point_key, ix.bits, ptile);
        if (int rc = check_launch("voxel_assign(keys)")) return rc;
    }
    // the voxels' index, and in the same scan launch the kept rows in front of every tile of rows
    if (ix.ntiles) {
        hipLaunchKernelGGL(sc_tile_total_kernel, dim3((unsigned)ix.ntiles), dim3(SC_T), 0, s, ix.ngroups, ix.bits, ix.tiles);
        if (int rc = check_launch("voxel_assign(totals)")) return rc;
    }
    hipLaunchKernelGGL(sc_scan_tiles_kernel, dim3(2), dim3(SC_T), 0, s, ncell ? ntp : 0, ptile, record, ix.ntiles, ix.tiles, record + 1);
    if (int rc = check_launch("voxel_assign(scan)")) return rc;
    if (!(ntp && ncell)) return 0;
    hipLaunchKernelGGL(sc_group_fill_kernel, dim3((unsigned)ix.ntiles), dim3(SC_T), 0, s, ix.ngroups, ix.bits, ix.tiles, ix.gprefix);
    if (int rc = check_launch("voxel_assign(prefix)")) return rc;
    hipLaunchKernelGGL(sc_sites_kernel, dim3((unsigned)divup(ix.nwords, SC_T)), dim3(SC_T), 0, s, ix.nwords, nx, ny, nz, ix.bits, ix.gprefix, (int)cap,
                       voxel_coords);
    if (int rc = check_launch("voxel_assign(voxels)")) return rc;
    hipLaunchKernelGGL(va_point_kernel, dim3((unsigned)ntp), dim3(SC_T), 0, s, N, C1, points, point_key, ptile, ix.bits, ix.gprefix, kept_idx, unq_inv,
                       voxel_count, reinterpret_cast<unsigned long long *>(sums));
    if (int rc = check_launch("voxel_assign(points)")) return rc;
    hipLaunchKernelGGL(fixed20_mean_kernel, dim3((unsigned)divup(cap * C, SCAN_T)), dim3(SCAN_T), 0, s, record, C, sums, voxel_count, voxel_mean);
    return check_launch("voxel_assign(mean)");
}

extern "C" size_t pdm_sparse_rulebook_workspace_bytes(int P_in, int B, int D, int H, int W, int kd, int kh, int kw, int sd, int sh, int sw, int pd,
                                                      int ph, int pw, int subm) {
    ScConv a;
    if (P_in < 0 || rb_conv("sparse_rulebook_workspace_bytes", &a, B, D, H, W, kd, kh, kw, sd, sh, sw, pd, ph, pw, subm)) return 0;
    return rb_workspace(P_in, a).total;
}

static int rb_args(const char *who, ScConv *a, RbWorkspace *w, int P_in, const int *in_indices, int B, int D, int H, int W, int kd, int kh, int kw,
                   int sd, int sh, int sw, int pd, int ph, int pw, int subm, void *workspace, size_t workspace_bytes) {
    if (int rc = rb_conv(who, a, B, D, H, W, kd, kh, kw, sd, sh, sw, pd, ph, pw, subm)) return rc;
    PDM_REQUIRE(P_in >= 0, PDM_E_BADARG, "%s: bad size", who);
    PDM_REQUIRE((long long)P_in * 27 <= 0x7fffffffll, PDM_E_TOOLARGE, "%s: %d rows x 27 offsets exceed int32", who, P_in);
    PDM_REQUIRE(P_in == 0 || in_indices, PDM_E_BADARG, "%s: null pointer", who);
    *w = rb_workspace(P_in, *a);
    PDM_REQUIRE(workspace, PDM_E_BADARG, "%s: null pointer", who);
    PDM_WS_ALIGNED(who, workspace);
    PDM_REQUIRE(workspace_bytes >= w->total, PDM_E_BADARG, "%s: workspace too small (%zu bytes, need %zu)", who, workspace_bytes, w->total);
    return 0;
}

// Step 1 of a rulebook: the input's occupancy index and, for a strided convolution, the output sites' index, both left in
// the workspace for pdm_sparse_rulebook.  in_indices (P_in, 4) int32 (b, z, y, x) in any row order, distinct sites.
// record[0] = the number of output sites (for a submanifold convolution: of input rows inside the grid).
extern "C" int pdm_sparse_sites(void *stream, int P_in, const int *in_indices, int B, int D, int H, int W, int kd, int kh, int kw, int sd, int sh,
                                int sw, int pd, int ph, int pw, int subm, int *record, void *workspace, size_t workspace_bytes) {
    ScConv a;
    RbWorkspace w;
    if (int rc = rb_args("sparse_sites", &a, &w, P_in, in_indices, B, D, H, W, kd, kh, kw, sd, sh, sw, pd, ph, pw, subm, workspace, workspace_bytes))
        return rc;
    PDM_REQUIRE(record, PDM_E_BADARG, "sparse_sites: null pointer");
    char *ws = static_cast<char *>(workspace);
    const ScIndex in = sc_index_at(ws + w.in_index, w.in_sz), out = sc_index_at(ws + w.out_index, w.out_sz);
    int *row_of_rank = reinterpret_cast<int *>(ws + w.row_of_rank), *slots = reinterpret_cast<int *>(ws + w.slots);
    hipStream_t s = as_stream(stream);
    // the two bitmaps are not neighbours in the workspace (each index keeps its prefixes behind its bits)
    if (int rc = zero_fill(stream, "sparse_sites(zero)", in.bits, w.in_sz.bits)) return rc;
    if (int rc = zero_fill(stream, "sparse_sites(zero)", out.bits, w.out_sz.bits)) return rc;
    if (P_in && B) {
        hipLaunchKernelGGL(rb_in_set_kernel, dim3((unsigned)divup(P_in, SC_T)), dim3(SC_T), 0, s, P_in, in_indices, a, in.bits);
        if (int rc = check_launch("sparse_sites(input)")) return rc;
        if (!a.subm) {
            const long long total = (long long)P_in * a.kvol;
            hipLaunchKernelGGL(rb_out_set_kernel, dim3((unsigned)divup(total, SC_T)), dim3(SC_T), 0, s, total, in_indices, a, out.bits);
            if (int rc = check_launch("sparse_sites(output)")) return rc;
        }
    }
    if (a.subm) {
        if (int rc = sc_index_scan(s, "sparse_sites(scan)", in, record, nullptr, nullptr)) return rc;
    } else {
        if (int rc = sc_index_scan(s, "sparse_sites(scan)", out, record, &in, slots)) return rc;
    }
    if (P_in && B) {
        hipLaunchKernelGGL(rb_in_rows_kernel, dim3((unsigned)divup(P_in, SC_T)), dim3(SC_T), 0, s, P_in, in_indices, a, in.bits, in.gprefix, row_of_rank);
        if (int rc = check_launch("sparse_sites(rows)")) return rc;
    }
    return 0;
}

// Step 2, on the workspace pdm_sparse_sites left: out_indices (P_out, 4) in ascending key order of the output grid (strided;
// not written for a submanifold convolution, whose sites are the input rows) and nbr (P_out, kvol): the input row at every
// offset, kx fastest, or -1.
extern "C" int pdm_sparse_rulebook(void *stream, int P_in, const int *in_indices, int P_out, int B, int D, int H, int W, int kd, int kh, int kw,
                                   int sd, int sh, int sw, int pd, int ph, int pw, int subm, int *out_indices, int *nbr, void *workspace,
                                   size_t workspace_bytes) {
    ScConv a;
    RbWorkspace w;
    if (int rc = rb_args("sparse_rulebook", &a, &w, P_in, in_indices, B, D, H, W, kd, kh, kw, sd, sh, sw, pd, ph, pw, subm, workspace, workspace_bytes))
        return rc;
    PDM_REQUIRE(P_out >= 0 && (!a.subm || P_out == P_in), PDM_E_BADARG, "sparse_rulebook: bad size");
    PDM_REQUIRE((long long)P_out * a.kvol <= 0x7fffffffll, PDM_E_TOOLARGE, "sparse_rulebook: %d sites x %d offsets exceed int32", P_out, a.kvol);
    if (P_out == 0) return 0;
    PDM_REQUIRE(nbr && (a.subm || out_indices), PDM_E_BADARG, "sparse_rulebook: null pointer");
    char *ws = static_cast<char *>(workspace);
    const ScIndex in = sc_index_at(ws + w.in_index, w.in_sz), out = sc_index_at(ws + w.out_index, w.out_sz);
    const int *row_of_rank = reinterpret_cast<const int *>(ws + w.row_of_rank);
    hipStream_t s = as_stream(stream);
    if (!a.subm) {
        hipLaunchKernelGGL(sc_sites_kernel, dim3((unsigned)divup(out.nwords, SC_T)), dim3(SC_T), 0, s, out.nwords, a.o[2], a.o[1], a.o[0], out.bits,
                           out.gprefix, P_out, out_indices);
        if (int rc = check_launch("sparse_rulebook(sites)")) return rc;
    }
    const long long total = (long long)P_out * a.kvol;
    hipLaunchKernelGGL(rb_nbr_kernel, dim3((unsigned)divup(total, SC_T)), dim3(SC_T), 0, s, total, a.subm ? in_indices : out_indices, a, in.bits,
                       in.gprefix, row_of_rank, nbr);
    return check_launch("sparse_rulebook(neighbours)");
}

// nbr (P_out, kvol) input rows or -1 -> nbr_t (P_in, kvol): the output row that reads input row j at offset k, or -1.  What the
// data gradient of a strided convolution walks: dx[j] = sum over k of W[k]^T dy[nbr_t[j][k]].
extern "C" int pdm_sparse_rulebook_transpose(void *stream, int P_out, int P_in, int kvol, const int *nbr, int *nbr_t) {
    PDM_REQUIRE(P_out >= 0 && P_in >= 0, PDM_E_BADARG, "sparse_rulebook_transpose: bad size");
    PDM_REQUIRE(kvol >= 1 && kvol <= 27, PDM_E_BADARG, "sparse_rulebook_transpose: %d offsets, at most 27", kvol);
    PDM_REQUIRE((long long)P_out * kvol <= 0x7fffffffll && (long long)P_in * kvol <= 0x7fffffffll, PDM_E_TOOLARGE,
                "sparse_rulebook_transpose: rows x %d offsets exceed int32", kvol);
    PDM_REQUIRE((P_out == 0 || nbr) && (P_in == 0 || nbr_t), PDM_E_BADARG, "sparse_rulebook_transpose: null pointer");
    hipStream_t s = as_stream(stream);
    const long long n_t = (long long)P_in * kvol, n = (long long)P_out * kvol;
    if (n_t == 0) return 0;
    hipLaunchKernelGGL(sd_fill_kernel, dim3((unsigned)divup(n_t, SC_T)), dim3(SC_T), 0, s, n_t, nbr_t);
    if (int rc = check_launch("sparse_rulebook_transpose(fill)")) return rc;
    if (n == 0) return 0;
    hipLaunchKernelGGL(rb_transpose_kernel, dim3((unsigned)divup(n, SC_T)), dim3(SC_T), 0, s, n, P_in, kvol, nbr, nbr_t);
    return check_launch("sparse_rulebook_transpose");
}

extern "C" size_t pdm_sparse_index_workspace_bytes(int P, int B, int D, int H, int W) {
    if (P < 0 || !si_grid_ok(B, D, H, W)) return 0;
    return si_workspace(P, B, D, H, W).total;
}

// The site index of a sparse tensor as an object of its own: indices (P, 4) int32 (b, z, y, x), distinct sites in any row
// order -> bitmap, group prefixes and row_of_rank in the workspace (the layout of sc_index.h's SiWorkspace), where
// pdm_roi_grid_pool reads them.  The submanifold rulebook's chain without the neighbour pass: zero, input bits, three scan
// launches, row_of_rank.  No host read; rows outside the grid take no part.
extern "C" int pdm_sparse_index(void *stream, int P, const int *indices, int B, int D, int H, int W, void *workspace, size_t workspace_bytes) {
    PDM_REQUIRE(P >= 0 && B >= 0 && D >= 1 && H >= 1 && W >= 1, PDM_E_BADARG, "sparse_index: bad size");
    PDM_REQUIRE(si_grid_ok(B, D, H, W), PDM_E_TOOLARGE, "sparse_index: more than 2^35 cells");
    PDM_REQUIRE(workspace && (P == 0 || indices), PDM_E_BADARG, "sparse_index: null pointer");
    PDM_WS_ALIGNED("sparse_index", workspace);
    const SiWorkspace w = si_workspace(P, B, D, H, W);
    PDM_REQUIRE(workspace_bytes >= w.total, PDM_E_BADARG, "sparse_index: workspace too small (%zu bytes, need %zu)", workspace_bytes, w.total);
    char *ws = static_cast<char *>(workspace);
    const ScIndex in = sc_index_at(ws + w.index, w.isz);
    int *row_of_rank = reinterpret_cast<int *>(ws + w.row_of_rank), *slot = reinterpret_cast<int *>(ws + w.slot);
    ScConv a{};
    a.B = B; a.D = D; a.H = H; a.W = W;
    hipStream_t s = as_stream(stream);
    if (int rc = zero_fill(stream, "sparse_index(zero)", in.bits, w.isz.bits)) return rc;
    if (P && B) {
        hipLaunchKernelGGL(rb_in_set_kernel, dim3((unsigned)divup(P, SC_T)), dim3(SC_T), 0, s, P, indices, a, in.bits);
        if (int rc = check_launch("sparse_index(input)")) return rc;
    }
    if (int rc = sc_index_scan(s, "sparse_index(scan)", in, slot, nullptr, nullptr)) return rc;
    if (P && B) {
        hipLaunchKernelGGL(rb_in_rows_kernel, dim3((unsigned)divup(P, SC_T)), dim3(SC_T), 0, s, P, indices, a, in.bits, in.gprefix, row_of_rank);
        if (int rc = check_launch("sparse_index(rows)")) return rc;
    }
    return 0;
}

static int sd_check(const char *who, int B, int D, int H, int W) {
    PDM_REQUIRE(B >= 0 && D >= 1 && H >= 1 && W >= 1, PDM_E_BADARG, "%s: bad grid", who);
    PDM_REQUIRE((long long)D * H * W <= 0x7fffffffll && (long long)B * D * H * W <= 0x7fffffffll, PDM_E_TOOLARGE, "%s: %lld cells exceed int32", who,
                (long long)B * D * H * W);
    return 0;
}
extern "C" size_t pdm_sparse_to_dense_workspace_bytes(int B, int D, int H, int W) {
    if (B < 0 || D < 1 || H < 1 || W < 1 || (long long)D * H * W > 0x7fffffffll || (long long)B * D * H * W > 0x7fffffffll) return 0;
    return align256(sizeof(int) * (size_t)B * D * H * W);
}

// features (P, C), indices (P, 4) (b, z, y, x) -> out (B, C, D, H, W): SparseConvTensor.dense().  A cell table in the
// workspace, then one launch that writes every element, zeros included.  Rows outside the grid are skipped.
extern "C" int pdm_sparse_to_dense(void *stream, int P, int C, const float *features, const int *indices, int B, int D, int H, int W, float *out,
                                   void *workspace, size_t workspace_bytes) {
    if (int rc = sd_check("sparse_to_dense", B, D, H, W)) return rc;
    PDM_REQUIRE(P >= 0 && C >= 1, PDM_E_BADARG, "sparse_to_dense: bad size");
    PDM_REQUIRE(B <= 65535, PDM_E_TOOLARGE, "sparse_to_dense: B at most 65535");
    if (B == 0) return 0;
    const long long plane = (long long)D * H * W, ncell = plane * B;
    PDM_REQUIRE(out && workspace && (P == 0 || (features && indices)), PDM_E_BADARG, "sparse_to_dense: null pointer");
    PDM_WS_ALIGNED("sparse_to_dense", workspace);
    PDM_REQUIRE(workspace_bytes >= sizeof(int) * (size_t)ncell, PDM_E_BADARG, "sparse_to_dense: workspace too small (%zu bytes, need %zu)",
                workspace_bytes, sizeof(int) * (size_t)ncell);
    int *table = static_cast<int *>(workspace);
    hipStream_t s = as_stream(stream);
    hipLaunchKernelGGL(sd_fill_kernel, dim3((unsigned)divup(ncell, SC_T)), dim3(SC_T), 0, s, ncell, table);
    if (int rc = check_launch("sparse_to_dense(fill)")) return rc;
    if (P) {
        hipLaunchKernelGGL(sd_set_kernel, dim3((unsigned)divup(P, SC_T)), dim3(SC_T), 0, s, P, indices, B, D, H, W, table);
        if (int rc = check_launch("sparse_to_dense(set)")) return rc;
    }
    hipLaunchKernelGGL(sd_scatter_kernel, dim3((unsigned)divup(plane, SC_T), (unsigned)B), dim3(SC_T), 0, s, C, plane, features, table, out);
    return check_launch("sparse_to_dense");
}

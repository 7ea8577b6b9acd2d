/*
 * include/pdmssd_hip.h — C ABI of libpdmssd_hip.so (hand-written HIP kernels for gfx950 / MI355X).
 *
 * This is the drop-in boundary for PDM-SSD's point-cloud hot path.  Each entry point replaces one
 * function of the reference's native extension `pointnet2_batch_cuda`
 * (/root/reference/pcdet/ops/pointnet2/pointnet2_batch/src/pointnet2_api.cpp:10-24); the
 * reference-side line each one replaces is cited on the declaration.  Integer/float arguments keep
 * the reference's names, order and meaning; tensors arrive as raw device pointers.
 *
 * Contract (differs from the reference only where the reference is unsafe):
 *   - `stream` is a hipStream_t (NULL = the null stream).  The reference launches on the legacy
 *     default stream with no device guard; here the caller picks the stream and the device is the
 *     one current on the calling thread.  All calls are asynchronous, re-entrant and stateless.
 *   - Ownership: the CALLER allocates and pre-initialises every output / scratch buffer exactly as
 *     the reference's Python does (idx zero-filled for ball_query, temp filled with 1e10 for FPS,
 *     grad buffers zero-filled); the callee only writes through the pointers it is given and
 *     retains nothing.
 *   - Errors: return 0 on success; a positive value is a hipError_t from the launch, a negative
 *     value an argument error (PDM_E_*).  Nothing here ever calls exit() (the reference does:
 *     ball_query_gpu.cu:68-72).  pdm_last_error() returns a thread-local message.
 *   - All tensors are contiguous; data is fp32, indices are int32; 64-bit offsets internally.
 *   - Alignment (DESIGN.md 7p lists every pointer): a typed pointer needs the natural alignment of its element type; a
 *     `void *workspace` that is not 8-byte aligned is rejected (PDM_E_BADARG) unless the entry rounds it up inside.  Beyond that an entry either HANDLES any offset and any size — it takes 16-byte accesses only
 *     where the address and the sizes allow and an element path otherwise, with the same results — or REJECTS a pointer that is
 *     not 16-byte aligned with PDM_E_BADARG before anything is launched.  "align: any" / "align: 16 B ..." on a declaration
 *     says which; an entry without a note handles any offset (element accesses only).
 *   - No host synchronisation, allocation or memcpy inside any call: every entry point is
 *     hipGraph-capturable.
 */
#ifndef PDMSSD_HIP_H
#define PDMSSD_HIP_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PDM_ABI_VERSION 1

#define PDM_E_BADARG (-1)   /* negative size, null pointer, unsupported parameter */
#define PDM_E_TOOLARGE (-2) /* size exceeds what the kernel's grid/indexing supports */

int pdm_abi_version(void);
const char *pdm_last_error(void);

/* ---- pointnet2_batch operators ------------------------------------------------------------ */

/* replaces ball_query_wrapper_fast            ball_query.cpp:29-39 -> ball_query_gpu.cu:15-73
 * new_xyz (B,M,3), xyz (B,N,3) -> idx (B,M,nsample), caller-zeroed. */
/* align: any (xyz is staged 16 bytes at a time only when n % 4 == 0 and xyz is 16-byte aligned). */
int pdm_ball_query(void *stream, int b, int n, int m, float radius, int nsample,
                   const float *new_xyz, const float *xyz, int *idx);

/* replaces group_points_wrapper_fast          group_points.cpp:27-36 -> group_points_gpu.cu:53-92
 * points (B,C,N), idx (B,npoints,nsample) -> out (B,C,npoints,nsample). */
/* align: any (16-byte forms need L = npoints * nsample % 4 == 0 and aligned points / idx / out). */
int pdm_group_points(void *stream, int b, int c, int n, int npoints, int nsample,
                     const float *points, const int *idx, float *out);

/* replaces group_points_grad_wrapper_fast     group_points.cpp:15-24 -> group_points_gpu.cu:14-50
 * grad_out (B,C,npoints,nsample), idx -> grad_points (B,C,N), caller-zeroed, accumulated. */
int pdm_group_points_grad(void *stream, int b, int c, int n, int npoints, int nsample,
                          const float *grad_out, const int *idx, float *grad_points);

/* QueryAndGroup's concat (pointnet2_utils.py:249-257) in channels-last memory for the training path: out (B, M, nsample,
 * 3+C) = an NHWC view of the reference's (B, 3+C, M, nsample) tensor, fp32 or (out_bf16 = 1) bf16 rounded to nearest even
 * from the fp32 value; feat_pm (B, N, C) point-major; idx (B, M, nsample) from pdm_ball_query. */
/* align: any for the whole pdm_group_concat_cl* family (eight bf16 channels per store need ld % 8 == 0 and an aligned out; the
 * backward reads 8-byte words when grad is bf16, ld % 8 == 0 and grad aligned), EXCEPT feat_bf16 = 1: out 16 B, ld % 8 == 0. */
int pdm_group_concat_cl(void *stream, int b, int n, int m, int c, int nsample, const float *xyz, const float *new_xyz,
                        const float *feat_pm, const int *idx, void *out, int out_bf16);
/* Its backward: grad (B, M, nsample, 3+C) fp32 or bf16 -> grad_feat_pm (B, N, C) fp32, fully written (the xyz channels carry
 * no gradient, as in the reference graph).  Scatter inverted into CSR lists in `workspace`
 * (pdm_group_concat_cl_grad_ws_bytes bytes), then one wave per source point adds its rows up: no atomics.  n <= 16384. */
size_t pdm_group_concat_cl_grad_ws_bytes(int b, int n, int m, int nsample);
int pdm_group_concat_cl_grad(void *stream, int b, int n, int m, int c, int nsample, const void *grad, int grad_bf16,
                             const int *idx, float *grad_feat_pm, void *workspace, size_t workspace_bytes);
/* Both with a row stride ld >= 3 + C: out / grad are (B, M, nsample, ld); the forward writes the channels 3 + C .. ld - 1 as
 * ZEROS (padding to 16-byte rows for the bf16 contractions of csrc/train_gemm.hip, ld = 3 + C rounded up to 8). */
int pdm_group_concat_cl_ld(void *stream, int b, int n, int m, int c, int nsample, const float *xyz, const float *new_xyz,
                           const float *feat_pm, const int *idx, void *out, int out_bf16, int ld);
/* the same, source features fp32 (feat_bf16 = 0) or bf16 rows (1: with the bf16 result and ld % 8 == 0; a bf16 feature passes through exactly) */
int pdm_group_concat_cl_ld_f(void *stream, int b, int n, int m, int c, int nsample, const float *xyz, const float *new_xyz,
                             const void *feat_pm, int feat_bf16, const int *idx, void *out, int out_bf16, int ld);
int pdm_group_concat_cl_grad_ld(void *stream, int b, int n, int m, int c, int nsample, const void *grad, int grad_bf16, int ld,
                                const int *idx, float *grad_feat_pm, void *workspace, size_t workspace_bytes);

/* The same backward with a caller-provided workspace (pdm_group_points_grad_ws_bytes bytes): scatter inverted into CSR lists,
 * accumulated without atomics (as pdm_three_interpolate_grad_ws).  Forwards to the plain entry point when a grad_out row
 * (npoints * nsample floats) exceeds 128 KB or n > 16384. */
size_t pdm_group_points_grad_ws_bytes(int b, int npoints, int nsample, int n);
int pdm_group_points_grad_ws(void *stream, int b, int c, int n, int npoints, int nsample, const float *grad_out,
                             const int *idx, float *grad_points, void *workspace, size_t workspace_bytes);

/* replaces gather_points_wrapper_fast         sampling.cpp:14-22 -> sampling_gpu.cu:15-51
 * points (B,C,N), idx (B,npoints) -> out (B,C,npoints). */
int pdm_gather_points(void *stream, int b, int c, int n, int npoints, const float *points,
                      const int *idx, float *out);

/* replaces gather_points_grad_wrapper_fast    sampling.cpp:25-34 -> sampling_gpu.cu:53-90 */
int pdm_gather_points_grad(void *stream, int b, int c, int n, int npoints, const float *grad_out,
                           const int *idx, float *grad_points);

/* replaces farthest_point_sampling_wrapper    sampling.cpp:37-46 -> sampling_gpu.cu:100-260
 * points (B,N,3), temp (B,N) caller-filled with 1e10 (read as the initial min-distances and left
 * holding the final ones) -> idx (B,m).  Tie order identical to the reference's block reduction
 * for block_size = min(2^floor(log2 n), 1024). */
int pdm_furthest_point_sampling(void *stream, int b, int n, int m, const float *points,
                                float *temp, int *idx);

/* Same operator for large clouds (n > 16384): the cloud is split over ceil(n/16384) cooperating workgroups
 * that keep their points in registers and exchange one record per iteration through `workspace`
 * (pdm_furthest_point_sampling_ws_bytes(b, n) bytes, 8-byte aligned, contents irrelevant).  Identical idx/temp.
 * The workgroups of a cloud wait for each other, so a launch holds at most pdm_fps_max_coresident_workgroups()
 * of them (compute units x resident workgroups per unit of the CURRENT device, from the runtime); the call cuts the
 * batch accordingly and takes the single-workgroup kernel where not even one cloud fits.  Every wait is bounded: a
 * workgroup that gives up raises a status word in the workspace, read back (with a stream synchronisation) by
 * pdm_furthest_point_sampling_status: *flag = 1 means the indices of that call must not be used. */
size_t pdm_furthest_point_sampling_ws_bytes(int b, int n);
int pdm_fps_max_coresident_workgroups(void);
/* align: workspace 8 B (checked), as workspace[q] of pdm_furthest_point_sampling_jobs. */
int pdm_furthest_point_sampling_ws(void *stream, int b, int n, int m, const float *points, float *temp,
                                   int *idx, void *workspace, size_t workspace_bytes);
int pdm_furthest_point_sampling_status(void *stream, int b, int n, const void *workspace, int *flag);

/* The same operator as resumable segments (no reference counterpart; same indices): job q computes samples
 * [j0[q], j1[q]) of its own batch of b clouds, continuing from the state an earlier segment left in temp[q] (running
 * min-distances, 1e10 everywhere before the first segment) and idx[q] (samples [0, j0)).  The 1..4 jobs of a call
 * belong to different batches and run side by side in one launch; host arrays of device pointers.  1024 < n <= 16384,
 * or 16384 < n <= 131072 with workspace[q] = pdm_furthest_point_sampling_ws_bytes(b, n) bytes per job (8-byte aligned;
 * the cooperating workgroups must all be resident: njobs * b * ceil(n/16384) <= pdm_fps_max_coresident_workgroups();
 * status per job workspace as above); workspace may be null otherwise. */
int pdm_furthest_point_sampling_jobs(void *stream, int njobs, int b, int n, int m, const float *const *points,
                                     float *const *temp, int *const *idx, const int *j0, const int *j1,
                                     void *const *workspace, size_t workspace_bytes);

/* replaces three_nn_wrapper_fast              interpolate.cpp:18-26 -> interpolate_gpu.cu:16-81
 * unknown (B,n,3), known (B,m,3) -> dist2 (B,n,3) squared distances, idx (B,n,3). */
int pdm_three_nn(void *stream, int b, int n, int m, const float *unknown, const float *known,
                 float *dist2, int *idx);

/* replaces three_interpolate_wrapper_fast     interpolate.cpp:29-41 -> interpolate_gpu.cu:84-124
 * points (B,C,M), idx/weight (B,N,3) -> out (B,C,N). */
int pdm_three_interpolate(void *stream, int b, int c, int m, int n, const float *points,
                          const int *idx, const float *weight, float *out);

/* replaces three_interpolate_grad_wrapper_fast interpolate.cpp:44-56 -> interpolate_gpu.cu:127-168
 * grad_out (B,C,N) -> grad_points (B,C,M), caller-zeroed, accumulated. */
int pdm_three_interpolate_grad(void *stream, int b, int c, int n, int m, const float *grad_out,
                               const int *idx, const float *weight, float *grad_points);

/* The same backward with a caller-provided workspace (pdm_three_interpolate_grad_ws_bytes(b, n, m) bytes): the scatter is
 * first inverted into per-cloud CSR lists (known point <- its contributions), the accumulation then needs no atomics.
 * Same sums in a different fp32 order; m <= 16384 and n <= 32768, otherwise it forwards to the plain entry point. */
size_t pdm_three_interpolate_grad_ws_bytes(int b, int n, int m);
int pdm_three_interpolate_grad_ws(void *stream, int b, int c, int n, int m, const float *grad_out, const int *idx,
                                  const float *weight, float *grad_points, void *workspace, size_t workspace_bytes);

/* ---- fused forms of the same path (additions; same arithmetic, fewer passes over HBM) ------ */

/* QueryAndGroup.forward as one call (pointnet2_utils.py:241-264, use_xyz=True):
 * idx = ball_query (written, caller need not zero it), out[:,0:3] = xyz[idx] - new_xyz,
 * out[:,3:3+C] = features[:, idx].  features (B,C,N) may be NULL when c == 0.
 * out is (B, 3+C, M, nsample). */
/* align: any (idx cleared with byte head and tail; 16-byte forms need nsample % 4 == 0 and aligned idx / out). */
int pdm_query_and_group(void *stream, int b, int n, int m, int c, float radius, int nsample,
                        const float *xyz, const float *new_xyz, const float *features, int *idx,
                        float *out);

/* Grid-accelerated form of pdm_ball_query: identical idx, bit for bit (same caller-zeroed contract),
 * O(candidates near each centre) instead of O(N) per centre.  Needs scratch memory, which this stateless
 * ABI takes from the caller: `workspace` of at least pdm_ball_query_grid_workspace_bytes(b, n) bytes,
 * contents irrelevant before and after the call. */
size_t pdm_ball_query_grid_workspace_bytes(int b, int n);
/* align: any for the grid family (16-byte row stores need nsample % 4 == 0 and an aligned idx; workspaces are rounded up inside). */
int pdm_ball_query_grid(void *stream, int b, int n, int m, float radius, int nsample,
                        const float *new_xyz, const float *xyz, int *idx, void *workspace,
                        size_t workspace_bytes);

/* The grid half and the query half of the call above as separate entry points, so ONE grid serves every query over the
 * same point set: both radii of an SA level (pointnet2_modules.py:37 loops its scales over the same xyz) and the
 * three_nn of the FP module whose known set it is.  Any grid gives exact results; radius_hint only sizes the cells
 * (0 = about two points per occupied cell, the nearest-neighbour setting).  workspace = pdm_ball_query_grid_workspace_bytes(b, n). */
int pdm_grid_build(void *stream, int b, int n, float radius_hint, const float *xyz, void *workspace, size_t workspace_bytes);
int pdm_ball_query_grid_prebuilt(void *stream, int b, int n, int m, float radius, int nsample, const float *new_xyz, int *idx,
                                 const void *workspace, size_t workspace_bytes);
int pdm_three_nn_grid_prebuilt(void *stream, int b, int n, int m, const float *unknown, float *dist2, int *idx,
                               const void *workspace, size_t workspace_bytes);

/* Grid-accelerated form of pdm_three_nn: identical dist2 / idx, bit for bit; needs m >= 1 and a
 * caller-provided workspace of pdm_three_nn_grid_workspace_bytes(b, m) bytes. */
size_t pdm_three_nn_grid_workspace_bytes(int b, int m);
int pdm_three_nn_grid(void *stream, int b, int n, int m, const float *unknown, const float *known,
                      float *dist2, int *idx, void *workspace, size_t workspace_bytes);

/* The reference's python glue between three_nn and three_interpolate in one launch: dist = sqrt(dist2)
 * (pointnet2_utils.py:98; optional, NULL to skip), weight = (1/(dist+1e-8)) / sum_k (1/(dist_k+1e-8))
 * (pointnet2_modules.py:154-156), same correctly-rounded fp32 operations in the same order.  rows = B*n. */
int pdm_three_nn_weights(void *stream, long long rows, const float *dist2, float *dist, float *weight);

/* The gather half of the above for a given idx (B,M,nsample): grouped xyz minus centre, grouped
 * features, concatenated on the channel axis -> out (B, 3+C, M, nsample)
 * (pointnet2_utils.py:250-257: two grouping_operation calls, the in-place subtract and torch.cat). */
/* align: any (as pdm_query_and_group). */
int pdm_group_concat(void *stream, int b, int n, int m, int c, int nsample, const float *xyz,
                     const float *new_xyz, const float *features, const int *idx, float *out);

/* Fused inference forms of one SA scale / one FP module on fp32 MFMA (BatchNorm folded into the
 * weights by the host; pdm_ssd_amd/fused.py builds `dims`, `wpack`, `bias`).  Features are POINT-MAJOR
 * here: feat_pm (B,N,cin), out_pm (B,M,out_stride) with this scale's channels at [out_coff, out_coff+cout).
 * dims = nlayers+1 host ints: padded (multiple-of-16) widths K0, C1..CL.  wpack = per layer, for each
 * 16x16 block (mb, kb): 64 lanes x float4 = W'[16mb + (lane&15)][16kb + 4(lane>>4) + 0..3]; bias = the
 * padded per-layer shifts.  SA input channel order is [features(cin), dx, dy, dz, zero pad].
 *
 * pdm_sa_mlp_fused == pointnet2_utils.py:250-257 (group xyz/features, subtract centre, cat) +
 *                     pointnet2_modules.py:40-52 (MLP, max_pool2d over nsample) for a given idx. */
/* align: 16 B for wpack, bias, out_pm (out_stride, out_coff % 4 == 0) and for feat_pm when cin % 4 == 0; xyz, new_xyz, idx any. */
int pdm_sa_mlp_fused(void *stream, int b, int n, int m, int cin, int nsample, const float *xyz,
                     const float *new_xyz, const float *feat_pm, const int *idx, int nlayers,
                     const int *dims, const float *wpack, const float *bias, float *out_pm,
                     int out_stride, int out_coff, int cout);

/* pdm_fp_mlp_fused == pointnet2_modules.py:158-170 (three_interpolate, cat with the skip features, MLP)
 * for given idx/weight (B,n,3): known_pm (B,m,c_known), skip_pm (B,n,c_skip) or NULL -> out_pm (B,n,out_stride). */
/* align: 16 B for wpack, bias, out_pm (out_stride % 4 == 0), for known_pm when c_known % 4 == 0 and skip_pm when c_skip % 4 == 0;
 * idx, weight any. */
int pdm_fp_mlp_fused(void *stream, int b, int n, int m, int c_known, int c_skip,
                     const float *known_pm, const float *skip_pm, const int *idx, const float *weight,
                     int nlayers, const int *dims, const float *wpack, const float *bias,
                     float *out_pm, int out_stride, int cout);

/* Per-row MLP on fp32 MFMA: in_pm (rows, cin) -> out_pm (rows, out_stride), same dims/wpack/bias packing.
 * relu_last = 0 leaves the last layer linear.  Serves 1x1 convolutions over point-major rows and the
 * pre-projections below. */
/* align: 16 B for wpack, bias, out_pm (out_stride % 4 == 0); in_pm 16 B when cin % 4 == 0 (the LDS-tiled GEMM form — one layer,
 * >= 256 tiles of 128 x 128 — takes any in_pm), any otherwise. */
int pdm_rows_mlp_fused(void *stream, int rows, int cin, const float *in_pm, int nlayers, const int *dims,
                       const float *wpack, const float *bias, int relu_last, float *out_pm, int out_stride,
                       int cout);

/* Two per-row MLPs of EQUAL widths (one dims table) over the SAME rows: out_a = MLP_a(in), out_b = MLP_b(in) — the point
 * head's class and box stacks, one module with two chains on one input
 * (/root/reference/pcdet/models/dense_heads/point_head_box.py:7-60, forward :85-86).  One launch where an instantiation
 * exists (128 -> 256 -> 256 -> <= 16 over >= 8192 rows: the rows are read once), otherwise two pdm_rows_mlp_fused calls;
 * bit-identical outputs either way. */
/* align: as pdm_rows_mlp_fused, for both stacks. */
int pdm_rows_mlp_fused_pair(void *stream, int rows, int cin, const float *in_pm, int nlayers, const int *dims,
                            const float *wpack_a, const float *bias_a, const float *wpack_b, const float *bias_b,
                            int relu_last, float *out_a, int out_stride_a, int cout_a, float *out_b, int out_stride_b,
                            int cout_b);

/* The backbone's LAST feature-propagation module and the point head's two stacks in one launch
 * (/root/reference/pcdet/models/backbones_3d/pointnet2_backbone.py:96-111 writes point_features, which
 * /root/reference/pcdet/models/dense_heads/point_head_box.py:71-76 reads straight back).  FP arguments as
 * pdm_fp_mlp_fused_pre (z = the first layer's known-feature part applied to the m known points), head arguments as
 * pdm_rows_mlp_fused_pair; out_pm receives the module's rows, out_a / out_b the stacks' outputs on them.  Bit-identical to the
 * two calls (FP through the register-resident chain kernel).  Shapes: <= 4 skip channels, dims {16, 128, 128}, hdims
 * {128, 256, 256, 16}, >= 32768 rows; PDM_E_BADARG otherwise (issue the two calls instead). */
/* align: 16 B for z_pm, wpack, bias, out_pm, hw_*, hb_*, out_a, out_b (strides % 4 == 0); skip_pm, idx, weight any. */
int pdm_fp_head_fused(void *stream, int b, int n, int m, int c_skip, const float *z_pm, int z_stride, const float *skip_pm,
                      const int *idx, const float *weight, const int *dims, const float *wpack, const float *bias,
                      float *out_pm, int out_stride, int cout, const int *hdims, const float *hw_a, const float *hb_a,
                      const float *hw_b, const float *hb_b, int relu_last, float *out_a, int out_stride_a, int cout_a,
                      float *out_b, int out_stride_b, int cout_b);
int pdm_tune_fused_pair(int on);   /* 0: always two launches (A/B and tests); returns the previous setting */

/* Point head in training: target assignment + sigmoid focal loss + weighted smooth-L1 loss + d L / d predictions, per point
 * (/root/reference/pcdet/models/dense_heads/point_head_template.py:51-206 with set_ignore_flag, PointResidualCoder with mean
 * sizes box_coder_utils.py:156-179, loss_utils.py:10-141).  n_total = B * n_per_sample points in sample order; box_idx / ext_idx =
 * pdm_points_in_boxes on the boxes / the enlarged boxes; gt_boxes (B, boxes_per_sample, 8); pred_bf16 = dtype of cls_preds
 * (n_total, num_class) and box_preds (n_total, 8) (row strides in elements) AND of the gradients dcls / dbox (contiguous);
 * code_weights: 8 floats on the HOST.  labels (n_total) int64; out (3): [L_cls, L_box, #positives], L_box = NaN when a positive's
 * class exceeds the mean-size table (the reference asserts).  Three launches, no atomics on floats: bit-reproducible. */
int pdm_point_head_loss(void *stream, long long n_total, int n_per_sample, int boxes_per_sample, int num_class, int n_mean,
                        int pred_bf16, const void *cls_preds, long long cls_stride, const void *box_preds, long long box_stride,
                        const float *xyz, long long xyz_stride, const int *box_idx, const int *ext_idx, const float *gt_boxes,
                        const float *mean_size, const float *code_weights, float beta, float alpha, float gamma, float cls_weight,
                        float box_weight, long long *labels, void *dcls, void *dbox, float *out, void *workspace,
                        size_t workspace_bytes);
size_t pdm_point_head_loss_workspace_bytes(long long n_total);

/* Heat-map head in training (the dense half of the hybrid head; /root/reference/pcdet/models/dense_heads/center_head.py:100-160
 * targets, :232 clamped sigmoid, /root/reference/pcdet/utils/loss_utils.py:266-304 penalty-reduced focal loss).
 * pdm_heatmap_targets: heatmap (B, C, H, W) fp32, zeroed here, then per gt box (B, M, 8) [x y z dx dy dz heading class >= 1] a
 *   gaussian of radius max(int(gaussian_radius(dx, dy in cells, min_overlap)), min_radius), window clipped at max_radius,
 *   max-merged (/root/reference/pcdet/models/model_utils/centernet_utils.py:9-70).  cell = (x - x0) / vx / stride.
 * pdm_heatmap_focal_loss: logits (B, C, H, W) fp32 / bf16 with element strides; out[0] = - weight * S / max(peaks, 1),
 *   out[1] = - weight / max(peaks, 1), out[2] = peaks; dlogits (B, C, H, W) contiguous fp32 = d S / d logit (multiply by
 *   out[1] and the incoming gradient).  Partial sums folded in double in a fixed order: bit-reproducible. */
int pdm_heatmap_targets(void *stream, int B, int M, int C, int H, int W, const float *gt_boxes, float x0, float y0, float vx,
                        float vy, float stride, double min_overlap, int min_radius, int max_radius, float *heatmap);
size_t pdm_heatmap_focal_loss_workspace_bytes(long long n);
int pdm_heatmap_focal_loss(void *stream, int B, int C, int H, int W, const void *logits, int logits_bf16, long long sb, long long sc,
                           long long sh, long long sw, const float *heatmap, float weight, float *dlogits, float *out,
                           void *workspace, size_t workspace_bytes);

/* ---- CenterHead (csrc/center_head.hip): targets, heat-map box decode and the L1 regression loss of
 * the reference's pcdet/models/dense_heads/center_head.py, model_utils/centernet_utils.py:155-241 and
 * utils/loss_utils.py:347-419, one launch chain per head for the whole batch.  Nothing synchronises, no float atomics on
 * results or gradients, safe to capture in a graph after one warm-up call.
 *
 * pdm_center_targets: gt_boxes (B, M, cols) fp32, cols = 7 + E + 1, global class (1-based, 0 = padding) last, NOT modified.
 *   local_of: HOST array of num_global + 1 ints, the head's 1-based class of each global class or 0.  A sample's boxes of the
 *   head's classes are compacted in their order; slot k < num_max_objs gets inds = cy * W + cx, mask = 1,
 *   target_boxes = [frac x, frac y, z, log dx, log dy, log dz, cos r, sin r, extras], target_boxes_src = the box with the
 *   head's class; a slot whose dx <= 0 or dy <= 0 stays used and zero (mask 0).  heatmap (B, C, H, W) = the gaussians of
 *   pdm_heatmap_targets (the same device code) with the window never clipped short of the map.  Every element is written.
 * pdm_center_decode: maps = HOST array of 6 device pointers [hm logits (C), center (2), center_z (1), dim (3), rot (2: cos,
 *   sin), vel (2) | NULL], bf16 = HOST array of 6 flags, strides = HOST array of 6 x 4 element strides (b, c, y, x).  Per
 *   sample the K <= H * W (K <= 16384) highest sigmoid(hm) over (class, y, x), ties by lower flat index (rank_select.h); per
 *   rank x = ((cx + center_x) * stride) * vx + x0 (each step one fp32 rounding), likewise y, z = center_z, dims = exp(dim),
 *   angle = atan2(sin, cos); kept iff x, y, z within limit_range (HOST [lo3, hi3], inclusive) and score > score_thresh;
 *   survivors compacted in rank order: boxes (B, K, 7 + E), scores (B, K), labels (B, K) int64 = global_of[class] + 1
 *   (global_of: HOST array of C ints), count (B) int32, padding rows zero.
 * pdm_center_reg_loss: chans = HOST array of D = 8 + E device pointers, the (B, H, W) plane of each regression channel in
 *   code order, bf16 / strides (D x 3: b, y, x) HOST arrays; inds, mask (B, num_max_objs) int64; target (B, num_max_objs, D);
 *   code_weights HOST array of D floats.  loss_per_code (D) = sum |pred m - gt m| / max(num, 1), m = mask * !isnan(target),
 *   num = sum(mask); out = [loc_loss = loc_weight * sum(loss_per_code * code_weights), max(num, 1), num]; grad (B, D, H, W) =
 *   d loc_loss / d map, slots of one cell added in slot order by the one thread that owns the cell, other cells exact zeros.
 *   workspace >= pdm_center_reg_loss_workspace_bytes(B, D), 8-byte aligned.  num_max_objs <= 8192, D <= 16. */
int pdm_center_targets(void *stream, int B, int M, int cols, int C, int H, int W, const float *gt_boxes, int num_global,
                       const int *local_of, float x0, float y0, float vx, float vy, float stride, int num_max_objs,
                       double min_overlap, int min_radius, float *heatmap, float *target_boxes, long long *inds,
                       long long *mask, float *target_boxes_src);
int pdm_center_decode(void *stream, int B, int C, int H, int W, int K, const void *const *maps, const int *bf16,
                      const long long *strides, float score_thresh, const float *limit_range, float x0, float y0,
                      float vx, float vy, float stride, const int *global_of, float *boxes, float *scores,
                      long long *labels, int *count);
size_t pdm_center_reg_loss_workspace_bytes(int B, int D);
int pdm_center_reg_loss(void *stream, int B, int num_max_objs, int D, int H, int W, const void *const *chans, const int *bf16,
                        const long long *strides, const long long *inds, const long long *mask, const float *target,
                        const float *code_weights, float loc_weight, float *loss_per_code, float *out, float *grad,
                        void *workspace, size_t workspace_bytes);

/* ---- TransFusionHead (csrc/attention.hip, csrc/transfusion.hip): fused attention forward, query
 * initialisation and query-wise box decode of the reference's pcdet/models/dense_heads/transfusion_head.py:151-218, :397-479.
 * Nothing synchronises, nothing is read on the host, no float atomics, single stream; safe to capture in a graph after one
 * warm-up call.
 *
 * pdm_mha_forward: q (B, P, C), k (B, N, C), v (B, N, C) fp32, each with its own ROW stride in elements (>= C; a sample is
 *   `rows` consecutive rows, so k and v may be the two halves of one (B, N, 2C) tensor); d = C / nheads.  out (B, P, C),
 *   contiguous = softmax(q_h k_h^T / sqrt(d)) v_h per head, heads concatenated (what lies between nn.MultiheadAttention's
 *   in- and out-projection with no mask and no dropout).  Supported: d in {16, 32}, C <= 256, P >= 1, N >= 1; anything
 *   else is PDM_E_BADARG.  The keys are cut into chunks of keys_per_chunk (0 = pdm_mha_default_keys_per_chunk()); one
 *   workgroup per (sample, head, chunk, 64 queries) runs an online softmax on the fp32 MFMA and writes (maximum, sum,
 *   unnormalised accumulator); a second launch folds the partials in chunk order.  The chunking depends on
 *   (N, keys_per_chunk) alone: two runs give the same bits.  workspace >= pdm_mha_forward_workspace_bytes(...), 8-byte
 *   aligned.  align: any (q and k are read 16 bytes at a time only when both are 16-byte aligned with strides % 4 == 0).
 * pdm_tf_proposals: logits (B, C, H, W) fp32 contiguous.  s = sigmoid(logit); a cell of class c keeps s if no cell of its
 *   nms_kernel x nms_kernel window (odd) has a greater s and the cell is at least nms_kernel / 2 from the border; a class in
 *   `exempt` (HOST array of num_exempt ints) keeps s everywhere; every other cell scores 0.  Per sample the P <= 16384
 *   highest scores over the flat (class, y, x) index, ties by lower index (rank_select.h): index (B, P) int64 = y * W + x,
 *   cls (B, P) int64, query_heatmap_score (B, C, P) = the masked score of every class at the cell, query_pos (B, P, 2) =
 *   (index % y_size + 0.5, index / y_size + 0.5), the reference's flipped `ij` mesh.  Three launches: the filter over all
 *   cells, a rank select of the best P of every slice of 4096 flat indices, a rank select over those candidates.
 *   workspace >= pdm_tf_proposals_workspace_bytes(B, C, H, W, P), 8-byte aligned.
 * pdm_tf_decode: heatmap (B, C, P) logits, center (B, 2, P) with the query position added, height (B, 1, P), dim (B, 3, P),
 *   rot (B, 2, P) = [sin, cos], vel (B, 2, P) | NULL, cls (B, P) int64, query_heatmap_score (B, C, P); all contiguous.
 *   Query p of class c: score = sigmoid(heatmap[c, p]) * query_heatmap_score[c, p]; x = (center_x * stride) * vx + x0 (each
 *   step one fp32 rounding), y likewise, z = height, sizes exp(dim), angle atan2(rot[0], rot[1]); kept iff score >
 *   score_thresh (>= 0, strict) and x, y, z within limit_range (HOST [lo3, hi3], inclusive); survivors compacted in query
 *   order: boxes (B, P, 7 | 9), scores (B, P), labels (B, P) int64 = c + 1, count (B) int32; padding rows zero. */
int pdm_mha_default_keys_per_chunk(void);
size_t pdm_mha_forward_workspace_bytes(int B, int P, int N, int C, int nheads, int keys_per_chunk);
int pdm_mha_forward(void *stream, int B, int P, int N, int C, int nheads, const float *q, long long q_stride,
                    const float *k, long long k_stride, const float *v, long long v_stride, int keys_per_chunk,
                    float *out, void *workspace, size_t workspace_bytes);
/* ---- Training through the fused attention (csrc/attention.hip, csrc/attention_bwd.hip).  Nothing
 * synchronises, nothing is read on the host, no float atomics: two runs give the same bits; capturable after one warm-up call.
 *
 * Attention dropout (csrc/draws.h): weight (b, h, query i, key j) is kept iff
 *   fmix32(draw_key(seed, step, b * H + h, i) ^ j * 0x9E3779B1) >= floor(dropout_p * 2^32),  0 <= dropout_p < 1,
 *   and a kept weight is multiplied by 1.0f / (1.0f - (float)dropout_p).  The softmax sum is the sum before dropout.
 *   dropout_p == 0: no draw is evaluated, step and used_step are not touched and may be NULL.
 * pdm_mha_forward_train: pdm_mha_forward (the same device code) plus the dropout and stats (B, H, P, 2) = the query's RAW
 *   score maximum over all keys and its softmax sum.  step: a device-resident counter; the call reads it, copies the value it
 *   used to used_step[0] (device) and advances it by one in its last launch.  With dropout_p == 0 `out` is pdm_mha_forward's
 *   bit for bit.  workspace >= pdm_mha_forward_train_workspace_bytes(...), 8-byte aligned.
 * pdm_mha_backward: q, k, v as the forward took them, out (B, P, C) and dout (B, P, C) contiguous, stats and used_step from the
 *   forward -> dq (B, P, C), dk (B, N, C), dv (B, N, C), each with its OWN row stride (dk and dv may be the halves of one
 *   (B, N, 2C) buffer; dq, dk, dv the thirds of a (B, P, 3C) one).  Key-stationary: a workgroup owns
 *   pdm_mha_backward_keys_per_block(N, keys_per_chunk) keys (16, 64 or 256) and walks the query tiles in ascending order, so dk
 *   and dv have one writer and one summation order; dq goes through one partial per key block in the workspace, folded in
 *   block order by a last launch.  The supported set is the forward's; a short workspace is refused.  align: any (16-byte
 *   accesses only when every buffer is 16-byte aligned with strides % 4 == 0).
 * pdm_mha_dropout_keep: keep (B, nheads, P, N) uint8 = the mask of step[0] (a device pointer; not advanced). */
size_t pdm_mha_forward_train_workspace_bytes(int B, int P, int N, int C, int nheads, int keys_per_chunk);
int pdm_mha_forward_train(void *stream, int B, int P, int N, int C, int nheads, const float *q, long long q_stride,
                          const float *k, long long k_stride, const float *v, long long v_stride, int keys_per_chunk,
                          double dropout_p, unsigned seed, unsigned *step, unsigned *used_step, float *stats,
                          float *out, void *workspace, size_t workspace_bytes);
int pdm_mha_backward_keys_per_block(int N, int keys_per_chunk);
size_t pdm_mha_backward_workspace_bytes(int B, int P, int N, int C, int nheads, int keys_per_chunk);
int pdm_mha_backward(void *stream, int B, int P, int N, int C, int nheads, const float *q, long long q_stride,
                     const float *k, long long k_stride, const float *v, long long v_stride, const float *out,
                     const float *dout, const float *stats, double dropout_p, unsigned seed,
                     const unsigned *used_step, int keys_per_chunk, float *dq, long long dq_stride, float *dk,
                     long long dk_stride, float *dv, long long dv_stride, void *workspace, size_t workspace_bytes);
int pdm_mha_dropout_keep(void *stream, int B, int nheads, int P, int N, double dropout_p, unsigned seed,
                         const unsigned *step, unsigned char *keep);
size_t pdm_tf_proposals_workspace_bytes(int B, int C, int H, int W, int P);
int pdm_tf_proposals(void *stream, int B, int C, int H, int W, const float *logits, int nms_kernel, int num_exempt,
                     const int *exempt, int P, int y_size, long long *index, long long *cls,
                     float *query_heatmap_score, float *query_pos, void *workspace, size_t workspace_bytes);
int pdm_tf_decode(void *stream, int B, int C, int P, const float *heatmap, const float *center, const float *height,
                  const float *dim, const float *rot, const float *vel, const long long *cls,
                  const float *query_heatmap_score, float score_thresh, const float *limit_range, float x0, float y0,
                  float vx, float vy, float stride, float *boxes, float *scores, long long *labels, int *count);

/* ---- TransFusionHead in training (csrc/tf_assign.hip): a batched linear-sum-assignment solver, the
 * Hungarian assigner's costs, matching and targets, and the head's three losses with their gradients.  Nothing synchronises;
 * no atomics on results except the order-free integer max that merges heat-map gaussians; two runs give the same bits.
 * pdm_lsap: cost (B, P, >= Gmax) fp32 with row stride row_stride (sample stride P * row_stride), num_gt (B) int32 on the DEVICE
 *   (clamped to [0, Gmax]).  Per sample, min sum cost over the matchings of size min(P, G) of the P x G leading block: what
 *   scipy.optimize.linear_sum_assignment returns wherever the optimum is unique.  gt_of_row (B, P) int32 = the matched column or
 *   -1; row_of_gt (B, Gmax) int32 = the matched row, or -1 (columns >= num_gt[b]; unmatched columns when G > P).  One workgroup
 *   per sample, shortest augmenting paths (Jonker-Volgenant / Crouse), duals and path lengths in fp64, ties by lower column
 *   index of the solver's matrix (rows = the smaller side).  Loop bounds: min(P, G) augmentations of at most max(P, G) steps.
 *   A cost that is not finite (NaN, +Inf, -Inf) is read as FLT_MAX (scipy raises instead).  1 <= P <= 1024, 0 <= Gmax <= 1024,
 *   anything else is PDM_E_BADARG.
 * pdm_tf_assign: the maps as pdm_tf_decode takes them; gt_boxes (B, M, gt_cols = 8 | 10) [x y z dx dy dz yaw (vx vy) class],
 *   class 1-based, zero rows = padding; a box is valid iff dx > 0 && dy > 0, valid boxes keep their order.  cost_cfg HOST
 *   doubles [cls weight, alpha, gamma, eps, reg weight, iou weight]; pc_range HOST [x0 y0 z0 x1 y1 z1].  cost = focal cost at
 *   the gt's class + L1 of the range-normalised centres + (- IoU3D) (z read as the box's bottom, as the reference's overlaps()
 *   does), each times its weight, in fp32; then pdm_lsap's solver; then labels (B, P) int64 = class - 1 | num_classes,
 *   label_weights (B, P) = 1, bbox_targets / bbox_weights (B, P, 8 | 10), ious (B, P) = the matched pair's IoU in [0, 1],
 *   assigned (B, P) int32 = index among the sample's valid boxes | -1, num_pos (1) int32, matched_ious (1) = mean over the
 *   samples of the per-sample mean, heatmap_target (B, C, H, W) = the gaussians of the valid boxes (radius from
 *   gaussian_overlap and min_radius over (dy, dx) cells, centre cell truncated; a centre cell outside the map draws nothing).
 *   workspace >= pdm_tf_assign_workspace_bytes(B, P, M), 8-byte aligned.  P <= 1024, M <= 1024.
 * pdm_tf_loss: SigmoidFocalClassificationLoss(alpha, gamma) of heatmap against the one-hot of labels times label_weights, and
 *   L1 of [center height dim rot (vel)] against bbox_targets times bbox_weights * code_weights (HOST, 8 | 10), each
 *   / max(num_pos, 1) (read on the device) times its weight; the dense heat-map term is pdm_heatmap_focal_loss.  out (6) =
 *   [cls, box, heat-map loss, the factor of g_dense, peaks, unused]; g_heatmap .. g_vel = d loss / d map, final; g_dense =
 *   d S / d dense_heatmap, to be multiplied by out[3].  workspace >= pdm_tf_loss_workspace_bytes(...), 8-byte aligned. */
int pdm_lsap(void *stream, int B, int P, int Gmax, const float *cost, long long row_stride, const int *num_gt, int *gt_of_row,
             int *row_of_gt);
size_t pdm_tf_assign_workspace_bytes(int B, int P, int M);
int pdm_tf_assign(void *stream, int B, int C, int P, int M, int gt_cols, int H, int W, const float *heatmap, const float *center,
                  const float *height, const float *dim, const float *rot, const float *vel, const float *gt_boxes,
                  const double *cost_cfg, const float *pc_range, float vx, float vy, float stride, double gaussian_overlap,
                  int min_radius, int num_classes, long long *labels, float *label_weights, float *bbox_targets,
                  float *bbox_weights, float *ious, int *assigned, int *num_pos, float *matched_ious, float *heatmap_target,
                  void *workspace, size_t workspace_bytes);
size_t pdm_tf_loss_workspace_bytes(int B, int C, int P, int with_vel, int H, int W);
int pdm_tf_loss(void *stream, int B, int C, int P, int H, int W, const float *heatmap, const float *center, const float *height,
                const float *dim, const float *rot, const float *vel, const float *dense_heatmap, const long long *labels,
                const float *label_weights, const float *bbox_targets, const float *bbox_weights, const int *num_pos,
                const float *heatmap_target, const float *code_weights, float cls_weight, float bbox_weight, float hm_weight,
                float alpha, float gamma, float *out, float *g_heatmap, float *g_center, float *g_height, float *g_dim,
                float *g_rot, float *g_vel, float *g_dense, void *workspace, size_t workspace_bytes);

/* OPT-IN: the same three-layer per-row MLP with fp32 EMULATED on the bf16 matrix pipe — every fp32 operand split into three
 * bf16 pieces (8 + 8 + 8 significand bits), a product formed from the six leading partial products on
 * v_mfma_f32_16x16x32_bf16 with fp32 accumulation (3/8 of the fp32-MFMA pipe time; dropped terms <= 2^-24 |a b|).
 * Only dims = {128, 256, 256, 16} (the point head's stacks, point_head_box.py:7-60); `wstream` = the pre-split weights in
 * consumption order (pdm_ssd_amd/fused.py::PackedMLPx3, pdm_rows_mlp_x3_stream_bytes bytes), bias fp32 padded. */
/* align: 16 B for in_pm, wstream, bias, out_pm. */
int pdm_rows_mlp_x3(void *stream, int rows, int cin, const float *in_pm, int nlayers, const int *dims, const void *wstream,
                    size_t wstream_bytes, const float *bias, int relu_last, float *out_pm, int out_stride, int cout);
size_t pdm_rows_mlp_x3_stream_bytes(int nlayers, const int *dims);
int pdm_tune_rows_x3_wg_per_cu(int n);

/* The same SA scale / FP module with the wide part of the FIRST layer hoisted out of the per-pair (per-fine-
 * point) loop — algebraically identical, fp32 rounding order differs (tests: <= 1e-4 of the oracle):
 *   SA:  W1 [f_nb ; x_nb - c] = z[nb] + W1[:, xyz] (x_nb - c),   z = W1[:, features] f  over the n source points;
 *   FP:  W1 [sum_k w_k f_k ; s] = sum_k w_k z[idx_k] + W1[:, skip] s,   z = W1[:, known] f  over the m known points.
 * z_pm rows hold the layer's padded C1 floats at [z_coff, z_coff + C1pad) of z_stride (pdm_rows_mlp_fused with
 * relu_last = 0 and zero bias); dims[0] is the padded width of what stays in the kernel (16 for xyz; the
 * padded skip width, or 16 with zero weights when c_skip == 0). */
/* align: as pdm_sa_mlp_fused / pdm_fp_mlp_fused, and 16 B for z_pm (z_stride, z_coff % 4 == 0). */
int pdm_sa_mlp_fused_pre(void *stream, int b, int n, int m, int nsample, const float *xyz,
                         const float *new_xyz, const float *z_pm, int z_stride, int z_coff, const int *idx,
                         int nlayers, const int *dims, const float *wpack, const float *bias, float *out_pm,
                         int out_stride, int out_coff, int cout);
int pdm_fp_mlp_fused_pre(void *stream, int b, int n, int m, int c_skip, const float *z_pm, int z_stride,
                         const float *skip_pm, const int *idx, const float *weight, int nlayers,
                         const int *dims, const float *wpack, const float *bias, float *out_pm,
                         int out_stride, int cout);

/* Neighbour-list compaction for the fused SA kernels (no reference counterpart: ball_query pads short
 * neighbourhoods with copies of the first hit, pointnet2/src/ball_query_gpu.cu:38-46, and the reference runs the
 * shared MLP over those copies; max-pool over a multiset = max-pool over the set, so they can be dropped).
 *   pdm_sa_pack: idx (B,M,nsample) int32, nsample 16 or 32 -> pack (pdm_sa_pack_rows(b,m,nsample) x 2 int32:
 *     {source row b*n + neighbour, centre b*m + j | -1 dead}) and meta (8 int32: first row of the segment classes
 *     L = 1,2,4,8,16,32, total rows, live rows).  A centre with cnt significant slots (1 + the last slot that differs
 *     from slot 0) owns 2^ceil(log2 cnt) consecutive rows; classes are tile-aligned, order = centre order.
 *   pdm_sa_mlp_packed: pdm_sa_mlp_fused (z_pm null) / pdm_sa_mlp_fused_pre (z_pm set) over that list; results are
 *     bit-identical to the unpacked entry points. */
size_t pdm_sa_pack_workspace_bytes(int b, int m);
size_t pdm_sa_pack_rows(int b, int m, int nsample);
/* align: idx 16 B (rows are read as int4), pack 8 B.  pdm_sa_mlp_packed and pdm_sa_mlp_packed_pair: pack 8 B and, as pdm_sa_mlp_fused /
 * pdm_sa_mlp_fused_pre, 16 B for wpack, bias, out_pm, z_pm (strides and offsets % 4 == 0) and for feat_pm when cin % 4 == 0. */
int pdm_sa_pack(void *stream, int b, int n, int m, int nsample, const int *idx, void *workspace,
                size_t workspace_bytes, int *pack, int *meta);
/* both scales of an MSG level in one count -> scan -> fill sequence (per-scale nsample / idx / workspace / pack / meta as HOST arrays
 * of two; each workspace of workspace_bytes >= pdm_sa_pack_workspace_bytes(b, m)) */
int pdm_sa_pack_pair(void *stream, int b, int n, int m, const int *nsample, const int *const *idx, void *const *workspace,
                     size_t workspace_bytes, int *const *pack, int *const *meta);
int pdm_sa_mlp_packed(void *stream, int b, int n, int m, int cin, int nsample, const float *xyz,
                      const float *new_xyz, const float *feat_pm, const float *z_pm, int z_stride, int z_coff,
                      const int *pack, const int *meta, int nlayers, const int *dims, const float *wpack,
                      const float *bias, float *out_pm, int out_stride, int out_coff, int cout);

/* The two scales of an MSG level (pointnet2_modules.py:58-99: the same centres, two radii / MLPs) in ONE launch: per-scale
 * arguments as HOST arrays of two (nsample, z_coff, pack, meta, nlayers, dims, wpack, bias, out_coff, cout), the level's xyz /
 * new_xyz / feat_pm / z_pm / out_pm shared.  One launch where both scales map to the same kernel instantiation (the deep levels
 * of PointNet2MSG: a few hundred row tiles per scale, which two launches run one after the other on a mostly idle chip),
 * otherwise two pdm_sa_mlp_packed launches; bit-identical either way. */
int pdm_sa_mlp_packed_pair(void *stream, int b, int n, int m, int cin, const int *nsample, const float *xyz,
                           const float *new_xyz, const float *feat_pm, const float *z_pm, int z_stride, const int *z_coff,
                           const int *const *pack, const int *const *meta, const int *nlayers, const int *const *dims,
                           const float *const *wpack, const float *const *bias, float *out_pm, int out_stride,
                           const int *out_coff, const int *cout);
int pdm_tune_sa_pair(int on);          /* 0: always two launches */

/* ---- pointnet2_stack: ragged ("stacked") batches -----------------------
 * One entry per function of the reference's pointnet2_stack_cuda extension that the PointNet++ modules use
 * (pcdet/ops/pointnet2/pointnet2_stack/src/pointnet2_api.cpp): points of all samples concatenated, per-sample
 * counts in int32 DEVICE arrays (*_batch_cnt, B entries, B <= 1024).  Same arithmetic as the batch entries.
 *   ball_query_wrapper_stack           ball_query.cpp      idx (M,nsample) LOCAL to the sample, caller-zeroed;
 *                                                           an empty ball stores idx[0] = -1 (ball_query_gpu.cu:66)
 *   group_points[_grad]_wrapper_stack  group_points.cpp    out (M,C,nsample); grad_features (N,C) caller-zeroed
 *   three_nn_wrapper_stack             interpolate.cpp     dist2 (N,3), idx (N,3) GLOBAL; +inf / start when the
 *                                                           sample has fewer than three known points
 *   three_interpolate[_grad]_wrapper_stack                 features (M,C) -> out (N,C); grad caller-zeroed
 *   stack_farthest_point_sampling_wrapper  sampling.cpp    GLOBAL indices, packed per sample; temp = 1e10 */
int pdm_stack_ball_query(void *stream, int B, int M, float radius, int nsample, const float *new_xyz,
                         const int *new_xyz_batch_cnt, const float *xyz, const int *xyz_batch_cnt, int *idx);
int pdm_stack_group_points(void *stream, int B, int M, int C, int nsample, const float *features,
                           const int *features_batch_cnt, const int *idx, const int *idx_batch_cnt, float *out);
int pdm_stack_group_points_grad(void *stream, int B, int M, int C, int N, int nsample, const float *grad_out,
                                const int *idx, const int *idx_batch_cnt, const int *features_batch_cnt,
                                float *grad_features);
int pdm_stack_three_nn(void *stream, int B, int N, const float *unknown, const int *unknown_batch_cnt,
                       const float *known, const int *known_batch_cnt, float *dist2, int *idx);
int pdm_stack_three_interpolate(void *stream, int N, int C, const float *features, const int *idx,
                                const float *weight, float *out);
int pdm_stack_three_interpolate_grad(void *stream, int N, int C, const float *grad_out, const int *idx,
                                     const float *weight, float *grad_features);
/* max_n = largest per-sample point count (host value; selects the kernel instantiation) */
int pdm_stack_furthest_point_sampling(void *stream, int B, int max_n, const float *xyz, float *temp,
                                      const int *xyz_batch_cnt, int *idxs, const int *num_sampled_points);

/* ---- pointnet2_stack: voxel query and the vector-pool family (second half) ------------
 * pcdet/ops/pointnet2/pointnet2_stack/src/pointnet2_api.cpp:14 and :25-30 bind
 *   voxel_query_wrapper                                  voxel_query.cpp:20 / voxel_query_gpu.cu:11-91
 *   query_stacked_local_neighbor_idxs_wrapper_stack      vector_pool.cpp:63  / vector_pool_gpu.cu:125-205
 *   query_three_nn_by_stacked_local_idxs_wrapper_stack   vector_pool.cpp:19  / vector_pool_gpu.cu:19-87
 *   vector_pool_wrapper, vector_pool_grad_wrapper        vector_pool.cpp:113, :170 / vector_pool_gpu.cu:245-443
 * The reference gives out slots of the stacked outputs with atomicAdd on a cursor and has python re-run the kernel
 * with a larger buffer on overrun; here the cursor is an exclusive prefix sum of per-centre counts (centre order —
 * one of the orders the race allows, and the same on every run), exposed as a count pass and a fill pass so a
 * caller can size the buffers exactly.  pdm_stack_query_local_neighbor_idxs is the reference's one-call form
 * (count + fill into a stack of avg_length * M slots, writes stop at the capacity, *cumsum += total).
 *
 * voxel_query: idx (M, nsample) GLOBAL indices, caller-zeroed; window cells visited z outer / x inner; kept when
 *   d2 <= radius^2; the first hit fills the row; idx[0] = -1 when nothing was found.
 * local neighbours: first by index, at most nsample when nsample > 0, never more than 1000; neighbor_type 1 = ball
 *   (d2 <= r^2), otherwise cube (|l| <= r per axis); start_len (M,2) = [offset, length]; indices GLOBAL.
 * three_nn_by_local_idxs: dist2 / idxs (M, num_total_grids, 3); idx -1 and +inf for an empty list; the best is
 *   repeated into unfilled second / third slots.  stack_len = valid length of stack_neighbor_idxs.
 * vector_pool: new_features (M, num_c_out) and new_local_xyz (M, 3G) are SUMS (overwritten, no zero-fill needed;
 *   python divides by point_cnt_of_grid); input channel i folds onto i % (num_c_out / G); pooling_type 0 = sum,
 *   1 = first point of each cell; grouped_idxs (num_max_sum_points, 3) = [support idx, centre, cell] at
 *   entry_start[centre] + rank; entries past num_max_sum_points are dropped.  (num_c_out + 4G) * 4 B <= 48 KB.
 * vector_pool_grad: grad_support_features (N, C_in) caller-zeroed, float atomics (order undefined, as upstream). */
int pdm_stack_voxel_query(void *stream, int M, int Z, int Y, int X, int nsample, float radius, int z_range, int y_range,
                          int x_range, const float *new_xyz, const float *xyz, const int *new_coords,
                          const int *point_indices, int *idx);
int pdm_stack_local_neighbor_count(void *stream, const float *support_xyz, const int *xyz_batch_cnt, const float *new_xyz,
                                   const int *new_xyz_batch_cnt, int *start_len, int *cumsum, float max_neighbour_distance,
                                   int batch_size, int M, int nsample, int neighbor_type);
int pdm_stack_local_neighbor_fill(void *stream, const float *support_xyz, const int *xyz_batch_cnt, const float *new_xyz,
                                  const int *new_xyz_batch_cnt, int *stack_neighbor_idxs, const int *start_len,
                                  long long stack_capacity, float max_neighbour_distance, int batch_size, int M, int nsample,
                                  int neighbor_type);
int pdm_stack_query_local_neighbor_idxs(void *stream, const float *support_xyz, const int *xyz_batch_cnt,
                                        const float *new_xyz, const int *new_xyz_batch_cnt, int *stack_neighbor_idxs,
                                        int *start_len, int *cumsum, int avg_length_of_neighbor_idxs,
                                        float max_neighbour_distance, int batch_size, int M, int nsample, int neighbor_type);
int pdm_stack_three_nn_by_local_idxs(void *stream, const float *support_xyz, const float *new_xyz_grid_centers,
                                     int *new_xyz_grid_idxs, float *new_xyz_grid_dist2, const int *stack_neighbor_idxs,
                                     const int *start_len, long long stack_len, int M, int num_total_grids);
/* entry_cnt (M) = entries each centre records, entry_start (M) = their exclusive prefix, *total += the sum */
int pdm_stack_vector_pool_count(void *stream, const float *support_xyz, const int *xyz_batch_cnt, const float *new_xyz,
                                const int *new_xyz_batch_cnt, int *entry_start, int *entry_cnt, int *total, int num_grid_x,
                                int num_grid_y, int num_grid_z, float max_neighbour_distance, int batch_size, int M,
                                int nsample, int neighbor_type, int pooling_type);
int pdm_stack_vector_pool(void *stream, const float *support_xyz, const float *support_features, const int *xyz_batch_cnt,
                          const float *new_xyz, float *new_features, float *new_local_xyz, const int *new_xyz_batch_cnt,
                          int *point_cnt_of_grid, int *grouped_idxs, const int *entry_start, int num_grid_x, int num_grid_y,
                          int num_grid_z, float max_neighbour_distance, int batch_size, int M, int num_c_in, int num_c_out,
                          int use_xyz, int num_max_sum_points, int nsample, int neighbor_type, int pooling_type);
int pdm_stack_vector_pool_grad(void *stream, const float *grad_new_features, const int *point_cnt_of_grid,
                               const int *grouped_idxs, float *grad_support_features, int N, int M, int num_c_out,
                               int num_c_in, int num_total_grids, int num_entries);

/* ---- training-mode BatchNorm + ReLU as one operator (configs[3], the shared MLPs' Conv/Linear -> BN -> ReLU triples:
 * pcdet/ops/pointnet2/pointnet2_batch/pointnet2_modules.py:19-55, models/dense_heads/point_head_template.py:35-48) ----
 * dtype 0 = fp32, 1 = bf16 activations (statistics, gamma/beta and gradients of gamma/beta always fp32).
 * layout 0: x is (n rows, C) with the channel fastest, C a multiple of 4 (fp32) / 8 (bf16); L ignored.
 * layout 1: x is (n, C, L) with the position fastest, L a multiple of 4 / 8.
 * forward: batch mean / biased variance per channel, y = [relu]((x - mean) * invstd * gamma + beta); running_mean /
 *   running_var (may be null) updated as torch.nn.BatchNorm does (momentum, unbiased variance); coef (4, C) fp32 =
 *   [mean | invstd | gamma*invstd | beta] is what the backward needs besides x.
 * backward: dx (same type and layout as x), grads (4, C) fp32 = [dgamma | dbeta | p | q] (dx = gamma invstd (g - p - (x - mean) q)).
 * partial: workspace of pdm_bn_parts(layout, n, C, L) * C * 2 floats (slice sums, folded in double: reproducible). */
/* align (every pdm_bn_* entry): 16 B for x, y, dy, dx, xmax, xmin, imax, imin, coef and grads; 8 B for partial. */
int pdm_bn_parts(int layout, long long n, int C, long long L);
int pdm_bn_relu_forward(void *stream, int dtype, int layout, long long n, int C, long long L, const void *x, void *y,
                        const float *gamma, const float *beta, float eps, float momentum, float *running_mean,
                        float *running_var, float *coef, float *partial, int relu);
/* the same forward with the statistics already taken by the producer of x (pdm_tg_gemm_nt's `stats`: [parts][C][2] column sums
 * of x and x^2): finalize + apply only, rows x C layout */
int pdm_bn_relu_forward_stats(void *stream, int dtype, long long n, int C, const void *x, void *y, const float *gamma,
                              const float *beta, float eps, float momentum, float *running_mean, float *running_var,
                              float *coef, const float *partial, int parts, int relu);
/* statistics only (rows x C; dtype 0 / 1): reduce + finalize -> coef (4, C) and the running statistics, no normalised tensor (a
 * consumer applies BatchNorm + ReLU while it reads x); partial: pdm_bn_parts(0, n, C, 1) * C * 2 floats */
int pdm_bn_forward_coef(void *stream, int dtype, long long n, int C, const void *x, const float *gamma, const float *beta, float eps,
                        float momentum, float *running_mean, float *running_var, float *coef, float *partial);
/* finalize only: coef (4, C) from the producer's sums + running statistics (the consumer normalises while it reads x) */
int pdm_bn_finalize_stats(void *stream, long long n, int C, const float *gamma, const float *beta, float eps, float momentum,
                          float *running_mean, float *running_var, float *coef, const float *partial, int parts);
int pdm_bn_relu_backward(void *stream, int dtype, int layout, long long n, int C, long long L, const void *x, const void *dy,
                         void *dx, const float *coef, float *grads, float *partial, int relu);
/* its two halves: `_stats` leaves grads (4, C) = [dgamma | dbeta | p | q] and writes no dx (a consumer forms dx while it reads
 * dy and x: pdm_tg_gemm_nt_dy); `_apply` writes dx = scale (dy [bn(x) > 0] - p - (x - mean) q) from grads already there */
int pdm_bn_relu_backward_stats(void *stream, int dtype, int layout, long long n, int C, long long L, const void *x, const void *dy,
                               const float *coef, float *grads, float *partial, int relu);
int pdm_bn_relu_backward_apply(void *stream, int dtype, int layout, long long n, int C, long long L, const void *x, const void *dy,
                               void *dx, const float *coef, float *grads, int relu);
/* finalize only: grads (4, C) from [parts][C][2] sums (sum g, sum g xhat) a producer of dy has already taken in its epilogue
 * (pdm_tg_gemm_nt_bs / pdm_tg_gemm_nt_dy_bs): pdm_bn_relu_backward_stats without its pass over dy and x */
int pdm_bn_finalize_bwd_stats(void *stream, long long n, int C, const float *coef, float *grads, const float *partial, int parts);

/* The tail of an SA scale in training — BatchNorm + ReLU + max over the ns neighbours of each group
 * (pointnet2_modules.py:46-52: the last (BatchNorm2d, ReLU) of the shared MLP, then F.max_pool2d over nsample) — as ONE
 * operator.  x is (G groups, ns <= 255, C) with the channel fastest; y (G, C).  relu(bn(.)) is monotone in x, so one pass
 * over x gives the statistics and each group's max / min (+ first index), the pooled output is the function of that
 * extreme, and the normalised tensor is never written; backward = sums over the pooled tensors + one pass for dx.
 * xmax / xmin (G, C, x's type) and imax / imin (G, C, bytes) are the forward's record for the backward.
 * pdm_bn_pool_parts: slices of `partial` ((parts, C, 2) floats). */
int pdm_bn_pool_parts(int dtype, long long G, int C);
int pdm_bn_relu_pool_forward(void *stream, int dtype, long long G, int ns, int C, const void *x, void *y, void *xmax, void *xmin,
                             unsigned char *imax, unsigned char *imin, const float *gamma, const float *beta, float eps,
                             float momentum, float *running_mean, float *running_var, float *coef, float *partial, int relu);
/* the forward when the producer of x (pdm_tg_gemm_nt_pool) has already left the column sums ([parts][C][2]) and every group's
 * max / min: finalize + pooled output only; bf16 (dtype 1) */
int pdm_bn_relu_pool_forward_kept(void *stream, int dtype, long long G, int ns, int C, void *y, const void *xmax, const void *xmin,
                                  const float *gamma, const float *beta, float eps, float momentum, float *running_mean,
                                  float *running_var, float *coef, const float *partial, int parts, int relu);
int pdm_bn_relu_pool_backward(void *stream, int dtype, long long G, int ns, int C, const void *x, const void *dy, void *dx,
                              const void *xmax, const void *xmin, const unsigned char *imax, const unsigned char *imin,
                              const float *coef, float *grads, float *partial, int relu);

/* ---- hybrid head (north_star configs[2]: "backbone + PDM neck + hybrid head"; no reference source: SURVEY.md F1) ----
 * Depthwise 3x3 convolution + folded BatchNorm + ReLU over the neck's channels-last BEV grid, the context stage of
 * the heat-map head (pdm_ssd_amd/dense_heads/pdm_heatmap_head.py); the point head's MLPs and the heat-map head's 1x1
 * stack run through pdm_rows_mlp_fused.  in / out (B, H, W, C) fp32, w (9, C) tap-major, shift (C); C % 4 == 0. */
/* align: 16 B for every pointer of the pdm_bev_depthwise3x3* entries and of pdm_bev_head_fused; pdm_point_head_decode: code 16 B
 * (code_stride % 4 == 0), the others any. */
int pdm_bev_depthwise3x3(void *stream, int B, int H, int W, int C, const float *in, const float *w, const float *shift,
                         float *out, int relu);
/* The heat-map head's inference stack in ONE launch: out[cell] = MLP(relu(depthwise3x3(map)[cell] + shift)), the
 * depthwise convolution formed on the fly as the prologue of the register-resident row MLP (csrc/rows_chain.hip); same
 * arithmetic order as pdm_bev_depthwise3x3 followed by pdm_rows_mlp_fused (bit-identical).  Packed weights as for
 * pdm_rows_mlp_fused.  Instantiated for C = 128 -> 64 -> 64 -> <= 16; PDM_E_BADARG for other widths. */
int pdm_bev_head_fused(void *stream, int B, int H, int W, int C, const float *map, const float *dw_w, const float *dw_shift,
                       int nlayers, const int *dims, const float *wpack, const float *bias, int relu_last, float *out_pm,
                       int out_stride, int cout);
/* Point head epilogue (point_head_box.py:97-113 in eval mode): score = sigmoid(max class logit), box = the
 * PointResidualCoder decoding (box_coder_utils.py:188-222, use_mean_size) of the code with the arg-max class's mean size,
 * for every point in one pass.  cls (N, cls_stride), code (N, code_stride >= 8, rows 16-byte aligned), pts (N, pts_stride >= 3),
 * mean_size (num_class, 3) -> boxes (N, 7), scores (N). */
int pdm_point_head_decode(void *stream, long long n, int num_class, const float *cls, int cls_stride, const float *code,
                          int code_stride, const float *pts, int pts_stride, const float *mean_size, float *boxes, float *scores);
/* Weight gradient of that convolution (training): gw (9, C), zeroed by the caller, += sum over cells of gout * in[tap].
 * The data gradient is pdm_bev_depthwise3x3 on gout with the nine taps mirrored. */
int pdm_bev_depthwise3x3_wgrad(void *stream, int B, int H, int W, int C, const float *in, const float *gout, float *gw);
/* the pair above with ONE side of the map held in bf16 (training under bf16 autocast; fp32 arithmetic, one rounding to nearest
 * even): forward fp32 -> bf16 (out_bf16), data gradient bf16 -> fp32 (in_bf16), weight gradient with a bf16 output gradient */
int pdm_bev_depthwise3x3_t(void *stream, int B, int H, int W, int C, const void *in, int in_bf16, const float *w, const float *shift,
                           void *out, int out_bf16, int relu);
int pdm_bev_depthwise3x3_wgrad_t(void *stream, int B, int H, int W, int C, const float *in, const void *gout, int gout_bf16, float *gw);

/* ---- rotated-box IoU / NMS ---------------------------------------------
 * One entry per function of the reference's iou3d_nms_cuda extension (pcdet/ops/iou3d_nms/src/iou3d_nms_api.cpp):
 *   boxes_overlap_bev_gpu / boxes_iou_bev_gpu        iou3d_nms.cpp:55,96     (na, nb) areas / BEV IoUs
 *   boxes_aligned_overlap_bev_gpu, paired_boxes_overlap_bev_gpu  :37,76      element-wise overlap of two box lists
 *   nms_gpu / nms_normal_gpu                         iou3d_nms.cpp:137,186   greedy suppression of score-sorted boxes
 * Boxes are rows of 7 floats [x, y, z, dx, dy, dz, heading].  pdm_nms differs from the reference in mechanism only:
 * the suppression mask is reduced on the device; keep (n) int64 and *num_out are DEVICE buffers, workspace >=
 * pdm_nms_workspace_bytes(n). */
int pdm_boxes_overlap_bev(void *stream, int na, const float *boxes_a, int nb, const float *boxes_b, float *out);
int pdm_boxes_iou_bev(void *stream, int na, const float *boxes_a, int nb, const float *boxes_b, float *out);
int pdm_boxes_aligned_overlap_bev(void *stream, int n, const float *boxes_a, const float *boxes_b, float *out);
size_t pdm_nms_workspace_bytes(int n);
int pdm_nms(void *stream, int n, const float *boxes, float thresh, int normal, void *workspace,
            size_t workspace_bytes, long long *keep, int *num_out);
/* Batched detector post-processing (post_process.hip; Detector3DTemplate.post_processing with
 * POST_PROCESSING.BATCHED): for all B samples at once, score threshold, the first pre_max candidates in
 * pdm_topk_sampling's order (score descending, equal scores by lower row), NMS as pdm_nms (bit-identical keep lists),
 * the first post_max survivors.  multi_class = 0: one segment per sample, score = max over the C columns (lowest
 * class wins a tie), label = argmax + 1.  multi_class = 1 (C <= 64): one segment per (sample, class k), score =
 * cls[:, k], label = k + 1, a sample's survivors class after class.  cls (rows, C) probabilities with row stride
 * cls_stride, boxes (rows, >= 7) with row stride box_stride; offsets (B + 1) int32 DEVICE rows of each sample;
 * batch_index (rows) float or NULL: when given, a row outside its sample's range or of another sample sets *err_flag.
 * Outputs (P = post_max, or C * post_max in multi-class mode), every entry written: out_rows (B, P) int64 row within
 * the sample (-1 padding), out_boxes (B, P, 7), out_scores (B, P), out_labels (B, P) int64, out_count (B) int32.
 * gt (B, G, gt_dim >= 7) or NULL: recall (1 + num_thresh) int64 = [gt rows, kept-box recall at each threshold]
 * summed over the batch (generate_recall_record: trailing all-zero gt rows trimmed, 3-D IoU max over the kept boxes
 * > threshold); recall_thresh is a HOST array of num_thresh <= 8 floats.  pre_max <= 16384, G <= 4096, B * segments
 * <= 65535; workspace >= pdm_post_process_workspace_bytes(segments, pre_max, post_max), of which the NMS mask is
 * segments * pre_max * ceil(pre_max / 64) * 8 bytes.  Nothing synchronises; counts, flag and recall stay on the device. */
size_t pdm_post_process_workspace_bytes(int num_segments, int pre_max, int post_max);
int pdm_post_process(void *stream, int B, int C, int multi_class, long long rows, const float *cls, int cls_stride,
                     const float *boxes, int box_stride, const int *offsets, const float *batch_index, float score_thresh,
                     int pre_max, int post_max, float nms_thresh, int nms_normal, int G, int gt_dim, const float *gt,
                     int num_thresh, const float *recall_thresh, void *workspace, size_t workspace_bytes, long long *out_rows,
                     float *out_boxes, float *out_scores, long long *out_labels, int *out_count, int *err_flag,
                     long long *recall);
/* roiaware_pool3d's points_in_boxes_gpu (roiaware_pool3d.cpp / roiaware_pool3d_kernel.cu:313-336): boxes (B,T,7),
 * pts (B,M,3) -> box_idx (B,M) = first containing box of the sample's list, -1 for background (every entry written). */
int pdm_points_in_boxes(void *stream, int B, int T, int M, const float *boxes, const float *pts, int *box_idx);

/* ---- RoI point pooling and RoI-aware pooling (csrc/roi_pool.hip) -----------------------------------------------------------
 * The reference's roipoint_pool3d_cuda.forward (pcdet/ops/roipoint_pool3d/src/roipoint_pool3d_kernel.cu:22-134): xyz (B,N,3),
 * boxes (B,M,7) ALREADY enlarged, feats (B,N,C) -> pooled (B,M,S,3+C), empty_flag (B,M) int32.  Per (sample, box): the points
 * inside (check_pt_in_box3d, the test of pdm_points_in_boxes) in ascending index, the first S of them; with 0 < cnt < S
 * row k >= cnt repeats row k % cnt; a row is [x, y, z, feats...] copied bit for bit.  cnt == 0: flag 1 and the box's S rows
 * are NOT written (the caller zero-fills, as the reference's); every flag is written.  One launch, no (B,N,M) intermediate,
 * nothing allocated.  B, N, M or S == 0: success, nothing written. */
/* align: any (rows are written with an element head up to a 16-byte boundary of the address). */
int pdm_roipoint_pool3d(void *stream, int B, int N, int M, int C, int S, const float *xyz, const float *boxes, const float *feats,
                        float *pooled, int *empty_flag);
/* The same with the PointRCNN head's epilogue (pcdet/models/roi_heads/pointrcnn_head.py:121-129) in the launch: rois
 * (B,M,roi_stride >= 7 floats per row) NOT enlarged — their three sizes grow by (extra_x, extra_y, extra_z) here —, the pooled
 * coordinates minus the RoI centre and rotated by -heading about z (fp32, one rounding per operation:
 * x' = x cos a + y (-sin a), y' = x sin a + y cos a, a = -heading), and ZEROS in all S rows of an empty box: no caller fill. */
int pdm_roipoint_pool3d_canonical(void *stream, int B, int N, int M, int C, int S, const float *xyz, const float *rois, int roi_stride,
                                  float extra_x, float extra_y, float extra_z, const float *feats, float *pooled, int *empty_flag);
/* The reference's roiaware_pool3d_cuda.forward / backward (pcdet/ops/roiaware_pool3d/src/roiaware_pool3d_kernel.cu:39-307).
 * rois (K,7), pts (P,3), feats (P,C), pool_method 0 = max, 1 = avg -> pts_idx_of_voxels (K,ox,oy,oz,max_pts) int32 (slot 0 the
 * count capped at max_pts - 1, then the voxel's first max_pts - 1 point indices ascending, zeros behind: FULLY written), argmax
 * (K,ox,oy,oz,C) int32 (max only: always written, -1 = no winner) and pooled (K,ox,oy,oz,C) (NOT written for a voxel without
 * winner / without points: the caller zero-fills).  Max is a strict > from -inf (first index wins ties, NaN never wins); avg adds
 * in list order and divides once by float(count).  Each out size 1 .. 256, max_pts >= 2.  workspace: K * ox * oy * oz ints when
 * the voxel grid of a box exceeds 8192 cells, else none (pdm_roiaware_pool3d_workspace_bytes).
 * backward: grad_out (K,ox,oy,oz,C) -> grad_in (P,C), FULLY written and deterministic (terms added in ascending (box, voxel)
 * order): max, grad_out to the argmax point; avg, grad_out * (1 / max(count, 1)) to every listed point.  It gathers per point, so
 * it takes rois and pts as well; argmax is read for max only, pts_idx_of_voxels for avg only. */
size_t pdm_roiaware_pool3d_workspace_bytes(int K, int out_x, int out_y, int out_z);
int pdm_roiaware_pool3d_forward(void *stream, int K, int P, int C, int max_pts, int out_x, int out_y, int out_z, const float *rois,
                                const float *pts, const float *feats, int pool_method, void *workspace, size_t workspace_bytes,
                                int *pts_idx_of_voxels, int *argmax, float *pooled);
int pdm_roiaware_pool3d_backward(void *stream, int K, int P, int C, int max_pts, int out_x, int out_y, int out_z, const float *rois,
                                 const float *pts, const int *pts_idx_of_voxels, const int *argmax, const float *grad_out,
                                 int pool_method, float *grad_in);
/* Part-A2's RoI-aware pooling for the whole batch, straight to sparse rows (csrc/roiaware_sparse.hip): what
 * pdm_roiaware_pool3d_forward 'avg' on part and 'max' on rpn per sample, `cat`, `sum(-1) != 0`, `nonzero` and a gather compute,
 * bit for bit, without the dense (B N, S^3, 4 + C) tensor.  rois (B, N, 7); pts (P, 3) batch-major with counts (B) int32 rows per
 * sample; part (P, 4); rpn (P, C).  Two calls around the caller's ONE host read:
 *   _index  count -> scan -> fill into the workspace; record (2) int32 = {Q, overflow}.  Q = active cells: those whose fp32 sum,
 *           in ascending channel order, of the four averaged part channels is non-zero.  overflow = 1: a box's point lists did
 *           not fit list_capacity ints (its rows are missing: refuse the result).  The lists hold a cell's first max_pts - 1
 *           points in ascending index, as the composed kernel's do.
 *   _emit   with that Q and the same workspace: coords (Q, 4) int32 rows (roi, x, y, z) ascending in ((roi ox + x) oy + y) oz + z,
 *           out_part (Q, 4) the average, out_rpn (Q, C) the maximum (0 where nothing wins).  Q == 0 launches nothing.
 * At most 4096 cells a box, B <= 1024, B N min(P, cells (max_pts - 1)) < 2^31.  No float atomics: two runs give the same bits. */
size_t pdm_roiaware_pool_sparse_workspace_bytes(int B, int N, int out_x, int out_y, int out_z, long long list_capacity);
int pdm_roiaware_pool_sparse_index(void *stream, int B, int N, int P, int max_pts, int out_x, int out_y, int out_z, const float *rois,
                                   const float *pts, const int *counts, const float *part, long long list_capacity, int *record,
                                   void *workspace, size_t workspace_bytes);
int pdm_roiaware_pool_sparse_emit(void *stream, int B, int N, int P, int C, int out_x, int out_y, int out_z, const float *part,
                                  const float *rpn, long long list_capacity, int Q, const void *workspace, size_t workspace_bytes,
                                  int *coords, float *out_part, float *out_rpn);
/* dense() of the RoI grids + the first shared FC of Part-A2's head without the dense tensor (csrc/sparse_fc.hip):
 * coords (Q, 4) int32 rows (box, x, y, z) ascending in ((box sx + x) sy + y) sz + z, one row per (box, cell) at most; xa (Q, C_a)
 * and xb (Q, C_b) or null with C_b = 0, read where they lie (channel c < C_a from xa, else from xb), C = C_a + C_b; wpack
 * (pdm_sparse_fc_packed_floats) [cell][kb][nb][lane][j] = W[16 nb + (lane & 15)][(16 kb + 4 (lane >> 4) + j) cells + cell] of the
 * Conv1d weight (Cout, C cells); scale / shift (Cout) both or neither; relu.
 * -> out (R, Cout) = epilogue(sum over the rows q of box r of W[:, :, cell(q)] x[q]), epilogue(v) = relu(v scale + shift) as one
 * multiply and one add; boxes without rows get epilogue(0).  The sum runs over pdm_sparse_fc_chunks(R, cells, Cout) partials of
 * ascending cells added in ascending order, the boundaries a function of those three sizes alone: no atomics, two runs give the
 * same bits.  C_a, C_b multiples of 4, C of 16 up to 512, Cout of 16 up to 1024; xa, xb, wpack 16-byte aligned.  No host read. */
size_t pdm_sparse_fc_packed_floats(int cells, int C, int Cout);
int pdm_sparse_fc_chunks(int R, int cells, int Cout);
size_t pdm_sparse_fc_workspace_bytes(long long Q, int R, int cells, int Cout);
int pdm_sparse_fc(void *stream, long long Q, int R, int sx, int sy, int sz, int Ca, int Cb, int Cout, const int *coords, const float *xa,
                  const float *xb, const float *wpack, const float *scale, const float *shift, int relu, float *out, void *workspace,
                  size_t workspace_bytes);

/* ---- input path -------------------------------------------------------
 * sample_points (pcdet/datasets/processor/data_processor.py:182-212) + the batch-index column of collate_batch
 * (pcdet/datasets/dataset.py:237-244) for B raw clouds resident in HBM: raw (sum counts, C) rows [x, y, z, ...],
 * counts (B) int32 on the device, out (B * num_points, 1 + C) rows [cloud, x, y, z, ...]; choice (B * num_points)
 * int32 or NULL receives the chosen raw row per output row.  The random draw is defined by counter-based hashes of
 * (seed, cloud, row) — DESIGN.md section 10 — not by numpy's RNG.  num_points <= 16384, 3 <= C <= 16. */
int pdm_sample_points(void *stream, int B, int num_points, unsigned seed, int C, const float *raw,
                      const int *counts, float *out, int *choice);

/* ---- training augmentation (csrc/augment.hip) --------------------------------------------
 * The reference's DataAugmentor.forward with gt_sampling, random_world_flip / _rotation / _scaling
 * (data_augmentor.py:290-318, database_sampler.py:130-147 / :365-443 / :445-502, augmentor_utils.py:8-92), limit_period,
 * and the range mask + class column of the data processor (data_processor.py:79-93, dataset.py:158-215), for B scenes
 * at once.  Box rows are 8 floats [x, y, z, dx, dy, dz, heading, class]: class > 0 a target (index + 1), < 0 a
 * non-target box that only blocks candidates, 0 padding.  Limits: B <= 1024, G <= 8 sample groups, K = sum of the
 * groups' sample numbers <= 256 candidate slots per scene, M <= 256 input boxes per scene, M_out <= 512,
 * 3 <= C <= 16 point features.  Group arrays (class index, sample number, database entries, first database index of
 * the class) are HOST arrays; everything else is on the device.  The draws are build-defined functions of
 * (seed, state, scene, group) documented in augment.hip.  workspace >= pdm_augment_workspace_bytes(B, K), shared by
 * the calls of one augmentation (draw -> select -> scene_count -> scene_fill on one stream).
 *   draw:   state (1 + 2G) int32 [step, (epoch, pointer) per group], advanced in place -> sampled (B, K) database
 *           indices (-1 padded; group t owns the slots from the sum of the earlier sample numbers), flip (B) bits
 *           (1 = x, 2 = y), angle (B), scale (B).  flip_axes: bit mask of the configured axes.
 *   select: collision test, accepted (B, K) (-1 padded) / num_accepted (B), out_boxes (B, M_out, 8) = the target and
 *           accepted boxes transformed, heading wrapped, range-masked (remove_outside), zero-padded; out_num_boxes (B).
 *           ops = the transform list, one nibble each from the lowest: 1 flip x, 2 flip y, 3 rotation, 4 scaling.
 *           point_cloud_range: HOST array of 6 floats.  Sampled indices outside [0, db_entries) count as padding.
 *   scene_count / scene_fill: rows = [object points of the accepted entries] + [scene points outside every accepted
 *           box enlarged by extra_width (HOST, 3 floats)], transformed, x / y range-masked; out_counts (B) and the
 *           overflow flag (total > capacity) are written by scene_count, the rows (scene after scene, C floats each,
 *           never past capacity) by scene_fill.  db_points (P, C) relative to the box centre, db_offsets (entries + 1). */
size_t pdm_augment_workspace_bytes(int B, int K);
int pdm_augment_draw(void *stream, int B, int G, const int *group_class, const int *group_num, const int *group_len,
                     const int *group_first, int limit_whole_scene, int M, const float *gt_boxes, unsigned seed, int *state,
                     int flip_axes, int use_rot, float rot_lo, float rot_hi, int use_scale, float scale_lo, float scale_hi,
                     int K, int *sampled, int *flip, float *angle, float *scale, void *workspace, size_t workspace_bytes);
int pdm_augment_select(void *stream, int B, int M, const float *gt_boxes, int G, const int *group_class,
                       const int *group_num, long long db_entries, const float *db_boxes, const long long *db_offsets, int K,
                       const int *sampled, const int *flip, const float *angle, const float *scale, unsigned ops,
                       const float *point_cloud_range, int remove_outside, int M_out, float *out_boxes, int *out_num_boxes,
                       int *accepted, int *num_accepted, void *workspace, size_t workspace_bytes);
int pdm_augment_scene_count(void *stream, int B, int C, const float *raw, const int *counts, const float *db_points,
                            const long long *db_offsets, const float *db_boxes, int K, const int *accepted,
                            const int *num_accepted, const int *flip, const float *angle, const float *scale, unsigned ops,
                            const float *point_cloud_range, const float *extra_width, long long capacity, int *out_counts,
                            int *overflow, float *out_rows, void *workspace, size_t workspace_bytes);
int pdm_augment_scene_fill(void *stream, int B, int C, const float *raw, const int *counts, const float *db_points,
                           const long long *db_offsets, const float *db_boxes, int K, const int *accepted,
                           const int *num_accepted, const int *flip, const float *angle, const float *scale, unsigned ops,
                           const float *point_cloud_range, const float *extra_width, long long capacity, int *out_counts,
                           int *overflow, float *out_rows, void *workspace, size_t workspace_bytes);

/* ---- second-stage training: proposal targets and rcnn losses (csrc/roi_targets.hip) -------------
 * pdm_proposal_targets: ProposalTargetLayer.forward + RoIHeadTemplate.assign_targets of the reference
 * (roi_heads/target_assigner/proposal_target_layer.py:13-228, roi_head_template.py:104-134) for the whole batch: per
 * sample the trailing zero-sum ground-truth rows are dropped (no row left: one all-zero box), every RoI gets its best 3-D
 * IoU and the ground truth that gives it (by_class: among the ground truth of the RoI's own label only; ties to the
 * lowest index), the RoIs split into fg / hard bg / easy bg, S = ROI_PER_IMAGE of them are drawn (fg first, then hard bg,
 * then easy bg) and the targets of the drawn RoIs are formed.  rois (B, R, 7), roi_scores (B, R), roi_labels (B, R)
 * int64, gt_boxes (B, M, 8) [box7, class].  fg_per_image = int(round(FG_RATIO * S)) and hard_bg_ratio (a double, used
 * as int(n_bg * ratio)) come from the host; the four thresholds are the configuration's doubles, compared as fp32 (the
 * 'roi_iou' ramp divides by fp32(CLS_FG_THRESH - CLS_BG_THRESH), the difference formed in double).  score_type 0 ('cls'): cls_labels (B, S) int64 in {1, 0, -1 = ignore};
 * 1 ('roi_iou'): cls_labels (B, S) float.  state: 2 int32 [step, error flag]; the step is advanced by the call, the
 * flag is OR-ed with 1 when a sample has neither fg nor bg (NaN overlaps; its slots then hold RoI 0).  Outputs, all
 * written in full: out_rois (B, S, 7), out_labels (B, S) int64, out_scores (B, S), out_iou (B, S), out_gt_src (B, S, 8),
 * out_gt_canon (B, S, 8) the ground truth in the RoI's frame with the heading folded into [-pi/2, pi/2],
 * reg_valid_mask (B, S) int64, sampled_inds (B, S) and gt_assignment (B, S) int32.  Limits: R <= 1024, M <= 256
 * (PDM_E_TOOLARGE), B <= 65535.  The draws are build-defined functions of (seed, step, sample, purpose, slot) written
 * down in roi_targets.hip.  Two launches, no workspace, no atomics on floats: a captured graph replays the same bits.
 *
 * pdm_rcnn_loss: get_box_cls_layer_loss (BinaryCrossEntropy) + get_box_reg_layer_loss (smooth-l1 with
 * CORNER_LOSS_REGULARIZATION) of roi_head_template.py:136-218 and their gradients over n = B S rows.  rcnn_cls (n),
 * rcnn_reg (n, 7), rois (n, 7), gt_of_rois / gt_of_rois_src (n, 8), reg_valid_mask (n) int64, cls_labels (n) int64
 * (labels_float 0) or float (1); code_weights: 7 floats on the HOST.  dcls (n) = d L_cls / d rcnn_cls, dreg (n, 7) =
 * d L_reg / d rcnn_reg, dcorner (n, 7) = d L_corner / d rcnn_reg, every row written.  loss_cls, loss_reg, loss_corner, fg_count: one float each (four separate
 * buffers), the losses already multiplied by their weights; use_corner 0 leaves L_corner 0.  workspace >=
 * pdm_rcnn_loss_workspace_bytes(n).  n <= 262144.  Two launches, fixed-order sums: bit-reproducible. */
int pdm_proposal_targets(void *stream, int B, int R, int M, int S, const float *rois, const float *roi_scores,
                         const long long *roi_labels, const float *gt_boxes, int by_class, int fg_per_image,
                         double hard_bg_ratio, double reg_fg_thresh, double cls_fg_thresh, double cls_bg_thresh,
                         double cls_bg_thresh_lo, int score_type, unsigned seed, int *state, float *out_rois,
                         long long *out_labels, float *out_scores, float *out_iou, float *out_gt_src, float *out_gt_canon,
                         long long *reg_valid_mask, void *cls_labels, int *sampled_inds, int *gt_assignment);
size_t pdm_rcnn_loss_workspace_bytes(long long n);
int pdm_rcnn_loss(void *stream, long long n, const float *rcnn_cls, const float *rcnn_reg, const float *rois,
                  const float *gt_of_rois, const float *gt_of_rois_src, const long long *reg_valid_mask,
                  const void *cls_labels, int labels_float, const float *code_weights, float beta, float cls_weight,
                  float reg_weight, float corner_weight, int use_corner, float *dcls, float *dreg, float *dcorner,
                  float *loss_cls, float *loss_reg, float *loss_corner, float *fg_count, void *workspace, size_t workspace_bytes);

/* ---- KITTI object evaluation (csrc/kitti_eval.hip) ---------------------------------------------
 * From the padded detections of pdm_post_process to the counts behind KITTI's AP, restating
 * pcdet/datasets/kitti/kitti_dataset.py:277-330, pcdet/utils/box_utils.py:203-288, pcdet/utils/calibration_kitti.py:65-84 and
 * pcdet/datasets/kitti/kitti_object_eval_python/eval.py:30-275.  No atomics anywhere: two runs give the same bits.
 *
 * pdm_kitti_boxes_to_camera: boxes (B, P, 7) lidar, count (B) live slots per sample, V2C (B, 3, 4), R0 (B, 3, 3), P2 (B, 3, 4),
 * image_shape (B, 2) int32 [height, width] or NULL (no clip) -> cam (B, P, 7) [x, y, z, l, h, w, ry], img (B, P, 4)
 * [x1, y1, x2, y2], alpha (B, P); slots at or past count are zeroed.
 *
 * The evaluator works on F ragged frames: gt_off, dt_off (F + 1) box ranges, ov_off (F + 1) the start of each frame's
 * (detections x ground truths) overlap block, NP = ov_off[F] pairs.  Boxes are doubles: bbox (n, 4), cam (n, 7).  A
 * combination is (metric, class, difficulty, overlap set) with index ((mi nC + c) nD + d) K + k; metrics[nM], classes[nC] and
 * difficulties[nD] are HOST arrays; class ids are 0 Car, 1 Pedestrian, 2 Cyclist, 3 Van, 4 Person_sitting, 5 Truck,
 * 6 DontCare, 7 anything else.  Flags (ign_gt (nC nD, NG), ign_dt (nC nD, ND)) are clean_data's 0 / 1 / -1 as bytes.
 *   overlaps (nM, NP): metric 0 image_box_overlap in fp64; 1 rotated BEV IoU on fp32 casts; 2 fp32 rotated intersection
 *     area, height overlap and union volume in fp64.
 *   pass1 (compute_fp = False): the scores of the true positives of (mi, k, c, d, frame f) go to
 *     slab[(mi K + k) SV + slot_off[(c nD + d)(F + 1) + f] ...], at most slot_off[.. f + 1] - slot_off[.. f] of them (the
 *     frame's valid ground truths), the rest of the slot range is filled with NaN.
 *   pass2 (compute_fp = True): thresholds (combinations, 41) fp64 with num_thresholds (combinations) ->
 *     sums (combinations, 41, 4) int64 = [tp, fp, fn, bits of the fp64 similarity sum] over all frames; workspace >=
 *     pdm_kitti_eval_workspace_bytes(F, combinations).
 * Limits: 4096 detections per frame, 1024 combinations, 8 classes. */
int pdm_kitti_boxes_to_camera(void *stream, int B, int P, const float *boxes, const int *count, const float *V2C,
                              const float *R0, const float *P2, const int *image_shape, float *cam, float *img, float *alpha);
int pdm_kitti_eval_overlaps(void *stream, int F, const int *gt_off, const int *dt_off, const int *ov_off, long long NP, int nM,
                            const int *metrics, const double *gt_bbox, const double *dt_bbox, const double *gt_cam,
                            const double *dt_cam, double *overlaps);
int pdm_kitti_eval_dt_flags(void *stream, long long ND, const double *dt_bbox, const int *dt_name, int nC, const int *classes,
                            int nD, const int *difficulties, signed char *ign_dt);
size_t pdm_kitti_eval_workspace_bytes(int F, int combinations);
int pdm_kitti_eval_pass1(void *stream, int F, const int *gt_off, const int *dt_off, const int *ov_off, int max_dt, int nM,
                         const int *metrics, int nC, int nD, int K, const double *overlaps, long long NP,
                         const signed char *ign_gt, long long NG, const signed char *ign_dt, long long ND,
                         const double *dt_score, const double *min_overlap, const int *slot_off, long long SV, double *slab);
int pdm_kitti_eval_pass2(void *stream, int F, const int *gt_off, const int *dt_off, const int *ov_off, int max_dt, int nM,
                         const int *metrics, int nC, int nD, int K, const double *overlaps, long long NP,
                         const signed char *ign_gt, long long NG, const signed char *ign_dt, long long ND,
                         const double *dt_score, const double *gt_alpha, const double *dt_alpha, const double *gt_bbox,
                         const double *dt_bbox, const int *gt_name, const double *min_overlap, const double *thresholds,
                         const int *num_thresholds, int compute_aos, void *workspace, size_t workspace_bytes, long long *sums);

/* ---- KITTI dataset front end (csrc/kitti_data.hip) ----------------------------------------
 * The per-point work of the reference's KittiDataset.get_infos / create_groundtruth_database / __getitem__
 * (pcdet/datasets/kitti/kitti_dataset.py:124-139, :150-275, :371-428) for B ragged frames at once.  Frames are packed as
 * the augmentor takes them: raw (total_rows, C) fp32 rows, counts (B) int32 on the device, frame b starting at the sum of
 * the earlier counts (nothing at or past total_rows is read); calibration V2C (B, 3, 4), R0 (B, 3, 3), P2 (B, 3, 4) fp32 and
 * image_shape (B, 2) int32 [height, width] per frame.  Limits: B <= 1024, M <= 256 boxes per frame, 3 <= C <= 16 (rows of
 * C = 4 floats must be 16 B aligned).  No atomics and no memset: two runs give the same bits.
 *
 * FOV crop (get_fov_flag o rect_to_img o lidar_to_rect, calibration_kitti.py:65-84, in double from the fp32 inputs in the
 * operation order written in kitti_data.hip): fov_count writes out_counts (B) = kept rows per frame, overflow (1) = the
 * total exceeds `capacity`, and, when flags != NULL, flags (total_rows) uint8 = 1 for a kept row; fov_fill writes the kept
 * rows, frame after frame in input order, never at or past `capacity` rows.  workspace >= pdm_kitti_data_fov_workspace_bytes(B),
 * shared by the two calls on one stream.
 *
 * Box membership: boxes (B, M, 7) fp32 lidar boxes, box_count (B) live boxes per frame.  boxes_count writes, per
 * (frame, box), num_points_in_gt (B, M) = points inside the FOV and inside the exact oriented box (box_utils.in_hull's
 * rule, in double) and db_count (B, M) = all points under points_in_boxes_cpu's rule (roiaware_pool3d.cpp:121-140, margin
 * 1e-2: the very test of the augmentation's point removal), both 0 at or past box_count; totals (2) int64 = [database
 * points P, database entries N = sum of box_count].  boxes_fill writes GTDatabase's layout: out_points (P, C) with xyz
 * relative to `centres` (B, M, 3) float64 (fp32(double(x) - centre), the other columns unchanged), in point order within
 * an entry; out_offsets (capacity_entries + 1) int64; out_boxes (N, 7).  Entries are ordered frame after frame, box after
 * box; a point inside two boxes goes to both.  Nothing is written at or past capacity_points rows / capacity_entries
 * entries.  workspace >= pdm_kitti_data_boxes_workspace_bytes(B, M), shared by boxes_count -> boxes_fill on one stream. */
/* align: raw, out_rows, out_points 16 B when C == 4 (rows read / written as float4), any otherwise. */
size_t pdm_kitti_data_fov_workspace_bytes(int B);
size_t pdm_kitti_data_boxes_workspace_bytes(int B, int M);
int pdm_kitti_data_fov_count(void *stream, int B, int C, long long total_rows, const float *raw, const int *counts,
                             const float *V2C, const float *R0, const float *P2, const int *image_shape, long long capacity,
                             int *out_counts, int *overflow, unsigned char *flags, void *workspace, size_t workspace_bytes);
int pdm_kitti_data_fov_fill(void *stream, int B, int C, long long total_rows, const float *raw, const int *counts,
                            const float *V2C, const float *R0, const float *P2, const int *image_shape, long long capacity,
                            int *out_counts, int *overflow, float *out_rows, void *workspace, size_t workspace_bytes);
int pdm_kitti_data_boxes_count(void *stream, int B, int C, long long total_rows, const float *raw, const int *counts,
                               const float *V2C, const float *R0, const float *P2, const int *image_shape, int M,
                               const float *boxes, const int *box_count, int *num_points_in_gt, int *db_count,
                               long long *totals, void *workspace, size_t workspace_bytes);
int pdm_kitti_data_boxes_fill(void *stream, int B, int C, long long total_rows, const float *raw, const int *counts,
                              const float *V2C, const float *R0, const float *P2, const int *image_shape, int M,
                              const float *boxes, const int *box_count, const double *centres, int *num_points_in_gt,
                              int *db_count, long long *totals, long long capacity_points, long long capacity_entries,
                              float *out_points, long long *out_offsets, float *out_boxes, void *workspace,
                              size_t workspace_bytes);

/* ---- rows form of the FP module's input for the training path (csrc/interpolate.hip) --------------------------------
 * out (B, n, ld) bf16 = [ three_interpolate(known, idx, weight) (C2) | skip (C1) | zeros ]: the reference's
 * cat([interpolated, unknow_feats], dim=1) (pointnet2_modules.py:158-165) written once as the rows the bf16 layers read, each
 * element the fp32 value (pinned fma order of pdm_three_interpolate) rounded to nearest even.  known (B, m, C2) and skip
 * (B, n, C1) are point-major rows, fp32 or bf16.  Backward: dx (B, n, ld) bf16 -> dknown (B, m, C2) fp32 through an inverted
 * (CSR) index, no atomics; the skip gradient is dx[..., C2 : C2 + C1].  workspace: pdm_three_interpolate_grad_ws_bytes(b, n, m). */
/* align: any (eight channels per thread need c2 % 8 == 0, ld % 8 == 0 and aligned known / out — dx / dknown in the backward —,
 * the element form otherwise: the forward gives the same bits; the backward's sums are added in the order of lists whose entry
 * order is not fixed between launches, so its last bits may differ from call to call in either form). */
int pdm_interp_concat_rows(void *stream, int b, int n, int m, int c2, int c1, int ld, const void *known, int known_bf16,
                           const void *skip, int skip_bf16, const int *idx, const float *weight, void *out);
int pdm_interp_concat_rows_grad(void *stream, int b, int n, int m, int c2, int ld, const void *dx, const int *idx,
                                const float *weight, float *dknown, void *workspace, size_t workspace_bytes);
/* the same, the gradient of the known rows written as fp32 (out_bf16 = 0) or bf16 (1: the rounding a cast of the fp32 result would do) */
int pdm_interp_concat_rows_grad_out(void *stream, int b, int n, int m, int c2, int ld, const void *dx, const int *idx,
                                    const float *weight, void *dknown, int out_bf16, void *workspace, size_t workspace_bytes);

/* ---- bf16 contractions of the training path (csrc/train_gemm.hip) ---------------------------------------------------
 * The shared MLPs' 1x1 convolutions / Linear layers in TRAINING (reference: torch Conv2d / Linear inside
 * pcdet/ops/pointnet2/pointnet2_batch/pointnet2_modules.py:91-97 and models/dense_heads/point_head_template.py:35-48)
 * over channels-last rows: bf16 operands, fp32 accumulation on v_mfma_f32_32x32x16_bf16, ONE rounding of the result.
 * All strides in elements and multiples of 8, K and N multiples of 8, pointers 16-byte aligned. */
/* Y (R, N) bf16 = X (R, K) . W (N, K)^T [+ bias (N) fp32, rounded to bf16 first].  stats: null, or
 * (pdm_tg_stats_parts(R, N), N, 2) fp32 = per persistent slot the column sums of y and y^2 of the ROUNDED outputs (BatchNorm
 * statistics without another pass over Y; pdm_bn_relu_forward_stats folds the parts).  The data gradient is the same call on
 * the transposed weights. */
/* align (every pdm_tg_* contraction): 16 B for X, W, Y, dZ, Yp, dX, dYout, dY, Bx, xmax, xmin, coef, grads, bcoef, the x_bn_coef and
 * workspace of pdm_tg_wgrad; 8 B for imax, imin; bias, stats, bstats, dW, out, scratch and the pack_weight buffers any. */
int pdm_tg_stats_parts(long long rows, int N);
/* x_bn_coef: null, or (4, K) fp32 [mean | invstd | gamma invstd | beta] from pdm_bn_finalize_stats: X holds the PRE-BatchNorm
 * outputs of the layer before and is read through bf16(relu((x - mean) scale + beta)) — that layer's BatchNorm + ReLU without
 * a pass (or a tensor) of its own; bit for bit what pdm_bn_relu_forward would have written. */
int pdm_tg_gemm_nt(void *stream, long long R, int K, int N, const void *X, long long ldx, const void *W, long long ldw,
                   void *Y, long long ldy, const float *bias, float *stats, const float *x_bn_coef);
/* Data gradient straight behind a BatchNorm + ReLU backward (the autograd rule of torch.nn.BatchNorm1d/2d + ReLU in
 * pointnet2_modules.py:91-97's stacks, fused into the contraction that consumes it): dX (R, N) = dY (R, K) . W (N, K)^T with
 * dY = scale (dZ [bn(Yp) > 0] - p - (Yp - mean) q) formed from dZ and Yp (R, K) while the operand is staged, and written to
 * dYout (R, K) on the way for the layer's weight gradient.  coef (4, K) from pdm_bn_finalize_stats, grads (4, K) from
 * pdm_bn_relu_backward_stats.  dYout is bit for bit pdm_bn_relu_backward's dx. */
int pdm_tg_gemm_nt_dy(void *stream, long long R, int K, int N, const void *dZ, long long lddz, const void *Yp, long long ldyp,
                      const void *W, long long ldw, void *dX, long long lddx, void *dYout, long long lddy, const float *coef,
                      const float *grads);
/* The two products above when their result IS the gradient of relu(bn(Bx)) — the data gradient of the layer that follows a
 * BatchNorm + ReLU in a stack (pointnet2_modules.py:91-97, point_head_template.py:35-48): the epilogue also leaves the statistics
 * that BatchNorm's backward needs, per slot and column the sums of g = y [bn(Bx) > 0] and of g (Bx - mean) invstd over the ROUNDED
 * outputs, in bstats (parts, N, 2) fp32 with parts = pdm_tg_stats_parts(R, N) / pdm_tg_dy_stats_parts(R, N) — the reduce pass of
 * pdm_bn_relu_backward_stats (a second read of Y and Bx) disappears; pdm_bn_finalize_bwd_stats folds the parts.
 * Bx (R, N) bf16 = that BatchNorm's input, bcoef (4, N) = its coefficients from pdm_bn_finalize_stats. */
int pdm_tg_gemm_nt_bs(void *stream, long long R, int K, int N, const void *X, long long ldx, const void *W, long long ldw,
                      void *Y, long long ldy, const void *Bx, long long ldbx, const float *bcoef, float *bstats);
/* pdm_tg_gemm_nt for the last layer of an SA scale (pointnet2_modules.py:46-52: ... -> BatchNorm -> ReLU -> max over nsample): rows
 * g ns .. g ns + ns - 1 are group g; the epilogue also leaves every group's per-channel max / min of the rounded outputs and the first
 * index attaining them (xmax, xmin (R / ns, N) bf16; imax, imin (R / ns, N) bytes) — pdm_bn_relu_pool_forward's statistics pass
 * without its read of Y; pdm_bn_relu_pool_forward_kept finishes the operator.  ns a power of two, 4 .. 128, dividing R. */
int pdm_tg_gemm_nt_pool(void *stream, long long R, int K, int N, const void *X, long long ldx, const void *W, long long ldw,
                        void *Y, long long ldy, const float *bias, float *stats, const float *x_bn_coef, int ns, void *xmax,
                        void *xmin, unsigned char *imax, unsigned char *imin);
int pdm_tg_dy_stats_parts(long long rows, int N);
int pdm_tg_gemm_nt_dy_bs(void *stream, long long R, int K, int N, const void *dZ, long long lddz, const void *Yp, long long ldyp,
                         const void *W, long long ldw, void *dX, long long lddx, void *dYout, long long lddy, const float *coef,
                         const float *grads, const void *Bx, long long ldbx, const float *bcoef, float *bstats);
size_t pdm_tg_wgrad_ws_bytes(long long R, int K, int N);
/* dW (N, K) fp32 (+)= dY (R, N)^T . X (R, K): row slabs summed in a fixed order (bit-reproducible) */
int pdm_tg_wgrad(void *stream, long long R, int K, int N, const void *dY, long long ldy, const void *X, long long ldx, float *dW,
                 int accumulate, void *workspace, size_t workspace_bytes, const float *x_bn_coef);
/* out (N) fp32 = column sums of Y (R, N) bf16 — the bias gradient; N a multiple of 8, <= 512; fixed summation order */
size_t pdm_tg_colsum_ws_floats(long long R, int N);
int pdm_tg_colsum(void *stream, long long R, int N, const void *Y, long long ld, float *out, float *scratch);
/* W (N, K) fp32 -> bf16 Wb (N, ldb) and / or its transpose Wt (K, ldt); either may be null; pad columns zero */
int pdm_tg_pack_weight(void *stream, int N, int K, const float *W, void *Wb, int ldb, void *Wt, int ldt);
/* the pair a layer needs, every element written: Wb (rows_to, cols_to) = W zero padded, Wt (cols_to, rows_to) = its transpose */
int pdm_tg_pack_weight_pair(void *stream, int N, int K, const float *W, void *Wb, void *Wt, int rows_to, int cols_to);
/* the same for many layers in one launch.  jobs: njobs records of 48 bytes in DEVICE memory,
 * { const float *W; void *Wb; void *Wt; int N, K, rows_to, cols_to; long long first_block; } with first_block[0] = 0,
 * first_block[j + 1] = first_block[j] + ceil(rows_to[j] * cols_to[j] / 256); total_blocks = their sum */
int pdm_tg_pack_weight_many(void *stream, int njobs, const void *jobs, long long total_blocks);


/* ---- diagnostics (process-global tuning switches used by tools/diag/ A/B measurements; every setting gives
 * identical results; each returns the previous value; not for production callers) ------------------------- */
int pdm_tune_fps_variant(int v);        /* 8192 < n <= 16384: 0 pruned 1024x16 (default), 3 pruned 512x32, 1 / 2 unpruned */
int pdm_tune_fused_waves(int w);        /* channel-split waves per workgroup: 0 heuristic, 1/2/4/8 */
int pdm_tune_fused_tiles(int t);        /* 16-position tiles per group: 0 heuristic, 1, 2 */
int pdm_tune_fused_groups(int n);       /* position groups per workgroup: 0 heuristic, 1/2/4/8 */
int pdm_tune_fused_wg_per_cu(int n);    /* grid cap = 256 CUs x n workgroups */
int pdm_tune_fused_lds_cap(int bytes);  /* LDS a two-tile workgroup may take (<= 160 KB) */
int pdm_tune_fused_reg(int on);         /* register-resident SA form for small scales */
int pdm_tune_fused_gemm(int on);        /* LDS-tiled GEMM for single-layer rows / two-layer FP with tiny skip */
int pdm_tune_fused_chain(int on);       /* register-resident chain kernels (rows_chain.hip) for many-row MLPs and FP modules 1-2 */
int pdm_tune_fused_swz(int on);         /* XOR-swizzled LDS tiles in the general chain kernels */
int pdm_tune_bq_quad(int form);         /* grid ball query: 1 four centres per wave (default), 2 one centre per lane, 3 per cloud by density (lane form for sparse, quad form for dense clouds), 0 one wave per centre; same indices */
int pdm_tune_bq_dense_ppc(int hundredths); /* form 3: points per occupied grid cell (x 100) from which a cloud counts as dense (default 300) */
int pdm_tune_grid_split(int min_n);     /* search-grid build: clouds of >= min_n points scatter from many workgroups (default 0 = never: measured slower) */
int pdm_tune_bq_small_waves(int w);     /* exhaustive ball query with <= 32768 centres in the call: waves per workgroup, 4 or 16 (default) */
int pdm_tune_bq_cpw(int centres);       /* lane form: centres per wave, 16 (default) / 32 / 64 */
int pdm_tune_bq_heavy(int candidates);  /* lane form: centres with more candidates than this take the whole-wave path (default 96) */
int pdm_tune_group_lds_floor(int bytes); /* LDS-staged group_points: request at least this much LDS per workgroup (caps the workgroups per CU so that kernels of other streams find wave slots beside a streaming gather); 0 = what the rows need */
int pdm_tune_group_rows(int packed);    /* group_points LDS form: 0 heuristics; variant (1 rows kernel, 2 round-2 kernel, 3 rows kernel in plain unit order) | rows per workgroup << 4 | parts of L << 8 | threads / 256 << 16 | index quads per lane and pass << 20 */
int pdm_tune_rows_chain_wg_per_cu(int n); /* grid cap of the many-row chain kernels = 256 CUs x n workgroups (default 12; 2 resident) */
int pdm_tune_fp_head_tiles(int n);           /* pdm_fp_head_fused: consecutive 64-row tiles per workgroup (default 2) */
int pdm_tune_rows_chain_dw_wg_per_cu(int n); /* the same for pdm_bev_head_fused (default 2: every workgroup resident from the start) */
int pdm_tune_rows_chain_xcd(int on);   /* heat-map chain kernel: contiguous patch range per XCD (default) / launch order */
int pdm_tune_bev_head_form(int form);  /* pdm_bev_head_fused: 0 every wave runs prologue and chain, 1 depthwise producer waves beside MFMA consumer waves (128 -> 64 -> 64 -> <= 16 only; other shapes take form 0) */
int pdm_tune_fp_chain_pad_lds(int bytes); /* diagnostic: extra LDS per workgroup of the FP chain kernel (occupancy experiments) */
int pdm_tune_fp_chain_nt(int on);      /* FP chain kernel: non-temporal output stores (default off) */
int pdm_tune_fp_chain_mask(int m);     /* which FP shapes take the register-resident chain kernel: bits 0-1 (default 2); m < 0 only reads */
int pdm_tune_group_nt(int on);         /* non-temporal stores of the grouped outputs (default on) */
int pdm_tune_copy_variant(int v);      /* pdm_copy_many: -1 by size (default); bit 0 non-temporal stores, bit 1 eight loads in flight per lane, bit 2 non-temporal loads */
int pdm_tune_copy_max_wg(int n);       /* pdm_copy_many: grid cap in workgroups per buffer (default 8192) */

/* count device-to-device copies dst[k] <- src[k] (bytes[k] each; host arrays) in one launch per 48 buffers.
 * Plumbing for the stream pipeline's hand-over buffers, not a reference operator. */
/* align: any, per transfer (16-byte pieces only when source and destination are both 16-byte aligned, then a byte tail). */
int pdm_copy_many(void *stream, int count, void *const *dst, const void *const *src, const size_t *bytes);
/* The same with device-side lengths: where dyn_count[k] != NULL only the first *dyn_count[k] * dyn_unit[k] bytes of buffer
 * k are copied (the count is read when the kernel runs): worst-case-sized buffers with a device-computed number of
 * live rows, e.g. the row lists of pdm_sa_pack (count = &meta[6], unit = 8). */
int pdm_copy_many_dyn(void *stream, int count, void *const *dst, const void *const *src, const size_t *bytes,
                      const int *const *dyn_count, const unsigned *dyn_unit);

/* ---- PDM neck (build-defined spec, DESIGN.md "PDM spec"; no reference source exists) ------- */

/* Multi-centre scatter-add of dilated, SH x Gaussian weighted point features into a BEV grid.
 * xyz (B,P,3), feat (B,P,C), sh (B,P,(degree+1)^2), inv2s2 (B,P); origin/cell/inv_cell are
 * 3 floats each passed by value; grid dims W (x), H (y), D (z); dilation kx,ky,kz odd.
 * layout 1: grid is (B,H,W,C*D) (channels-last storage of the logical (B,C*D,H,W) tensor,
 * inner index c*D+z); layout 0: (B,C*D,H,W) contiguous.  wsum (B,H,W,D).  Both caller-zeroed. */
int pdm_scatter_bev(void *stream, int B, int P, int C, int degree, const float *xyz,
                    const float *feat, const float *sh, const float *inv2s2, float ox, float oy,
                    float oz, float cx, float cy, float cz, float icx, float icy, float icz, int W,
                    int H, int D, int kx, int ky, int kz, int layout, float *grid, float *wsum);

/* grid[cell] /= wsum[cell] where |wsum| > eps */
/* align: any (the float4 form needs layout 1, C * D % 4 == 0 and an aligned grid). */
int pdm_bev_normalize(void *stream, int B, int C, int W, int H, int D, int layout, float eps,
                      float *grid, const float *wsum);

/* Gather form of pdm_scatter_bev (+ pdm_bev_normalize when normalize != 0) for layout 1: every cell of
 * grid (B,H,W,C*D) and wsum (B,H,W,D) is WRITTEN (no zero-fill by the caller), without atomics and in a fixed
 * summation order (ascending point index), so the result is bitwise reproducible.  workspace >=
 * pdm_gather_bev_workspace_bytes(...) bytes. */
size_t pdm_gather_bev_workspace_bytes(int B, int P, int W, int H, int kx, int ky);
/* align: any (features are staged 16 bytes at a time when C % 4 == 0 and feat is aligned). */
int pdm_gather_bev(void *stream, int B, int P, int C, int degree, const float *xyz, const float *feat,
                   const float *sh, const float *inv2s2, float ox, float oy, float oz, float cx, float cy,
                   float cz, float icx, float icy, float icz, int W, int H, int D, int kx, int ky, int kz,
                   int normalize, float eps, float *grid, float *wsum, void *workspace, size_t workspace_bytes);

/* Backward of pdm_bev_normalize for layout 1 (channels-last): y = the normalised grid, dy its gradient ->
 * dx (B,H,W,C*D) and dwsum (B,H,W,D), both fully written.  dx may be NULL (dwsum only: pdm_scatter_bev_grad_normalized
 * applies the division on its own reads of dy). */
/* align: any (the float4 form needs D == 1, C % 4 == 0 and aligned y, dy, dx). */
int pdm_bev_normalize_grad(void *stream, int B, int C, int W, int H, int D, float eps, const float *y,
                           const float *wsum, const float *dy, float *dx, float *dwsum);

/* backward of pdm_scatter_bev w.r.t. feat, sh, inv2s2 (outputs fully written, no zero-fill needed);
 * dwsum may be NULL. */
/* align: any (channel pairs — 8-byte accesses — need layout 1, D == 1, an even C and 8-byte aligned feat, dgrid / dy, dfeat). */
int pdm_scatter_bev_grad(void *stream, int B, int P, int C, int degree, const float *xyz,
                         const float *feat, const float *sh, const float *inv2s2, float ox,
                         float oy, float oz, float cx, float cy, float cz, float icx, float icy,
                         float icz, int W, int H, int D, int kx, int ky, int kz, int layout,
                         const float *dgrid, const float *dwsum, float *dfeat, float *dsh,
                         float *dinv2s2);
/* The same for the NORMALISED map y = grid / wsum (where |wsum| > eps): dy = dL/dy as it arrives, wsum (B,H,W,D) as the
 * forward left it, dwsum = pdm_bev_normalize_grad's second output (required).  No dL/dgrid tensor is formed. */
int pdm_scatter_bev_grad_normalized(void *stream, int B, int P, int C, int degree, const float *xyz,
                                    const float *feat, const float *sh, const float *inv2s2, float ox,
                                    float oy, float oz, float cx, float cy, float cz, float icx, float icy,
                                    float icz, int W, int H, int D, int kx, int ky, int kz, int layout,
                                    const float *dy, const float *wsum, float eps, const float *dwsum,
                                    float *dfeat, float *dsh, float *dinv2s2);

/* SURVEY.md section 8(f) row N4 -- score-ranked (instance-aware) sampling instead of FPS.  The sampling code of the
 * PDM-SSD / IA-SSD lineage is absent from the reference snapshot; its analog there is torch.topk over per-point scores.
 * Build-defined total order: score descending on the order-preserving integer image of the float (-0.0 < +0.0, NaN of
 * either sign ranks above +inf as in torch.topk), equal images by lower index.
 * scores (B,n) f32 -> idx (B,k) int32, idx[b,r] = index of the r-th ranked point; k <= n, k <= 16384. */
int pdm_topk_sampling(void *stream, int b, int n, int k, const float *scores, int *idx);

/* The pillar front end (csrc/pillar.hip, DESIGN.md "Pillar path"): dynamic pillars without a host loop, float atomics or a
 * sort.  Every result is a function of the input alone, bit for bit.  int32 indices throughout: B * nx * ny and N * C1 must
 * fit int32 (PDM_E_TOOLARGE), nz must be 1 (PDM_E_BADARG).
 *
 * pdm_pillar_assign: points (N, C1) fp32 rows (batch_idx, x, y, z, ...), any row order.  cell = floor((x - x0) / vx) in fp32
 *   with an IEEE division; a row is kept iff 0 <= cx < nx, 0 <= cy < ny and 0 <= batch_idx < B (z is not tested).  Pillars
 *   are the occupied cells in ascending b * nx * ny + cx * ny + cy.  Outputs are sized at capacity (cap = min(N, B nx ny)) and
 *   written up to N' kept rows / P pillars: kept_idx (N) kept rows in input order, unq_inv (N) their pillar, voxel_coords
 *   (cap, 4) = (b, 0, cy, cx), pillar_count (cap), pillar_mean (cap, 3) = float(double(sum of llrint(x * 2^20)) * 2^-20 /
 *   count), cell_table (B nx ny) pillar id or -1 in key order (all written), seg_start (cap + 1) / seg_rows (N) the kept rows
 *   of every pillar (slot order unspecified), record (2) = {N', P}.  workspace >= pdm_pillar_assign_workspace_bytes, 8-byte
 *   aligned.  N = 0 is valid.
 * pdm_pillar_features: out (n_kept, F) = [points[:, 1:] | points[:, 4:], xyz - mean, xyz - cell centre, |xyz| if with_dist];
 *   the cell centre is float(cx) * vx + xoff, product and sum rounded separately; xoff = fp32(vx / 2 + x0 in double).
 * pdm_pillar_segment_max: x (n_kept, K) -> x_max (P, K), arg (P, K) the winning row, ties to the lower row;
 *   pdm_pillar_segment_max_grad: grad_x (n_kept, K) = grad_max at the winning rows, zero elsewhere, all written.
 * pdm_pillar_fused_pfn: features -> weight (K, F <= 16) -> * scale + shift -> ReLU -> max per pillar: out (P, K); the
 *   (n_kept, K) activations are never stored.
 * pdm_pillar_cell_table: the table from voxel_coords (P, 4).  pdm_pillar_scatter: features (P, C) -> canvas (B, C, ny, nx),
 *   every element written in one pass, B <= 65535; pdm_pillar_scatter_grad: grad_features (P, C) gathered from grad_canvas. */
/* align: any (4-byte accesses only). */
size_t pdm_pillar_assign_workspace_bytes(int N, int B, int nx, int ny);
int pdm_pillar_assign(void *stream, int N, int C1, const float *points, int B, int nx, int ny, int nz, float x0, float y0,
                      float vx, float vy, int *kept_idx, int *unq_inv, int *voxel_coords, int *pillar_count,
                      float *pillar_mean, int *cell_table, int *seg_start, int *seg_rows, int *record, void *workspace,
                      size_t workspace_bytes);
int pdm_pillar_features(void *stream, int n_kept, int C1, const float *points, const int *kept_idx, const int *unq_inv,
                        const int *voxel_coords, const float *pillar_mean, int abs_xyz, int with_dist, float vx, float vy,
                        float xoff, float yoff, float zoff, float *out);
int pdm_pillar_segment_max(void *stream, int P, int K, const float *x, const int *seg_start, const int *seg_rows, float *x_max,
                           int *arg);
int pdm_pillar_segment_max_grad(void *stream, int n_kept, int K, const float *grad_max, const int *arg, const int *unq_inv,
                                float *grad_x);
int pdm_pillar_fused_pfn(void *stream, int P, int K, int C1, const float *points, const int *kept_idx, const int *voxel_coords,
                         const float *pillar_mean, const int *seg_start, const int *seg_rows, int abs_xyz, int with_dist,
                         float vx, float vy, float xoff, float yoff, float zoff, const float *weight, const float *scale,
                         const float *shift, float *out);
int pdm_pillar_cell_table(void *stream, int P, const int *voxel_coords, int B, int nx, int ny, int nz, int *cell_table);
int pdm_pillar_scatter(void *stream, int P, int C, const float *pillar_features, const int *cell_table, int B, int nx, int ny,
                       int nz, float *canvas);
int pdm_pillar_scatter_grad(void *stream, int P, int C, const float *grad_canvas, const int *voxel_coords, int B, int nx, int ny,
                            int nz, float *grad_features);

/* Hard voxels (csrc/hard_voxel.hip, DESIGN.md "Hard voxels"): the reference's voxel generator and its MeanVFE / PillarVFE
 * without a host loop, a sort or a float atomic: every result is a function of the input alone, bit for bit.  A grid may hold
 * up to 2^35 cells (64-bit keys; PDM_E_TOOLARGE beyond, the size query returns 0); rows x columns must fit int32.
 *
 * pdm_hard_voxelize: points (N, C1) fp32 rows (batch_idx, x, y, z, ...); the rows of a sample contiguous, samples ascending.
 *   cell = floor((v - v0) / size) in fp32 with an IEEE division on x, y and z; a row is dropped when a cell is out of range (NaN
 *   drops, z is tested on a pillar grid too) or batch_idx is outside [0, B).  Per sample, cells are ranked by their first row;
 *   a cell whose rank is below max_voxels is voxel `rank` of the sample and keeps its T smallest rows in ascending order; the
 *   rows of the other cells are dropped.  Samples ascend in the output.  T = points per voxel, 1 <= T <=
 *   pdm_hard_voxel_max_points() = 128, max_voxels >= 1 (PDM_E_BADARG otherwise).  Outputs at capacity cap = min(N, B max_voxels,
 *   cells), only the first M voxels written: slot_rows (cap, T) input rows, -1 padding; voxel_coords (cap, 4) = (b, cz, cy, cx);
 *   voxel_num_points (cap); voxels (cap, T, C1 - 1) or null (not written): bit copies of the rows past batch_idx, every padding
 *   element zero.  record (2) = {M, unsorted}: unsorted = 1 when batch_idx[i] <= batch_idx[i + 1] fails for some i (a NaN
 *   fails); then M = 0 and no output is valid.  workspace >= pdm_hard_voxelize_workspace_bytes, 8-byte aligned.  N = 0 is valid.
 * pdm_hard_voxel_materialize: slot_rows (M, T) -> voxels (M, T, C1 - 1), every element written.
 * pdm_hard_voxel_mean: out (M, C1 - 1) = the fp32 sum of the voxel's slots in slot order / max(num, 1), one IEEE division.
 * pdm_hard_pillar_pfn: the reference's PillarVFE with one PFN layer in eval mode in one launch: columns [points[:, 1:] |
 *   points[:, 4:], xyz - fp32 mean of the kept slots, xyz - cell centre on x, y and z (float(cell) * voxel + offset, product and
 *   sum rounded separately), |xyz| if with_dist] -> weight (K, F <= 16) -> * scale + shift -> ReLU -> max over the slots; a
 *   voxel with fewer than T points also takes relu(shift[k]), its padding rows' value: out (M, K). */
/* align: any (4-byte accesses), except the workspace: 8 B (PDM_E_BADARG otherwise). */
int pdm_hard_voxel_max_points(void);
size_t pdm_hard_voxelize_workspace_bytes(int N, int B, int nx, int ny, int nz);
int pdm_hard_voxelize(void *stream, int N, int C1, const float *points, int B, int nx, int ny, int nz, float x0, float y0, float z0,
                      float vx, float vy, float vz, int T, int max_voxels, int *slot_rows, int *voxel_coords,
                      int *voxel_num_points, float *voxels, int *record, void *workspace, size_t workspace_bytes);
int pdm_hard_voxel_materialize(void *stream, int M, int T, int C1, const float *points, const int *slot_rows, float *voxels);
int pdm_hard_voxel_mean(void *stream, int M, int T, int C1, const float *points, const int *slot_rows, const int *voxel_num_points,
                        float *out);
int pdm_hard_pillar_pfn(void *stream, int M, int K, int T, int C1, const float *points, const int *slot_rows,
                        const int *voxel_num_points, const int *voxel_coords, int abs_xyz, int with_dist, float vx, float vy, float vz,
                        float xoff, float yoff, float zoff, const float *weight, const float *scale, const float *shift, float *out);

/* The anchor head (csrc/anchor_head.hip, DESIGN.md "Anchor head"): AxisAlignedTargetAssigner.assign_targets, the head's three
 * loss terms with their gradients, and generate_predicted_boxes, each for the whole batch on the caller's stream with no host
 * read and no float atomics on a result: two calls give the same bits.  Anchors are ordered y, x, slot (A = H W A_loc); a map
 * is (B, A_loc * width, H, W), channel = slot * width + column, fp32 or bf16 with any element strides.
 *
 * pdm_anchor_targets: anchors (A, 7) fp32; set_of_slot = HOST array of A_loc anchor sets; set_of_class = HOST array of
 *   num_class + 1 ints, [g] = the set of global class g (1-based) or -1; matched / unmatched = HOST arrays of num_sets
 *   thresholds; gt_boxes (B, M, cols >= 8) fp32, class last, NOT modified; M <= 1024 (PDM_E_TOOLARGE beyond).  A box takes part
 *   against the anchors of its class's set only; overlap = nearest-BEV IoU in fp32 (DESIGN.md gives the operation order).
 *   -> box_cls_labels (B, A) int32, box_reg_targets (B, A, 7), reg_weights (B, A), num_pos (B) int32 = #labels > 0, all written.
 *   workspace >= pdm_anchor_targets_workspace_bytes(B, M, num_sets), 8-byte aligned.
 * pdm_anchor_head_loss: maps = HOST array of 3 device pointers [cls (width num_class), box (7), dir (num_dir_bins <= 8) | NULL];
 *   bf16 = HOST array of 3 flags; strides = HOST array of 3 x 4 element strides (b, c, y, x); anchor_rot = HOST array of A_loc
 *   rotations; code_weights = HOST array of 7.  out[0..2] = cls / loc / dir term, each summed over the sample divided by
 *   max(num_pos, 1), then by B, times its weight; grad_cls / grad_box / grad_dir fp32 (B, channels, H, W) contiguous = d term / d
 *   map, every element written.  workspace >= pdm_anchor_head_loss_workspace_bytes(B, H, W), 8-byte aligned.
 * pdm_anchor_decode: maps = HOST array of 2 device pointers [box, dir | NULL], bf16 / strides alike -> batch_box_preds
 *   (B, A, 7) fp32: residual decode, arg-max direction bin (lower bin on equal logits), heading folded into the bin's period. */
/* align: any (two cells along W per access only where W is even, the strides allow it and the pointers are aligned; the
 * decode moves its staged pieces 16 bytes at a time only where the table and the output are 16-byte aligned). */
size_t pdm_anchor_targets_workspace_bytes(int B, int M, int num_sets);
int pdm_anchor_targets(void *stream, int B, int M, int cols, int A, int A_loc, int num_sets, int num_class, const float *anchors,
                       const int *set_of_slot, const int *set_of_class, const float *matched, const float *unmatched,
                       const float *gt_boxes, int norm_by_num_examples, int *box_cls_labels, float *box_reg_targets,
                       float *reg_weights, int *num_pos, void *workspace, size_t workspace_bytes);
size_t pdm_anchor_head_loss_workspace_bytes(int B, int H, int W);
int pdm_anchor_head_loss(void *stream, int B, int H, int W, int A_loc, int num_class, int num_dir_bins, const void *const *maps,
                         const int *bf16, const long long *strides, const int *labels, const float *targets, const int *num_pos,
                         const float *anchor_rot, const float *code_weights, float cls_weight, float loc_weight, float dir_weight,
                         float dir_offset, float beta, float alpha, float gamma, float *out, float *grad_cls, float *grad_box,
                         float *grad_dir, void *workspace, size_t workspace_bytes);
int pdm_anchor_decode(void *stream, int B, int H, int W, int A_loc, int num_dir_bins, const void *const *maps, const int *bf16,
                      const long long *strides, const float *anchors, float dir_offset, float dir_limit_offset,
                      float *batch_box_preds);

/* The voxel path (csrc/sparse_conv.hip, csrc/sparse_conv_mfma.hip, DESIGN.md "Voxel path"): dynamic voxels with means, the
 * rulebook of a sparse 3-D convolution, the convolution on the exact f32 MFMA, and the dense canvas.  No host loop, sort, hash
 * or float atomic: every result is a function of the input alone, bit for bit.  A cell's key is
 * ((b * nx + x) * ny + y) * nz + z as a 64-bit value; a grid may hold up to 2^35 cells (PDM_E_TOOLARGE beyond), row counts and
 * rows x offsets must fit int32.  Indices are int32 rows (b, z, y, x).
 *
 * pdm_voxel_assign: points (N, C1) fp32 rows (batch_idx, x, y, z, ...), any row order.  cell = floor((v - v0) / size) in fp32
 *   with an IEEE division on x, y and z; a row is kept iff all three cells are in range (NaN drops) and 0 <= batch_idx < B.
 *   Voxels are numbered in ascending key order.  Outputs at capacity cap = min(N, cells): kept_idx (N) kept rows in input
 *   order, unq_inv (N) their voxel, voxel_coords (cap, 4) = (b, cz, cy, cx), voxel_count (cap), voxel_mean (cap, C1 - 1) =
 *   float(double(sum of llrint(v * 2^20)) * 2^-20 / count) of every column, record (2) = {N', P}.  workspace >=
 *   pdm_voxel_assign_workspace_bytes, 8-byte aligned.  N = 0 is valid.
 * pdm_sparse_sites, then pdm_sparse_rulebook on the same workspace (>= pdm_sparse_rulebook_workspace_bytes, 8-byte aligned)
 *   and the same geometry: in_indices (P_in, 4) distinct sites in any row order on the grid (B, D, H, W); kernel, stride and
 *   padding per axis (z, y, x), at most 27 offsets.  subm: the output sites are the input rows, the neighbour at offset k is
 *   the row at coord + k - K / 2 (stride 1, padding unused).  Otherwise the output grid is (in + 2 p - k) / s + 1 per axis,
 *   site o exists iff an input lies at o s - p + k for some k, and sites ascend in the key of the output grid.
 *   pdm_sparse_sites writes record[0] = P_out (the caller's one host read for a strided convolution); pdm_sparse_rulebook
 *   writes out_indices (P_out, 4) (strided only; may be null for subm) and nbr (P_out, kvol), kx fastest: input row or -1.
 * pdm_sparse_conv: out (P_out, Cout) = epilogue(sum over k ascending of W[k] x[nbr[:, k]]); epilogue = * scale + shift (both or
 *   neither), + residual (P_out, Cout), ReLU, each optional, in this order.  Cin in {3..8, 16, 32, 64, 128}, Cout in {16, 32,
 *   64, 128} (PDM_E_BADARG otherwise).  wpack: pdm_sparse_conv_packed_floats floats, [k][kb][nb][lane][j] =
 *   W[k][cin = 16 kb + 4 (lane >> 4) + j][cout = 16 nb + (lane & 15)], zero past Cin.
 * pdm_sparse_to_dense: features (P, C), indices (P, 4) -> out (B, C, D, H, W), every element written by one launch behind a
 *   cell table built in the workspace (>= pdm_sparse_to_dense_workspace_bytes); B D H W must fit int32, B <= 65535. */
/* align: any (4-byte accesses, 16-byte ones only where the pointer allows), except wpack: 16 B (PDM_E_BADARG otherwise). */
size_t pdm_voxel_assign_workspace_bytes(int N, int C1, int B, int nx, int ny, int nz);
int pdm_voxel_assign(void *stream, int N, int C1, const float *points, int B, int nx, int ny, int nz, float x0, float y0, float z0,
                     float vx, float vy, float vz, int *kept_idx, int *unq_inv, int *voxel_coords, int *voxel_count,
                     float *voxel_mean, int *record, void *workspace, size_t workspace_bytes);
size_t pdm_sparse_rulebook_workspace_bytes(int P_in, int B, int D, int H, int W, int kd, int kh, int kw, int sd, int sh, int sw, int pd,
                                           int ph, int pw, int subm);
int pdm_sparse_sites(void *stream, int P_in, const int *in_indices, int B, int D, int H, int W, int kd, int kh, int kw, int sd, int sh,
                     int sw, int pd, int ph, int pw, int subm, int *record, void *workspace, size_t workspace_bytes);
int pdm_sparse_rulebook(void *stream, int P_in, const int *in_indices, int P_out, int B, int D, int H, int W, int kd, int kh, int kw,
                        int sd, int sh, int sw, int pd, int ph, int pw, int subm, int *out_indices, int *nbr, void *workspace,
                        size_t workspace_bytes);
size_t pdm_sparse_conv_packed_floats(int kvol, int Cin, int Cout);
int pdm_sparse_conv(void *stream, int P_out, int P_in, int kvol, int Cin, int Cout, const float *x, const int *nbr, const float *wpack,
                    const float *scale, const float *shift, const float *residual, int relu, float *out);
size_t pdm_sparse_to_dense_workspace_bytes(int B, int D, int H, int W);
int pdm_sparse_to_dense(void *stream, int P, int C, const float *features, const int *indices, int B, int D, int H, int W, float *out,
                        void *workspace, size_t workspace_bytes);

/* The gradients of pdm_sparse_conv (csrc/sparse_conv.hip, csrc/sparse_conv_wgrad.hip).  No float atomics: two
 * runs and a graph replay give the same bits.
 * pdm_sparse_rulebook_transpose: nbr (P_out, kvol) -> nbr_t (P_in, kvol), nbr_t[nbr[i][k]][k] = i and -1 elsewhere (at most one
 *   writer per entry); an entry of nbr outside [0, P_in) counts as -1.  The data gradient of a strided convolution is
 *   pdm_sparse_conv over nbr_t with the weights packed transposed; a submanifold convolution with odd kernels needs no table
 *   (nbr_t[j][k] == nbr[j][kvol - 1 - k]).
 * pdm_sparse_conv_split: pdm_sparse_conv with the same arguments and checks, adding every offset's products in an accumulator of
 *   their own and that to a running sum (the order of `per offset mm, then add`: about a third of the rounding error of one long
 *   chain).  The training path's forward and data gradient; as deterministic, but not the same bits as pdm_sparse_conv.
 * pdm_sparse_conv_wgrad: dy (P_out, Cout), x (P_in, Cin), nbr (P_out, kvol) -> dw (Cout, kvol, Cin) =
 *   sum over i of dy[i][co] x[nbr[i][k]][ci] on the exact f32 MFMA, every element written (zeros for P_out == 0).  Phase one
 *   writes one (Cout, Cin padded to 16) partial per (row chunk, offset) to `workspace` (>=
 *   pdm_sparse_conv_wgrad_workspace_bytes, 8-byte aligned, at most 64 MiB or one chunk's partials), phase two adds the chunks
 *   in ascending order.  A chunk holds pdm_sparse_conv_wgrad_chunk_rows rows, a function of (P_out, kvol, Cin, Cout) alone.
 *   Channel sets and kvol <= 27 as pdm_sparse_conv (PDM_E_BADARG otherwise; the two queries return 0). */
/* align: any (4-byte accesses, 16-byte ones only where the pointer allows), except the workspace: 8 B and wpack: 16 B
 * (PDM_E_BADARG otherwise). */
int pdm_sparse_rulebook_transpose(void *stream, int P_out, int P_in, int kvol, const int *nbr, int *nbr_t);
int pdm_sparse_conv_split(void *stream, int P_out, int P_in, int kvol, int Cin, int Cout, const float *x, const int *nbr, const float *wpack,
                          const float *scale, const float *shift, const float *residual, int relu, float *out);
int pdm_sparse_conv_wgrad_chunk_rows(int P_out, int kvol, int Cin, int Cout);
size_t pdm_sparse_conv_wgrad_workspace_bytes(int P_out, int kvol, int Cin, int Cout);
int pdm_sparse_conv_wgrad(void *stream, int P_out, int P_in, int kvol, int Cin, int Cout, const float *dy, const float *x,
                          const int *nbr, float *dw, void *workspace, size_t workspace_bytes);

/* The sparse convolution and its weight gradient up to 256 channels (csrc/sparse_conv_mfma.hip, csrc/sparse_conv_wgrad.hip,
 * DESIGN.md 7zb): what a sparse 2-D pillar backbone's 128 -> 256 and 256 -> 256 layers run.  Arguments, checks, epilogue,
 * alignment and determinism as the narrow counterparts; Cin in {3..8, 16, 32, 64, 128, 256}, Cout in {16, 32, 64, 128, 256}
 * (PDM_E_BADARG otherwise, before any launch).  The narrow entries keep refusing 256.
 * pdm_sparse_conv_wide, pdm_sparse_conv_wide_split: pdm_sparse_conv, pdm_sparse_conv_split.  wpack as there
 *   (pdm_sparse_conv_packed_floats covers 256).  One accumulator chain per output element over the present offsets k ascending
 *   and the 16-channel blocks kb ascending, whatever the blocking of the output columns: for Cin, Cout <= 128 the narrow
 *   entries' bits; columns [0, 128) and [128, 256) of a Cout = 256 run are the bits of two Cout = 128 runs on the weight's halves.
 *   The data gradient is pdm_sparse_conv_wide_split with the channels swapped, as in the narrow form.
 * pdm_sparse_conv_wide_wgrad: pdm_sparse_conv_wgrad.  A 256-wide side runs as two 128-wide sub-blocks, each on its columns of
 *   dy and x; every element of every (Cout, Cin padded to 16) partial has one writer, phase two adds the chunks in ascending
 *   order.  pdm_sparse_conv_wide_wgrad_chunk_rows and pdm_sparse_conv_wide_wgrad_workspace_bytes: the narrow rule over the wide
 *   channel sets, a function of (P_out, kvol, Cin, Cout) alone (0 for sizes the operator rejects); for Cin, Cout <= 128 the
 *   narrow entry's chunks and bits. */
/* align: any (4-byte accesses, 16-byte ones only where the pointer allows), except the workspace: 8 B and wpack: 16 B
 * (PDM_E_BADARG otherwise). */
int pdm_sparse_conv_wide(void *stream, int P_out, int P_in, int kvol, int Cin, int Cout, const float *x, const int *nbr, const float *wpack,
                         const float *scale, const float *shift, const float *residual, int relu, float *out);
int pdm_sparse_conv_wide_split(void *stream, int P_out, int P_in, int kvol, int Cin, int Cout, const float *x, const int *nbr,
                               const float *wpack, const float *scale, const float *shift, const float *residual, int relu, float *out);
int pdm_sparse_conv_wide_wgrad_chunk_rows(int P_out, int kvol, int Cin, int Cout);
size_t pdm_sparse_conv_wide_wgrad_workspace_bytes(int P_out, int kvol, int Cin, int Cout);
int pdm_sparse_conv_wide_wgrad(void *stream, int P_out, int P_in, int kvol, int Cin, int Cout, const float *dy, const float *x,
                               const int *nbr, float *dw, void *workspace, size_t workspace_bytes);

/* Voxel R-CNN's RoI-grid pooling (csrc/sparse_conv.hip, csrc/roi_grid_pool.hip).
 * pdm_sparse_index: indices (P, 4) int32 rows (b, z, y, x), distinct sites in any row order on the grid (B, D, H, W) -> the
 *   level's site index in `workspace` (>= pdm_sparse_index_workspace_bytes, 8-byte aligned): occupancy bitmap, group prefixes
 *   and row_of_rank, so that row_of_rank[rank(key)] is the row at a cell.  Six launches, no host read, graph-capturable.  Up to
 *   2^35 cells (PDM_E_TOOLARGE beyond; the size query returns 0).
 * pdm_roi_grid_pool: one launch per (level, scale).  rois (B, n, roi_stride >= 7) rows (x, y, z, dx, dy, dz, heading, ...); grid
 *   point g of RoI r (g = (ix G + iy) G + iz) is local = (i + 0.5) / G size - size / 2 turned by the heading plus the centre, its
 *   cell floor(floor((p - p0) / voxel) / stride) per axis, its sample r / n.  The window of (2 rz + 1)(2 ry + 1)(2 rx + 1) cells
 *   around it is walked z outermost, x innermost; a set cell whose centre (c + 0.5) (voxel stride) + p0 lies within `radius` of
 *   the grid point is a hit, the first nsample hits are the group.  pooled[c] = max over the group of
 *   relu(features_in[row][c] + fma(dot(wp[c], centre - p), scale_p[c], shift_p[c])), relu(shift_p[c]) for an empty group;
 *   out[r G^3 + g][out_offset + j] = relu(fma(dot(wout[j], pooled), scale_o[j], shift_o[j])) on the exact f32 MFMA, rows of
 *   out_stride floats.  site_index: what pdm_sparse_index left for the same P and grid.  features_in (P, C1); wp (C1, 3); wout:
 *   the (C2, C1) weight in pdm_sparse_conv's packed order with kvol = 1.  C1, C2 in {16, 32, 64}, G <= 8, rz, ry, rx <= 4,
 *   nsample <= 32 (PDM_E_BADARG otherwise).  No atomics: two runs give the same bits. */
/* align: any (4-byte accesses, 16-byte ones only where the pointer allows), except wout: 16 B and the workspaces: 8 B
 * (PDM_E_BADARG otherwise). */
size_t pdm_sparse_index_workspace_bytes(int P, int B, int D, int H, int W);
int pdm_sparse_index(void *stream, int P, const int *indices, int B, int D, int H, int W, void *workspace, size_t workspace_bytes);
int pdm_roi_grid_pool(void *stream, int B, int n, int roi_stride, const float *rois, int G, int D, int H, int W, int stride, float vx,
                      float vy, float vz, float x0, float y0, float z0, int P, const void *site_index, size_t site_index_bytes, int C1,
                      const float *features_in, const float *wp, const float *scale_p, const float *shift_p, int rz, int ry, int rx,
                      float radius, int nsample, int C2, const float *wout, const float *scale_o, const float *shift_o, float *out,
                      int out_stride, int out_offset);

/* The training form of the RoI-grid pooling (csrc/roi_grid_train.hip): a query that keeps the groups, a pooling
 * over the kept groups that records the winning slot, and the gradients.  M = B n G^3 <= 2^22 grid points (PDM_E_TOOLARGE
 * beyond; the size queries return 0), S = nsample <= 32, C1 in {16, 32, 64} (PDM_E_BADARG otherwise).  No float atomics, no
 * host read; the three entry points can be captured in a graph from the calling thread: two runs and a graph replay give the
 * same bits.
 * pdm_roi_grid_query: the geometry, window and site_index arguments and rules of pdm_roi_grid_pool, the same fp32 operation
 *   order.  grp_row (M, S) int32: the rows of the group in window order, -1 in unused slots; grp_off (M, S, 3) fp32: centre - p
 *   as (x, y, z), 0 in unused slots; moments (9) float64: [sum x, y, z, xx, xy, xz, yy, yz, zz] of the offsets over the M S slots
 *   of the reference's padded tensor (slot s < count once, slot 0 a further S - count times, an empty group S zero offsets).
 *   One partial per tile of 16 grid points in `workspace` (>= pdm_roi_grid_query_workspace_bytes), added in ascending order by
 *   one workgroup.  Two launches.
 * pdm_roi_grid_pool_train: pooled[m][c] = max over the group of relu(features_in[row][c] + fma(dot(wp[c], off), scale_p[c],
 *   shift_p[c])) with dot = fma(wz, dz, fma(wy, dy, wx dx)), relu(shift_p[c]) for an empty group (grp_row[m][0] == -1): the bits
 *   of pdm_roi_grid_pool's pooled value.  arg[m][c] uint8: the lowest slot that attains the maximum, 0xFF where pooled is 0, 0
 *   for an empty group with shift_p[c] > 0.  A slot whose value is NaN (non-finite inputs only) never wins the strict
 *   comparison: it is passed over, where torch's relu / max_pool would hand the NaN on.  One launch.
 * pdm_roi_grid_pool_grad: for every (m, c) with s = arg[m][c] != 0xFF and g = gpool[m][c]: dshift_p[c] += g, and unless the
 *   group is empty dfeatures_in[grp_row[m][s]][c] += g, dscale_p[c] += g dot, dwp[c][:] += g scale_p[c] grp_off[m][s][:].
 *   dfeatures_in is summed as llrint(g 2^k) in 64 bits with integer atomics, 2^k the power of two that puts max|gpool| (an
 *   integer maximum on the device) in [2^40, 2^41), and converted once; a non-finite gpool makes all of it NaN.  The parameter
 *   sums: one partial per pdm_roi_grid_pool_grad_chunk_points(M, C1) grid points, added in ascending order.  Every element of
 *   the four outputs is written.  Four launches behind one zero fill of `workspace`
 *   (>= pdm_roi_grid_pool_grad_workspace_bytes). */
/* align: any (4-byte accesses), except moments and the workspaces: 8 B (PDM_E_BADARG otherwise). */
size_t pdm_roi_grid_query_workspace_bytes(long long M);
int pdm_roi_grid_query(void *stream, int B, int n, int roi_stride, const float *rois, int G, int D, int H, int W, int stride, float vx,
                       float vy, float vz, float x0, float y0, float z0, int P, const void *site_index, size_t site_index_bytes, int rz,
                       int ry, int rx, float radius, int nsample, int *grp_row, float *grp_off, double *moments, void *workspace,
                       size_t workspace_bytes);
int pdm_roi_grid_pool_train(void *stream, long long M, int nsample, int P, int C1, const int *grp_row, const float *grp_off,
                            const float *features_in, const float *wp, const float *scale_p, const float *shift_p, float *pooled,
                            unsigned char *arg);
int pdm_roi_grid_pool_grad_chunk_points(long long M, int C1);
size_t pdm_roi_grid_pool_grad_workspace_bytes(long long M, int P, int C1);
int pdm_roi_grid_pool_grad(void *stream, long long M, int nsample, int P, int C1, const float *gpool, const unsigned char *arg,
                           const int *grp_row, const float *grp_off, const float *wp, const float *scale_p, float *dfeatures_in,
                           float *dwp, float *dscale_p, float *dshift_p, void *workspace, size_t workspace_bytes);

/* PV-RCNN's two operators (csrc/pv_rcnn.hip).  Both check every argument before any launch, use no atomics (two
 * runs give the same bits), read nothing on the host and can be captured in a graph.
 * pdm_bev_interpolate: keypoints (K, 4) fp32 rows (b, x, y, z) of all samples; spatial_features (B, C, H, W) fp32 contiguous, the
 *   map as HeightCompression leaves it.  x = ((kx - x0) / vx) / bev_stride and y likewise (IEEE divisions), corners
 *   clamp(floor, 0, n - 1) and clamp(floor + 1, 0, n - 1), weights from the CLAMPED corners,
 *   out[k][col0 + c] = Ia wa + Ib wb + Ic wc + Id wd summed left to right in fp32 without contraction (Ia = im[y0][x0],
 *   Ib = im[y1][x0], Ic = im[y0][x1], Id = im[y1][x1]): the bits of the reference's bilinear_interpolate_torch.  Rows of ld floats,
 *   columns [col0, col0 + C); a row whose b is outside [0, B) gets zeros.  One launch.
 * pdm_roi_keypoint_query: rois (B, n, roi_stride >= 7); grid point g of RoI r as pdm_roi_grid_pool forms it (the same code).
 *   xyz (K, 3): the keypoints of all samples stacked, xyz_batch_cnt (B) int32 on the device; max_per_sample: the caller's bound
 *   on those counts (it sizes the LDS the workgroup stages a sample in; a sample above it is cut to its first max_per_sample
 *   keypoints), at most pdm_roi_keypoint_query_cap() = 4096 (PDM_E_TOOLARGE beyond).  Per scale s < nscales (1 or 2), with
 *   pdm_stack_ball_query's rules (pinned squared distance, strict <, first nsample_s by index, padding with the first hit):
 *   idx_s (B n G^3, nsample_s) int32 GLOBAL rows of xyz, empty_s (B n G^3) bytes, 1 for a ball without a hit, whose slots all
 *   hold row 0 of the sample.  grid_points (B n G^3, 3).  G <= 8, nsample <= 64, B <= 1024, K >= 1 (PDM_E_BADARG
 *   otherwise: an empty ball needs a row to point at).  One launch for all scales. */
/* align: any (4-byte accesses). */
int pdm_bev_interpolate(void *stream, int K, const float *keypoints, int B, int C, int H, int W, const float *spatial_features,
                        float x0, float y0, float vx, float vy, int bev_stride, float *out, int ld, int col0);
int pdm_roi_keypoint_query_cap(void);
int pdm_roi_keypoint_query(void *stream, int B, int n, int roi_stride, const float *rois, int G, int K, const float *xyz,
                           const int *xyz_batch_cnt, int max_per_sample, int nscales, float radius0, int nsample0, float radius1,
                           int nsample1, float *grid_points, int *idx0, unsigned char *empty0, int *idx1, unsigned char *empty1);

/* PV-RCNN++'s proposal-centric partition (csrc/spc.hip): sample_points_with_roi and the front half of sector_fps of
 * the reference's voxel_set_abstraction.py, for the whole batch.  Every argument is checked before any launch; nothing is read on
 * the host; no atomic cursor (two runs and a graph replay give the same bits); five launches.
 *   xyz (N, 3) fp32, sample-major stacked rows; xyz_batch_cnt (B <= 1024) int32 on the device (rows past the counts' sum belong
 *   to no sample and are ignored); rois (B, n, roi_stride >= 7) fp32, 1 <= n <= pdm_spc_partition_max_rois() = 1024
 *   (PDM_E_TOOLARGE beyond); num_sectors S in [0, pdm_spc_partition_max_sectors() = 64]; num_keypoints K >= 1 when S > 0.
 * KEEP: a row is kept when d_min < fl(||dims / 2|| + radius), d = sqrt_rn(sqdist(p - centre)) (common.h's pinned squared
 *   distance), the rois of its sample walked in ascending index with a strict < (ties to the lower index), ||dims / 2|| =
 *   sqrt_rn(sqdist) of the halved dimensions of the roi that gave d_min.  All-zero roi rows are rois at the origin of size zero.
 *   mask (N) bytes, when not null: that verdict, 0 / 1, for every row of a sample.
 * FALLBACK (fallback != 0): a sample with points of which none is kept yields its first row alone (points[:1]); mask stays 0.
 *   A sample without points yields nothing: every count of it is 0.
 * SECTOR (S > 0): s = floor(fl(fl(atan2f(y, x) + PI_F) / SIZE_F)) clamped to [0, S], SIZE_F = (float)(2 pi / S), IEEE fp32
 *   division.  s = S is no sector: the row is dropped from the output but counted in kept_cnt.  S = 0: one segment a sample.
 * OUT: seg_xyz (N, 3) and seg_row (N) int32 source rows, written up to the sum of seg_cnt: sample-major, sector ascending, source
 *   order inside a sector.  seg_cnt (B max(S, 1)); kept_cnt (B) = the sample's kept rows N', dropped ones included;
 *   seg_take (B S; not written and may be null when S = 0) = min(c, ceil(c / N' * K)) evaluated in double in that order.
 * workspace: pdm_spc_partition_ws_bytes(N, B, num_sectors) bytes (0 for sizes the call refuses), contents irrelevant. */
/* align: xyz, rois, outputs any (4-byte and 1-byte accesses); workspace 8 B (checked). */
int pdm_spc_partition_max_rois(void);
int pdm_spc_partition_max_sectors(void);
size_t pdm_spc_partition_ws_bytes(int N, int B, int num_sectors);
int pdm_spc_partition(void *stream, int N, const float *xyz, int B, const int *xyz_batch_cnt, int n, int roi_stride, const float *rois,
                      float radius, int num_sectors, int num_keypoints, int fallback, float *seg_xyz, int *seg_row, int *seg_cnt,
                      int *seg_take, int *kept_cnt, unsigned char *mask, void *workspace, size_t workspace_bytes);

/* SECOND-IoU's RoI pooling (csrc/bev_roi_crop.hip).  Both check every argument before any launch, use no atomics (two
 * runs give the same bits), read nothing on the host and can be captured in a graph.  Neither has a gradient: the head detaches the
 * map and the rois in front of this step.
 * pdm_bev_roi_crop: rois (B, n, roi_stride >= 7) fp32 rows (x, y, z, dx, dy, dz, heading, ...); spatial_features_2d (B, C, H, W) fp32
 *   contiguous, as BaseBEVBackbone leaves it, read in place; (x0, y0) the range minima; cell_x, cell_y = VOXEL_SIZE * DOWNSAMPLE_RATIO
 *   (the double product rounded once to fp32); 2 <= G <= 8 (G = 1 has no corner-aligned lattice: PDM_E_BADARG).
 *   -> pooled (B n, C, G, G), rows of ld >= C G^2 floats, column c G^2 + i G + j: the reference's affine_grid + grid_sample
 *   (align_corners = True, zero padding) of the RoI's rotated rectangle.  Pixel position of cell (i, j), fp32, one rounding per
 *   operation, in this order:  cx = (x - x0) / cell_x; hx = (dx * 0.5) / cell_x; cy, hy likewise; (s, c) = sincosf(heading);
 *   u = (2 j - (G - 1)) / (G - 1); v = (2 i - (G - 1)) / (G - 1);
 *   px = (((hx c) u) - ((hx s) v)) + cx;  py = (((hy s) u) + ((hy c) v)) + cy
 *   (theta multiplied out: the (W - 1), (H - 1) terms cancel).  fx = px - floor(px), fy likewise;
 *   value = ((v00 ((1 - fx)(1 - fy)) + v01 (fx (1 - fy))) + v10 ((1 - fx) fy)) + v11 (fx fy), v00 = im[floor py][floor px], v01 its
 *   right, v10 its lower, v11 its lower right neighbour; a corner outside the map is 0 and is not read; a position outside
 *   (-1, W) x (-1, H), or NaN, gives exactly 0.  H, W in [2, 32768], C <= 65536.  One launch.
 * pdm_bev_roi_crop_fc: out (B n, Cout) = epilogue(crop(r) . W^T) without the (B n, C G^2) tensor; epilogue(v) = relu(v scale + shift)
 *   as one multiply and one add, scale / shift (Cout) both or neither.  wpack (pdm_bev_roi_crop_fc_packed_floats, 16-byte aligned):
 *   [kb][nb][lane][j] = W[16 nb + (lane & 15)][16 kb + 4 (lane >> 4) + j] of the Conv1d weight (Cout, C G^2).  The crop's values
 *   have pdm_bev_roi_crop's bits (the same device routine); the products go through mfma_f32_16x16x4f32 (an fp32 fma chain in
 *   ascending k) and the contraction K = C G^2 is cut into pdm_bev_roi_crop_fc_chunks(R, C, G, Cout) runs of whole 128-index
 *   stages, a function of those four numbers alone, whose partials are added in ascending order.  C a multiple of 16 up to 512,
 *   Cout a multiple of 16 up to 1024, R Cout < 2^31.  workspace: pdm_bev_roi_crop_fc_workspace_bytes bytes (0 for sizes the call
 *   refuses), 16-byte aligned, contents irrelevant.  Two launches. */
/* align: rois, map, pooled, out any (4-byte accesses); wpack and workspace 16 B (checked). */
int pdm_bev_roi_crop(void *stream, int B, int n, int roi_stride, const float *rois, int C, int H, int W, const float *spatial_features_2d,
                     float x0, float y0, float cell_x, float cell_y, int G, float *pooled, long long ld);
size_t pdm_bev_roi_crop_fc_packed_floats(int C, int G, int Cout);
int pdm_bev_roi_crop_fc_chunks(int R, int C, int G, int Cout);
size_t pdm_bev_roi_crop_fc_workspace_bytes(int R, int C, int G, int Cout);
int pdm_bev_roi_crop_fc(void *stream, int B, int n, int roi_stride, const float *rois, int C, int H, int W, const float *spatial_features_2d,
                        float x0, float y0, float cell_x, float cell_y, int G, int Cout, const float *wpack, const float *scale,
                        const float *shift, int relu, float *out, void *workspace, size_t workspace_bytes);

/* ---- DSVT: the set partition of one stage and the fused set attention (csrc/dsvt.hip) ----------------------------------------
 * pdm_dsvt_partition_count, then pdm_dsvt_partition with the same geometry and workspace: voxel_coords (N, 4) int32 (b, z, y, x),
 *   distinct voxels in any row order on the sparse shape (sx, sy, sz) of B samples; windows[6] = the window (wx, wy, wz) of shift 0
 *   and of shift 1, shifts[6] = the two shift vectors (x, y, z), 0 <= shift <= window (host arrays; the z shift counts as 0 where
 *   the window spans z); set_size >= 1.  A voxel lies in window ((b MX + X / wx) MY + Y / wy) MZ + Z / wz with (X, Y, Z) = (x, y, z) +
 *   shift and M* = ceil(shape / w) + 1; occupied windows are numbered in ascending order of that id, a window of n voxels gets
 *   ceil(n / set_size) sets, and slot k of its sets holds its voxel number floor(k n / (sets set_size)) under the key
 *   (iy wx + ix) wz + iz (axis 0) or (ix wy + iy) wz + iz (axis 1) of the in-window position.
 *   _count: coors_in_win (2, N, 3) int32 (z, y, x in the window, per shift) and set_counts[2] (HOST) = the sets of each shift,
 *   after ONE host read (the call synchronises the stream).  A coordinate outside the sparse shape is PDM_E_BADARG, found on
 *   the device and reported by this call.  workspace >= pdm_dsvt_partition_workspace_bytes(...) (0 for sizes the calls refuse),
 *   8-byte aligned; a window volume the workspace was not sized for is PDM_E_BADARG.
 *   pdm_dsvt_partition: set_voxel_inds{0,1} (2, S_shift, set_size) int64 and set_voxel_mask{0,1} (2, S_shift, set_size) bytes
 *   (1 = the slot equals its left neighbour in the set), every element written once, by one thread: two runs give the same bits.
 *   One launch, no host read.  No sort, no hash, no float atomics, no cursors: an occupancy bitmap and two tiled scans.
 * pdm_set_attention: q, k, v (N, C) fp32, each with its own ROW stride in elements (>= C; the thirds of one (N, 3C) buffer serve),
 *   set_voxel_inds (S, set_size) int64 -> out (N, C) contiguous: for every set and head softmax(q_h k_h^T / sqrt(d) + mask) v_h over
 *   the set's rows, written at the row of every slot that differs from its left neighbour; a slot that equals it is masked as a
 *   key and skipped as a query (the mask is derived from the indices, not read).  Rows that no set names are not written.
 *   d = C / nheads in {16, 24, 32}, C <= 256, 1 <= set_size <= 128; anything else is PDM_E_BADARG.  Indices are clamped into
 *   [0, N).  One launch, one wave per (set, head), both products on mfma_f32_16x16x4f32, no workspace, no LDS, no atomics: two
 *   runs give the same bits; capturable in a graph. */
/* align: any (4-byte accesses; 16-byte ones only where the pointers and strides allow), except set_voxel_inds and the workspace: 8 B
 * (PDM_E_BADARG otherwise). */
size_t pdm_dsvt_partition_workspace_bytes(int N, int B, int sx, int sy, int sz, const int *windows);
int pdm_dsvt_partition_count(void *stream, int N, const int *voxel_coords, int B, int sx, int sy, int sz, const int *windows,
                             const int *shifts, int set_size, int *coors_in_win, int *set_counts, void *workspace, size_t workspace_bytes);
int pdm_dsvt_partition(void *stream, int N, const int *voxel_coords, int B, int sx, int sy, int sz, const int *windows,
                       const int *shifts, int set_size, int S0, int S1, long long *set_voxel_inds0, unsigned char *set_voxel_mask0,
                       long long *set_voxel_inds1, unsigned char *set_voxel_mask1, void *workspace, size_t workspace_bytes);
int pdm_set_attention(void *stream, int S, int set_size, int N, int C, int nheads, const float *q, long long q_stride,
                      const float *k, long long k_stride, const float *v, long long v_stride, const long long *set_voxel_inds,
                      float *out);

/* Diagnostics: *slot = the device's constant-rate counter (100 MHz) when `stream` reaches this point. */
int pdm_mark_time(void *stream, unsigned long long *slot);

#ifdef __cplusplus
}
#endif
#endif /* PDMSSD_HIP_H */

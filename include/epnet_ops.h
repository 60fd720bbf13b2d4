/*
 * epnet_ops.h -- C ABI of the MI355X (gfx950) point-cloud geometry library, libepnet_hip.so.
 *
 * Every entry point below replaces one launcher of the reference's three CUDA extensions
 * (pointnet2_cuda, iou3d_cuda, roipool3d_cuda); the reference interface it stands in for is
 * cited as path:line relative to the reference checkout. Conventions:
 *
 *   - plain pointers and sizes only; no torch / pybind types;
 *   - every device pointer is a HIP device address of a contiguous fp32 / int32 / int64 array
 *     laid out exactly as the reference lays it out (shapes in the comments);
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream); all device entry
 *     points are asynchronous on that stream, allocate nothing, keep no state between calls and
 *     are re-entrant (the reference's ops are called concurrently from several host threads
 *     under nn.DataParallel, tools/train_rcnn.py:221-223); the one process-wide setting, the
 *     kernel-selection overrides of epnet_set_tuning, picks among kernels of identical results;
 *   - return value: EPNET_OK (0) or a negative EPNET_E* code; the library never calls exit()
 *     (the reference does: e.g. pointnet2_lib/pointnet2/src/ball_query_gpu.cu:62-65);
 *   - scratch memory is supplied by the caller (`*_workspace_bytes` + `workspace`), replacing
 *     the per-call cudaMalloc/cudaFree of lib/utils/iou3d/src/iou3d.cpp:87,98 and
 *     lib/utils/roipool3d/src/roipool3d_kernel.cu:214,222,231-232.
 *
 * Arithmetic contract (DESIGN.md "Parity definition"): IEEE fp32, source order, no fused
 * contraction; integer outputs bit-exact versus oracle/ (the CPU restatement of the reference
 * kernels), float copies exact, float sums to 1e-5 -- except the deterministic gradients (*_det,
 * below), whose scatter-adds are bit-exact versus the oracle's sequential loops.
 */
#ifndef EPNET_OPS_H
#define EPNET_OPS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define EPNET_ABI_VERSION 1

#define EPNET_OK 0
#define EPNET_EINVAL (-1)   /* bad size / NULL pointer */
#define EPNET_ELAUNCH (-2)  /* hipLaunch / hipGetLastError reported a failure */
#define EPNET_ENOMEM (-3)   /* workspace too small */
#define EPNET_ELIMIT (-4)   /* problem size outside what the kernels support */

typedef void *epnet_stream_t;

int epnet_abi_version(void);
const char *epnet_strerror(int code);
/* last HIP error string recorded by this thread's most recent failing call ("" if none) */
const char *epnet_last_hip_error(void);

/* kernel-selection overrides for tests and A/B measurements; names as the EPNET_* variables,
   value -1 = the library's own choice. EPNET_EINVAL for an unknown name or a value out of range.
   The table is seeded once, on first use, from the environment variables of the same names; an
   override that does not fit a launch's shape is ignored there. No workspace size depends on it.
     EPNET_FPS_PRUNE            0 | 1     0: brute-force FPS instead of the spatially pruned kernel
     EPNET_FPS_PRUNE_MIN        >= 0      pruned FPS only above this many points (default 1024)
     EPNET_FPS_PWAVES           4 | 8     waves of the self-sorting pruned FPS kernel
     EPNET_FPS_WAVES            1 .. 16   waves of the register-resident FPS kernel (a power of two)
     EPNET_BQ_PAIR              0 | 1     two centres per wave in the indexed ball query
     EPNET_BQ_STREAM            0 | 1     streaming hit lists instead of the bitmap (paired query)
     EPNET_BQ_ORDERED           0 | 1     centres served in their spatial order (epnet_ball_query_ordered)
     EPNET_NN_TILE_MIN_BUCKETS  >= 0      bucket-of-unknowns three_nn from this many buckets (default 4096) */
int epnet_set_tuning(const char *name, int value);
int epnet_get_tuning(const char *name, int *value);

/* ----------------------------------------------------------------------------------------
 * pointnet2 (pointnet2_lib/pointnet2/src/pointnet2_api.cpp:10-24)
 * -------------------------------------------------------------------------------------- */

/* furthest_point_sampling_kernel_launcher, sampling_gpu.cu:211-253 (wrapper sampling.cpp:36-46).
 * xyz (B,N,3) f32; temp (B,N) f32 in/out running min squared distance, caller-filled with 1e10
 * (pointnet2_utils.py:26); idx (B,M) i32 out. idx[:,0] = 0. Tie-breaks reproduce the reference
 * block reduction for block size opt_n_threads(N) (cuda_utils.h:10-14). temp may be NULL: the
 * kernel then starts from 1e10 and does not write the distances back. */
int epnet_furthest_point_sampling(int b, int n, int m, const float *xyz, float *temp, int *idx,
                                  epnet_stream_t stream);

/* gather_points_kernel_launcher_fast, sampling_gpu.cu:26-43. points (B,C,N), idx (B,M) -> out (B,C,M) */
int epnet_gather_points(int b, int c, int n, int npoints, const float *points, const int *idx,
                        float *out, epnet_stream_t stream);

/* gather_points_grad_kernel_launcher_fast, sampling_gpu.cu:65-83.
 * grad_out (B,C,M), idx (B,M) -> grad_points (B,C,N) accumulated into (caller-zeroed, pointnet2_utils.py:67) */
int epnet_gather_points_grad(int b, int c, int n, int npoints, const float *grad_out, const int *idx,
                             float *grad_points, epnet_stream_t stream);

/* ball_query_kernel_launcher_fast, ball_query_gpu.cu:48-66 (note: new_xyz before xyz, ball_query.cpp:14).
 * new_xyz (B,M,3), xyz (B,N,3) -> idx (B,M,nsample) i32. Every slot is written (zeros when the
 * ball is empty; the reference leaves the caller's zero fill, pointnet2_utils.py:218). */
int epnet_ball_query(int b, int n, int m, float radius, int nsample, const float *new_xyz,
                     const float *xyz, int *idx, epnet_stream_t stream);

/* Same result as epnet_ball_query, with caller-supplied device scratch (16-byte aligned) that lets the
 * library index the scene spatially (Morton-sorted copy + per-bucket boxes) instead of scanning all N
 * points per centre; bit-identical output. epnet_ball_query_workspace_bytes() == 0 means the direct scan
 * is used anyway (small or very large scenes) and workspace may be NULL. */
size_t epnet_ball_query_workspace_bytes(int b, int n, int m);
int epnet_ball_query_ws(int b, int n, int m, float radius, int nsample, const float *new_xyz, const float *xyz,
                        int *idx, void *workspace, size_t workspace_bytes, epnet_stream_t stream);

/* group_points_kernel_launcher_fast, group_points_gpu.cu:69-86.
 * points (B,C,N), idx (B,M,ns) -> out (B,C,M,ns) */
int epnet_group_points(int b, int c, int n, int npoints, int nsample, const float *points,
                       const int *idx, float *out, epnet_stream_t stream);

/* group_points_grad_kernel_launcher_fast, group_points_gpu.cu:27-44.
 * grad_out (B,C,M,ns), idx (B,M,ns) -> grad_points (B,C,N) accumulated into (caller-zeroed) */
int epnet_group_points_grad(int b, int c, int n, int npoints, int nsample, const float *grad_out,
                            const int *idx, float *grad_points, epnet_stream_t stream);

/* Fused tail of QueryAndGroup.forward (pointnet2_utils.py:250-257): one call writes
 *   out (B, 3+C, M, ns) = [ xyz[b, idx[b,i,s], :] - new_xyz[b,i,:]   (3 channels, if use_xyz)
 *                           features[b, :, idx[b,i,s]]               (C channels) ]
 * reading xyz in its (B,N,3) layout -- no transposed copy of xyz, no separate centre-subtraction pass over the
 * grouped tensor and no torch.cat copy of it. features may be NULL when c == 0. Values are bit-identical to the
 * reference composition (a gather and one fp32 subtraction). */
int epnet_group_concat(int b, int c, int n, int npoints, int nsample, const float *xyz, const float *new_xyz,
                       const float *features, const int *idx, float *out, int use_xyz, epnet_stream_t stream);
/* the same with caller scratch: where the feature rows are too long for on-chip staging (n > 16384 points: BASELINE config
 * 5) the features are turned point-major once in the scratch and gathered as contiguous rows. workspace_bytes = 0 (or
 * workspace NULL): plain epnet_group_concat. */
size_t epnet_group_concat_workspace_bytes(int b, int c, int n, int npoints, int nsample);
int epnet_group_concat_ws(int b, int c, int n, int npoints, int nsample, const float *xyz, const float *new_xyz,
                          const float *features, const int *idx, float *out, int use_xyz, void *workspace,
                          size_t workspace_bytes, epnet_stream_t stream);

/* gradient of the above w.r.t. features: grad_out (B, 3+C | C, M, ns) -> grad_features (B,C,N) accumulated into */
int epnet_group_concat_grad(int b, int c, int n, int npoints, int nsample, const float *grad_out, const int *idx,
                            float *grad_features, int use_xyz, epnet_stream_t stream);

/* Gradients of the two grouping forms with caller-supplied device scratch: the scatter-add is inverted (the
 * positions are grouped by target point, then every target sums its own list out of LDS) so that no atomic
 * is needed. Same result up to the summation order, which the reference's atomicAdd leaves unspecified too.
 * A workspace size of 0 means the scratch-free kernels are used anyway. */
size_t epnet_group_points_grad_workspace_bytes(int b, int n, int npoints, int nsample);
int epnet_group_points_grad_ws(int b, int c, int n, int npoints, int nsample, const float *grad_out, const int *idx,
                               float *grad_points, void *workspace, size_t workspace_bytes, epnet_stream_t stream);
int epnet_group_concat_grad_ws(int b, int c, int n, int npoints, int nsample, const float *grad_out, const int *idx,
                               float *grad_features, int use_xyz, void *workspace, size_t workspace_bytes,
                               epnet_stream_t stream);

/* three_nn_kernel_launcher_fast, interpolate_gpu.cu:55-74.
 * unknown (B,n,3), known (B,m,3) -> dist2 (B,n,3) f32 squared distances, idx (B,n,3) i32 */
int epnet_three_nn(int b, int n, int m, const float *unknown, const float *known, float *dist2,
                   int *idx, epnet_stream_t stream);

/* Same result as epnet_three_nn with caller-supplied device scratch (16-byte aligned): the known points are
 * indexed spatially and each unknown point only visits the buckets that can hold one of its three
 * nearest; bit-identical output. A workspace size of 0 means the direct scan is used (workspace may be NULL). */
size_t epnet_three_nn_workspace_bytes(int b, int n, int m);
int epnet_three_nn_ws(int b, int n, int m, const float *unknown, const float *known, float *dist2, int *idx,
                      void *workspace, size_t workspace_bytes, epnet_stream_t stream);

/* three_interpolate_kernel_launcher_fast, interpolate_gpu.cu:99-117 (argument order b,c,m,n).
 * points (B,C,m), idx (B,n,3), weight (B,n,3) -> out (B,C,n) */
int epnet_three_interpolate(int b, int c, int m, int n, const float *points, const int *idx,
                            const float *weight, float *out, epnet_stream_t stream);

/* three_interpolate_grad_kernel_launcher_fast, interpolate_gpu.cu:144-161 (argument order b,c,n,m).
 * grad_out (B,C,n), idx, weight (B,n,3) -> grad_points (B,C,m) accumulated into (caller-zeroed) */
int epnet_three_interpolate_grad(int b, int c, int n, int m, const float *grad_out, const int *idx,
                                 const float *weight, float *grad_points, epnet_stream_t stream);

/* the groupings of all scales of an MSG level in one call (two scales: the feature rows are staged in LDS once for both).
 * nsamples / idx / out are HOST arrays of nscales entries; out[k] is (b, 3+c | c, npoints, nsamples[k]). Same results as
 * nscales calls of epnet_group_concat. */
int epnet_group_concat_multi(int b, int c, int n, int npoints, int nscales, const int *nsamples, const float *xyz,
                             const float *new_xyz, const float *features, const int *const *idx, float *const *out,
                             int use_xyz, epnet_stream_t stream);

/* atomic-free form of the above with caller scratch (inverse index over the known points); 0 bytes = not used */
size_t epnet_three_interpolate_grad_workspace_bytes(int b, int n, int m);
int epnet_three_interpolate_grad_ws(int b, int c, int n, int m, const float *grad_out, const int *idx,
                                    const float *weight, float *grad_points, void *workspace, size_t workspace_bytes,
                                    epnet_stream_t stream);

/* The first shared-MLP layer of an SA level folded into its grouping. The reference materialises
 * [xyz[idx] - centre ; features[idx]] (pointnet2_utils.py:250-257) and runs a 1x1 convolution W over it
 * (pointnet2_modules.py:61); that convolution is linear and pointwise, so W . [dxyz ; F[:, idx]] =
 * W_xyz . dxyz + (W_f . F)[:, idx]. With z = W_f . F (b, c, n) computed by the caller (a dense GEMM over n columns instead of
 * npoints * nsample), this writes the layer's pre-activations out (b, c, npoints, nsample):
 *   out[b,co,m,s] = z[b,co,idx[b,m,s]] + (w_xyz[co][0]*dx + w_xyz[co][1]*dy + w_xyz[co][2]*dz) (+ bias[co]),
 *   (dx,dy,dz) = xyz[b,idx[b,m,s]] - new_xyz[b,m]; w_xyz (c,3), bias (c) or NULL. */
int epnet_group_linear(int b, int c, int n, int npoints, int nsample, const float *xyz, const float *new_xyz, const float *z,
                       const int *idx, const float *w_xyz, const float *bias, float *out, epnet_stream_t stream);

/* gradient of epnet_group_linear w.r.t. w_xyz: grad_w (c,3) += sum over (b,m,s) of grad_out[b,co,m,s] * (xyz[b,idx[b,m,s]] -
 * new_xyz[b,m])[k]; the caller zero-fills grad_w (accumulated with float atomics: summation order unspecified). The gradient
 * w.r.t. z is epnet_group_points_grad of grad_out, the one w.r.t. bias its sum over (b,m,s). */
int epnet_group_linear_grad_w(int b, int c, int n, int npoints, int nsample, const float *grad_out, const float *xyz,
                              const float *new_xyz, const int *idx, float *grad_w, epnet_stream_t stream);

/* the neighbourhood max-pool of an SA level, F.max_pool2d(kernel_size=[1, nsample]) of pointnet2_modules.py:61-68: x
 * (rows, nsample) contiguous (rows = B * C * npoint) -> out (rows) = the row maximum (ties: lowest position; NaN
 * propagates), arg (rows) i32 or NULL = its position for the backward. epnet_pool_max_grad: grad_x (rows, nsample) =
 * grad_out[row] at arg[row], zero elsewhere (every element is written). */
int epnet_pool_max(long long rows, int nsample, const float *x, float *out, int *arg, epnet_stream_t stream);
int epnet_pool_max_grad(long long rows, int nsample, const float *grad_out, const int *arg, float *grad_x,
                        epnet_stream_t stream);

/* The same three byte movers on 16-bit feature rows (csrc/rows16.hip; torch.autocast). dtype names the type of the `void *`
 * rows; coordinates, weights, bias and indices stay fp32 / i32. ONE rule: the result is the value the fp32 entry point above
 * gives on the rows upcast to fp32, rounded once to the 16-bit type (to nearest, ties to even; denormals kept; overflow gives
 * +-inf; NaN stays NaN). The max-pool and its gradient move the element's own 16 bits. Same argument validation and error
 * codes as the fp32 twins; an unknown dtype is EPNET_EINVAL. No alignment is required beyond the element's (the kernels
 * pick their 16- and 8-byte paths from the pointers). */
#define EPNET_F16 1
#define EPNET_BF16 2
int epnet_group_linear_h(int b, int c, int n, int npoints, int nsample, const float *xyz, const float *new_xyz, const void *z,
                         const int *idx, const float *w_xyz, const float *bias, void *out, int dtype, epnet_stream_t stream);
int epnet_pool_max_h(long long rows, int nsample, const void *x, void *out, int *arg, int dtype, epnet_stream_t stream);
int epnet_pool_max_grad_h(long long rows, int nsample, const void *grad_out, const int *arg, void *grad_x, int dtype,
                          epnet_stream_t stream);
int epnet_three_interpolate_h(int b, int c, int m, int n, const void *points, const int *idx, const float *weight, void *out,
                              int dtype, epnet_stream_t stream);

/* LI-Fusion's point-to-pixel sampler: Feature_Gather of lib/net/pointnet2_msg.py:107-120 =
 * torch grid_sample(feature_map (b,c,h,w), xy (b,1,n,2) in [-1,1]) -> out (b,c,n), bilinear, zero padding, with the
 * torch.gather of xy over the FPS indices (:214-217) folded in: idx (b,n) i32 or NULL picks the rows of xy (b,n_src,2)
 * (NULL: n_src == n, row q of xy), xy_out (b,n,2) or NULL receives the picked coordinates for the next level.
 * align_corners as in torch (the reference was written for torch <= 1.2, where grid_sample behaved as align_corners=True).
 * epnet_feature_gather_grad: grad_feature_map (b,c,h,w), zero-filled by the caller, += the bilinear scatter of grad_out
 * (b,c,n) at xy (b,n,2) (float atomics). */
int epnet_feature_gather(int b, int c, int h, int w, int n_src, int n, int align_corners, const float *feature_map,
                         const float *xy, const int *idx, float *out, float *xy_out, epnet_stream_t stream);
int epnet_feature_gather_grad(int b, int c, int h, int w, int n, int align_corners, const float *grad_out, const float *xy,
                              float *grad_feature_map, epnet_stream_t stream);

/* ----------------------------------------------------------------------------------------
 * Deterministic gradients (torch.use_deterministic_algorithms(True) in the Python surface). The default gradient entry
 * points above add with float atomics, so their bits change from run to run. The *_det forms below give bits that depend
 * on nothing but the inputs and the shape: not on the stream, concurrent work, epnet_set_tuning, the placement of
 * workgroups or the batch position of a scene. They use no float atomics, allocate nothing and synchronise nothing (graph
 * capturable); the scratch is the caller's: workspace (256-byte aligned) of at least the matching *_det_workspace_bytes,
 * which depends on the shape alone and is 0 only for an empty problem. Same EPNET_ELIMIT limits as the default entry
 * point; in addition the entries of one scene (npoints * nsample, 3 n, 4 n) must stay below 2^31.
 *
 * Scatter-add gradients (gather_points_grad, group_points_grad, group_concat_grad, three_interpolate_grad): grad_points
 * receives exactly the bits that the oracle's sequential loop (oracle/epnet_oracle.c: oracle_gather_points_grad,
 * oracle_group_points_grad, oracle_three_interpolate_grad) leaves in the same buffer from the same contents. For each
 * (scene, channel) the terms are taken in ascending entry order -- for three_interpolate_grad (unknown, then k = 0, 1, 2) --
 * each term is one fp32 product where there is a weight (grad_out * weight), and each is added to the running value with
 * one fp32 add, g[j] = g[j] + term, starting from the buffer's incoming value (so accumulating calls, e.g. two scales into
 * one buffer, equal the oracle called twice). Entries whose index lies outside [0, n) add nothing (outside the bit-exact
 * claim; the default entry points leave them undefined).
 *
 * epnet_feature_gather_grad_det: for each (scene, channel) the points in ascending order, each point's in-bounds taps in
 * the order nw, ne, sw, se; term = grad_out * tap weight (the weights of epnet_feature_gather); the same sequential fold
 * from the buffer's contents.
 *
 * epnet_group_linear_grad_w_det: a fixed order that depends on the shape alone. The positions q of a scene (p = npoints *
 * nsample) are cut into tiles of 4096; in a tile, slot i (0..255) sums the terms of positions tile * 4096 + i + 256 k,
 * k ascending, from 0 (term = grad_out[b,co,q] * (xyz[b,idx] - new_xyz[b,m])[d], one fp32 subtraction and one product);
 * the 64 slots of each quarter are combined by the butterfly v[i] = v[i] + v[i ^ o], o = 32, 16, 8, 4, 2, 1; the
 * quarters are added in order from 0; the tiles of a scene in ascending order from 0; the scenes in ascending order from
 * 0; and the total is added to grad_w once: grad_w = grad_w + total. Values stay within the default's bound against the
 * oracle.
 * -------------------------------------------------------------------------------------- */
size_t epnet_gather_points_grad_det_workspace_bytes(int b, int n, int npoints);
int epnet_gather_points_grad_det(int b, int c, int n, int npoints, const float *grad_out, const int *idx, float *grad_points,
                                 void *workspace, size_t workspace_bytes, epnet_stream_t stream);
size_t epnet_group_points_grad_det_workspace_bytes(int b, int n, int npoints, int nsample);
int epnet_group_points_grad_det(int b, int c, int n, int npoints, int nsample, const float *grad_out, const int *idx,
                                float *grad_points, void *workspace, size_t workspace_bytes, epnet_stream_t stream);
size_t epnet_group_concat_grad_det_workspace_bytes(int b, int n, int npoints, int nsample);
int epnet_group_concat_grad_det(int b, int c, int n, int npoints, int nsample, const float *grad_out, const int *idx,
                                float *grad_features, int use_xyz, void *workspace, size_t workspace_bytes, epnet_stream_t stream);
size_t epnet_three_interpolate_grad_det_workspace_bytes(int b, int n, int m);
int epnet_three_interpolate_grad_det(int b, int c, int n, int m, const float *grad_out, const int *idx, const float *weight,
                                     float *grad_points, void *workspace, size_t workspace_bytes, epnet_stream_t stream);
size_t epnet_feature_gather_grad_det_workspace_bytes(int b, int h, int w, int n);
int epnet_feature_gather_grad_det(int b, int c, int h, int w, int n, int align_corners, const float *grad_out, const float *xy,
                                  float *grad_feature_map, void *workspace, size_t workspace_bytes, epnet_stream_t stream);
size_t epnet_group_linear_grad_w_det_workspace_bytes(int b, int c, int npoints, int nsample);
int epnet_group_linear_grad_w_det(int b, int c, int n, int npoints, int nsample, const float *grad_out, const float *xyz,
                                  const float *new_xyz, const int *idx, float *grad_w, void *workspace, size_t workspace_bytes,
                                  epnet_stream_t stream);

/* ----------------------------------------------------------------------------------------
 * scene index: one spatial sort of a level's points (1024 <= n <= 65536), built once in caller scratch and
 * shared by the sampling and both ball queries of that level (the reference has no counterpart: every one of
 * its kernels scans all n points). Results are identical to the plain entry points.
 * epnet_scene_index_bytes returns 0 where no index applies; the *_indexed entry points then (or with
 * index == NULL) run the plain path. For n > 16384 the last part of the buffer is scratch of the sampling kernel
 * (its running distances in sorted order): two samplings over ONE index buffer must not run concurrently there;
 * the ball queries and three_nn never touch that part. The three sampling entry points therefore take the index as a NON-const
 * pointer (they write that tail; the sorted points and boxes in front of it are only read), everybody else as const.
 * -------------------------------------------------------------------------------------- */
size_t epnet_scene_index_bytes(int b, int n);
int epnet_scene_index_build(int b, int n, const float *xyz, void *index, size_t index_bytes, epnet_stream_t stream);
/* The index of the n points xyz_src[idx[0 .. n)] of every scene (rows of a (b, n_src, 3) cloud: the centres a sampling has just
 * picked, pointnet2_modules.py:39-45), which are also written to gathered (b, n, 3) in that order: the centre gather of an SA level
 * and the index build of the next level in one launch. 1024 <= n <= 16384; idx values in [0, n_src). */
int epnet_scene_index_build_gathered(int b, int n_src, int n, const float *xyz_src, const int *idx, float *gathered, void *index,
                                     size_t index_bytes, epnet_stream_t stream);
/* same contract as epnet_furthest_point_sampling (sampling_gpu.cu:211-253) */
int epnet_furthest_point_sampling_indexed(int b, int n, int m, const float *xyz, void *index,
                                          size_t index_bytes, float *temp, int *idx, epnet_stream_t stream);
/* the head of an SA module in one call (pointnet2_modules.py:39-45): furthest point sampling from a fresh state
 * (all running distances 1e10, pointnet2_utils.py:26) and new_xyz (b,m,3) = the selected rows of xyz. temp = scratch
 * (b,n) or NULL (allowed for 64 <= n <= 16384); index = scene index of xyz or NULL */
int epnet_sample_centres(int b, int n, int m, const float *xyz, void *index, size_t index_bytes, float *temp,
                         int *idx, float *new_xyz, epnet_stream_t stream);
/* epnet_sample_centres for the levels of a sampling pyramid (SA level l+1 samples the centres of level l). Furthest point
 * sampling is nested: while every round's maximum is unique, the first m samples of a furthest-point sequence ARE the
 * furthest-point samples of that sequence -- idx = 0 .. m-1, bit for bit what sampling_gpu.cu:94-209 computes on the centres
 * (its tie-break matters among equal maxima only). prefix_in (b ints or NULL): leading rounds of the sampling that produced xyz
 * in which the maximum was unique up to exact twins -- points with identical coordinates, as the reference's loader creates when
 * it pads a short scene (kitti_rcnn_dataset.py:338-342): the unpicked twin is at distance 0 from then on and cannot be sampled
 * while the maximum is positive, so the sequence of sampled COORDINATES does not depend on the tie-break (= the prefix_out of
 * that call); scenes with prefix_in[b] >= m take the identity, the others
 * run the rounds. prefix_out (b ints or NULL): the same knowledge about this call's output (at least that many rounds), 0 where
 * the kernel cannot tell; ties are looked for during the first prefix_cap rounds only (<= 0: all) -- pass the next level's m.
 * new_xyz may be NULL here (indices only: the centres then come out of epnet_scene_index_build_gathered of the next level). */
int epnet_sample_centres_chain(int b, int n, int m, const float *xyz, void *index, size_t index_bytes, float *temp,
                               int *idx, float *new_xyz, const int *prefix_in, int *prefix_out, int prefix_cap,
                               epnet_stream_t stream);
/* epnet_sample_centres_chain followed by epnet_scene_index_build_gathered(b, n, m, xyz, idx, new_xyz, next_index, ...): the centres
 * AND their scene index, which is what the next level of the pyramid starts with. next_index: epnet_scene_index_bytes(b, m) bytes,
 * 16-byte aligned; 1024 <= m <= 16384; new_xyz is required. For 8192 < n <= 16384 over an index, 1024 <= m <= 4096 and
 * prefix_in == NULL the sampling workgroup of a scene does both in the epilogue of its rounds (no dispatch in between: on a busy
 * chip a small dispatch mostly waits for a place); every other shape issues the two launches. idx, new_xyz and prefix_out are the
 * same bits either way; inside a grid cell of the index the order of the points is unspecified, as for every index build. */
int epnet_sample_centres_chain_index(int b, int n, int m, const float *xyz, void *index, size_t index_bytes, float *temp,
                                     int *idx, float *new_xyz, const int *prefix_in, int *prefix_out, int prefix_cap,
                                     void *next_index, size_t next_index_bytes, epnet_stream_t stream);
/* same contract as epnet_three_nn (interpolate_gpu.cu:55-74); known_index = scene index of `known` (NULL: plain
 * path), unknown_index = scene index of `unknown` or NULL */
int epnet_three_nn_indexed(int b, int n, int m, const float *unknown, const float *known, const void *unknown_index,
                           size_t unknown_index_bytes, const void *known_index, size_t known_index_bytes, float *dist2,
                           int *idx, epnet_stream_t stream);
/* same contract as epnet_ball_query (ball_query_gpu.cu:48-66) */
int epnet_ball_query_indexed(int b, int n, int m, float radius, int nsample, const float *new_xyz, const float *xyz,
                             const void *index, size_t index_bytes, int *idx, epnet_stream_t stream);
/* the nscales ball queries of an MSG level (same centres, same points, nested balls) in ONE launch: every distance is
 * computed once. radii / nsamples / idx are HOST arrays of nscales entries, idx[k] a device (b, m, nsamples[k])
 * buffer. Same results as nscales calls of epnet_ball_query_indexed (which is what happens unless nscales == 2). */
int epnet_ball_query_indexed_multi(int b, int n, int m, int nscales, const float *radii, const int *nsamples,
                                   const float *new_xyz, const float *xyz, const void *index, size_t index_bytes,
                                   int *const *idx, epnet_stream_t stream);
/* The same queries with the centres served in THEIR spatial order (ball_query_gpu.cu:9-45 gives thread i centre i; the centres of an
 * SA level come in furthest-point order, which scatters consecutive centres over the whole scene). centre_index = the scene index
 * (epnet_scene_index_build / _build_gathered) of the cloud new_xyz (b, m, 3), in that order -- the next SA level samples the
 * centres, so the stack has it anyway: wave w serves the w-th centre of that order, its neighbours walk the same point buckets,
 * which are then cache hits. nscales 1 or 2 (otherwise, or with centre_index == NULL, or for m < 1024:
 * epnet_ball_query_indexed_multi). Results identical to epnet_ball_query per scale. */
int epnet_ball_query_ordered(int b, int n, int m, int nscales, const float *radii, const int *nsamples, const float *new_xyz,
                             const float *xyz, const void *index, size_t index_bytes, const void *centre_index,
                             size_t centre_index_bytes, int *const *idx, epnet_stream_t stream);

/* ----------------------------------------------------------------------------------------
 * iou3d (lib/utils/iou3d/src/iou3d.cpp:174-179); boxes are (N,5) [x1,y1,x2,y2,ry] f32
 * -------------------------------------------------------------------------------------- */

/* boxesoverlapLauncher, iou3d_kernel.cu:354-363: ans (num_a,num_b) rotated-rectangle overlap area */
int epnet_boxes_overlap_bev(int num_a, const float *boxes_a, int num_b, const float *boxes_b,
                            float *ans_overlap, epnet_stream_t stream);

/* boxesioubevLauncher, iou3d_kernel.cu:365-372: ans (num_a,num_b) rotated BEV IoU */
int epnet_boxes_iou_bev(int num_a, const float *boxes_a, int num_b, const float *boxes_b,
                        float *ans_iou, epnet_stream_t stream);

/* boxes_iou3d_gpu of lib/utils/iou3d/iou3d_utils.py:21-53 in one launch: boxes (.,7) [x,y,z,h,w,l,ry] ->
 * ans (num_a,num_b) 3-D IoU = BEV overlap x height overlap / union volume (clamped at 1e-7). The reference
 * composes boxes3d_to_bev_torch + boxes_overlap_bev_gpu + ~10 elementwise torch kernels; same fp32 operations
 * in the same order here. */
int epnet_boxes_iou3d(int num_a, const float *boxes_a, int num_b, const float *boxes_b, float *ans_iou3d,
                      epnet_stream_t stream);

/* the same for k (a_i, b_i) PAIRS -> ans (k): one launch for what lib/rpn/proposal_target_layer.py:220-247
 * does with up to 640 single-pair calls per scene */
int epnet_boxes_iou3d_pairs(int k, const float *boxes_a, const float *boxes_b, float *ans_iou3d, epnet_stream_t stream);

/* aug_roi_by_noise_torch, lib/rpn/proposal_target_layer.py:220-247, for all k sampled ROIs of
 * a scene in one launch. The reference's host loop per ROI -- `while temp_iou < pos_thresh and cnt < aug_times`:
 * coin (keep the ROI, p = 0.2) or random_aug_box3d (:250-275), single-pair boxes_iou3d_gpu, read the IoU back --
 * takes its random draws from the caller's tables instead of np.random / torch.rand, indexed [roi][try]:
 * keep_draw (k, aug_times) u8 (1 = keep the original box), noise (k, aug_times, 7) f32 = pos_shift[3], hwl_scale[3],
 * angle_rot (the noisy box is [xyz + shift, hwl * scale, ry + rot]). roi_boxes3d (k,7) is updated in place with the
 * box of the last try (:242), iou_of_rois (k) receives iou3d_src[k] when that try kept the ROI (or no try ran) and
 * the last IoU otherwise (:243-246). gt_boxes3d (k,7) = the ground-truth box assigned to each ROI. tries (k) i32 or
 * NULL: per-ROI try limit min(tries[i], aug_times) -- foreground ROIs get ROI_FG_AUG_TIMES tries and background ROIs
 * one (:164-176), so the ROIs of a whole batch go through one launch. */
int epnet_aug_roi_by_noise(int k, int aug_times, float pos_thresh, float *roi_boxes3d, const float *gt_boxes3d,
                           const float *iou3d_src, const int *tries, const unsigned char *keep_draw,
                           const float *noise, float *iou_of_rois, epnet_stream_t stream);

/* sample_rois_for_rcnn, lib/rpn/proposal_target_layer.py:85-218, for all b scenes in one call with no host synchronisation
 * and no allocation (the reference reads three `nonzero` results per scene and draws on the host). rois (b,m,7); gt_boxes3d
 * (b,g,gc), 7 <= gc <= 16, zero-padded as collate_batch pads; the caller's draw tables fg_key (b,m) and slot_u (b,r), uniform
 * in [0,1); keep_draw (b*r,t) u8 and noise (b*r,t,7) as epnet_aug_roi_by_noise takes them (NULL allowed when aug_times t == 0);
 * r = ROI_PER_IMAGE. Per scene, in this order:
 *   padding (:105-108): num_gt = 1 + the last row whose fp32 sum over all gc columns, taken in ascending column order, is not
 *     0; zero rows in front of it stay (boxes with IoU 0). A scene WITHOUT such a row (the reference indexes below 0 there) is
 *     treated as num_gt = 1 with the zero row 0: every IoU is 0, every ROI easy background; scene_info reports num_gt 0.
 *   assignment: max_overlaps[i] = max over j < num_gt of the 3-D IoU of (roi_i, gt_j), bit for bit epnet_boxes_iou3d's value;
 *     gt_assignment[i] = the FIRST j that reaches it (a NaN IoU wins over every number; the first one stays).
 *   classes, each list in ascending ROI index (torch.nonzero): fg ov >= fg_thresh; easy ov < cls_bg_thresh_lo; hard
 *     ov < cls_bg_thresh && ov >= cls_bg_thresh_lo. A NaN maximum is in no list.
 *   selection (:129-156, :191-218) with pick(list, u) = list[min((int)(u * (float)len), len - 1)], one fp32 multiply, entry 0
 *     for a NaN or negative u:
 *     case 0, fg and bg present: fg_this = min(fg_per_image, fg_num); slots 0..fg_this-1 are the fg_this foreground candidates
 *       with the smallest fg_key in ascending key order, ties by ascending ROI index (keys compared as floats, -0 == +0, every
 *       NaN above +inf): a uniform subset without replacement in uniform order, np.random.permutation's distribution. Slots
 *       j >= fg_this use slot_u[j]: with hard and easy both present the first (int)((r - fg_this) * hard_bg_ratio) of them
 *       (a double product, as Python's) pick from hard and the rest from easy; with one kind present all pick from it.
 *     case 1, fg only: every slot is pick(fg, slot_u[j]), fg_this = r.    case 2, bg only: fg_this = 0, the background rule
 *       over all r slots.    case 3, neither (the reference stops in pdb): slot j takes ROI min((int)(slot_u[j] * m), m - 1),
 *       fg_this = 0 (such rows have an IoU between the thresholds: class -1 and no regression later).
 *   gather: batch_rois = rois[src], batch_gt_of_rois = columns 0..6 of gt[gt_assignment[src]], iou_src = max_overlaps[src];
 *     tries = aug_times for the slots below fg_this, (aug_times > 0 ? 1 : 0) for the others (:164-176).
 *   noise loop (:158-179): with aug_times > 0, epnet_aug_roi_by_noise's kernels over all b * r rows with pos_thresh =
 *     fg_thresh update batch_rois in place and write batch_roi_iou; with aug_times == 0 batch_roi_iou = iou_src.
 * Results: batch_rois (b,r,7), batch_gt_of_rois (b,r,7), batch_roi_iou (b,r), scene_info (b,6) i32 = [num_gt as counted (0 if
 * none), fg_num, hard_num, easy_num, fg_this, case]; optional (NULL allowed) src_inds (b,r) i32, iou_src (b,r), tries (b,r)
 * i32, max_overlaps (b,m), gt_assignment (b,m) i32. Every element of every given output is written; no float atomics: the bits
 * depend on the inputs alone. Limits, checked before any launch: 1 <= m <= 4096, 1 <= r <= 1024, g >= 1, b <= 65535, else
 * EPNET_ELIMIT; a NULL required pointer, gc out of range or fg_per_image > r: EPNET_EINVAL; a workspace below
 * epnet_rcnn_sample_rois_workspace_bytes(b, m, g, r) (pure arithmetic: num_gt, the (b,m,g) IoU matrix, maxima, assignment,
 * tries, iou_src, each rounded up to 16 bytes; 0 outside the limits): EPNET_ENOMEM; b == 0 returns EPNET_OK and writes nothing.
 * PRECONDITION: no output may alias an input. */
size_t epnet_rcnn_sample_rois_workspace_bytes(int b, int m, int g, int r);
int epnet_rcnn_sample_rois(int b, int m, int g, int gc, int r, int fg_per_image, float fg_thresh, float cls_bg_thresh,
                           float cls_bg_thresh_lo, double hard_bg_ratio, int aug_times, const float *rois,
                           const float *gt_boxes3d, const float *fg_key, const float *slot_u,
                           const unsigned char *keep_draw, const float *noise, void *workspace, size_t workspace_bytes,
                           float *batch_rois, float *batch_gt_of_rois, float *batch_roi_iou, int *scene_info, int *src_inds,
                           float *iou_src, int *tries, float *max_overlaps, int *gt_assignment, epnet_stream_t stream);

/* ProposalLayer.forward after the box decoding, lib/rpn/proposal_layer.py:34-55 with distance_based_proposal :58-119
 * (distance_based != 0: two bins 0 < z <= 40 and 40 < z <= 80 with 70 % / 30 % of the pre- and post-NMS budgets, the far bin
 * falling back to the near bin's next boxes when it is empty) or score_based_proposal :121-142 (one bin), for all b
 * scenes with no host synchronisation. proposals (b,n,7) decoded boxes, scores (b,n), order (b,n)
 * i64 = positions sorted by descending score (torch.sort, :35). rotated: RPN.NMS_TYPE 'rotate' (nms_gpu) or 'normal'
 * (nms_normal_gpu) (:104-107; score_based_proposal always uses the rotated one, :137). Results: ret_bbox3d
 * (b, post_nms_top_n, 7) and ret_scores (b, post_nms_top_n), zero-padded behind the kept boxes (:38-39, :52-54);
 * ret_count (b) i32 or NULL = kept boxes per scene. */
size_t epnet_rpn_proposals_workspace_bytes(int b, int distance_based, int pre_nms_top_n, int post_nms_top_n);
int epnet_rpn_proposals(int b, int n, const float *proposals, const float *scores, const int64_t *order,
                        int distance_based, int pre_nms_top_n, int post_nms_top_n, float nms_thresh, int rotated,
                        void *workspace, size_t workspace_bytes, float *ret_bbox3d, float *ret_scores, int *ret_count,
                        epnet_stream_t stream);

/* decode_bbox_target, lib/utils/bbox_transform.py:25-262, in ONE launch, for both stages: anchors (rows, anchor_cols) with
 * anchor_cols 3 (the RPN's points) or 7 (the RCNN stage's ROIs), pred_reg (rows, channels) with the channel layout
 * [x bins | z bins | x residuals | z residuals (with xz_fine)] [y offset | y bins, y residuals (with y_by_bin)]
 * [ry bins | ry residuals] [h, w, l residuals] -> boxes (rows, 7) [x, y, z, h, w, l, ry]. bins_xz and bins_y are the caller's
 * int(scope / bin_size) * 2 (no float-to-int conversion happens here); anchor_size: 3 floats in HOST memory, copied at the call
 * (they travel by value in the kernel arguments: the call is graph-capturable). x, z: the soft-max weighted mean of (bin centre +
 * residual) with avg_by_bin, else the FIRST maximal bin (torch.argmax; a NaN counts as the maximum) plus, with xz_fine, its
 * residual; y: anchor y + offset, or the arg-max y bin; heading: the arg-max bin -- coarse (ry_fine == 0): the full turn in
 * num_head_bin bins, taken modulo 2 pi with the sign of the divisor and wrapped into (-pi, pi]; fine: a quarter turn around the
 * ROI's own heading -- or, with ry_with_bin, the probability-weighted mean over the likelier of the two sides (:146-238); sizes
 * residual * anchor_size + anchor_size; for 7-wide anchors (x, z) is rotated by -roi_ry and ry += roi_ry; x, z += the anchor's;
 * with y_to_bottom y += h / 2 (lib/rpn/proposal_layer.py:31). fp32 in source order without contraction. Checked before any
 * launch: channels == (xz_fine ? 4 : 2) * bins_xz + (y_by_bin ? 2 * bins_y : 1) + 2 * num_head_bin + 3, avg_by_bin only with
 * xz_fine (the reference asserts), anchor_cols in {3, 7}, a NULL pointer: EPNET_EINVAL; channels > 255: EPNET_ELIMIT;
 * rows == 0 returns EPNET_OK and writes nothing. PRECONDITION: boxes does not alias an input. */
int epnet_decode_bbox_target(long long rows, int anchor_cols, const float *anchors, const float *pred_reg, int channels,
                             int bins_xz, int bins_y, double loc_scope, double loc_bin_size, double loc_y_scope,
                             double loc_y_bin_size, int num_head_bin, const float *anchor_size, int xz_fine, int y_by_bin,
                             int ry_fine, int avg_by_bin, int ry_with_bin, int y_to_bottom, float *boxes, epnet_stream_t stream);

/* The per-scene STABLE descending order of scores (b,n) as order (b,n) i64, the layout epnet_rpn_proposals reads, in one
 * launch of one workgroup per scene (torch.sort, lib/rpn/proposal_layer.py:35, leaves the order of equal scores open). The key
 * rule is epnet_rcnn_detections': compared as floats, -0.0 == +0.0, a NaN ranks before every number, EQUAL scores in ASCENDING
 * index. No float atomics: the result depends on the inputs alone. 1 <= n <= 16384 and b <= 65535, else EPNET_ELIMIT before
 * the launch; b == 0 returns EPNET_OK; a NULL pointer: EPNET_EINVAL. */
int epnet_score_order(int b, int n, const float *scores, int64_t *order, epnet_stream_t stream);

/* lib/net/point_rcnn.py:44-52 with lib/rpn/proposal_layer.py:23-55 for the whole batch in one call with no host
 * synchronisation, no allocation and no state: scores (b,n) = rpn_cls[:, :, 0], rpn_reg (b,n,channels), xyz (b,n,3), the decode
 * parameters of epnet_decode_bbox_target (anchor_cols = 3, y_to_bottom = 1), score_thresh, and epnet_rpn_proposals' parameters.
 * Launches, fixed by the code whatever the data: ONE that decodes the boxes and writes proposals, seg_mask and pts_depth (scores
 * and xyz are read once), ONE that orders the scores (epnet_score_order), then epnet_rpn_proposals' own, unchanged: 7 with the
 * rotated NMS, 6 with the normal one. Results, every element of every given output written: ret_bbox3d (b, post_nms_top_n, 7),
 * ret_scores (b, post_nms_top_n); optional (NULL allowed): ret_count (b) i32; seg_mask (b,n) = sigmoid(score) > score_thresh as
 * 1.0 / 0.0 (a NaN score gives 0); pts_depth (b,n) = sqrt(x^2 + y^2 + z^2); proposals (b,n,7) the decoded boxes; order (b,n)
 * i64. Without a caller's buffer, proposals and order live in the workspace. 1 <= n <= 16384, b <= 32767, channels <= 255, else
 * EPNET_ELIMIT before any launch; a NULL required pointer, post_nms_top_n < 1 or a channel count that does not fit:
 * EPNET_EINVAL; a workspace below epnet_rpn_handover_workspace_bytes (pure arithmetic: (b,n,7) floats and (b,n) i64, each
 * rounded up to 16 bytes, plus epnet_rpn_proposals_workspace_bytes; 0 outside the limits): EPNET_ENOMEM; b == 0 returns EPNET_OK.
 * PRECONDITION: no output aliases an input. */
size_t epnet_rpn_handover_workspace_bytes(int b, int n, int distance_based, int pre_nms_top_n, int post_nms_top_n);
int epnet_rpn_handover(int b, int n, int channels, const float *scores, const float *rpn_reg, const float *xyz, int bins_xz,
                       int bins_y, double loc_scope, double loc_bin_size, double loc_y_scope, double loc_y_bin_size,
                       int num_head_bin, const float *anchor_size, int xz_fine, int y_by_bin, int ry_fine, int avg_by_bin,
                       int ry_with_bin, float score_thresh, int distance_based, int pre_nms_top_n, int post_nms_top_n,
                       float nms_thresh, int rotated, void *workspace, size_t workspace_bytes, float *ret_bbox3d,
                       float *ret_scores, int *ret_count, float *seg_mask, float *pts_depth, float *proposals, int64_t *order,
                       epnet_stream_t stream);

/* The end of eval_one_epoch_joint, tools/eval_rcnn.py:663-683, for all b scenes with no host synchronisation: score
 * threshold, sort, rotated NMS, gather. boxes3d (b,m,7) decoded boxes, raw_scores / norm_scores (b,m). Per scene the
 * candidates are the ROIs with norm_scores > score_thresh (a NaN is never one), ordered by DESCENDING raw_scores compared
 * as floats (-0.0 == +0.0; a NaN raw score ranks before every number, as torch.sort(descending=True) places it), EQUAL
 * scores in ASCENDING ROI index (torch.sort leaves that open; this op fixes it). Rotated NMS (nms_gpu) at nms_thresh over
 * their BEV boxes [x - l/2, z - w/2, x + l/2, z + w/2, ry] (kitti_utils.boxes3d_to_bev_torch :137-150). Results:
 * det_boxes3d (b,m,7) the kept boxes (copies of the input rows) and det_scores (b,m) their RAW scores in kept order, zero
 * rows behind; det_count (b) i32 how many. A scene without a candidate gives count 0 and zero rows (the reference
 * `continue`s, :667-668). 1 <= m <= 4096 and b <= 65535, else EPNET_ELIMIT before any launch; b == 0 returns EPNET_OK.
 * The workspace size depends on (b, m) only. */
size_t epnet_rcnn_detections_workspace_bytes(int b, int m);
int epnet_rcnn_detections(int b, int m, const float *boxes3d, const float *raw_scores, const float *norm_scores,
                          float score_thresh, float nms_thresh, void *workspace, size_t workspace_bytes,
                          float *det_boxes3d, float *det_scores, int *det_count, epnet_stream_t stream);

/* The recall and segmentation counts of eval_one_epoch_joint, tools/eval_rcnn.py:598-632, for all b scenes in one call with no
 * host synchronisation, no allocation and no float atomics (the reference trims the ground truth on the host, calls
 * boxes_iou3d_gpu twice per scene and reads eleven scalars back). pred_boxes3d (b,m,7) the refined boxes; roi_boxes3d (b,m,7)
 * the ROIs, or NULL (the ROI counters are then written as 0); gt_boxes3d (b,g,gc), 7 <= gc <= 16, zero-padded as collate_batch
 * pads (may be NULL when g == 0); thresholds: nt <= 8 floats in HOST memory, copied at the call (they travel by value in the
 * kernel arguments: the call is graph-capturable); seg_result / rpn_cls_label (b,n) i32, both NULL together with seg_counts
 * (RPN.FIXED). Per scene:
 *   padding (:600-607): num_gt = 1 + the last row whose fp32 sum over all gc columns, taken in ascending column order, is not
 *     0; zero rows in front of it stay (boxes with IoU 0). A scene WITHOUT such a row contributes nothing (:606, tmp_idx < 0):
 *     num_gt 0, all its counters 0.
 *   iou[i,j] for i < m, j < num_gt: the 3-D IoU of (box_i, gt_j), bit for bit epnet_boxes_iou3d's value, for both box sets.
 *   gt_max[j] = max over i of iou[i,j] (:611, :622); a NaN IoU wins over every number, as torch.max propagates it.
 *   recalled[t] = the number of j < num_gt with gt_max[j] > thresholds[t]: strict, in fp32, against the float the caller passed
 *     (a NaN maximum is recalled at no threshold), for the refined set and for the ROI set (:614-615, :624-625).
 * Over the WHOLE batch tensor, as :628-630 does inside its per-scene loop: correct = the elements with label > 0 and seg ==
 * label, fg = those with label > 0, pos = those with seg > 0.
 * Results, every element of every given output written: scene_stats (b, 1 + 2 nt) i32 = [num_gt, recalled_refined[nt],
 * recalled_roi[nt]]; seg_counts (3) i64 = [correct, fg, pos], NULL exactly when the segmentation inputs are; optional (NULL
 * allowed): totals (1 + 2 nt) i64, the caller's running epoch sums, to which the column sums of scene_stats are ADDED (integer
 * adds: their order does not matter); gt_max_pred / gt_max_roi (b,g), 0 in the columns at or beyond num_gt (gt_max_roi: all 0
 * without roi_boxes3d); pred_max_iou (b,m) = max over j < num_gt of iou[i,j] for the refined boxes (refined_iou of :612, NaN
 * wins), 0 where the scene has no ground truth. Limits, checked before any launch: 1 <= m <= 4096, g >= 0, b <= 65535, nt <= 8,
 * else EPNET_ELIMIT; a NULL required pointer, gc out of range, or seg_counts given without its inputs (or the reverse):
 * EPNET_EINVAL; a workspace below epnet_eval_recall_workspace_bytes(b, m, g) (pure arithmetic: the per-workgroup segmentation
 * sums, the (b,2,g) column maxima and the (b,g,m) IoU matrix of the refined boxes, each rounded up to 16 bytes; 0 outside the
 * limits): EPNET_ENOMEM; b == 0 returns EPNET_OK and writes nothing. PRECONDITION: no output may alias an input. */
size_t epnet_eval_recall_workspace_bytes(int b, int m, int g);
int epnet_eval_recall(int b, int m, int g, int gc, int n, int nt, const float *thresholds, const float *pred_boxes3d,
                      const float *roi_boxes3d, const float *gt_boxes3d, const int *seg_result, const int *rpn_cls_label,
                      void *workspace, size_t workspace_bytes, int *scene_stats, int64_t *seg_counts, int64_t *totals,
                      float *gt_max_pred, float *gt_max_roi, float *pred_max_iou, epnet_stream_t stream);

/* save_kitti_format, tools/eval_rcnn.py:76-101, for all b scenes in ONE launch: the KITTI result records of the boxes instead of
 * a text file per scene. boxes3d (b,m,7) [x,y,z,h,w,l,ry], scores (b,m); count (b) i32 on the device or NULL: with a count only
 * the first min(max(count[k], 0), m) rows of scene k are boxes (epnet_rcnn_detections' det_count), with NULL all m rows are
 * (--save_result on ROIs and refined boxes); P2 (b,3,4) f32 the camera matrix of each scene, img_shape (b,2) i32 = [h, w].
 * All arithmetic is fp32 in source order without contraction; cos / sin / atan2 are correctly rounded via double, divisions
 * correctly rounded, pi is the fp32 constant, sign(0) = 0 (the conventions of epnet_roipool3d_train). Per box:
 *   corners (kitti_utils.py:66-103), k = 0..7: xc = (l/2, l/2, -l/2, -l/2, l/2, l/2, -l/2, -l/2), yc = (0, 0, 0, 0, -h, -h, -h, -h),
 *     zc = (w/2, -w/2, -w/2, w/2, w/2, -w/2, -w/2, w/2), c = cos(ry), s = sin(ry),
 *     X = x + (xc * c + zc * s), Y = y + yc, Z = z + (xc * (-s) + zc * c).
 *   projection (calibration.py:106-118): p_r = ((X * P[r][0] + Y * P[r][1]) + Z * P[r][2]) + P[r][3], u = p_0 / p_2, v = p_1 / p_2.
 *   image box: (min u, min v, max u, max v) over the eight corners, a NaN propagating as np.min does; then x1, x2 clipped to
 *     [0, w - 1] and y1, y2 to [0, h - 1] (a NaN stays).
 *   validity (:85-87): (x2 - x1) < (float)(w * 0.8) && (y2 - y1) < (float)(h * 0.8), the products in double as Python's and
 *     rounded to fp32; a row with a NaN image coordinate is not valid.
 *   alpha (:94-96): beta = atan2(z, x), alpha = ((-sign(beta) * pi) / 2 + beta) + ry (epnet_roipool3d_train's formula, in fp32:
 *     DESIGN.md "Evaluation epoch").
 *   text round trip: each value of [alpha, x1, y1, x2, y2, h, w, l, x, y, z, ry, score] becomes r4(v) = rint((double)v * 1e4) /
 *     1e4 in double (csrc/r4.h): exactly the double that printing v with %.4f and parsing the text back gives; non-finite values
 *     pass through.
 * Results: records (b,m,13) f64 = the valid rows of each scene, compacted in input order, zero rows behind; rec_count (b) i32;
 * optional (NULL allowed) bbox_raw (b,m,4) f32 = the clipped, unrounded image boxes of ALL rows and valid (b,m) i32, both zero in
 * the rows at or beyond the count. Every element of every given output is written. 1 <= m <= 4096 and b <= 65535, else
 * EPNET_ELIMIT before the launch; b == 0 returns EPNET_OK. PRECONDITION: no output may alias an input. */
int epnet_kitti_records(int b, int m, const float *boxes3d, const float *scores, const int *count, const float *P2,
                        const int *img_shape, double *records, int *rec_count, float *bbox_raw, int *valid,
                        epnet_stream_t stream);

/* bytes of device scratch epnet_nms / epnet_nms_normal need for `boxes_num` boxes */
size_t epnet_nms_workspace_bytes(int boxes_num);

/* nms_gpu, iou3d.cpp:73-120 (nmsLauncher iou3d_kernel.cu:374-379 + the host sweep :100-116).
 * boxes (N,5) sorted by descending score. The suppression bit-mask and the greedy sweep both
 * run on the device: keep (N) i64 device array receives the kept positions in increasing order,
 * *num_keep (device i32) their count. The caller copies those back if it wants the reference's
 * host-side `keep` (the Python shim does). */
int epnet_nms(const float *boxes, int boxes_num, float nms_overlap_thresh, void *workspace,
              size_t workspace_bytes, int64_t *keep, int *num_keep, epnet_stream_t stream);

/* nms_normal_gpu, iou3d.cpp:123-170 (axis-aligned IoU of the [x1,y1,x2,y2] part, iou3d_kernel.cu:295-303) */
int epnet_nms_normal(const float *boxes, int boxes_num, float nms_overlap_thresh, void *workspace,
                     size_t workspace_bytes, int64_t *keep, int *num_keep, epnet_stream_t stream);

/* ----------------------------------------------------------------------------------------
 * roipool3d (lib/utils/roipool3d/src/roipool3d.cpp:198-203); boxes3d are (.,7) [x,y,z,h,w,l,ry]
 * -------------------------------------------------------------------------------------- */

size_t epnet_roipool3d_workspace_bytes(int batch_size, int boxes_num, int sampled_pts_num);

/* roipool3dLauncher, roipool3d_kernel.cu:209-237 (also serves forward_slow, :197-206: same result).
 * xyz (B,N,3), boxes3d (B,M,7), pts_feature (B,N,C) -> pooled_features (B,M,S,3+C) f32,
 * pooled_empty_flag (B,M) i32. Rows of empty boxes are left untouched and the flag of non-empty
 * boxes is left untouched, as in the reference (caller zero-fills both, roipool3d_utils.py:21-23). */
int epnet_roipool3d(int batch_size, int pts_num, int boxes_num, int feature_in_len,
                    int sampled_pts_num, const float *xyz, const float *boxes3d,
                    const float *pts_feature, float *pooled_features, int *pooled_empty_flag,
                    void *workspace, size_t workspace_bytes, epnet_stream_t stream);

/* roipool3d_gpu + the canonical transformation of RCNNNet.forward's eval branch (lib/net/rcnn_net.py:151-164) in ONE launch
 * that writes every element of both outputs (no zero-fill by the caller). rois (B,M,7) are the ROIs as given: the
 * kernel enlarges them itself for the membership test (kitti_utils.enlarge_box3d :153-163: h, w, l + 2 * extra, y + extra),
 * so the choice of the S rows and the feature columns are exactly epnet_roipool3d's on the enlarged boxes. The xyz columns
 * of a sampled point p for the ROI [x, y, z, h, w, l, ry] are, in fp32 and source order without contraction,
 *   dx = p.x - x, dy = p.y - y, dz = p.z - z, c = (float)cos((double)ry), s = (float)sin((double)ry),
 *   (dx * c + dz * (-s), dy, dx * s + dz * c)
 * (the subtraction of :155, rotate_pc_along_y_torch :45-63). An empty box: flag 1, all S rows hold the same formula with
 * p = 0 (what the reference's zero rows become) and 0 in the feature columns; a non-empty box: flag 0. Limits as
 * epnet_roipool3d, checked before the launch. */
int epnet_roipool3d_canonical(int batch_size, int pts_num, int boxes_num, int feature_in_len, int sampled_pts_num,
                              float pool_extra_width, const float *xyz, const float *rois, const float *pts_feature,
                              float *pooled_features, int *pooled_empty_flag, epnet_stream_t stream);

/* The tail of ProposalTargetLayer.forward (lib/rpn/proposal_target_layer.py:16-83) in ONE launch: roipool3d_gpu on the
 * enlarged ROIs, data_augmentation (:292-349) per ROI, the canonical transformation (:51-62) and the labels (:64-73).
 * xyz (B,N,3), pts_feature (B,N,C); rois (B,R,7), gt_of_rois (B,R,7) and roi_iou (B,R) as epnet_rcnn_sample_rois returns them;
 * aug (B,R,3) = [angle, scale, flip (+1 / -1)] per ROI, or NULL (AUG_DATA False: no augmentation step at all).
 * Membership and the choice of the S rows are exactly epnet_roipool3d_canonical's on the ROI as given. All arithmetic below
 * is fp32 in source order without contraction; cos / sin / atan2 are correctly rounded via double; pi and 2 pi are the fp32
 * constants; sign(0) = 0.
 *   box rule, applied to the ROI and to its ground-truth row [x, y, z, h, w, l, ry] (with aug):
 *     beta = atan2(z, x), alpha = ((-sign(beta) * pi) / 2 + beta) + ry, ca = cos(angle), sa = sin(angle),
 *     x' = x * ca + z * (-sa), z' = x * sa + z * ca, beta' = atan2(z', x'), ry' = ((sign(beta') * pi) / 2 + alpha) - beta',
 *     columns 0..5 times scale, x times flip, ry'' = [flip == 1] * ry' + [flip == -1] * (sign(ry') * pi - ry').
 *   a sampled point p (with aug): x1 = p.x * ca + p.z * (-sa), z1 = p.x * sa + p.z * ca, q = ((x1 * scale) * flip, p.y * scale,
 *     z1 * scale); without aug q = p. With the augmented ROI A: d = q - A.centre, c = cos(A.ry), s = sin(A.ry),
 *     sampled_pts row = (d.x * c + d.z * (-s), d.y, d.x * s + d.z * c).
 *   ground truth G (augmented): m = A.ry mod 2 pi (the sign of the divisor, torch's %), e = G.centre - A.centre,
 *     gt_out = (e.x * cos m + e.z * (-sin m), e.y, e.x * sin m + e.z * cos m, G.h, G.w, G.l, G.ry - m).
 *   labels: valid = the box holds a point; reg_valid_mask = roi_iou > reg_fg_thresh && valid; cls_label = roi_iou >
 *     cls_fg_thresh, -1 where cls_bg_thresh < roi_iou < cls_fg_thresh, -1 where not valid.
 *   mask_score = the sum of feature column 0 over the S rows (per-thread partial sums of rows t, t + 256, ..., folded by a
 *     butterfly over each wave and then over the 4 waves in order: fixed) divided by S; 0 when C == 0.
 * Results, each a contiguous tensor of its own: sampled_pts (B*R,S,3), pts_feature_out (B*R,S,C), rois_out (B*R,7) augmented,
 * gt_out (B*R,7) canonical, cls_label (B*R) i32, reg_valid_mask (B*R) i32, mask_score (B*R), pooled_empty_flag (B,R) i32.
 * An empty ROI: flag 1, all S rows hold the point formula with p = 0 (what the reference's zero rows become), features 0,
 * class -1, mask score 0. Every element of every output is written. Limits as epnet_roipool3d, checked before the launch. */
int epnet_roipool3d_train(int batch_size, int pts_num, int boxes_num, int feature_in_len, int sampled_pts_num,
                          float pool_extra_width, float reg_fg_thresh, float cls_fg_thresh, float cls_bg_thresh,
                          const float *xyz, const float *pts_feature, const float *rois, const float *gt_of_rois,
                          const float *roi_iou, const float *aug, float *sampled_pts, float *pts_feature_out,
                          float *rois_out, float *gt_out, int *cls_label, int *reg_valid_mask, float *mask_score,
                          int *pooled_empty_flag, epnet_stream_t stream);

/* ----------------------------------------------------------------------------------------
 * training losses (lib/net/train_functions.py:92-284 over lib/utils/loss_utils.py:79-350)
 * -------------------------------------------------------------------------------------- */

/* get_rpn_loss / get_rcnn_loss with get_reg_loss and the classification loss, forward and backward in one call, for `rows`
 * rows (points of the RPN, ROIs of the RCNN stage) with no host synchronisation: the reference selects the foreground rows by
 * boolean masks, branches on their count on the host and reads some 25 scalars back per step.
 * pred_reg (rows, c), c = 4 nb + 1 + 2 num_head_bin + 3 with nb = (int)(loc_scope / loc_bin_size) * 2, columns
 * [x_bin nb | z_bin nb | x_res nb | z_res nb | y_offset | ry_bin nh | ry_res nh | size 3] (get_xz_fine, y by offset);
 * cls_logit (rows); reg_label (rows, 7) [dx, dy, dz, h, w, l, ry]; cls_label (rows) i32: -1 ignored, 0 negative, > 0 positive;
 * reg_mask (rows) i32 or NULL: the foreground rows are reg_mask > 0 (NULL: cls_label > 0); iou_branch_pred (rows) or NULL:
 * the USE_IOU_BRANCH term (loss_utils.py:263-269); anchor (3) = CLS_MEAN_SIZE; ry_fine: get_ry_fine (RCNN) or not (RPN).
 * Regression terms are sums over the foreground rows divided by max(count, 1): without a foreground row they are exactly 0
 * with zero gradients. The scalars are those of the Python calls (doubles that meet fp32 tensors).
 *   terms (EPNET_BOX_LOSS_TERMS floats), in this order: total = loss * w_train; loss = loss_cls * w_cls + loss_reg * w_reg;
 *     loss_cls, its positive and negative parts (focal only); loss_reg = loc + angle + size + iou + iou_branch; loss_loc;
 *     loss_angle; loss_size (x 3); loss_iou (x ce_weight); loss_x_bin, z_bin, x_res, z_res, y_offset, ry_bin, ry_res;
 *     iou_branch_loss; the counts of foreground, positive, negative and valid (label >= 0) rows as floats (exact below 2^24);
 *     loss_size and loss_iou without the callers' weights (the entries of reg_loss_dict).
 *   grad_cls (rows), grad_reg (rows, c), grad_iou_branch (rows; NULL exactly when iou_branch_pred is): d total / d input,
 *     every element written (zero rows for background).
 * Sums over rows are folded in a fixed order without float atomics: the bits depend on the inputs and the shape alone.
 * workspace: 16-byte aligned, epnet_box_loss_workspace_bytes(rows, c) = 4096 + ceil(rows / 64) * 64 bytes. nb and
 * num_head_bin up to 32, else EPNET_ELIMIT; rows == 0 returns EPNET_OK and writes nothing. */
#define EPNET_BOX_LOSS_TERMS 24
#define EPNET_LOSS_IOU_RAW 0
#define EPNET_LOSS_IOU_CLS_MASK_WITH_BIN 1
#define EPNET_LOSS_CLS_FOCAL 0  /* SigmoidFocalLoss: weights (pos + neg) / max(sum pos, 1), focal_alpha, focal_gamma */
#define EPNET_LOSS_CLS_BCE 1    /* BinaryCrossEntropy: fg_weight on the positive rows, mean over the valid rows */
#define EPNET_LOSS_CLS_NONE 2   /* no classification term (the caller adds its own, e.g. DiceLoss) */
size_t epnet_box_loss_workspace_bytes(long long rows, int c);
int epnet_box_loss(long long rows, int c, double loc_scope, double loc_bin_size, int num_head_bin, int ry_fine,
                   int iou_loss_type, int cls_loss_type, double focal_alpha, double focal_gamma, double fg_weight,
                   double w_cls, double w_reg, double w_train, double ce_weight, const float *cls_logit,
                   const float *pred_reg, const float *reg_label, const int *cls_label, const int *reg_mask,
                   const float *iou_branch_pred, const float *anchor, float *terms, float *grad_cls, float *grad_reg,
                   float *grad_iou_branch, void *workspace, size_t workspace_bytes, epnet_stream_t stream);

/* ----------------------------------------------------------------------------------------
 * RPN training targets (lib/datasets/kitti_rcnn_dataset.py:378-408: data_augmentation :698-755,
 * generate_rpn_training_labels :547-576)
 * -------------------------------------------------------------------------------------- */

/* The loader's augmentation and per-point RPN labels of a whole batch in ONE launch with no host synchronisation: the
 * reference runs them per scene on a host core (two scipy Delaunay point-in-hull tests per box over all points).
 * pts (b,n,3); gt_boxes3d (b,g,7) [x,y,z,h,w,l,ry], zero-padded as collate_batch pads; gt_alpha (b,g), zero where the row is
 * padding (NULL allowed when aug is NULL); aug (b,4) = [rotate 0/1, angle, scale, flip 0/1] per scene, or NULL for no augmentation; extra_width >= 0: the
 * ignore margin (the reference uses 0.2).
 * Augmentation, per scene, in the reference's order (stage 1): with rotate != 0, x' = x cos a - z sin a, z' = x sin a +
 * z cos a for the points and the box centres, evaluated in double from the fp32 inputs and the angle and rounded once
 * (rotate_pc_along_y's float64 np.dot), then ry' = sign(beta) * pi / 2 + gt_alpha - beta with beta = atan2(z', x') in fp32
 * (with rotate == 0 the incoming ry is kept: a rotation by 0 is not the identity on ry); all point coordinates and box
 * columns 0..5 times scale in fp32 (1 = off); with flip != 0, x = -x and ry = sign(ry) * pi - ry. Zero rows stay zero.
 * Labels, from the augmented values: a row is a box when h, w and l are all > 0. With c = (x, y - h/2, z), d = p - c,
 * lx = d.x cos ry + d.z (-sin ry), lz = d.x sin ry + d.z cos ry (fp32, source order, no contraction; cos / sin correctly
 * rounded via double, as epnet_roipool3d's predicate), a point is in the box when |lx| <= l/2, |d.y| <= h/2, |lz| <= w/2 and
 * in the enlarged box (kitti_utils.enlarge_box3d: h, w, l + 2 extra_width about the same centre) when the same holds with
 * (l + 2e)/2, (h + 2e)/2, (w + 2e)/2. With the boxes in ascending row order, as the reference's loop:
 *   cls_label (b,n) i32: decided by the LAST box whose enlarged form holds the point -- 1 if that box itself holds it, else
 *     -1; 0 if none does;
 *   reg_label (b,n,7): decided by the LAST box that holds the point, independently of the class (a later box's margin may
 *     turn the class to -1 and the row stays): [c - p, h, w, l, ry]; zeros if none does.
 * A NaN coordinate is in no box: class 0, zero row. g == 0 is valid (all labels zero); any g works (the kernel takes the
 * boxes 64 at a time). pts_out (b,n,3) and gt_out (b,g,7) receive the augmented values; both may be NULL when aug is NULL
 * (given there, they receive copies). Every element of every output is written. No atomics: the bits depend on the inputs
 * alone. PRECONDITION: no output may alias an input (pts_out != pts, gt_out != gt_boxes3d; every workgroup of a scene
 * reads all of that scene's box rows). b == 0 or n == 0 returns EPNET_OK and writes nothing; b > 65535 is EPNET_ELIMIT
 * before any launch. */
int epnet_rpn_targets(int b, int n, int g, float extra_width, const float *pts, const float *gt_boxes3d,
                      const float *gt_alpha, const float *aug, float *pts_out, float *gt_out, int *cls_label,
                      float *reg_label, epnet_stream_t stream);

/* ----------------------------------------------------------------------------------------
 * RPN inputs from the raw scans (lib/datasets/kitti_rcnn_dataset.py:281-356, the first half of get_rpn_with_li_fusion:
 * Calibration.lidar_to_rect / rect_to_img, lib/utils/calibration.py:51-70; get_valid_flag :229-251; the sampling to npoints
 * :325-346; get_image_rgb_with_normal, lib/datasets/kitti_dataset.py:37-57)
 * -------------------------------------------------------------------------------------- */

/* The loader's transform, view / scope filter and sampling to n points for a whole batch, with no host synchronisation: the
 * reference runs them per scene on a host core and draws from numpy's stream; here the draws are device tables, so nothing
 * is read back. pts_lidar (b,p,4) [x, y, z, intensity] in the velodyne frame, 16-byte aligned, scene k's rows at or beyond
 * num_raw[k] are padding (num_raw (b) i32 on the device, clamped to [0, p]); V2C (b,3,4), R0 (b,3,3), P2 (b,3,4) f32 the
 * calibration of each scene; img_shape (b,2) i32 = [h, w]; keys (b,p) i32, compared as UNSIGNED, one draw per raw point;
 * slot_perm (b,n) i32, a permutation of 0..n-1 per scene, or NULL; scope = 6 doubles in HOST memory [x0, x1, y0, y1, z0, z1]
 * (PC_AREA_SCOPE row-major; NULL allowed when reduce_by_range == 0), copied at the call; near_depth: the reference's 40.0.
 * Per raw point, all arithmetic fp32 in source order without contraction, divisions correctly rounded (the conventions of
 * epnet_kitti_records):
 *   composite matrix: M[k][j] = (V2C[0][k] * R0[j][0] + V2C[1][k] * R0[j][1]) + V2C[2][k] * R0[j][2], k = 0..3, j = 0..2;
 *   rectified coordinate: rect_j = ((x * M[0][j] + y * M[1][j]) + z * M[2][j]) + M[3][j], (X, Y, Z) = rect;
 *   projection: p_r = ((X * P2[r][0] + Y * P2[r][1]) + Z * P2[r][2]) + P2[r][3]; u = p_0 / Z, v = p_1 / Z -- the divisor is
 *     the rectified Z, not p_2 (calibration.py:68); depth = p_2 - P2[2][3];
 *   valid: u >= 0 && u < (float)w && v >= 0 && v < (float)h && depth >= 0, and with reduce_by_range != 0 also
 *     scope[2j] <= (double)rect_j <= scope[2j+1] for j = 0..2, both ends inclusive. The comparison is in double, as numpy
 *     (NEP 50) compares a float32 array with PC_AREA_SCOPE's float64 entries; legacy value-based casting compared in
 *     float32 and differs only for a coordinate equal to (float)70.4 (which is above 70.4 and is outside here). A NaN
 *     anywhere makes the point invalid, and so is every row at or beyond num_raw;
 *   a valid point is NEAR when Z < near_depth and FAR otherwise.
 * Selection (:325-346). V = the valid points of the scene, F = the far ones. "The r smallest of a set" means smallest by
 * (unsigned key, raw index): equal keys go to the lower raw index. The list L has length n: q copies of a forced set S0,
 * each copy in raw order, then the r smallest of a candidate set S1 in raw order:
 *   case 0: V > n and F <= n                S0 = far, q = 1          S1 = near, r = n - F
 *   case 5: F > n (the reference raises)    S0 = none                S1 = far, r = n
 *   case 1: V == n, case 2: n/2 <= V < n    S0 = valid, q = 1        S1 = valid, r = n - V
 *   case 3: 0 < V < n/2 (ref. raises)       S0 = valid, q = n div V  S1 = valid, r = n mod V
 *   case 4: V == 0 (the reference raises)   every output row zero, choice -1
 * (n/2 is the exact half: case 2 is 2 V >= n.) In cases 0, 1 and 2 uniform keys give the reference's distribution:
 * np.random.choice(replace = False) is a uniform r-subset, np.random.shuffle is slot_perm. Output row slot_perm[k][j]
 * receives point L[j] (row j with NULL). PRECONDITION, not checked: slot_perm is a permutation per scene (an entry outside
 * [0, n) writes nothing, a repeated one leaves a row unwritten). Cost: case 3 writes its q copies of a forced point one
 * after the other from one lane, O(q) per point (q = n with a single valid point): correct, and slow only on the degenerate
 * scenes the reference raises on. get_rpn_sample without LI-Fusion is the same rule without
 * pts_origin_xy and is served by this call.
 * Outputs, per row: pts_rect (b,n,3) the rectified xyz; pts_intensity (b,n) = intensity - 0.5f; pts_origin_xy (b,n,2) the raw
 * (u, v) (pointnet2_msg.py:208-210 normalises them later); pts_input (b,n,4) = [xyz, intensity - 0.5] or NULL; choice (b,n) i32
 * the raw index; scene_info (b,6) i32 = [num_raw clamped, V, F, case, r, q]. Every element of every given output is written.
 * No float atomics: the bits depend on the inputs alone. Nothing is allocated, nothing synchronises, and the launches are
 * four whatever the data. PRECONDITION: no output may alias an input or another output. workspace: at least
 * epnet_scan_prepare_workspace_bytes(b, p, n) bytes, 8-byte aligned, contents irrelevant before and after (too small:
 * EPNET_ENOMEM). 1 <= n <= 65536, 1 <= p <= 1048576, b <= 65535, else EPNET_ELIMIT before any launch (and 0 from the size
 * query); b == 0 returns EPNET_OK; a NULL required pointer or a misaligned pts_lidar / workspace: EPNET_EINVAL. */
size_t epnet_scan_prepare_workspace_bytes(int b, int p, int n);
int epnet_scan_prepare(int b, int p, int n, int reduce_by_range, const double *scope, float near_depth,
                       const float *pts_lidar, const int *num_raw, const float *V2C, const float *R0, const float *P2,
                       const int *img_shape, const int *keys, const int *slot_perm, void *workspace,
                       size_t workspace_bytes, float *pts_rect, float *pts_intensity, float *pts_origin_xy,
                       float *pts_input, int *choice, int *scene_info, epnet_stream_t stream);

/* get_image_rgb_with_normal for b scenes from the 8-bit image, in the layout and type the network takes after model_fn's
 * .float() and permute: img (b,h_in,w_in,3) u8 RGB on the device, out (b,3,h_out,w_out) f32;
 *   out[k][c][y][x] = (float)((((double)img[k][y][x][c] / 255.0) - mean[c]) / std[c]) for y < min(h_k, h_out), x < min(w_k, w_out),
 * and 0 elsewhere -- the reference's float64 expression rounded once; h_k, w_k = img_shape[k] ((b,2) i32 = [h, w] on the
 * device, clamped to [0, h_in] x [0, w_in]) or h_in, w_in with NULL. mean and std are 3 doubles each in HOST memory, copied
 * at the call. One launch, 16-byte stores when w_out % 4 == 0 and out is 16-byte aligned. Every element of out is written.
 * b > 65535 or an image of more than 2^31 / 3 pixels: EPNET_ELIMIT; b == 0 returns EPNET_OK. PRECONDITION: out does not
 * alias img. */
int epnet_image_normalise(int b, int h_in, int w_in, int h_out, int w_out, const uint8_t *img, const int *img_shape,
                          const double *mean, const double *std, float *out, epnet_stream_t stream);

/* ----------------------------------------------------------------------------------------
 * GT-database augmentation of the point-only loader (lib/datasets/kitti_rcnn_dataset.py:590-696, apply_gt_aug_to_one_scene,
 * called from get_rpn_sample :443-455, :506-509; the box geometry of lib/utils/kitti_utils.py:66-103 and :198-238)
 * -------------------------------------------------------------------------------------- */
#define EPNET_GT_AUG_MAX_TRIES 128     /* tries per scene (the reference uses 100) */
#define EPNET_GT_AUG_MAX_EXISTING 224  /* rows of all_gt_boxes3d per scene */
#define EPNET_GT_AUG_MAX_ACCEPT 32     /* accepted objects per scene (k_max) */

/* The reference's placement loop for b scenes in one launch (one wave per scene), the random decisions given as device tables.
 * The database: db_boxes (D,7) f32 [x, y, z, h, w, l, ry], db_alpha (D) f32, db_npts (D) i32. Tables: apply (b) i32, extra_num
 * (b) i32 (used as min(extra_num, k_max - 1); extra_max is the caller's bound on it and must be below k_max), cand (b,T) i32
 * the database row of each try. The scene: all_boxes (b,a,7) with num_all (b) rows (every labelled object, for the overlap
 * test), gt_boxes (b,g,7) / gt_alpha (b,g) with num_gt (b) rows (the label rows), road_plane (b,4) f64 [a, b, c, d]; counts
 * are clamped to their capacity. scope as for epnet_scan_prepare. Per scene with apply != 0, tries t = 0..T-1 in order:
 *   1. stop when cnt > extra_num;
 *   2. with reduce_by_range, skip the candidate when its centre (x, y, z) is outside scope (compared in double, both ends
 *      inclusive); a row outside [0, D) is skipped likewise;
 *   3. skip it when db_npts < 5;
 *   4. cur_height = ((-d - a * (double)x) - c * (double)z) / b; move = (double)y - cur_height; y' = (float)((double)y - move);
 *   5. cnt += 1;
 *   6. reject it (info[5]) when it overlaps a current box: the scene's all_boxes rows with w + 0.5f, l + 0.5f, then the
 *      accepted candidates in the same form. Two boxes overlap when their vertical intervals [y - h, y] share a positive length
 *      and overlap3d / union3d >= 1e-8, all in double on the float32 box values: the BEV rectangle has the corners
 *      (x + dx cos ry + dz sin ry, z - dx sin ry + dz cos ry), dx = +-l/2, dz = +-w/2; overlap3d = shared area * shared
 *      height, union3d = area_a * h_a + area_b * h_b - overlap3d (get_iou3d). A box with w or l of 0 shares no area. With no
 *      current box the candidate is accepted;
 *   7. reject it (info[6]) when k_max objects are accepted or its points do not fit in what is left of e rows;
 *   8. else accept: [x, y', z, h, w + 0.5f, l + 0.5f, ry] joins the current boxes, [x, y', z, h + 2.0f, w, l, ry] is its
 *      removal box, [x, y', z, h, w, l, ry] with db_alpha its label row, and its points take rows row0 .. row0 + npts of the
 *      scene's extra rows, row0 the points accepted before it.
 * The reference lowers the database object itself (obj.pos, :656), so a second use in one worker drifts; here the label is
 * always the placed box. Outputs, every element written: acc_db (b,k_max) i32 the database row, -1 behind the count; acc_box
 * (b,k_max,7), acc_move (b,k_max) f64, acc_row0 (b,k_max) i32, remove_boxes (b,k_max,7), zeros behind; gt_out (b,g+k_max,7)
 * and alpha_out (b,g+k_max): the num_gt label rows, the accepted boxes directly behind them, zeros behind; info (b,8) i32 =
 * [applied, extra_num, tries used, cnt, accepted, overlap rejections, capacity rejections, extra points]. T <=
 * EPNET_GT_AUG_MAX_TRIES, a <= EPNET_GT_AUG_MAX_EXISTING, 1 <= k_max <= EPNET_GT_AUG_MAX_ACCEPT, extra_max < k_max,
 * e <= 1048576, D >= 1, b <= 65535, else EPNET_ELIMIT before the launch; b == 0 returns EPNET_OK. */
int epnet_gt_aug_place(int b, int T, int a, int g, int k_max, int e, int D, int extra_max, int reduce_by_range,
                       const double *scope, const float *db_boxes, const float *db_alpha, const int *db_npts,
                       const int *apply, const int *extra_num, const int *cand, const float *all_boxes, const int *num_all,
                       const float *gt_boxes, const float *gt_alpha, const int *num_gt, const double *road_plane,
                       int *acc_db, float *acc_box, double *acc_move, int *acc_row0, float *remove_boxes, float *gt_out,
                       float *alpha_out, int *info, epnet_stream_t stream);

/* The accepted objects' points in one launch: db_points (S,4) f32 [x, y, z, intensity] packed, object d at rows db_offsets[d]
 * .. db_offsets[d+1] (db_offsets (D+1) i32); acc_db, acc_move, acc_row0, info as epnet_gt_aug_place wrote them. extra_pts
 * (b,e,4): row acc_row0[k] + i of scene s is point i of its k-th accepted object with y = (float)((double)y - acc_move[k]);
 * rows at or beyond info[7] are zero. Every element is written. 16-byte row loads and stores when db_points and extra_pts are
 * 16-byte aligned, scalar ones otherwise. e == 0 or b == 0 returns EPNET_OK. */
int epnet_gt_aug_points(int b, int e, int k_max, int D, int S, const float *db_points, const int *db_offsets,
                        const int *acc_db, const double *acc_move, const int *acc_row0, const int *info, float *extra_pts,
                        epnet_stream_t stream);

/* epnet_scan_prepare over the index space [0, p) raw rows then [p, p + e) extra rows; keys is (b,p+e). A raw row is valid by
 * epnet_scan_prepare's rule AND outside every one of the scene's num_remove[k * count_stride] removal boxes (remove_boxes
 * (b,k_max,7), clamped to k_max <= EPNET_GT_AUG_MAX_ACCEPT); the membership test is pt_in_box3d's as epnet_roipool3d
 * evaluates it (fp32, the 10 m gate included). An extra row (extra_pts (b,e,4) [x, y, z, intensity], rectified already,
 * 16-byte aligned) below num_extra[k * count_stride] (clamped to e) is always valid, near or far by its z; its pts_origin_xy is
 * the projection of the rectified point, its intensity column is lowered by 0.5f like a raw row's. count_stride >= 1 lets
 * both counts be read from columns 4 and 7 of epnet_gt_aug_place's info. choice >= p names extra row choice - p. scene_info
 * (b,8) i32 = [num_raw clamped, V, F, case, r, q, raw points removed, extra rows]. Four launches. With e == 0 and no removal
 * box the outputs are epnet_scan_prepare's bits. p + e <= 1048576, else as epnet_scan_prepare. */
size_t epnet_scan_prepare_aug_workspace_bytes(int b, int p, int e, int n);
int epnet_scan_prepare_aug(int b, int p, int e, int n, int k_max, int reduce_by_range, const double *scope, float near_depth,
                           const float *pts_lidar, const int *num_raw, const float *V2C, const float *R0, const float *P2,
                           const int *img_shape, const float *extra_pts, const int *num_extra, const float *remove_boxes,
                           const int *num_remove, int count_stride, const int *keys, const int *slot_perm, void *workspace,
                           size_t workspace_bytes, float *pts_rect, float *pts_intensity, float *pts_origin_xy,
                           float *pts_input, int *choice, int *scene_info, epnet_stream_t stream);

/* ---- The KITTI AP evaluator (tools/kitti_object_eval_python: rotate_iou.py:18-296, a numba.cuda kernel, and eval.py:84-332,
 * numba CPU JIT). All frames of a call are ragged: frame f owns rows *_off[f] .. *_off[f+1] of the arrays that go with the
 * offset array (F+1 int32 each) and the dt_num[f] x gt_num[f] float64 block at ov_off[f] (F+1 int64), detection-major as
 * eval.py:204 indexes it (overlaps[j, i], j = detection, i = ground truth). Nothing is padded; no kernel reads at or past
 * *_off[F]. The offsets live on the device, so the caller states the largest per-frame counts (max_*); beyond the limits
 * below the calls return EPNET_ELIMIT before any launch. These are end-of-epoch calls: asynchronous on `stream` like every
 * other entry point, but combo_* arrays are HOST memory (at most EPNET_KITTI_MAX_COMBOS entries, copied at the call). */
#define EPNET_KITTI_MAX_DT 1024        /* detections per frame */
#define EPNET_KITTI_MAX_GT 256         /* ground-truth rows per frame */
#define EPNET_KITTI_MAX_DC 256         /* DontCare boxes per frame */
#define EPNET_KITTI_MAX_COMBOS 16      /* (difficulty, min_overlap) combinations per call */
#define EPNET_KITTI_MAX_THRESHOLDS 64  /* score thresholds per combination (the evaluator uses up to 41) */

/* The per-frame blocks of calculate_iou_partly (eval.py:334-408) for one metric, rows = the frame's `boxes` (detections, as
 * eval.py:467 passes them), cols = its `query_boxes`; out[ov_off[f] + j * cols_f + i], float64.
 *   metric 0, boxes (n,4) f64: image_box_overlap (eval.py:85-111) in float64, source order; criterion -1 (IoU), 0 (over the row
 *     box's area, the DontCare pass of eval.py:247) or 1;
 *   metric 1, boxes (n,5) f64 [x, z, l, w, ry]: rotate_iou_gpu_eval(criterion -1): cast to float32, devRotateIoUEval(col, row)
 *     (rotate_iou.py:293: the query box is rbox1) in float32, source order, cos / sin correctly rounded via double; widened;
 *   metric 2, boxes (n,7) f64 [x, y, z, l, h, w, ry]: d3_box_overlap (eval.py:120-152): the float32 intersection area of columns
 *     [0,2,3,5,6], then height overlap min(y) - max(y - h), volumes and the ratio in float64, stored through float32 as the
 *     reference's `rinc` array does; criterion -1.
 * Frames with no rows or no cols write nothing. max_rows <= EPNET_KITTI_MAX_DT, max_cols <= EPNET_KITTI_MAX_GT. */
int epnet_kitti_overlaps(int metric, int criterion, int frames, int max_rows, int max_cols, const int *row_off,
                         const int *col_off, const int64_t *ov_off, const double *row_boxes, const double *col_boxes,
                         double *overlaps, epnet_stream_t stream);

/* Pass 1, compute_statistics_jit(thresh = 0, compute_fp = False) (eval.py:486-498), of every frame for every combination
 * c = (combo_difficulty[c], combo_min_overlap[c]) in one launch. ignored_gt (num_difficulty, total_gt) and ignored_dt
 * (num_difficulty, total_dt) are clean_data's tables (1 / 0 / -1) as int32; dt_score (total_dt) f64. matched (combos, total_gt)
 * f64: the matched detection's score where the reference appends one to `thresholds`, NaN elsewhere; every element is
 * written. min_overlap >= 0 (else EPNET_EINVAL). The result is that of the sequential loops: among equal scores the lowest
 * detection index wins. */
int epnet_kitti_match(int frames, int total_gt, int total_dt, int max_gt, int max_dt, int num_difficulty, int combos,
                      const int *combo_difficulty, const double *combo_min_overlap, const int *gt_off, const int *dt_off,
                      const int64_t *ov_off, const double *overlaps, const double *dt_score, const int *ignored_gt,
                      const int *ignored_dt, double *matched, epnet_stream_t stream);

/* bytes of epnet_kitti_pr's workspace (the per-frame partial sums); pure arithmetic; 0 for an empty problem or outside the limits */
size_t epnet_kitti_pr_workspace_bytes(int frames, int combos, int tstride);

/* Pass 2, fused_compute_statistics (eval.py:285-331): compute_statistics_jit(compute_fp = True) of every frame for every
 * combination c and each of its combo_num_thresholds[c] <= tstride thresholds (thresholds (combos, tstride) f64, device), in
 * one launch; the per-frame tp / fp / fn and similarity go to the workspace and a second kernel adds them in an order that
 * depends on `frames` alone (no atomics: same inputs, same bits). pr_counts (combos, tstride, 3) i32 = tp, fp, fn and
 * pr_similarity (combos, tstride) f64 (the sum of (1 + cos(gt_alpha - dt_alpha)) / 2 over the true positives, when compute_aos);
 * rows t >= combo_num_thresholds[c] are written as zeros. metric 0 runs the DontCare pass of eval.py:246-259 on dt_bbox
 * (total_dt,4) and dc_bbox (rows of dc_off, 4), both f64. A detection is dropped by a threshold when score < threshold. */
int epnet_kitti_pr(int frames, int total_gt, int total_dt, int max_gt, int max_dt, int max_dc, int num_difficulty, int combos,
                   int tstride, int metric, int compute_aos, const int *combo_difficulty, const double *combo_min_overlap,
                   const int *combo_num_thresholds, const int *gt_off, const int *dt_off, const int *dc_off,
                   const int64_t *ov_off, const double *overlaps, const double *dt_score, const int *ignored_gt,
                   const int *ignored_dt, const double *dt_bbox, const double *dc_bbox, const double *gt_alpha,
                   const double *dt_alpha, const double *thresholds, void *workspace, size_t workspace_bytes,
                   int *pr_counts, double *pr_similarity, epnet_stream_t stream);

/* ----------------------------------------------------------------------------------------
 * the optimiser step (tools/train_utils/train_utils.py:126-136: clip_grad_norm_, then fastai_optim.py:132-149 OptimWrapper.step
 * with true_wd and bn_wd over torch.optim.Adam, under learning_schedules_fastai.py:40-73 OneCycle)
 * -------------------------------------------------------------------------------------- */

/* One `adam_onecycle` training step over any number of tensors in three launches (norm partials, finish, update), with no host
 * synchronisation and no host-side scalar: the step index comes from a device counter and everything that depends on it from a
 * row table built once, so a captured graph replays the step with a new learning rate every time. The reference sets lr and
 * beta1 as Python floats per iteration, reads one .item() per parameter in the clip and launches one decay per tensor.
 *   tensor_table (tensors): where each tensor is; grad NULL = no gradient this step; state_offset = its first element in
 *     exp_avg / exp_avg_sq (two flat fp32 buffers of the caller's; a multiple of 4 keeps the 16-byte path). Frozen parameters
 *     are simply not in the table.
 *   chunk_table (chunks, 2) i32: (tensor, first element); chunk c covers min(EPNET_OPTIM_CHUNK, numel - first) elements of its
 *     tensor. Every element of every tensor belongs to exactly one chunk; one workgroup per chunk.
 *   rows (total_steps, EPNET_OPTIM_ROW) fp32, for step t = 0 .. total_steps-1, computed in double and rounded once:
 *     [decay = 1 - wd lr, b1 = mom, 1 - b1, step_size = lr / (1 - b1^(t+1)), bc2_sqrt = sqrt(1 - b2^(t+1)), lr, mom, 0] with
 *     lr[t], mom[t] the one-cycle schedule. The device evaluates no cos and no pow: the host's numbers are the definition.
 *   counter (1) i64: t is read from it and t + 1 written back. t >= total_steps uses the last row and sets the flag in stats
 *     (the reference's scheduler would run past the cosine's end; its trainer never gets there).
 * Clip: total_norm = sqrt of the sum of g^2 over every gradient present, in double (one partial per chunk, then the partials
 * in an order that depends on `chunks` alone; no float atomics: same inputs, same bits); coef = min(1, clip / (total_norm +
 * 1e-6)) in double, rounded to fp32. A partial does not depend on the gradient's alignment.
 * Update, per element, fp32 in source order without contraction, / and sqrt correctly rounded:
 *     g' = g coef;  p = p decay;  m = m b1 + (1 - b1) g';  v = v b2 + (1 - b2) g' g';
 *     p = p - step_size (m / (sqrt(v) / bc2_sqrt + eps))
 * (b2, 1 - b2 and eps rounded to fp32 from the doubles given) -- torch.optim.Adam's present form, eps outside the bias
 * correction, after the wrapper's p *= 1 - wd lr. A tensor without a gradient only decays; its state is not touched.
 * With zero_grads != 0 every gradient present is stored as zeros afterwards (the buffers persist, their addresses stay).
 * Full chunks whose p, m, v addresses are multiples of 16 move 16 bytes per lane and access; so does g where its address allows,
 * else (a gradient that is a view at an odd offset of a bucket) g alone is read and zeroed in dword accesses. A short chunk (a
 * small tensor, a tensor's last piece) or a parameter at an odd address goes element by element.
 *   stats (EPNET_OPTIM_STATS) f64: total_norm, coef, lr, mom (the row's fp32 values), the step used, 1 if t >= total_steps,
 *     then zeros.
 *   workspace: 16-byte aligned, epnet_adam_onecycle_workspace_bytes(chunks) = 64 + 8 chunks bytes (0 for chunks <= 0).
 * max_numel: the largest numel in the table (the table lives on the device); above 2^31-1: EPNET_ELIMIT. A NULL required
 * pointer, total_steps < 1, clip not > 0, eps < 0 or b2 outside [0, 1): EPNET_EINVAL; a missing or short workspace:
 * EPNET_ENOMEM; tensors == 0 or chunks == 0 returns EPNET_OK and writes nothing (the counter stays).
 * PRECONDITION: no tensor appears twice, and no parameter, gradient or state range overlaps another. */
#define EPNET_OPTIM_CHUNK 4096
#define EPNET_OPTIM_ROW 8
#define EPNET_OPTIM_STATS 8
typedef struct {
    float *param;
    float *grad;
    long long numel;
    long long state_offset;
} epnet_optim_tensor;
size_t epnet_adam_onecycle_workspace_bytes(long long chunks);
int epnet_adam_onecycle_step(int tensors, long long chunks, long long max_numel, const epnet_optim_tensor *tensor_table,
                             const int *chunk_table, const float *rows, long long total_steps, double clip, double eps,
                             double b2, int zero_grads, long long *counter, float *exp_avg, float *exp_avg_sq,
                             double *stats, void *workspace, size_t workspace_bytes, epnet_stream_t stream);

/* The same step with loss scaling and non-finite step skipping: still three launches, nothing read back, and every value that
 * changes from step to step (the scale, its growth tracker, the skip count) read from device memory, so a captured graph replays
 * it. The gradients are those of loss * scale; torch.amp.GradScaler in front of the step above costs one more read-modify-write
 * pass over every gradient and a host read of found_inf.
 *   scale (1) fp32, scaler_state (2) i64 = [growth_tracker, skipped_total], both read and written.
 * Unscaling: inv = (float)(1.0 / (double)scale[0]); every gradient enters the step as gu = g * inv, rounded to fp32, and the step
 * is the one above on gu: the norm is the float64 sum of (double)gu * (double)gu in the same order, coef comes from that norm, and
 * Adam uses g' = gu coef. The result is "g *= inv in stock fp32, then epnet_adam_onecycle_step", bit for bit, for any scale (not
 * only powers of two).
 * Detection: the step is non-finite iff the reduced float64 sum of squares is not finite -- a NaN or an infinity in any
 * gradient, or an overflow of g * inv; squares of finite floats cannot overflow a double. No extra pass, no atomics.
 * A non-finite step is skipped: parameters, exp_avg and exp_avg_sq keep their bits (no weight decay either, also for a tensor
 * without a gradient), the counter does not advance -- the schedule's row and Adam's bias corrections count APPLIED steps, as
 * with GradScaler, which skips optimizer.step() --, skipped_total += 1, and with zero_grads != 0 the gradients are still stored
 * as zeros.
 * Scale update, after the scale's value was taken for this step: torch._amp_update_scale_'s rule, the product taken in double
 * and rounded once to fp32 as there. Non-finite step: scale = max((float)(scale * backoff_factor), (float)min_scale), tracker = 0.
 * Otherwise tracker += 1, and when it equals growth_interval: scale = (float)(scale * growth_factor) if that is finite (else the
 * scale stays), tracker = 0. growth_interval == 0 is a static scale: detection, skipping and the two counts only, the scale is
 * never written (a static scale of 1.0 is a non-finite guard for bf16 / fp32 training).
 *   stats: [0..5] as above; on a skipped step [0] is the non-finite norm, [1] is 0 and [2..5] describe the row that would have
 *     been used; [6] the scale this step used, [7] skipped_total after the step.
 * Errors as above, and EPNET_EINVAL for growth_factor < 1, backoff_factor outside (0, 1], growth_interval < 0, min_scale not
 * > 0 (or any of them NaN or beyond fp32), a NULL scale or scaler_state. Workspace as above. */
int epnet_adam_onecycle_step_scaled(int tensors, long long chunks, long long max_numel, const epnet_optim_tensor *tensor_table,
                                    const int *chunk_table, const float *rows, long long total_steps, double clip, double eps,
                                    double b2, int zero_grads, long long *counter, float *exp_avg, float *exp_avg_sq,
                                    double *stats, float *scale, long long *scaler_state, double growth_factor,
                                    double backoff_factor, long long growth_interval, double min_scale, void *workspace,
                                    size_t workspace_bytes, epnet_stream_t stream);

/* LI-Fusion's image head evaluated at the points only (inference). In eval mode the end of the
 * two-stream backbone -- cat_l(DeConv_l(F_l)) -> 1x1 convolution -> batch norm -> ReLU -> bilinear sampler
 * (lib/net/pointnet2_msg.py:237-246) -- is pointwise per output pixel in front of the sampler (the deconvolutions have
 * kernel == stride), so only the pixels under the four bilinear taps of each point are evaluated and the two full-resolution
 * maps are never formed. For scene b, point n, output channel c:
 *   out[b, c, n] = sum over the in-bounds taps, in the order nw, ne, sw, se, of weight_tap * relu(shift[c] + s_c(tap))
 *   s_c(tap)     = sum_j in ascending order of wf[c, j] * d[j](tap), started from 0
 *   d(tap)       = cat_l(d_l),  d_l[r] = sum_ci in ascending order of wd_l[Y % k_l, X % k_l, ci, r] * F_l[b, ci, Y / k_l, X / k_l]
 * for the tap's pixel (Y, X); taps and weights are those of epnet_feature_gather. float32 in that order, no contraction, no
 * float atomics: a tap's value depends on its pixel, its scene's maps and the weights alone.
 *   levels: 1..8; chans[l] = C_l >= 1, kernels[l] = k_l in {1, 2, 4, 8, 16}, each dividing the largest; reduce[l] = R_l >= 1
 *     (host arrays of `levels` ints); h, w multiples of the largest kernel
 *   maps[l]: DEVICE pointer to F_l (b, C_l, h / k_l, w / k_l) fp32 contiguous; weights[l]: DEVICE pointer to wd_l packed
 *     (k_l, k_l, C_l, R_l) (maps, weights: host arrays of `levels` pointers, read during the call)
 *   wf (q, sum R) = the 1x1 weight times the batch-norm scale; shift (q) = everything constant per channel (batch-norm
 *     shift, 1x1 bias, the 1x1 image of the deconvolution biases); xy (b, n, 2) normalised; out (b, q, n)
 * A fixed number of launches (levels transposes + 5), no host synchronisation, no allocation; records into a HIP graph.
 * Scratch: epnet_image_head_points_workspace_bytes, pure arithmetic (pixel-major copies of the maps, the per-tap values, the
 * tap order and four tables of 256 bins; each part rounded up to 256 bytes; 0 outside the limits); the workspace must be
 * 16-byte aligned. sum R <= 240, q <= 120, 4 * b * n < 2^31, b <= 65535, else EPNET_ELIMIT before any launch; an unsupported
 * kernel size or map size, a NULL required pointer: EPNET_EINVAL; a short workspace: EPNET_ENOMEM; b == 0 or n == 0 returns
 * EPNET_OK and writes nothing. PRECONDITION: neither out nor the workspace aliases an input. */
size_t epnet_image_head_points_workspace_bytes(int b, int n, int h, int w, int levels, const int *chans, const int *kernels,
                                               const int *reduce, int q);
int epnet_image_head_points(int b, int n, int h, int w, int levels, const int *chans, const int *kernels, const int *reduce,
                            const float *const *maps, const float *const *weights, int q, const float *wf, const float *shift,
                            const float *xy, int align_corners, float *out, void *workspace, size_t workspace_bytes,
                            epnet_stream_t stream);

/* The same head on 16-bit maps (torch.autocast inference), on v_mfma_f32_16x16x32_{f16,bf16}. T = dtype = EPNET_F16 or EPNET_BF16;
 * every map, both packs and out are of type T; shift and xy stay fp32. The rule (it is NOT the "fp32 op on the upcast inputs,
 * rounded once" rule of the other *_h entries: the weights and the intermediate d are rounded to T, as autocast rounds the
 * weights and the activations of the dense head):
 *   out[b, c, n] = round_T( sum over the in-bounds taps (nw, ne, sw, se) of weight_tap * relu(shift[c] + sum_j wf16[c, j] * d16[j](tap)) )
 *   d16[j](tap)  = round_T( sum_ci wd16_l[Y % k_l, X % k_l, ci, r] * F_l[b, ci, Y / k_l, X / k_l] ),  j = (sum of R before l) + r
 *   wd16_l = round_T(wd_l), wf16 = round_T(wf) of the fp32 pack above.
 * Products are exact in fp32 and the sums over ci and j are accumulated in fp32 in the order the MFMA takes (not pinned); the
 * four taps are blended in fp32 in the fixed order, as above. Every round_T is to nearest even, keeps denormals and overflows to
 * infinity. Taps, tap weights and the in-bounds rule are those of epnet_feature_gather. No float atomics: a tap's value depends
 * on its pixel, its scene's maps and the weights alone (each row of an MFMA result depends on its own A row only).
 * Packed weights, in the MFMA's B-fragment order, with Cp_l = C_l rounded up to 32, Rp_l = R_l rounded up to 16,
 * SRp = sum R rounded up to 32 and qp = q rounded up to 16:
 *   weights16[l]: (k_l, k_l, Rp_l / 16, Cp_l / 32, 4, 16, 8) of T, element [py][px][nb][ks][kq][col][e] =
 *     wd16_l[py, px, ci = 32 ks + 8 kq + e, r = 16 nb + col], an exact zero where ci >= C_l or r >= R_l
 *   wf16: (qp / 16, SRp / 32, 4, 16, 8) of T, element [qb][ks][kq][col][e] = wf16[c = 16 qb + col, j = 32 ks + 8 kq + e], an exact
 *     zero where c >= q or j >= sum R
 * Both 16-byte aligned, else EPNET_EINVAL; maps[l] and out may sit at any 2-byte aligned address.
 * Workspace, each part rounded up to 256 bytes, in this order: per level the pixel-major copy (b, h / k_l * w / k_l, Cp_l) of T
 * with the channels C_l .. Cp_l - 1 written as zeros (2 b P_l Cp_l bytes); val (4 b n, q) fp32; the tap order 4 b n int32; the four
 * tables (256 + 256 + 257 + 257) int32. 16-byte aligned. epnet_image_head_points_h_workspace_bytes is that sum, pure arithmetic,
 * 0 outside the limits or for an empty problem.
 * levels + 5 launches and one memset whatever the data, no host synchronisation, no allocation; records into a HIP graph. Limits
 * and error codes of the fp32 entry, all answered before any launch; an unknown dtype: EPNET_EINVAL. */
size_t epnet_image_head_points_h_workspace_bytes(int b, int n, int h, int w, int levels, const int *chans, const int *kernels,
                                                 const int *reduce, int q);
int epnet_image_head_points_h(int b, int n, int h, int w, int levels, const int *chans, const int *kernels, const int *reduce,
                              int dtype, const void *const *maps, const void *const *weights16, int q, const void *wf16,
                              const float *shift, const float *xy, int align_corners, void *out, void *workspace,
                              size_t workspace_bytes, epnet_stream_t stream);

/* The tail of an SA level's shared MLP for inference: the last 1x1 convolution with its batch norm
 * folded into the weights, the ReLU and the max-pool over the nsample axis in one kernel; the (b, c, p, s) activation is never
 * written.
 *   x (b, k, p, s) fp32 contiguous: the hidden tensor, or the pre-activation of the previous convolution together with
 *     s_in, t_in (k) (both or neither; the previous unit's folded batch norm) and relu_in != 0 (its ReLU)
 *   w (c, k) with the batch-norm scale folded in, bias (c) or NULL (= zeros), y (b, c, p)
 * The rule, float32, bit for bit (-0 and +0 counted as equal):
 *   x'[k]      = fmaf(x[k], s_in[k], t_in[k]) when s_in is given, then max(x', 0) when relu_in is set (a NaN stays a NaN)
 *   a[c, p, s] = ONE fmaf chain over k = 0 .. k-1 ascending, started from +0: acc = fmaf(w[c, k], x'[k, p, s], acc)
 *   y[c, p]    = max(max_s a[c, p, s] + bias[c], 0); a NaN anywhere in the window gives NaN, as epnet_pool_max does
 * (v_mfma_f32_32x32x2_f32 walked over k in order into one accumulator is that chain: no split-K.) No float atomics: an output
 * depends on its own window and the weights alone. One launch, no host synchronisation, no allocation; records into a HIP
 * graph. Every pointer may sit at any 4-byte aligned address.
 * s in {1, 2, 4, 8, 16} or a multiple of 32, p * s < 2^31, k * c < 2^31, at most 2^31 - 1 workgroups, else EPNET_ELIMIT before any launch; a NULL
 * required pointer, one of s_in / t_in without the other, k < 1 or c < 1: EPNET_EINVAL; b == 0 or p == 0 returns EPNET_OK and
 * writes nothing. PRECONDITION: y does not alias an input. */
int epnet_sa_tail_f32(int b, int k, int c, int p, int s, const float *x, const float *w, const float *bias, const float *s_in,
                      const float *t_in, int relu_in, float *y, epnet_stream_t stream);

/* Host-memory ops: these are CPU ops in the reference itself (called from DataLoader worker
 * processes, lib/datasets/kitti_rcnn_dataset.py:672,767,811,1029,1157), not a fallback.
 * pts_in_boxes3d_cpu, roipool3d.cpp:97-125: pts (N,3), boxes3d (M,7) -> pts_flag (M,N) i64 */
int epnet_pts_in_boxes3d_host(int64_t *pts_flag, const float *pts, const float *boxes3d,
                              int64_t boxes_num, int64_t pts_num);

/* roipool3d_cpu, roipool3d.cpp:127-195: -> pooled_pts (M,S,3), pooled_features (M,S,C), flag (M) i64 */
int epnet_roipool3d_host(const float *pts, const float *boxes3d, const float *pts_feature,
                         float *pooled_pts, float *pooled_features, int64_t *pooled_empty_flag,
                         int64_t boxes_num, int64_t pts_num, int64_t feature_len,
                         int64_t sampled_pts_num);

/* get_thresholds (eval.py:8-25), a host op: `matched` (n) f64 HOST memory as epnet_kitti_match wrote it (NaN entries are
 * skipped), sorted descending, then the recall rule for num_sample_pts points in float64. Writes at most `capacity`
 * thresholds and their number to *count; EPNET_ENOMEM if there are more. */
int epnet_kitti_thresholds_host(const double *matched, int64_t n, int64_t num_gt, int num_sample_pts,
                                double *thresholds, int capacity, int *count);

#ifdef __cplusplus
}
#endif
#endif /* EPNET_OPS_H */

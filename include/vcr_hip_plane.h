/*
 * vcr_hip_plane.h -- surface normals on the device and the point-to-plane refinement that needs them:
 * Open3D's estimate_normals with a kNN search, and its registration_icp with TransformationEstimationPointToPlane, on top of
 * vcr_hip_refine.h's loop.  An extension of vcr_hip.h like that header (same library, same conventions, same error codes); it
 * adds no symbol to the other headers and moves none of their layouts, so VCR_ABI_VERSION is unchanged.
 *
 * vcr_normals_f32, for point i of a cloud, over the m = k + 1 rows { i } U idx[i][0..k) (an entry outside [0, N) reads as i):
 *   d_j = x_j - x_i                         fp32, component-wise
 *   S_d [3], S_dd = sum d d^T (six)         nine fp64 sums over j in idx's order (the products of two fp32 values are exact in
 *                                           fp64: only the additions round)
 *   C = S_dd / m - (S_d / m)(S_d / m)^T     fp64
 *   lambda0 <= lambda1 <= lambda2           C's eigenvalues; n = the unit eigenvector of lambda0 (fp64 cyclic Jacobi), rounded
 *                                           to fp32 at the end
 *   sign                                    with a viewpoint v: ((n0 e0 + n1 e1) + n2 e2) >= 0, e = (double)v - (double)x_i, n the
 *                                           fp32 normal, in fp64; on zero, and without a viewpoint: the component of n of largest
 *                                           magnitude is positive, the lowest index among equals
 *   curvature = (float)(lambda0 / ((lambda0 + lambda1) + lambda2)), 0 when that sum is 0
 *   C not finite (a NaN or inf row in the set): n = (0,0,1), curvature NaN.  C == 0 (all rows equal): n = (0,0,1), curvature 0.
 *   Two vanishing eigenvalues (collinear rows): some unit vector of the null space.
 * A point's result depends on its own rows alone: not on B, the launch or the rest of the batch.
 *
 * vcr_refine_plane_f32: vcr_refine_f32's loop (vcr_hip_refine.h) word for word -- the fp64 pose, the evaluation by
 * vcr_nn_score_f32's definition, the rel_* test, the per-cloud stop, everything enqueued up front -- with another fit.  Over the
 * inliers of eval_k, p the moved source point in the bits the search used, q = tgt[nn], nrm = tgt_normals[nn], all in fp64:
 *   r = ((p0 nrm0 + p1 nrm1) + p2 nrm2) - ((q0 nrm0 + q1 nrm1) + q2 nrm2)
 *   J = (p x nrm, nrm)                      six values: p1 nrm2 - p2 nrm1, p2 nrm0 - p0 nrm2, p0 nrm1 - p1 nrm0, nrm
 *   A = sum J J^T (21 distinct), g = sum J r (6)       in sum_d2's order, as vcr_refine_f32's sums
 *   A x = -g by Cholesky; a pivot that is not finite or not above 1e-12 times its diagonal entry of A: the system is singular
 *   R_i = Rz(x2) Ry(x1) Rx(x0), t_i = (x3, x4, x5)     Open3D's TransformVector6dToMatrix4d
 *   pose_{k+1} = (R_i R_k, R_i t_k + t_i) in fp64;  iterations += 1
 * A cloud with fewer than 6 inliers or a singular system stops: the pose stays, converged = 0.  A non-finite sum: R_i, t_i are
 * NaN, as in vcr_refine_f32.  The closing invariant carries over: fitness, rmse, inliers, sum_d2, nn_idx, nn_d2 are what
 * vcr_nn_score_f32 returns for (R_out, t_out, max_dist), bit for bit, in every launch form.
 */
#ifndef VCR_HIP_PLANE_H
#define VCR_HIP_PLANE_H

#include "vcr_hip_refine.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VCR_NORMALS_MAX_K 62              /* vcr_knn_f32's limit: VCR_EUNSUPPORTED beyond */

typedef struct {
  uint32_t struct_bytes;        /* sizeof(vcr_normals_args) as the CALLER was compiled (see vcr_fps_args); the mandatory part ends
                                   behind normals: 0, shorter than that or longer than this library knows: VCR_EINVAL */
  const float* xyz4;            /* [B,N,4] rows as vcr_rows4_f32 writes them, 16-B aligned; the fourth value is not read */
  const int* idx;               /* [B,N,k]: the neighbours vcr_knn_f32 wrote for C == 4 (cloud-local; outside [0, N): the row itself) */
  int B, N, k;                  /* B, N >= 1, N <= 131 072, B N < 2^31; 1 <= k <= VCR_NORMALS_MAX_K */
  const float* viewpoint;       /* optional [B,3]: the normals look at it; NULL: the largest component is positive */
  float* normals;               /* [B,3,N] channels-first, mandatory */
  float* curvature;             /* optional [B,N] */
} vcr_normals_args;

/* One launch, asynchronous on the stream, no workspace.  Runs no search of its own. */
int    vcr_normals_f32(const vcr_normals_args*, vcr_stream_t);

typedef struct {
  uint32_t struct_bytes;        /* sizeof(vcr_refine_plane_args) as the CALLER was compiled; the mandatory part is all of it today */
  /* vcr_refine_args' fields, in its order and with its meaning */
  const float* src; const float* tgt;
  int B, Ns, Nt;
  const float* R; const float* t;
  float max_dist;
  int max_iterations;
  float rel_fitness, rel_rmse;
  float* R_out; float* t_out;
  float* fitness; float* rmse;
  float* R_ba; float* t_ba;
  int* inliers; double* sum_d2;
  int* iterations; int* converged;
  int* nn_idx; float* nn_d2;
  int variant;
  const float* tgt_normals;     /* [B,3,Nt] channels-first, mandatory (NULL: VCR_EINVAL): the target's normals, as vcr_normals_f32 writes them */
} vcr_refine_plane_args;

/* As vcr_refine_workspace_bytes, vcr_refine_f32 and vcr_refine_form (vcr_hip_refine.h), for the point-to-plane fit. */
size_t vcr_refine_plane_workspace_bytes(const vcr_refine_plane_args*, int cu_count);
int    vcr_refine_plane_f32(const vcr_refine_plane_args*, void* workspace, size_t workspace_bytes, vcr_stream_t);
int    vcr_refine_plane_form(const vcr_refine_plane_args*, int cu_count, int* queries_per_lane, int* target_splits);

#ifdef __cplusplus
}
#endif
#endif

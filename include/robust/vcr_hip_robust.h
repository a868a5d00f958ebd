/*
 * vcr_hip_robust.h -- a point-to-plane refinement that outliers inside max_dist do not pull along, and the information matrix
 * of a registered pair: Open3D's TransformationEstimationPointToPlane(kernel) with HuberLoss,
 * CauchyLoss, GMLoss and TukeyLoss, and its get_information_matrix_from_point_clouds, on top of vcr_hip_refine.h's loop.  An
 * extension of vcr_hip.h like vcr_hip_plane.h (same library, same conventions, same error codes); it adds no symbol to the other
 * headers and moves none of their layouts, so VCR_ABI_VERSION is unchanged.
 *
 * vcr_refine_robust_f32: vcr_refine_plane_f32's definition (vcr_hip_plane.h) word for word -- vcr_refine_f32's loop, the fp64
 * pose, the evaluation by vcr_nn_score_f32's definition, the rel_* test, fewer than 6 inliers, the singular rule, the solve,
 * the composed pose, the closing invariant -- with a WEIGHT per inlier.  With r and J of vcr_hip_plane.h, all in fp64, and
 * k = (double)args.k:
 *   VCR_LOSS_L2       w = 1
 *   VCR_LOSS_HUBER    a = fabs(r);  w = a <= k ? 1 : k / a
 *   VCR_LOSS_CAUCHY   u = r / k;  w = 1 / (1 + u * u)
 *   VCR_LOSS_GM       s = k + r * r;  w = k / (s * s)
 *   VCR_LOSS_TUKEY    a = fabs(r), u = r / k, v = 1 - u * u;  w = a <= k ? v * v : 0
 *   Jw_i = w J_i                             six values
 *   A_rc = sum Jw_r J_c (r <= c, 21),  g_r = sum Jw_r r (6)         in sum_d2's order, as vcr_refine_plane_f32's sums
 *   A x = -g by Cholesky, vcr_refine_plane_f32's pivot rule;  R_i = Rz(x2) Ry(x1) Rx(x0), t_i = (x3, x4, x5)
 *   pose_{k+1} = (R_i R_k, R_i t_k + t_i) in fp64;  iterations += 1
 * (Open3D's weights: rho'(r) / r of the loss.)  A source point that is no inlier has r = 0 and J = 0: its weight is finite
 * because k > 0, and it contributes exact zeros.  VCR_LOSS_L2, and VCR_LOSS_HUBER with a k no residual exceeds, return
 * vcr_refine_plane_f32's outputs bit for bit.
 * If every weight is zero (VCR_LOSS_TUKEY with every |r| > k), A = 0: the system is singular and the cloud stops with the pose
 * it has, converged = 0, like a cloud with fewer than 6 inliers.  A non-finite sum: R_i, t_i are NaN, as in vcr_refine_f32.
 * fitness, rmse, inliers, sum_d2, nn_idx, nn_d2 are the GEOMETRIC figures: what vcr_nn_score_f32 returns for (R_out, t_out,
 * max_dist), bit for bit, in every launch form -- never the weighted residual.
 * The redescending losses (VCR_LOSS_GM, VCR_LOSS_TUKEY) give a pair far off the surface next to no pull: from a poor start,
 * where the GOOD pairs are far off, they lose the pose.  Run VCR_LOSS_L2 or VCR_LOSS_CAUCHY first and start them there.
 * k is the noise scale of the caller's sensor, in the clouds' unit; there is no default.
 * L1 is not built: Open3D's weight 1 / |r| divides by zero on an exact hit.
 *
 * vcr_information_f32: over the inliers of vcr_nn_score_f32 at (R, t, max_dist) -- a target point counts once per source point
 * that chose it --, with q = (x, y, z) = tgt[nn] in fp64, nine sums in sum_d2's order (the products of two fp32 values are
 * exact):  Sx, Sy, Sz, Sxx, Syy, Szz, Sxy, Sxz, Syz;  n their count.  Then, row-major,
 *   information = [ Syy+Szz  -Sxy     -Sxz      0    -Sz    Sy ]
 *                 [ -Sxy     Sxx+Szz  -Syz      Sz    0    -Sx ]
 *                 [ -Sxz     -Syz     Sxx+Syy  -Sy    Sx    0  ]
 *                 [  0        Sz      -Sy       n     0     0  ]
 *                 [ -Sz       0        Sx       0     n     0  ]
 *                 [  Sy      -Sx       0        0     0     n  ]
 * Open3D's GTG = sum G^T G with its three rows a pair, G = [ -[q]x | I ]: the weight of a pose-graph edge in multiway
 * registration.  No inlier gives the zero matrix; a sum that is not finite is written as it is.  The call is ONE round of
 * vcr_refine_f32's loop -- the search, the merge, the per-cloud evaluation -- and a launch that writes the matrix from the
 * merge's partials: max_iterations must be 0 (anything else: VCR_EINVAL), R_out / t_out return the given pose (R_ba, t_ba its
 * inverse), iterations and converged are 0, and the evaluation outputs are vcr_nn_score_f32's, bit for bit.
 *
 * The grid siblings (vcr_refine_robust_grid_*, vcr_information_grid_*) are vcr_hip_gridnn.h's in every respect: the same loop
 * behind the capped search on the target's grid, the same bits but the -1 / +inf of a source point without a partner.
 */
#ifndef VCR_HIP_ROBUST_H
#define VCR_HIP_ROBUST_H

#include "../vcr_hip_plane.h"
#include "../vcr_hip_gridnn.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VCR_LOSS_L2     0
#define VCR_LOSS_HUBER  1
#define VCR_LOSS_CAUCHY 2
#define VCR_LOSS_GM     3
#define VCR_LOSS_TUKEY  4

typedef struct {
  uint32_t struct_bytes;        /* sizeof(vcr_refine_robust_args) as the CALLER was compiled; the mandatory part is all of it today */
  /* vcr_refine_plane_args' fields, in its order and with its meaning */
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
  const float* tgt_normals;     /* [B,3,Nt] channels-first, mandatory (NULL: VCR_EINVAL): the target's unit normals */
  int loss;                     /* VCR_LOSS_*; any other value: VCR_EINVAL */
  float k;                      /* the loss' scale, in the clouds' unit: finite and > 0 (else VCR_EINVAL); VCR_LOSS_L2 does not read it */
} vcr_refine_robust_args;

/* As vcr_refine_plane_workspace_bytes, vcr_refine_plane_f32 and vcr_refine_plane_form (vcr_hip_plane.h): the same form and the
   same workspace for the same shape. */
size_t vcr_refine_robust_workspace_bytes(const vcr_refine_robust_args*, int cu_count);
int    vcr_refine_robust_f32(const vcr_refine_robust_args*, void* workspace, size_t workspace_bytes, vcr_stream_t);
int    vcr_refine_robust_form(const vcr_refine_robust_args*, int cu_count, int* queries_per_lane, int* target_splits);

/* The grid siblings, as vcr_refine_plane_grid_* (vcr_hip_gridnn.h): V = 29. */
size_t vcr_refine_robust_grid_workspace_bytes(const vcr_refine_robust_args*, const vcr_grid_nn_args*, int cu_count);
int    vcr_refine_robust_grid_f32(const vcr_refine_robust_args*, const vcr_grid_nn_args*, void* workspace, size_t workspace_bytes, vcr_stream_t);
int    vcr_refine_robust_grid_form(const vcr_refine_robust_args*, const vcr_grid_nn_args*, int cu_count, int* cells_per_cloud, int* order, int* queries_per_workgroup);

typedef struct {
  uint32_t struct_bytes;        /* sizeof(vcr_information_args) as the CALLER was compiled; the mandatory part is all of it today */
  /* vcr_refine_args' fields, in its order and with its meaning; max_iterations must be 0 */
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
  double* information;          /* [B,6,6] row-major, mandatory (NULL: VCR_EINVAL): every element is written */
} vcr_information_args;

/* As vcr_refine_workspace_bytes, vcr_refine_f32 and vcr_refine_form (vcr_hip_refine.h): V = 11. */
size_t vcr_information_workspace_bytes(const vcr_information_args*, int cu_count);
int    vcr_information_f32(const vcr_information_args*, void* workspace, size_t workspace_bytes, vcr_stream_t);
int    vcr_information_form(const vcr_information_args*, int cu_count, int* queries_per_lane, int* target_splits);

size_t vcr_information_grid_workspace_bytes(const vcr_information_args*, const vcr_grid_nn_args*, int cu_count);
int    vcr_information_grid_f32(const vcr_information_args*, const vcr_grid_nn_args*, void* workspace, size_t workspace_bytes, vcr_stream_t);
int    vcr_information_grid_form(const vcr_information_args*, const vcr_grid_nn_args*, int cu_count, int* cells_per_cloud, int* order, int* queries_per_workgroup);

#ifdef __cplusplus
}
#endif
#endif

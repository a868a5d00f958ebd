/*
 * vcr_hip_colored.h -- refining a registration by colour AND shape: Open3D's registration_colored_icp
 * (Park, Zhou, Koltun: Colored Point Cloud Registration Revisited, ICCV 2017) on top of vcr_hip_refine.h's loop, and the colour
 * gradients of the target it reads.  An extension of vcr_hip.h like vcr_hip_plane.h (same library, same conventions, same error
 * codes); it adds no symbol to the other headers and moves none of their layouts, so VCR_ABI_VERSION is unchanged.
 *
 * A colour is one fp32 INTENSITY per point here ([B,N]); the caller takes it from RGB as it likes (Open3D: the mean).
 *
 * vcr_color_gradient_f32, for point i of a cloud with unit normal n and intensity I_i, over the entries j of its row
 * idx[i][0..k), in the row's order.  An entry is skipped when it lies outside [0, N), when it equals i, or when radius > 0 and
 * its squared distance exceeds radius * radius (both in fp32; d2 = (d0 d0 + d1 d1) + d2 d2 of the d below; a d2 that is NaN is
 * not skipped).  Open3D's KDTreeSearchParamHybrid(2 r, 30) is radius = 2 r with k = 29.  Over the m entries that remain:
 *   d_j  = x_j - x_i                                       fp32, component-wise, widened to fp64; fp64 from here on
 *   a_j  = d_j - ((d_j0 n0 + d_j1 n1) + d_j2 n2) n         the neighbour projected into the tangent plane
 *   S_aa = sum a_j a_j^T (six distinct), S_ab = sum a_j ((double)I_j - (double)I_i) (three)
 *   M_rc = S_aa_rc + ((double)m (double)m) (n_r n_c)       Open3D's extra row (nn - 1) n . x = 0: it ties x to the tangent plane
 *   M x  = S_ab by Cholesky; a pivot that is not finite or not above 1e-12 times its diagonal entry of M: singular
 *   gradient[.][i] = (float)x
 * The gradient is EXACTLY ZERO when m < 3 (Open3D: nn >= 4 with the point itself), when one of the nine sums is not finite, or
 * when M is singular.  A point's result depends on its own row alone: not on B, the launch or the rest of the batch.
 *
 * vcr_refine_colored_f32: vcr_refine_f32's loop (vcr_hip_refine.h) word for word -- the fp64 pose, the evaluation by
 * vcr_nn_score_f32's definition, the rel_* test, the per-cloud stop, everything enqueued up front -- with a fourth fit.  Over
 * the inliers of eval_k, all in fp64 from the fp32 inputs: p the moved source point in the bits the search used and I_s its
 * intensity; q = tgt[nn], n = tgt_normals[nn], d = tgt_gradient[nn], I_t = tgt_intensity[nn]; lam = (double)lambda_geometric:
 *   s    = ((p0 n0 + p1 n1) + p2 n2) - ((q0 n0 + q1 n1) + q2 n2)          vcr_refine_plane_f32's residual (p - q) . n
 *   r_G  = sqrt(lam) s                                      J_G = sqrt(lam) (p x n, n)
 *   Md   = d - ((d0 n0 + d1 n1) + d2 n2) n
 *   e_c  = (p_c - s n_c) - q_c                              p projected onto the neighbour's tangent plane, from q
 *   r_I  = sqrt(1 - lam) ((I_t + ((d0 e0 + d1 e1) + d2 e2)) - I_s)          J_I = sqrt(1 - lam) (p x Md, Md)
 *   (u x v = (u1 v2 - u2 v1, u2 v0 - u0 v2, u0 v1 - u1 v0))
 *   A_rc = sum (J_G,r J_G,c + J_I,r J_I,c) (r <= c, 21),  g_r = sum (J_G,r r_G + J_I,r r_I) (6)      in sum_d2's order
 *   A x = -g by Cholesky, vcr_refine_plane_f32's pivot rule;  R_i = Rz(x2) Ry(x1) Rx(x0), t_i = (x3, x4, x5)
 *   pose_{k+1} = (R_i R_k, R_i t_k + t_i) in fp64;  iterations += 1
 * At lambda_geometric = 1 the photometric terms are exact zeros (for finite colours) and every output equals
 * vcr_refine_plane_f32's bit for bit.  A cloud with fewer than 6 inliers or a singular system (a target of one colour on a
 * plane) stops: the pose stays, converged = 0.  A non-finite sum -- a NaN intensity or gradient of an inlier -- : R_i, t_i are
 * NaN, as in vcr_refine_f32.  The closing invariant carries over: fitness, rmse, inliers, sum_d2, nn_idx, nn_d2 are what
 * vcr_nn_score_f32 returns for (R_out, t_out, max_dist), bit for bit, in every launch form.  They are the GEOMETRIC figures:
 * Open3D reports the joint residual sqrt(sum (r_G^2 + r_I^2) / n) as inlier_rmse, this call the Euclidean one.
 *
 * The grid siblings (vcr_refine_colored_grid_*) are vcr_hip_gridnn.h's in every respect: the same loop behind the capped search
 * on the target's grid, the same bits but the -1 / +inf of a source point without a partner.
 */
#ifndef VCR_HIP_COLORED_H
#define VCR_HIP_COLORED_H

#include "../vcr_hip_plane.h"
#include "../vcr_hip_gridnn.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct {
  uint32_t struct_bytes;        /* sizeof(vcr_color_gradient_args) as the CALLER was compiled; the mandatory part is all of it today */
  const float* xyz4;            /* [B,N,4] rows as vcr_rows4_f32 writes them, 16-B aligned; the fourth value is not read */
  const int* idx;               /* [B,N,k]: a neighbour row per point, as vcr_normals_f32 takes it (cloud-local) */
  int B, N, k;                  /* B, N >= 1, N <= 131 072, B N < 2^31; 1 <= k <= VCR_NORMALS_MAX_K */
  const float* normals;         /* [B,3,N] channels-first, mandatory: unit normals */
  const float* intensity;       /* [B,N], mandatory */
  float radius;                 /* 0: every entry of a row counts; finite and > 0: those within it; else VCR_EINVAL */
  float* gradient;              /* [B,3,N] channels-first, mandatory: every element is written */
} vcr_color_gradient_args;

/* One launch, asynchronous on the stream, no workspace.  Runs no search of its own. */
int    vcr_color_gradient_f32(const vcr_color_gradient_args*, vcr_stream_t);

typedef struct {
  uint32_t struct_bytes;        /* sizeof(vcr_refine_colored_args) as the CALLER was compiled; the mandatory part is all of it today */
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
  const float* tgt_normals;     /* [B,3,Nt] channels-first, mandatory (NULL: VCR_EINVAL): the target's unit normals */
  const float* tgt_gradient;    /* [B,3,Nt] channels-first, mandatory: the target's colour gradients, as vcr_color_gradient_f32 writes them */
  const float* tgt_intensity;   /* [B,Nt], mandatory */
  const float* src_intensity;   /* [B,Ns], mandatory */
  float lambda_geometric;       /* the weight of the geometric term; finite and in [0, 1] (anything else: VCR_EINVAL).  Open3D: 0.968 */
} vcr_refine_colored_args;

/* As vcr_refine_workspace_bytes, vcr_refine_f32 and vcr_refine_form (vcr_hip_refine.h), for the colored fit: the form is
   vcr_refine_form's for the same shape, the workspace vcr_refine_plane_workspace_bytes'. */
size_t vcr_refine_colored_workspace_bytes(const vcr_refine_colored_args*, int cu_count);
int    vcr_refine_colored_f32(const vcr_refine_colored_args*, void* workspace, size_t workspace_bytes, vcr_stream_t);
int    vcr_refine_colored_form(const vcr_refine_colored_args*, int cu_count, int* queries_per_lane, int* target_splits);

/* The grid siblings, as vcr_refine_plane_grid_* (vcr_hip_gridnn.h): V = 29. */
size_t vcr_refine_colored_grid_workspace_bytes(const vcr_refine_colored_args*, const vcr_grid_nn_args*, int cu_count);
int    vcr_refine_colored_grid_f32(const vcr_refine_colored_args*, const vcr_grid_nn_args*, void* workspace, size_t workspace_bytes, vcr_stream_t);
int    vcr_refine_colored_grid_form(const vcr_refine_colored_args*, const vcr_grid_nn_args*, int cu_count, int* cells_per_cloud, int* order, int* queries_per_workgroup);

#ifdef __cplusplus
}
#endif
#endif

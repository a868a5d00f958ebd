/*
 * vcr_hip_gicp.h -- the plane-to-plane refinement: Open3D's registration_generalized_icp on top of
 * vcr_hip_refine.h's loop, with the normals of BOTH clouds (vcr_hip_plane.h's vcr_normals_f32 writes them).  An extension of
 * vcr_hip.h like those headers (same library, same conventions, same error codes); it adds no symbol to the other headers and
 * moves none of their layouts, so VCR_ABI_VERSION is unchanged.
 *
 * A point's covariance is built from its unit normal n as Open3D builds it, C = Rot diag(epsilon, 1, 1) Rot^T with Rot's first
 * column n, which equals I - (1 - epsilon) n n^T: so the normals and epsilon are all the fit reads.  Covariances of the
 * caller's own are not taken.
 *
 * vcr_refine_gicp_f32: vcr_refine_f32's loop word for word -- the fp64 pose, the evaluation by vcr_nn_score_f32's (Euclidean)
 * definition, the rel_* test, the per-cloud stop, everything enqueued up front -- with another fit.  Over the inliers of eval_k,
 * all in fp64 from the fp32 inputs; p the moved source point in the bits the search used, q = tgt[nn], m = tgt_normals[nn],
 * R_k the fp32 pose the search ran under, s = src_normals[i]:
 *   n_c  = (R_k[3c] s0 + R_k[3c+1] s1) + R_k[3c+2] s2                 the source normal, turned (products of fp32 values: exact)
 *   kap  = 1 - (double)epsilon
 *   M_ij = (i == j ? 2 : 0) - kap (m_i m_j + n_i n_j)                 = C_t + R C_s R^T, six distinct (i <= j)
 *   cofactors  K00 = M11 M22 - M12 M12   K01 = M02 M12 - M01 M22   K02 = M01 M12 - M02 M11
 *              K11 = M00 M22 - M02 M02   K12 = M01 M02 - M00 M12   K22 = M00 M11 - M01 M01
 *   det  = (M00 K00 + M01 K01) + M02 K02;   W_ij = K_ij / det         = M^-1, symmetric, six distinct
 *   d    = p - q                                                      component-wise
 *   for a vector v:  a_0.v = p1 v2 - p2 v1,  a_1.v = p2 v0 - p0 v2,  a_2.v = p0 v1 - p1 v0,  a_{3+c}.v = v_c
 *                                                                     (a_0 ... a_5 are the columns of [-skew(p) | I])
 *   u_c  = W a_c:  u_0 = p1 W_.2 - p2 W_.1,  u_1 = p2 W_.0 - p0 W_.2,  u_2 = p0 W_.1 - p1 W_.0,  u_{3+c} = W_.c   (W_.c: column c)
 *   e    = W d:    e_i = (W_i0 d0 + W_i1 d1) + W_i2 d2
 *   A_rc = sum a_r.u_c (r <= c, 21),  g_r = sum a_r.e (6)             in sum_d2's order, as vcr_refine_f32's sums
 *   A x = -g by Cholesky, vcr_refine_plane_f32's pivot rule;  R_i = Rz(x2) Ry(x1) Rx(x0), t_i = (x3, x4, x5)
 *   pose_{k+1} = (R_i R_k, R_i t_k + t_i) in fp64;  iterations += 1
 * With W = m m^T these are vcr_refine_plane_f32's J J^T and J r.  The normals are expected to be unit vectors and are not
 * normalised; their signs do not enter (every term is even in m and in s, and a negation is exact): flipping any of them changes
 * no bit of any output.
 * A cloud with fewer than 3 inliers or a singular system (collinear inliers) stops: the pose stays, converged = 0.  A non-finite
 * sum -- from a NaN normal of an inlier, or an M that normals longer than unit made singular -- : R_i, t_i are NaN, as in
 * vcr_refine_f32.  The closing invariant carries over: fitness, rmse, inliers, sum_d2, nn_idx, nn_d2 are what vcr_nn_score_f32
 * returns for (R_out, t_out, max_dist), bit for bit, in every launch form.
 */
#ifndef VCR_HIP_GICP_H
#define VCR_HIP_GICP_H

#include "vcr_hip_plane.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct {
  uint32_t struct_bytes;        /* sizeof(vcr_refine_gicp_args) as the CALLER was compiled; the mandatory part is all of it today */
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
  const float* src_normals;     /* [B,3,Ns] channels-first, mandatory (NULL: VCR_EINVAL): the source's unit normals, in the source's frame */
  float epsilon;                /* the covariance along the normal; finite, > 0 and <= 1 (anything else: VCR_EINVAL).  Open3D: 1e-3 */
} vcr_refine_gicp_args;

/* As vcr_refine_workspace_bytes, vcr_refine_f32 and vcr_refine_form (vcr_hip_refine.h), for the plane-to-plane fit: the form is
   vcr_refine_form's for the same shape, the workspace vcr_refine_plane_workspace_bytes'. */
size_t vcr_refine_gicp_workspace_bytes(const vcr_refine_gicp_args*, int cu_count);
int    vcr_refine_gicp_f32(const vcr_refine_gicp_args*, void* workspace, size_t workspace_bytes, vcr_stream_t);
int    vcr_refine_gicp_form(const vcr_refine_gicp_args*, int cu_count, int* queries_per_lane, int* target_splits);

#ifdef __cplusplus
}
#endif
#endif

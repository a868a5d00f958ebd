/*
 * vcr_hip_posegraph.h -- multiway registration: a pose graph optimised on the device, after Open3D's
 * global_optimization with GlobalOptimizationLevenbergMarquardt, the line process over uncertain edges and the pruning pass.
 * An extension of vcr_hip.h (same library, same conventions, same error codes); it adds no symbol to the other headers and
 * moves none of their layouts, so VCR_ABI_VERSION is unchanged.  It lives alone in include/posegraph/.
 *
 * ONE launch: a workgroup takes a graph and runs the whole Levenberg-Marquardt loop, both passes; a batch of G graphs takes a
 * workgroup each.  Everything is fp64.  No atomic: every sum has a fixed order, so a graph's outputs do not depend on the batch
 * it sits in, on the form of the launch or on what the workspace held.
 *
 * The graph.  K nodes with poses T_i = (R_i, t_i), node frame to world.  E edge slots; edge e holds src, dst, X_e = (R_e, t_e)
 * taking the SOURCE node's frame into the TARGET node's frame (what a pairwise registration of (source cloud, target cloud)
 * returns), info (6 x 6, rotation first, translation behind: the layout of information_matrix) and uncertain (non-zero: a loop closure the line process
 * may switch off).  An edge with src < 0 is a BLANK: that is how a batch pads.  On the device an edge with an index outside
 * [0, K) or with src == dst is a blank too; vcr_posegraph_check_edges refuses those on the host.
 *
 * Residual of an edge.  M = X_e^-1 T_dst^-1 T_src, r_e = vec6(M), the inverse of R = Rz(x2) Ry(x1) Rx(x0):
 *   sy = sqrt(M00^2 + M10^2);  sy > 1e-6: (atan2(M21, M22), atan2(-M20, sy), atan2(M10, M00));  else (atan2(-M12, M11),
 *   atan2(-M20, sy), 0);  then (M03, M13, M23).
 * Jacobians, for the update T_i <- euler(d_i) T_i:  column k of J_src = lin6(X_e^-1 T_dst^-1 G_k T_src), G_k the generators
 * (rotation about x, y, z, translation along x, y, z), lin6(M) = ((M21-M12)/2, (M02-M20)/2, (M10-M01)/2, M03, M13, M23);
 * J_dst = -J_src.
 * Line process.  q_e = r_e^T info_e r_e.  A certain edge has l_e = 1; an uncertain one l_e = s_e^2, s_e = mu / (mu + q_e);
 * mu = max_correspondence_distance^2 times the mean of info_e[5][5] over the uncertain edges that are no blanks, added in edge
 * order (no such edge: mu = 0).  The residual of the graph is sum_e (l_e q_e + [uncertain] mu (s_e - 1)^2), added in edge
 * order (a blank adds +0).
 * System.  H (6K x 6K) and b (6K): edge e adds l J_a^T info J_b to block (a, b) and -l J_a^T info r to b_a, a, b in {src, dst};
 * every block and every segment of b is the sum of its edges' terms in ASCENDING EDGE INDEX (two edges between the same two
 * nodes are allowed).  The anchor's rows and columns are the identity's and its entries of b are 0.
 * The loop.  lambda = 1e-5 max diag(H), nu = 2.  Up to max_iteration outer iterations of up to max_iteration_lm trials.  A trial:
 *   (H + lambda I) d = b by block Cholesky (6 x 6 blocks); a pivot that is not finite or <= 1e-12 times its diagonal entry of
 *   H + lambda I, or a d that is not finite, ends the CALL with the poses it has, converged = 0;
 *   |d| <= min_relative_increment (|x| + min_relative_increment), x the stacked vec6(T_i): stop, converged;
 *   trial poses euler(d_i) T_i, res_new their residual under the l in force;
 *   rho = (res - res_new) / (d . (lambda d + b) + 1e-3);
 *   rho > 0: the trial poses are taken and res = res_new; stop, converged, if sqrt(res_old) - sqrt(res_new) <
 *     min_relative_residual_increment sqrt(res_old); else lambda *= max(lower_scale_factor, 1 - (2 rho - 1)^3), nu = 2, l, H and b
 *     are rebuilt, stop, converged, if max |b| <= min_right_term; the outer iteration ends;
 *   otherwise lambda *= nu, nu *= 2.
 * After an outer iteration: stop, converged, if res < min_residual.  max_iteration used up: converged = 0.
 * upper_scale_factor is taken and NOT used: the rule above has no upper clamp.
 * Pruning.  prune != 0: after the first pass every uncertain edge with l_e < edge_prune_threshold becomes a blank, and the loop
 * runs again from the poses reached (mu, l, H, b, lambda and nu from the start), in the same launch.  prune == 0: one pass.
 * max_iteration == 0: one linearisation, nothing moves and nothing is pruned, converged = 0.
 */
#ifndef VCR_HIP_POSEGRAPH_H
#define VCR_HIP_POSEGRAPH_H

#include "../vcr_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VCR_POSEGRAPH_MAX_NODES 128
#define VCR_POSEGRAPH_MAX_EDGES 65536
#define VCR_POSEGRAPH_MAX_TRIALS 4096      /* max_iteration * max_iteration_lm above this: VCR_EINVAL */
#define VCR_POSEGRAPH_FORM_LDS 1           /* the factor of H + lambda I lives in LDS */
#define VCR_POSEGRAPH_FORM_GLOBAL 2        /* ... in the workspace */

/* G < 1, K < 1, E < 0, a missing mandatory pointer (with E == 0 the edge arrays, weight and kept may be NULL), anchor outside
 * [0, K), max_correspondence_distance or edge_prune_threshold not finite or < 0, max_iteration or max_iteration_lm < 0 or
 * > 4096, max_iteration * max_iteration_lm > 4096, a min_* that is NaN or < 0, lower_scale_factor or upper_scale_factor not finite or
 * <= 0, variant outside 0 ... 2, variant 1 with a K whose factor does not fit LDS: VCR_EINVAL.
 * K > 128, E > 65 536 or G * max(E, 1) >= 2^31: VCR_EUNSUPPORTED. */
typedef struct {
  uint32_t struct_bytes;        /* sizeof(vcr_posegraph_args) as the CALLER was compiled; the mandatory part ends behind
                                   converged: 0, shorter than that or longer than this library knows: VCR_EINVAL */
  int G, K, E;
  const double* R; const double* t;             /* [G,K,3,3] row-major, [G,K,3]: the initial poses */
  const int* src; const int* dst;               /* [G,E] */
  const double* R_edge; const double* t_edge;   /* [G,E,3,3], [G,E,3] */
  const double* information;                    /* [G,E,6,6] */
  const int* uncertain;                         /* [G,E] */
  int anchor;                                   /* the node whose pose does not move */
  int prune;
  double max_correspondence_distance;
  double edge_prune_threshold;
  int max_iteration, max_iteration_lm;
  double min_relative_increment, min_relative_residual_increment, min_right_term, min_residual;
  double lower_scale_factor, upper_scale_factor;
  int variant;                  /* 0: the plan's form; VCR_POSEGRAPH_FORM_LDS / _GLOBAL force one: the same bits */
  double* R_out; double* t_out; /* [G,K,3,3], [G,K,3] */
  double* weight;               /* [G,E]: the last l_e (of a pruned edge: the one that pruned it); NaN on an edge blank at entry */
  int* kept;                    /* [G,E]: 1 on an edge that is no blank at the end */
  double* residual;             /* [G,2]: at the start of the first pass and at the end of the last */
  int* iterations;              /* [G,2]: outer iterations begun in each pass */
  int* converged;               /* [G]: of the last pass run */
  /* optional, NULL = not wanted */
  int* trials;                  /* [G,2]: solves in each pass */
  double* H; double* b;         /* [G,6K,6K], [G,6K]: the system at the INITIAL poses */
  double* residual0; double* l0;   /* [G], [G,E]: the residual and l_e at the initial poses (NaN on a blank) */
  double* delta0;               /* [G,6K]: the first solve's d (not written with max_iteration == 0) */
  double* lambda0;              /* [G]: the first lambda */
} vcr_posegraph_args;

/* Bytes of workspace vcr_posegraph_optimize_f64 needs; 0 for arguments it would refuse.  Host only: the form depends on K
 * alone, cu_count (>= 0) is taken for symmetry with the other headers. */
size_t vcr_posegraph_optimize_workspace_bytes(const vcr_posegraph_args*, int cu_count);
/* Asynchronous on the stream: no host synchronisation, no allocation, ONE launch.  workspace: device memory, 16-B aligned, at
 * least _workspace_bytes; its contents need not be initialised. */
int    vcr_posegraph_optimize_f64(const vcr_posegraph_args*, void* workspace, size_t workspace_bytes, vcr_stream_t);
/* The form the call takes (VCR_POSEGRAPH_FORM_*) and the bytes of LDS its workgroup asks for; either pointer may be NULL. */
int    vcr_posegraph_optimize_form(const vcr_posegraph_args*, int cu_count, int* form, int* lds_bytes);
/* HOST arrays src, dst [G*E]: VCR_EINVAL for an edge with an index >= K or with src == dst >= 0 (src < 0: a blank). */
int    vcr_posegraph_check_edges(const int* src, const int* dst, int G, int K, int E);

#ifdef __cplusplus
}
#endif
#endif

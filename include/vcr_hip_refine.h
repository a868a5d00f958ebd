/*
 * vcr_hip_refine.h -- refining a registration on the FULL clouds: a trimmed point-to-point ICP on the
 * device, Open3D's registration_icp with a correspondence-distance cap, on top of vcr_hip_score.h's nearest-neighbour search.
 * An extension of vcr_hip.h like that header (same library, same conventions, same error codes); it adds no symbol to either
 * and moves none of their layouts, so VCR_ABI_VERSION is unchanged.
 *
 * Per cloud, independently of the rest of the batch (the running pose is kept in fp64; the search and the caller see its
 * fp32 rounding, round32):
 *   eval_0 = evaluate(pose_0)                      nn, inliers, sum_d2, fitness, rmse: vcr_nn_score_f32's definition, bit for bit
 *   for k = 0 .. max_iterations - 1:
 *     inliers_k < 3                                the cloud stops: the pose stays, converged = 0
 *     (R_i, t_i)  the best rigid fit of { p_n -> tgt[nn_n] } over the inliers n of eval_k, p_n the moved source point in the
 *                 bits the search used.  Sixteen fp64 sums -- count n, S_p, S_q, S_pq = sum p q^T (products of two fp32 values
 *                 are exact in fp64: only the additions round) -- in sum_d2's order: per 256 consecutive source points the wave
 *                 butterfly 32 ... 1, the four waves ascending, then the partials ascending.
 *                 H = S_pq - S_p S_q^T / n;  H = U S V^T (fp64 one-sided Jacobi);  R_i = V U^T, with the column of V of the
 *                 smallest singular value flipped when det < 0 (vcr_rigid_svd_f32's solve);  t_i = S_q / n - R_i S_p / n.
 *                 A non-finite sum: R_i, t_i are NaN -- the next evaluation finds no inlier and the cloud stops.
 *                 (The rel_* test runs on that evaluation first, as on any other: with thresholds above the previous
 *                 fitness and rmse such a cloud reports converged = 1.  A NaN in R_out says what happened.)
 *     pose_{k+1} = (R_i R_k, R_i t_k + t_i) in fp64;  iterations += 1
 *     eval_{k+1} = evaluate(round32(pose_{k+1}))
 *     |fitness_{k+1} - fitness_k| < rel_fitness and |rmse_{k+1} - rmse_k| < rel_rmse (fp32 differences of the fp32 results,
 *                 strict):  converged = 1, the cloud stops
 * Everything returned is a function of the input alone -- every launch form returns the same bits -- and fitness, rmse, inliers,
 * sum_d2, nn_idx, nn_d2 are what vcr_nn_score_f32 returns for (R_out, t_out, max_dist), bit for bit.
 */
#ifndef VCR_HIP_REFINE_H
#define VCR_HIP_REFINE_H

#include "vcr_hip_score.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VCR_REFINE_MAX_ITERATIONS 4096    /* three launches are enqueued per round: VCR_EUNSUPPORTED beyond */

typedef struct {
  uint32_t struct_bytes;        /* sizeof(vcr_refine_args) as the CALLER was compiled (see vcr_fps_args); the mandatory part ends
                                   behind rmse: 0, shorter than that or longer than this library knows: VCR_EINVAL */
  const float* src; const float* tgt;   /* [B,3,Ns], [B,3,Nt] channels-first fp32, contiguous */
  int B, Ns, Nt;
  const float* R; const float* t;       /* the initial pose [B,3,3], [B,3]; both NULL = identity */
  float max_dist;                        /* correspondence cap, inlier: d2 <= max_dist*max_dist (fp32 product); finite, >= 0 */
  int max_iterations;                    /* pose updates at most, >= 0 (0: the score of the initial pose) */
  float rel_fitness, rel_rmse;           /* stop when both changes are below these (strict <); finite, >= 0; 0 = never */
  float* R_out; float* t_out;            /* [B,3,3], [B,3], mandatory: the refined pose (src -> tgt) */
  float* fitness; float* rmse;           /* [B] each, mandatory: of the refined pose */
  float* R_ba; float* t_ba;              /* optional [B,3,3], [B,3]: its inverse, vcr_pose_step_f32's expression */
  int* inliers; double* sum_d2;          /* optional [B] each */
  int* iterations; int* converged;       /* optional [B] each: pose updates applied; 1 = stopped by the rel_* test */
  int* nn_idx; float* nn_d2;             /* optional [B,Ns] each: the neighbours under the refined pose */
  int variant;                           /* VCR_NN_SCORE_VARIANT's encoding: forces the form of the search (0 = the plan decides) */
} vcr_refine_args;

/* Bytes of workspace vcr_refine_f32 needs for these arguments (their variant included) on a device of cu_count compute units;
 * 0 for arguments the call would refuse.  cu_count 0 = the current device's; with an explicit cu_count nothing touches a
 * device. */
size_t vcr_refine_workspace_bytes(const vcr_refine_args*, int cu_count);
/* Asynchronous on the stream: no host synchronisation, no allocation; 1 + 3 (max_iterations + 1) launches, those of a cloud
 * that has stopped return at once.  workspace: device memory, 16-B aligned, at least vcr_refine_workspace_bytes(args, 0) bytes
 * (VCR_EWORKSPACE below that); its contents need not be initialised.  Limits and error codes are vcr_nn_score_f32's. */
int    vcr_refine_f32(const vcr_refine_args*, void* workspace, size_t workspace_bytes, vcr_stream_t);
/* Host-only query (nothing is launched): the form of the search -- source points per lane, target splits. */
int    vcr_refine_form(const vcr_refine_args*, int cu_count, int* queries_per_lane, int* target_splits);

#ifdef __cplusplus
}
#endif
#endif

/*
 * vcr_hip_match.h -- a pose from features alone: the nearest neighbour across two clouds in the 33-d
 * feature space of vcr_fpfh_f32 (vcr_hip_fpfh.h), and a RANSAC over the resulting correspondences -- Open3D's
 * registration_ransac_based_on_feature_matching with ransac_n = 3 and its edge-length and distance checkers.  An extension of
 * vcr_hip.h (same library, same conventions, same error codes); it adds no symbol to that header or to its other extensions and
 * moves none of their layouts, so VCR_ABI_VERSION is unchanged.
 *
 * vcr_feat_nn_f32 -- per row i of a (the source) its nearest row j of b (the target).  The result is a function of the input
 * alone: every launch form, every B and every batch returns the same bits.
 *   d_c        a[c][i] - b[c][j] in fp32, c = 0 .. 32
 *   d2         acc_0 = d_0 * d_0;  acc_c = fmaf(d_c, d_c, acc_{c-1});  d2 = acc_32      (differences: FPFH rows have squared
 *              norms of 1e4 .. 1.2e5, the expansion |a|^2 + |b|^2 - 2 a.b would spend the mantissa on them)
 *   neighbour  the smallest d2, among equal d2 the LOWEST j; a candidate replaces the best only on d2 < best, the best starts
 *              at (+inf, -1): a NaN / +inf d2 never wins, a row without a finite candidate reports (-1, +inf)
 *   rev        the same search with the roles exchanged: per row j of b its nearest row of a
 *   mutual     != 0: nn_idx[i] = j is kept iff rev[j] == i, otherwise nn_idx[i] = -1; nn_d2[i] keeps its value
 *
 * vcr_ransac_f32 -- per cloud, independently of the batch (every cloud uses the same seed):
 *   pairs      the source indices i with 0 <= corr[i] < Nt, ascending: pair_0 .. pair_{M-1}
 *   mix32(x)   x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16           (uint32, wrapping)
 *   pick_j     pair[ ((uint64)mix32(seed ^ mix32(3 t + j)) * M) >> 32 ],  j = 0, 1, 2, for trial t = 0 .. trials - 1
 *              (M == 0: the picks are -1 and the trial has status 1)
 *   status 1   two picks are equal (every trial where M < 3)
 *   status 2   similarity != 0, edge lengths: for the pick pairs (0,1), (0,2), (1,2), ds2 and dt2 are
 *              fmaf(dz, dz, fmaf(dy, dy, dx * dx)) of the fp32 differences (first minus second) of the two source points and
 *              of their two partners, s2 = similarity * similarity in fp32; the trial fails unless
 *              ds2 >= s2 * dt2 && dt2 >= s2 * ds2 for all three (fp32 products; a NaN fails)
 *   solve      vcr_hip_refine.h's step with n = 3 on the three (source point p, partner q): the fp32 values widened to fp64,
 *              every sum (x_0 + x_1) + x_2 in pick order -- S_p, S_q, S_pq = sum p q^T (the products are exact) --
 *              H = S_pq - (S_p S_q^T) * (1.0 / 3.0), the one-sided Jacobi and the tail of vcr_rigid_svd_f32's solve,
 *              t = S_q * (1.0 / 3.0) - R (S_p * (1.0 / 3.0)); a non-finite sum: R, t are NaN.  pose32 = round32(R, t)
 *   status 3   pose32 holds a non-finite value
 *   status 4   distance check: for one of the three picks d2 > max_dist * max_dist (the fp32 product), d2 by vcr_hip_score.h's
 *              `moved source` and `distance` expressions under pose32 against the pick's partner
 *   status 0   valid: count_t = the number of ALL M pairs with d2 <= max_dist * max_dist under pose32, the same expressions
 *   best       the valid trial with the highest count, among equal counts the LOWEST t.  None valid: best_trial = -1,
 *              R = I, t = 0, inliers = 0
 * trial_pose holds pose32 for a trial of status 0, 3 or 4 and twelve zeros for status 1 or 2; trial_inliers is -1 for a trial
 * that is not valid.  Against Open3D's loop: all trials run (its confidence = 1: no early stop); a trial with a repeated pick is
 * dropped, not redrawn; ties go to the lower trial, not to the lower RMSE -- counts are integers, so the choice is exact and
 * independent of the launch form.
 */
#ifndef VCR_HIP_MATCH_H
#define VCR_HIP_MATCH_H

#include "vcr_hip_score.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VCR_FEAT_NN_C 33                  /* the one feature width: any other C is VCR_EUNSUPPORTED */
#define VCR_RANSAC_MAX_TRIALS 1048576     /* 2^20 */

/* variant: VCR_NN_SCORE_VARIANT's encoding (rows of the searching side per lane: 1, 2 or 4; splits of the searched side:
 * 1 ... 128), 0 = the plan decides; it holds for both directions.  Limits and error codes are vcr_nn_score_f32's: B, Ns, Nt < 1,
 * a missing a, b or nn_idx, a bad variant: VCR_EINVAL; C != 33, Ns or Nt > 131 072, B * max(Ns, Nt) >= 2^31: VCR_EUNSUPPORTED. */
typedef struct {
  uint32_t struct_bytes;        /* sizeof(vcr_feat_nn_args) as the CALLER was compiled (see vcr_fps_args); the mandatory part
                                   ends behind rev_idx: 0, shorter than that or longer than this library knows: VCR_EINVAL */
  const float* a; const float* b;   /* [B,C,Ns], [B,C,Nt] channels-first fp32, contiguous, as vcr_fpfh_f32 writes them */
  int B, C, Ns, Nt;
  int* nn_idx; float* nn_d2;    /* [B,Ns] each; nn_d2 is optional */
  int mutual;                   /* != 0: keep only mutual neighbours in nn_idx */
  int* rev_idx;                 /* optional [B,Nt]: per row of b its nearest row of a */
  int variant;                  /* 0 = plan decides; otherwise forces a form (tests, benchmarks) */
} vcr_feat_nn_args;

/* Bytes of workspace vcr_feat_nn_f32 needs for these arguments (their variant included) on a device of cu_count compute
 * units; 0 for arguments the call would refuse.  cu_count 0 = the current device's; with an explicit cu_count nothing
 * touches a device. */
size_t vcr_feat_nn_workspace_bytes(const vcr_feat_nn_args*, int cu_count);
/* Asynchronous on the stream: no host synchronisation, no allocation.  workspace: device memory, 16-B aligned, at least
 * vcr_feat_nn_workspace_bytes(args, 0) bytes (VCR_EWORKSPACE below that); its contents need not be initialised. */
int    vcr_feat_nn_f32(const vcr_feat_nn_args*, void* workspace, size_t workspace_bytes, vcr_stream_t);
/* Host-only query (nothing is launched): the form of the a -> b search -- rows of a per lane, splits of b. */
int    vcr_feat_nn_form(const vcr_feat_nn_args*, int cu_count, int* queries_per_lane, int* target_splits);

/* B, Ns, Nt < 1, a missing src, tgt, corr, R_out or t_out, max_dist negative or not finite, similarity outside [0, 1] or NaN,
 * trials < 1: VCR_EINVAL.  trials > VCR_RANSAC_MAX_TRIALS, Ns or Nt > 131 072, B * max(Ns, Nt) >= 2^31 or
 * B * trials >= 2^29: VCR_EUNSUPPORTED. */
typedef struct {
  uint32_t struct_bytes;        /* as above; the mandatory part ends behind t_out */
  const float* src; const float* tgt;   /* [B,3,Ns], [B,3,Nt] channels-first fp32, contiguous */
  const int* corr;              /* [B,Ns]: the target index per source point; outside [0, Nt) = none */
  int B, Ns, Nt;
  float max_dist;               /* finite, >= 0 */
  float similarity;             /* 0: no edge-length test; otherwise in (0, 1] */
  int trials;                   /* T: 1 ... VCR_RANSAC_MAX_TRIALS */
  uint32_t seed;
  float* R_out; float* t_out;   /* [B,3,3], [B,3], mandatory */
  int* best_trial; int* inliers; int* pairs;   /* optional [B] each; pairs = M */
  int* trial_status;            /* optional [B,T] */
  int* trial_picks;             /* optional [B,T,3]: source indices */
  float* trial_pose;            /* optional [B,T,12]: R row-major, then t */
  int* trial_inliers;           /* optional [B,T]: count_t, -1 for a trial that is not valid */
} vcr_ransac_args;

size_t vcr_ransac_workspace_bytes(const vcr_ransac_args*, int cu_count);
/* Asynchronous on the stream: no host synchronisation, no allocation; four launches.  workspace as above. */
int    vcr_ransac_f32(const vcr_ransac_args*, void* workspace, size_t workspace_bytes, vcr_stream_t);

#ifdef __cplusplus
}
#endif
#endif

/*
 * vcr_hip_score.h -- scoring a registration on the FULL clouds: for every source point, moved by
 * the pose, its nearest target point; per cloud the fraction of source points within max_dist of the target ("fitness") and
 * the RMS residual of those points ("inlier RMSE") -- Open3D's evaluate_registration, on the device, without an Ns x Nt
 * matrix.  An extension of vcr_hip.h (same library, same conventions, same error codes); it adds no symbol to that header
 * and moves none of its layouts, so VCR_ABI_VERSION is unchanged.
 *
 * The result is a function of the input alone -- every launch form returns the same bits:
 *   moved source   p_c = fmaf(R[c][2], z, fmaf(R[c][1], y, R[c][0] * x)) + t[c]     (vcr_pose_step_f32's expression;
 *                  R == t == NULL: p is the source point itself)
 *   distance       dx = p_x - q_x, dy, dz in fp32;  d2 = fmaf(dz, dz, fmaf(dy, dy, dx * dx))    (differences, no expansion)
 *   neighbour      the smallest d2, among equal d2 the LOWEST target index; a candidate replaces the best only on d2 < best,
 *                  the best starts at (+inf, -1): a NaN / +inf d2 never wins, a source point without a finite candidate
 *                  reports index -1, d2 = +inf and is no inlier
 *   inlier         index >= 0 and d2 <= max_dist * max_dist (the fp32 product)
 *   sum_d2         the inliers' d2 in fp64: one partial per 256 consecutive source points (lane values folded by the wave
 *                  butterfly, offsets 32, 16, ... 1, then the four waves in ascending order), the partials in ascending order
 *   fitness        (float)inliers / (float)Ns            rmse   (float)sqrt(sum_d2 / inliers), 0 without inliers
 */
#ifndef VCR_HIP_SCORE_H
#define VCR_HIP_SCORE_H

#include "vcr_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* variant: 0 = the plan decides.  Otherwise bits 0-3 force the source points per lane (1, 2 or 4; 0 = the plan's) and
 * bits 8-15 the number of target splits (1 ... 128; 0 = the plan's for that many points per lane).  Any other bit or value:
 * VCR_EINVAL.  1 <= Ns, Nt <= 131 072 and B * max(Ns, Nt) < 2^31, VCR_EUNSUPPORTED beyond. */
#define VCR_NN_SCORE_VARIANT(queries_per_lane, target_splits) ((queries_per_lane) | ((target_splits) << 8))
typedef struct {
  uint32_t struct_bytes;        /* sizeof(vcr_nn_score_args) as the CALLER was compiled (see vcr_fps_args); the mandatory part
                                   ends behind rmse: 0, shorter than that or longer than this library knows: VCR_EINVAL */
  const float* src; const float* tgt;   /* [B,3,Ns], [B,3,Nt] channels-first fp32, contiguous */
  int B, Ns, Nt;
  const float* R; const float* t;       /* [B,3,3], [B,3]; both NULL = identity (src is used as it is) */
  float max_dist;                        /* inlier: d2 <= max_dist*max_dist (fp32 product); must be finite, >= 0 */
  int* nn_idx; float* nn_d2;             /* optional [B,Ns] each */
  int* inliers; double* sum_d2;          /* optional [B] each */
  float* fitness; float* rmse;           /* [B] each, mandatory */
  int variant;                           /* 0 = plan decides; otherwise forces a form (tests, benchmarks) */
} vcr_nn_score_args;

/* Bytes of workspace vcr_nn_score_f32 needs for these arguments (their variant included) on a device of cu_count compute
 * units; 0 for arguments the call would refuse.  cu_count 0 = the current device's; with an explicit cu_count nothing
 * touches a device. */
size_t vcr_nn_score_workspace_bytes(const vcr_nn_score_args*, int cu_count);
/* Asynchronous on the stream: no host synchronisation, no allocation.  workspace: device memory, 16-B aligned, at least
 * vcr_nn_score_workspace_bytes(args, 0) bytes (VCR_EWORKSPACE below that); its contents need not be initialised. */
int    vcr_nn_score_f32(const vcr_nn_score_args*, void* workspace, size_t workspace_bytes, vcr_stream_t);
/* Host-only query (nothing is launched): the form vcr_nn_score_f32 would run -- source points per lane, target splits. */
int    vcr_nn_score_form(const vcr_nn_score_args*, int cu_count, int* queries_per_lane, int* target_splits);

#ifdef __cplusplus
}
#endif
#endif

/*
 * vcr_hip_segment.h -- the dominant plane of a cloud by RANSAC and the split of the cloud along it:
 * Open3D's segment_plane with ransac_n = 3 and every trial run (probability = 1), and select_by_index(inliers) together with its
 * inverse.  An extension of vcr_hip.h (same library, same conventions, same error codes); it adds no symbol to that header or to
 * its other extensions and moves none of their layouts, so VCR_ABI_VERSION is unchanged.
 *
 * The definition.  The result is a function of the cloud alone: every B, every batch and every launch form returns the same bits,
 * and every slot of every output is written.  Per cloud:
 *   candidates   the points with three finite coordinates and (where mask is given) a mask other than 0, in ascending index
 *                order; M is their number
 *   picks        pick_j = candidate[(uint64(mix32(seed ^ mix32(3 t + j))) * M) >> 32], j = 0, 1, 2: vcr_hip_match.h's draws, same
 *                text (csrc/corr_pairs.h).  trial_picks holds the picks' point indices, -1 where M == 0
 *   status 1     two picks have the same index: every trial where M < 3
 *   trial plane  p0, p1, p2 the picks' points; e1 = p1 - p0, e2 = p2 - p0 per component in fp32, widened to fp64;
 *                n = (e1.y e2.z - e1.z e2.y, e1.z e2.x - e1.x e2.z, e1.x e2.y - e1.y e2.x) in fp64 (the products are exact);
 *                nn = (n.x n.x + n.y n.y) + n.z n.z, and likewise e1.e1 and e2.e2
 *   status 2     (collinear) nn > 2^-40 ((e1.e1) (e2.e2)) does not hold; a NaN fails
 *   unit normal  n32 = round32(n / sqrt(nn)) per component (fp64 division and square root, then one rounding to fp32)
 *   distance     for a candidate x: r = x - p0 per component in fp32; d = fmaf(n32.z, r.z, fmaf(n32.y, r.y, n32.x * r.x)).
 *                Distances come from coordinate DIFFERENCES, so a cloud far from the origin needs no centring
 *   inlier       fabsf(d) <= distance_threshold; a point that is no candidate is never an inlier
 *   count        count_t = the number of candidates that are inliers of trial t (-1 for a trial whose status is not 0)
 *   winner       the status-0 trial with the highest count, the lowest t among equals; inlier and count are the winner's
 *   no winner    best_trial -1, plane and point NaN, every inlier flag 0, count 0
 *   refit        (Open3D returns the least-squares plane of the winner's inliers.)  Where count >= 3: o = the winner's p0;
 *                the nine fp64 sums (sx sy sz sxx sxy sxz syy syz szz) of r = x - o (fp32 differences, widened; the products are
 *                exact) over the inliers.  THE ORDER, a function of N alone: the cloud is cut into blocks of 256 consecutive
 *                point indices; in a block, lane l holds point 256 blk + l's terms (zeros for a point that is no inlier or lies
 *                behind N), each wave of 64 lanes adds them by the butterfly v += v[l ^ o], o = 32, 16, 8, 4, 2, 1, and the four
 *                waves' sums are added ascending from wave 0's; then the blocks' sums are added ascending from 0.
 *                m = s / count; C = sxx / count - m.x m.x and so on; where C is finite and not all zero, csrc/normals_point.h's
 *                cyclic Jacobi (at most 16 sweeps of (0,1), (0,2), (1,2)), the column of the smallest eigenvalue (the lowest
 *                index among equals), e / sqrt((e0 e0 + e1 e1) + e2 e2) rounded to fp32, negated where its fp64 dot product
 *                ((n.x t.x + n.y t.y) + n.z t.z) with the trial's n32 is below 0.  Otherwise (count < 3, a C that is not finite
 *                or all zero, a normal that is not finite) the plane is the trial's own: normal n32, point p0
 *   outputs      plane = (n.x, n.y, n.z, d), q = o + m in fp64 (q = p0 for the trial's own plane), point = round32(q) and
 *                d = round32(-((n.x q.x + n.y q.y) + n.z q.z)) with the fp32 normal widened
 *
 * vcr_plane_ransac_f32 is asynchronous on the stream: no host synchronisation, no allocation.  Launches: the candidates (mark,
 * offsets, gather: 16-B rows (x, y, z, index) by a ballot prefix over blocks of 256), the trials (a lane a trial), the count, the
 * best (a workgroup a cloud: the maximum of (count << 32) | (0xFFFFFFFF - t)), the flags with the blocks' sums (a lane a point),
 * the refit (a workgroup a cloud: the blocks ascending, then one lane's Jacobi).
 *
 * The count's launch forms.  A trial's count is a sum of integers over the candidates, so it may be cut over the candidates in any
 * way and combined exactly (vector integer atomic adds onto the zero the trial kernel wrote).  Two forms return the same bits:
 *   VCR_PLANE_TRIAL   a lane a trial, its n32 and p0 in registers; the candidates are cut into `splits` ranges, a workgroup walks
 *                     one range for 256 trials, every candidate row the same address for all its lanes (scalar loads)
 *   VCR_PLANE_POINT   a lane holds VCR_PLANE_POINT_PER_LANE candidates in registers and walks 64 trials, each trial's values
 *                     wave-uniform (scalar loads); a trial's count in a wave is a ballot's popcount, kept by the lane of the
 *                     trial's number.  The candidates are cut into `splits` ranges here too, a workgroup per range and 64 trials
 * vcr_plane_ransac_form decides (the one place): POINT with splits = ceil(N / (256 VCR_PLANE_POINT_PER_LANE)) where
 * N >= VCR_PLANE_POINT_MIN_N or trials >= VCR_PLANE_POINT_MIN_T, else TRIAL with as many splits as bring the launch to
 * VCR_PLANE_FILL workgroups a CU, each range no shorter than VCR_PLANE_TRIAL_MIN_RANGE points.  As measured (DESIGN.md section
 * 4.25) the POINT form's count launch is the faster one at 16 384 and 131 072 points a cloud for every trial count (by up to 3.5
 * times at 10 000 trials) and at 1 024 points from some thousand trials on; the TRIAL form wins at 16 clouds of 1 024 points with
 * 100 and 1 000 trials, where ranges of 64 points were faster than ranges of 256.  variant = form | splits << 8 forces both
 * (splits 0: the plan's for that form).
 *
 * vcr_plane_split_f32 compacts a cloud twice in ascending index order by the outlier filters' tail (vcr_hip_outlier.h): the points
 * whose inlier flag is > 0, and all the others (points with non-finite coordinates included, as select_by_index(invert=True)).
 */
#ifndef VCR_HIP_SEGMENT_H
#define VCR_HIP_SEGMENT_H

#include "../vcr_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VCR_PLANE_MAX_N 131072
#define VCR_PLANE_MAX_TRIALS 1048576
#define VCR_PLANE_TRIAL 1
#define VCR_PLANE_POINT 2
#define VCR_PLANE_MAX_SPLITS 512
#define VCR_PLANE_POINT_PER_LANE 4        /* candidates a lane of the POINT form holds */
#define VCR_PLANE_POINT_MIN_N 8192        /* points a cloud from which the plan takes the POINT form */
#define VCR_PLANE_POINT_MIN_T 4096        /* ... and trials from which it takes it for smaller clouds too */
#define VCR_PLANE_FILL 4                  /* workgroups a CU the TRIAL form's splits aim at */
#define VCR_PLANE_TRIAL_MIN_RANGE 64      /* ... no range shorter than this */

/* A missing mandatory pointer, B < 1, a negative or non-finite distance_threshold, trials < 1, a bad variant, a trial_plane that
 * is not 16-B aligned, a bad struct_bytes, a workspace that is NULL, short or not 256-B aligned: VCR_EINVAL.  ransac_n != 3,
 * N outside [1, 131 072], trials > 2^20, B * N >= 2^31 or B * trials >= 2^29: VCR_EUNSUPPORTED. */
typedef struct {
  uint32_t struct_bytes;        /* sizeof(vcr_plane_ransac_args) as the CALLER was compiled (see vcr_fps_args); the mandatory part
                                   ends behind count: 0, shorter than that or longer than this library knows: VCR_EINVAL */
  const float* xyz;             /* [B,3,N] channels-first */
  const int* mask;              /* optional [B,N]: a point with mask 0 is neither drawn nor counted */
  int B, N;
  float distance_threshold;     /* >= 0, finite */
  int ransac_n;                 /* 3 */
  int trials;                   /* 1 ... 2^20 */
  uint32_t seed;
  int variant;                  /* 0 = vcr_plane_ransac_form decides; else form | splits << 8 */
  float* plane;                 /* out [B,4]: (a, b, c, d), a x + b y + c z + d = 0, (a, b, c) of unit length */
  int* inlier;                  /* out [B,N]: 1 / 0 */
  int* count;                   /* out [B] */
  float* point;                 /* optional out [B,3]: a point on the plane */
  int* best_trial;              /* optional out [B] */
  int* candidates;              /* optional out [B]: M */
  int* trial_status;            /* optional out [B,trials] */
  int* trial_picks;             /* optional out [B,trials,3] */
  float* trial_plane;           /* optional out [B,trials,8], 16-B aligned: (n32.x, n32.y, n32.z, 0, p0.x, p0.y, p0.z, 0); zeros
                                   for a trial whose status is not 0 */
  int* trial_count;             /* optional out [B,trials] */
  double* refit_sums;           /* optional out [B,9]: the refit's nine sums (zeros without a winner) */
} vcr_plane_ransac_args;

/* 0 for arguments vcr_plane_ransac_f32 refuses.  cu_count is accepted and not used (>= 0): the workspace is no form's. */
size_t vcr_plane_ransac_workspace_bytes(const vcr_plane_ransac_args*, int cu_count);
int vcr_plane_ransac_f32(const vcr_plane_ransac_args*, void* workspace, size_t workspace_bytes, vcr_stream_t);
/* Host-only query (nothing is launched), the one place that decides the count launch's form and its number of splits.  The
 * pointers of the args are not looked at.  cu_count < 0: VCR_EINVAL; 0: 256.  Either result pointer may be NULL. */
int vcr_plane_ransac_form(const vcr_plane_ransac_args*, int cu_count, int* form, int* splits);

/* A missing pointer (the two index arrays are optional), B < 1, a bad struct_bytes, a workspace that is NULL, short or not 256-B
 * aligned: VCR_EINVAL.  N outside [1, 131 072] or B * N >= 2^31: VCR_EUNSUPPORTED. */
typedef struct {
  uint32_t struct_bytes;        /* the mandatory part ends behind rest_count */
  const float* xyz;             /* [B,3,N] channels-first */
  const int* inlier;            /* [B,N]: > 0 the plane's side */
  int B, N;
  float* plane_points;          /* out [B,3,N]: the plane's points in ascending index order, NaN behind them */
  int* plane_count;             /* out [B] */
  float* rest_points;           /* out [B,3,N]: the others, likewise */
  int* rest_count;              /* out [B] */
  int* plane_index;             /* optional out [B,N]: the kept points' indices, -1 behind them */
  int* rest_index;              /* optional out [B,N] */
} vcr_plane_split_args;

size_t vcr_plane_split_workspace_bytes(const vcr_plane_split_args*, int cu_count);
int vcr_plane_split_f32(const vcr_plane_split_args*, void* workspace, size_t workspace_bytes, vcr_stream_t);

#ifdef __cplusplus
}
#endif
#endif

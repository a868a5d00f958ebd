/*
 * vcr_hip_outlier.h -- removing a cloud's stray points on the device: Open3D's
 * remove_statistical_outlier and remove_radius_outlier, the step between the voxel grid (vcr_hip_voxel.h) and the normals
 * (vcr_hip_plane.h).  An extension of vcr_hip.h (same library, same conventions, same error codes); it adds no symbol to that
 * header or to its other extensions and moves none of their layouts, so VCR_ABI_VERSION is unchanged.
 *
 * The result for a cloud is a function of that cloud and the parameters alone -- every launch form and every batch returns the
 * same bits.  Both calls end alike: the points with keep_i set are compacted in ascending index order,
 *   points[:, s]   for s < count[b] the bits of the s-th kept point, NaN behind them
 *   index[b, s]    for s < count[b] that point's index, -1 behind them
 *   count[b]       the number of kept points
 * and every slot of every output is written.
 *
 * vcr_outlier_stat_f32 -- remove_statistical_outlier(nb_neighbors = k + 1, std_ratio).  It runs no search of its own (like
 * vcr_normals_f32): idx holds point i's k neighbours; Open3D's neighbour list also holds the point itself at distance 0, so its
 * nb_neighbors is m = k + 1.  Per point i:
 *   j               an idx entry outside [0, N) reads as i
 *   dx              (double)(x_j - x_i): the fp32 difference, widened (as in vcr_normals_f32); dy, dz likewise
 *   d_ij            sqrt((dx dx + dy dy) + dz dz) in fp64
 *   s_i             the fp64 sum of d_ij in idx's order
 *   mean_dist_i     (float)(s_i / (double)m)
 *   valid           point i is valid iff mean_dist_i is finite
 * Per cloud, every sum in sum_d2's order (vcr_hip_score.h): one partial per 256 consecutive points, folded by the wave butterfly
 * with offsets 32 ... 1, then the four waves ascending, then the partials ascending; a point that is not valid adds 0:
 *   n               the number of valid points
 *   mu              (sum of (double)mean_dist_i) / n
 *   var             (sum of dev_i dev_i) / (n - 1),  dev_i = (double)mean_dist_i - mu
 *   sigma           sqrt(var); 0 when n < 2
 *   thr             mu + (double)std_ratio sigma
 *   keep_i          valid and (double)mean_dist_i <= thr
 * n = 0 gives NaN statistics and keeps nothing.  The decision is taken on the fp32 mean_dist the call returns, so everything
 * behind it can be recomputed from the outputs.  Two deliberate departures from Open3D:
 *   <=              where Open3D has <: a lattice, whose mean distances are all equal and whose sigma is 0, would lose every point
 *   mean_dist 0     (a point among its own copies) is kept: Open3D's "> 0" guards its -1 sentinel for "no neighbours", which
 *                   cannot occur here
 *
 * vcr_outlier_radius_f32 -- remove_radius_outlier(nb_points, radius):
 *   r2              radius * radius in fp32, one rounding
 *   d2(i, j)        vcr_nn_score_f32's expression on the unmoved points: dx = x_i - x_j ..., fmaf(dz, dz, fmaf(dy, dy, dx * dx))
 *   c_i             #{ j in [0, N) : d2(i, j) <= r2 }.  A finite point counts itself, as Open3D's radius search does; a
 *                   comparison with NaN is false, so a non-finite point has c_i = 0 and is counted by nobody
 *   keep_i          c_i > nb_points
 * The counts are integer sums: every split of the scan gives the same bits.
 */
#ifndef VCR_HIP_OUTLIER_H
#define VCR_HIP_OUTLIER_H

#include "vcr_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VCR_OUTLIER_MAX_K 62              /* vcr_knn_f32's limit: VCR_EUNSUPPORTED beyond */

/* B < 1, k < 1, std_ratio negative or not finite, a missing mandatory pointer or xyz4 not 16-B aligned: VCR_EINVAL.
 * k > VCR_OUTLIER_MAX_K, N outside [1, 131 072] or B * N >= 2^31: VCR_EUNSUPPORTED. */
typedef struct {
  uint32_t struct_bytes;        /* sizeof(vcr_outlier_stat_args) as the CALLER was compiled (see vcr_fps_args); the mandatory part
                                   ends behind count: 0, shorter than that or longer than this library knows: VCR_EINVAL */
  const float* xyz4;            /* [B,N,4] rows as vcr_rows4_f32 writes them, 16-B aligned; the fourth value is not read */
  const int* idx;               /* [B,N,k]: the neighbours vcr_knn_f32 wrote for C == 4 (cloud-local) */
  int B, N, k;                  /* 1 <= N <= 131 072, B N < 2^31; 1 <= k <= VCR_OUTLIER_MAX_K */
  float std_ratio;              /* finite, >= 0 */
  float* points;                /* [B,3,N] channels-first, mandatory */
  int* count;                   /* [B], mandatory */
  int* index;                   /* optional [B,N] */
  float* mean_dist;             /* optional [B,N] */
  int* valid;                   /* optional [B]: n */
  double* stats;                /* optional [B,3]: mu, sigma, thr */
} vcr_outlier_stat_args;

/* Bytes of workspace vcr_outlier_stat_f32 needs for these arguments; 0 for arguments the call would refuse.  Host only: the
 * size does not depend on the device (cu_count is taken for symmetry; negative: 0).  With up(v) = v rounded up to a multiple of
 * 256 and nblk = ceil(N / 256):
 *   up(4 B N) + up(40 B) + 2 up(8 B nblk) + 2 up(4 B nblk)
 * (mean_dist; per cloud n, mu, var, sigma, thr; per 256 points a sum of mean distances and one of squared deviations, a count of
 * valid and one of kept points). */
size_t vcr_outlier_stat_workspace_bytes(const vcr_outlier_stat_args*, int cu_count);
/* Asynchronous on the stream: no host synchronisation, no allocation.  workspace: device memory, 16-B aligned, at least
 * vcr_outlier_stat_workspace_bytes(args, 0) bytes (VCR_EWORKSPACE below that); its contents need not be initialised. */
int    vcr_outlier_stat_f32(const vcr_outlier_stat_args*, void* workspace, size_t workspace_bytes, vcr_stream_t);

/* variant: 0 = the plan decides.  Otherwise VCR_NN_SCORE_VARIANT's encoding (vcr_hip_score.h): bits 8-15 force the number of
 * segments S the scan cuts the cloud into (1 ... 128; 0 = the plan's), bits 0-3 are 0 or 1 (the scan runs one point per lane).
 * Any other bit or value, radius not finite or <= 0, or nb_points < 0: VCR_EINVAL.  1 <= N <= 131 072 and B * N < 2^31,
 * VCR_EUNSUPPORTED beyond. */
typedef struct {
  uint32_t struct_bytes;        /* as above; the mandatory part ends behind count */
  const float* xyz;             /* [B,3,N] channels-first fp32, contiguous */
  int B, N;
  float radius;                 /* finite, > 0 */
  int nb_points;                /* >= 0: a point is kept if MORE than nb_points points (itself included) lie within radius */
  float* points;                /* [B,3,N], mandatory */
  int* count;                   /* [B], mandatory */
  int* index;                   /* optional [B,N] */
  int* neighbours;              /* optional [B,N]: c_i */
  int variant;                  /* 0 = plan decides; otherwise forces a form (tests, benchmarks) */
} vcr_outlier_radius_args;

/* As vcr_voxel_workspace_bytes: for a device of cu_count compute units (0 = the current device's; with an explicit cu_count
 * nothing touches a device).  With S the segments vcr_outlier_radius_form reports:
 *   up(4 S B N) + up(4 B N) + up(4 B nblk)
 * (per segment and point a count; per point c_i; per 256 points a count of kept points). */
size_t vcr_outlier_radius_workspace_bytes(const vcr_outlier_radius_args*, int cu_count);
int    vcr_outlier_radius_f32(const vcr_outlier_radius_args*, void* workspace, size_t workspace_bytes, vcr_stream_t);
/* Host-only query (nothing is launched): the form vcr_outlier_radius_f32 would run -- points per lane (always 1), segments:
 * vcr_nn_score_form's split for (B, N, N). */
int    vcr_outlier_radius_form(const vcr_outlier_radius_args*, int cu_count, int* points_per_lane, int* splits);

#ifdef __cplusplus
}
#endif
#endif

/*
 * vcr_hip_voxel.h -- down-sampling a cloud on a voxel grid: the points that fall into one cell of a
 * grid of edge voxel_size are replaced by their mean -- Open3D's voxel_down_sample, on the device, with the order of the
 * voxels and of every sum fixed.  An extension of vcr_hip.h (same library, same conventions, same error codes); it adds no
 * symbol to that header or to its other extensions and moves none of their layouts, so VCR_ABI_VERSION is unchanged.
 *
 * The result is a function of the cloud and voxel_size (h) alone -- every launch form and every batch returns the same bits.
 * Per cloud, the points numbered in ascending index order:
 *   finite         a point is finite if its three coordinates are; any other point belongs to no voxel
 *   origin         lo_c = the fp32 minimum of coordinate c over the finite points;  origin_c = (double)lo_c - 0.5 * (double)h
 *                  (Open3D's min_bound - voxel_size / 2)
 *   cell           cell_c(i) = floor(((double)x_c(i) - origin_c) / (double)h): one fp64 subtraction, one fp64 division (no
 *                  reciprocal); never negative.  Two finite points share a voxel when their three cells are equal
 *   voxel order    a voxel's representative is its lowest point index; the voxels are numbered 0 ... M-1 by ascending
 *                  representative, that is in order of first appearance (Open3D leaves the order to a hash map)
 *   points[:, v]   per coordinate the fp64 sum over the voxel's members in ascending index order, which STARTS AS the first
 *                  member's value (not from 0), then (float)(sum / (double)n): Open3D's accumulation.  A voxel of one point
 *                  returns that point's bits, -0.0 included
 *   count[b]       M; 0 for a cloud without a finite point
 *   voxel_points   [b, v] = the voxel's number of members for v < M, 0 beyond
 *   point_voxel    [b, i] = the point's voxel number, -1 for a point that is not finite
 *   every slot of every output is written: points[:, v >= M] is NaN
 *   too fine       if the cell of any finite point would be >= 2^21 (three cells pack into one 64-bit key): count[b] = -1,
 *                  point_voxel all -1, voxel_points all 0, points all NaN -- for that cloud alone (Open3D throws there; an
 *                  asynchronous entry point cannot: vcr_rigid_svd_f32's NaN pose is the same rule)
 */
#ifndef VCR_HIP_VOXEL_H
#define VCR_HIP_VOXEL_H

#include "vcr_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VCR_VOXEL_MAX_CELLS (1 << 21)   /* cells per axis */

/* variant: 0 = the plan decides.  Otherwise VCR_NN_SCORE_VARIANT's encoding (vcr_hip_score.h): bits 8-15 force the number of
 * segments S the scan cuts the cloud into (1 ... 128; 0 = the plan's), bits 0-3 are 0 or 1 (the scan runs one point per lane).
 * Any other bit or value, or voxel_size not finite or <= 0: VCR_EINVAL.  1 <= N <= 131 072 and B * N < 2^31, VCR_EUNSUPPORTED
 * beyond. */
typedef struct {
  uint32_t struct_bytes;        /* sizeof(vcr_voxel_args) as the CALLER was compiled (see vcr_fps_args); the mandatory part ends
                                   behind count: 0, shorter than that or longer than this library knows: VCR_EINVAL */
  const float* xyz;             /* [B,3,N] channels-first fp32, contiguous */
  int B, N;
  float voxel_size;
  float* points;                /* [B,3,N], mandatory */
  int* count;                   /* [B], mandatory */
  int* point_voxel;             /* optional [B,N] */
  int* voxel_points;            /* optional [B,N] */
  int variant;                  /* 0 = plan decides; otherwise forces a form (tests, benchmarks) */
} vcr_voxel_args;

/* Bytes of workspace vcr_voxel_f32 needs for these arguments (their variant included) on a device of cu_count compute units;
 * 0 for arguments the call would refuse.  cu_count 0 = the current device's; with an explicit cu_count nothing touches a
 * device.  With up(v) = v rounded up to a multiple of 256, S the segments vcr_voxel_form reports and nblk = ceil(N / 256):
 *   up(32 B) + up(8 B N) + 2 up(4 S B N) + 4 up(4 B N) + up(4 B nblk)
 * (per cloud the grid's origin and state; a 64-bit key per point; per segment and point a (first, members) candidate; per
 * point its first match, its voxel's members, its voxel number and the voxel's representative; a count per 256 points). */
size_t vcr_voxel_workspace_bytes(const vcr_voxel_args*, int cu_count);
/* Asynchronous on the stream: no host synchronisation, no allocation.  workspace: device memory, 16-B aligned, at least
 * vcr_voxel_workspace_bytes(args, 0) bytes (VCR_EWORKSPACE below that); its contents need not be initialised. */
int    vcr_voxel_f32(const vcr_voxel_args*, void* workspace, size_t workspace_bytes, vcr_stream_t);
/* Host-only query (nothing is launched): the form vcr_voxel_f32 would run -- points per lane (always 1), segments. */
int    vcr_voxel_form(const vcr_voxel_args*, int cu_count, int* points_per_lane, int* splits);

#ifdef __cplusplus
}
#endif
#endif

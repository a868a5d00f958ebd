/*
 * vcr_hip_voxel_sort.h -- the voxel grid of vcr_hip_voxel.h by a stable device radix sort, with member lists (DESIGN.md section
 * 4.21).  An extension of vcr_hip.h (same library, same conventions, same error codes); it adds no symbol to that header or to
 * its other extensions and moves none of their layouts, so VCR_ABI_VERSION is unchanged.
 *
 * The definition is vcr_hip_voxel.h's, word for word: the finite points, the origin, the fp64 cell, the voxels in order of first
 * appearance, every sum in ascending member order starting AS the first member, the NaN padding and the too-fine rule.  points,
 * count, point_voxel and voxel_points are bit-equal to vcr_voxel_f32's.  What differs is the route -- a few passes linear in N
 * where the scan form makes two N x N ones -- and two more optional outputs, the voxels' member lists (Open3D's
 * voxel_down_sample_and_trace):
 *   members      int32 [B,N]: the indices of the finite points, voxel 0's first, then voxel 1's, ... (the voxels in order of
 *                first appearance); ascending inside every voxel; -1 behind the finite points
 *   voxel_start  int32 [B,N]: [b, v] = the slot of members[b] where voxel v begins, for v < count[b]; the number of finite
 *                points for every v beyond.  So voxel v's members are members[b, voxel_start[b, v] : voxel_start[b, v] +
 *                voxel_points[b, v]]
 *   too fine     members all -1, voxel_start all 0 (and for a cloud without a finite point)
 *
 * How it is sorted (nothing of this shows in the result).  Per cloud the largest cell of every axis gives the axis its bit width
 * w_c <= 21; a finite point's key is its three cells packed to W = w_x + w_y + w_z <= 63 bits, any other point's is the single
 * bit above them.  A least-significant-digit radix sort of (key, index) of digit width d, every pass stable, leaves every
 * voxel's members contiguous and in ascending index order; ceil((W + 1) / d) passes do, the launches are those 64 bits need.
 */
#ifndef VCR_HIP_VOXEL_SORT_H
#define VCR_HIP_VOXEL_SORT_H

#include "vcr_hip_voxel.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct {
  uint32_t struct_bytes;   /* sizeof(vcr_voxel_sort_args) as the CALLER was compiled; the mandatory part ends behind variant: 0,
                              shorter than that or longer than this library knows: VCR_EINVAL */
  int variant;             /* 0 = the plan's digit width; 4, 8 or 11 force it (tests, benchmarks); anything else: VCR_EINVAL */
  int* members;            /* optional [B,N] */
  int* voxel_start;        /* optional [B,N] */
} vcr_voxel_sort_args;

/* The three entry points take vcr_voxel_f32's args struct first, with its meaning, limits and error codes -- its variant must
 * be 0 (VCR_EINVAL otherwise: the scan's forms do not apply) --, then the sort's.  A NULL vcr_voxel_sort_args: VCR_EINVAL.
 *
 * _workspace_bytes: 0 for arguments the call would refuse; the form does not depend on the device (cu_count >= 0 is accepted
 * and ignored).  With up(v) = v rounded up to a multiple of 256, d the digit width and e the elements per lane _form reports,
 * R = 2^d, T = 256 e (the elements of one workgroup of the sort), nt = ceil(N / T) and nb = ceil(N / 256):
 *   up(64 B) + up(4 B) + up(24 B nt) + 2 up(8 B N) + 2 up(4 B N) + up(4 B R nt) + up(4 B R) + 5 up(4 B N) + 2 up(4 B nb)
 * (per cloud the grid's state and its number of passes; the bounds of every T points; the keys and the indices, twice; a digit
 * histogram per workgroup and the digits' totals; per point the slot of a representative, per voxel its first slot, the voxel
 * of a point, the members of a voxel and their count below it in its 256; two counts per 256) -- a function of (B, N, d) alone.
 * _f32: asynchronous on the stream: no host synchronisation, no allocation.  workspace: device memory, 16-B aligned, at least
 * _workspace_bytes (VCR_EWORKSPACE below that); its contents need not be initialised.  Every slot of every output is written.
 * 10 + 3 ceil(64 / d) launches whose shapes depend on (B, N, d) alone.
 * _form: host-only (nothing is launched): the digit width d, the passes launched ceil(64 / d) and the elements per lane e. */
size_t vcr_voxel_sort_workspace_bytes(const vcr_voxel_args*, const vcr_voxel_sort_args*, int cu_count);
int    vcr_voxel_sort_f32(const vcr_voxel_args*, const vcr_voxel_sort_args*, void* workspace, size_t workspace_bytes, vcr_stream_t);
int    vcr_voxel_sort_form(const vcr_voxel_args*, const vcr_voxel_sort_args*, int cu_count, int* digit_bits, int* passes, int* elements_per_lane);

#ifdef __cplusplus
}
#endif
#endif

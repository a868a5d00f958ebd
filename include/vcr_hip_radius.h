/*
 * vcr_hip_radius.h -- ALL points within a radius of every point of a cloud, searched on the cloud's uniform grid (DESIGN.md
 * section 4.22): rows of varying length in CSR form (Open3D's search_radius_vector_3d, what KDTreeSearchParamRadius asks for),
 * and the grid sibling of vcr_outlier_radius_f32 (vcr_hip_outlier.h), which counts the same hits.  An extension of vcr_hip.h
 * (same library, same conventions, same error codes); it adds no symbol to that header or to its other extensions and moves
 * none of their layouts, so VCR_ABI_VERSION is unchanged.
 *
 * The definition.  Per cloud, in fp32 without contraction (d2 is vcr_hip_grid.h's, word for word):
 *   finite       a point is finite if its three coordinates are
 *   r2           radius * radius in fp32, one rounding, as in vcr_outlier_radius_f32.  The calls of THIS header require r2 to be
 *                finite (VCR_EINVAL otherwise); the scan filter vcr_outlier_radius_f32 accepts a radius whose square overflows
 *                (every pair of finite points is then within it) -- the one input the two filters do not both accept
 *   d2(i, j)     dx = x_j - x_i,  dy = y_j - y_i,  dz = z_j - z_i,   d2 = fmaf(dz, dz, fmaf(dy, dy, dx * dx)).  The filter's
 *                x_i - x_j gives the same bits: the differences are exact negatives
 *   hit          for a finite query i, a finite j != i with d2(i, j) <= r2.  A point ON the sphere is a hit, as in the filter
 *   row i        ALL hits, ascending under the total order (d2, j).  Copies of a point are ordinary hits at d2 = 0; the query
 *                is excluded by its INDEX.  A query that is not finite has an empty row and is in nobody's row
 *   n_i, c_i     n_i = row i's length; c_i = n_i + 1 for a finite i and 0 otherwise: exactly vcr_outlier_radius_f32's c_i
 *   count        [B, N] int32: n_i
 *   row_start    [B, N + 1] int64: row_start[b, i] = the sum of n_i' over i' < i;  total[b] = row_start[b, N] (int64 [B]).
 *                Both are exact whatever the size
 *   idx, d2      [B, capacity] int32 and (optional) [B, capacity] fp32.  They are written for cloud b iff total[b] <= capacity:
 *                row i is then at row_start[b, i] ... row_start[b, i + 1], and every slot behind total[b] holds -1 / +inf.  So
 *                does every slot of a cloud that does not fit.  count, row_start and total are written whether it fits or not
 *   count only   idx == NULL asks for the counts alone; capacity must then be 0, and d2 without idx is VCR_EINVAL
 *   every slot of every output is written by the call.  The result is a function of the cloud, the radius and the capacity alone:
 *   it never depends on the grid, the launch form, the batch or the run.
 *
 * How it is searched (nothing of this shows in the result).  The grid is vcr_hip_grid.h's in every respect -- bounds, cells under
 * the budget VCR_GRID_CELLS(N), faces, cells by comparison, Chebyshev rings, the ring bound -- with two differences:
 *   edge         cell = 0 takes h = radius (one ring of 27 cells holds every hit of a query in the middle of its cell's reach);
 *                a forced cell > 0 is taken as is; either is widened under the budget as there
 *   stop         after ring r the walk stops when bound > r2, STRICTLY (an unseen point at exactly r2 is a hit), or when the
 *                grid is exhausted
 * The rows are ordered by a rank sort: the keys (d2 bits) << 32 | j of a row are distinct, so the number of keys below a key is
 * its place.  Its cost is QUADRATIC in the row's length -- meant for neighbourhoods, not for a radius that spans the cloud.
 */
#ifndef VCR_HIP_RADIUS_H
#define VCR_HIP_RADIUS_H

#include "vcr_hip_outlier.h"
#include "vcr_hip_gridnn.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VCR_RADIUS_MAX_N 131072
#define VCR_RADIUS_CHUNK 128               /* keys of a row the wave-per-row ordering stages through LDS at a time */

/* variant: 0 = the plan decides.  Otherwise bits 0-3 force the order the queries are served in (1 = in cell order, the plan's;
 * 2 = in index order) and bits 4-7 the form of the ordering (1 = a wave per row, its keys staged through LDS in chunks of
 * VCR_RADIUS_CHUNK -- the plan's, whatever the shape; 2 = a lane per row, which lost every measurement), each 0 for the plan's:
 * VCR_RADIUS_VARIANT(order, form).  Any other bit or value: VCR_EINVAL.  Every form returns the same bits.
 * VCR_EINVAL: B < 1; a missing xyz, count, row_start or total; radius not finite, <= 0, or with an infinite square; cell
 * negative, NaN or infinite; capacity < 0; idx == NULL with capacity != 0; d2 without idx.
 * VCR_EUNSUPPORTED: N outside [1, 131 072]; B * N >= 2^31; B * capacity >= 2^31. */
#define VCR_RADIUS_VARIANT(order, form) ((order) | (form) << 4)
typedef struct {
  uint32_t struct_bytes;        /* sizeof(vcr_grid_radius_args) as the CALLER was compiled (see vcr_fps_args); the mandatory part
                                   ends behind total: 0, shorter than that or longer than this library knows: VCR_EINVAL */
  const float* xyz;             /* [B,3,N] channels-first fp32, contiguous */
  int B, N;
  float radius;                 /* finite, > 0, radius * radius finite */
  float cell;                   /* 0 = the edge is the radius; a finite value > 0 forces the cells' edge */
  int capacity;                 /* slots of idx / d2 a cloud; 0 with idx == NULL */
  int* count;                   /* [B,N], mandatory: n_i */
  int64_t* row_start;           /* [B,N+1], mandatory */
  int64_t* total;               /* [B], mandatory */
  int* idx;                     /* optional [B,capacity] */
  float* d2;                    /* optional [B,capacity]; needs idx */
  int variant;                  /* 0 = plan decides; otherwise forces a form (tests, benchmarks) */
} vcr_grid_radius_args;

/* Bytes of workspace vcr_grid_radius_f32 needs for these arguments; 0 for arguments the call would refuse.  A function of
 * (B, N, capacity) alone: the form does not depend on the device (cu_count >= 0 is accepted and ignored).  With up(v) = v
 * rounded up to a multiple of 256 and G = VCR_GRID_CELLS(N):
 *   up(64 B) + up(4 B N) + up(4 B (G + 2)) + up(16 B N) + up(8 B capacity)
 * (vcr_grid_knn_workspace_bytes' grid -- the count needs nothing more a point: it writes n_i to `count` --, then a cloud's
 * unordered keys, 8 bytes a slot). */
size_t vcr_grid_radius_workspace_bytes(const vcr_grid_radius_args*, int cu_count);
/* Asynchronous on the stream: no host synchronisation, no allocation; seven launches for the counts alone, ten with idx.
 * workspace: device memory, 16-B aligned, at least vcr_grid_radius_workspace_bytes(args, 0) bytes (VCR_EWORKSPACE below that);
 * its contents need not be initialised. */
int    vcr_grid_radius_f32(const vcr_grid_radius_args*, void* workspace, size_t workspace_bytes, vcr_stream_t);
/* Host-only query (nothing is launched): the cell budget per cloud G(N), the queries a workgroup serves and the form the
 * ordering takes (1 = a wave per row, 2 = a lane per row; 0 for a call that orders nothing: idx == NULL). */
int    vcr_grid_radius_form(const vcr_grid_radius_args*, int cu_count, int* cells_per_cloud, int* queries_per_workgroup, int* order_form);

/* vcr_outlier_radius_f32's grid sibling, in the shape of vcr_hip_gridnn.h's: the scan sibling's args struct first, with its
 * meaning, limits and error codes -- its variant must be 0 (VCR_EINVAL otherwise: the scan's forms do not apply), and radius *
 * radius must be finite (VCR_EINVAL: see r2 above) --, then the grid's: cell = 0 means the radius; order 0 and 1 serve the
 * queries in cell order, 2 in index order.  A NULL vcr_grid_nn_args: VCR_EINVAL.  points, count, index and neighbours are
 * bit-equal to vcr_outlier_radius_f32's for every input both accept.
 * _workspace_bytes: up(64 B) + up(4 B N) + up(4 B (G + 2)) + up(16 B N) + up(4 B N) + up(4 B nblk), nblk = ceil(N / 256) (the
 * grid; per point c_i; per 256 points a count of kept points) -- a function of (B, N) alone.
 * _f32: nine launches (the grid's five, the count, vcr_outlier_radius_f32's mark, offsets and write).
 * _form: the cell budget G(N), the order taken (1 or 2) and the queries a workgroup serves. */
size_t vcr_outlier_radius_grid_workspace_bytes(const vcr_outlier_radius_args*, const vcr_grid_nn_args*, int cu_count);
int    vcr_outlier_radius_grid_f32(const vcr_outlier_radius_args*, const vcr_grid_nn_args*, void* workspace, size_t workspace_bytes, vcr_stream_t);
int    vcr_outlier_radius_grid_form(const vcr_outlier_radius_args*, const vcr_grid_nn_args*, int cu_count, int* cells_per_cloud, int* order, int* queries_per_workgroup);

#ifdef __cplusplus
}
#endif
#endif

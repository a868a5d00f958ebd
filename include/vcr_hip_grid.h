/*
 * vcr_hip_grid.h -- the exact k nearest neighbours of every point of a cloud among the cloud's other points, searched on a
 * uniform grid: the 3-d search in front of estimate_normals, compute_fpfh_feature and
 * remove_statistical_outlier for large clouds.  An extension of vcr_hip.h (same library, same conventions, same error codes);
 * it adds no symbol to that header or to its other extensions and moves none of their layouts, so VCR_ABI_VERSION is unchanged.
 *
 * The result is a function of the cloud and k alone -- every grid (automatic or forced), every launch form, every batch and
 * every run returns the same bits.  Per cloud:
 *   finite       a point is finite if its three coordinates are; a point that is not finite is nobody's neighbour
 *   d2(i, j)     for a finite query i and a finite candidate j != i, in fp32 without contraction:
 *                  dx = x_j - x_i,  dy = y_j - y_i,  dz = z_j - z_i,   d2 = fmaf(dz, dz, fmaf(dy, dy, dx * dx))
 *                (section 4.8's expression: differences, so any translation that is exact in fp32 leaves every d2 unchanged).
 *                A d2 that is +inf (overflow) is no candidate
 *   row i        the k smallest candidates under the total order (d2, j): ascending d2, the lower index among equals.  Copies
 *                of a point are ordinary candidates with d2 = 0.  idx[b, i, :] holds those indices in that order, d2[b, i, :]
 *                (optional) the fp32 values
 *   short rows   a query that is not finite, fewer than k candidates, k + 1 > N: the remaining slots hold the query's own index
 *                i and d2 = +inf.  So every index written is in [0, N), whatever the input
 *   every slot of every output is written by the call.
 *
 * How it is searched (nothing of this shows in the result).  Per cloud, with lo_c / hi_c the fp32 minimum / maximum of
 * coordinate c over the finite points and e_c = hi_c - lo_c:
 *   edge         cell > 0: h = cell.  cell = 0, the automatic grid: with D the number of axes with e_c > 0 and V the product of
 *                those e_c in fp64, h = (float)pow(V / N, 1 / D) -- one point a cell of the bounding box; D = 0: h = 1
 *   cells        n_c = floor(e_c / h) + 1 cells along axis c (one cell across a flat axis); while n_x n_y n_z exceeds the
 *                cell budget G(N) = VCR_GRID_CELLS(N) the edge is widened, h <- 1.25 h (never an error)
 *   faces        face_c[j] = fmaf((float)j, h, lo_c), monotone in j; a point is in cell j of axis c iff
 *                face_c[j] <= x_c < face_c[j + 1], the last cell open above -- decided by comparing against the faces
 *   prune        the cells are visited in Chebyshev rings around the query's cell (q_x, q_y, q_z).  After ring r a point not
 *                yet seen lies at or above face_c[q_c + r + 1] or below face_c[q_c - r] for some axis c; per side that exists
 *                g = face - x_q (or x_q - face), one fp32 subtraction, and bound = the minimum of g * g over those sides.
 *                The walk stops only when the row's k-th d2 is STRICTLY below bound, or when the grid is exhausted
 */
#ifndef VCR_HIP_GRID_H
#define VCR_HIP_GRID_H

#include "vcr_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VCR_GRID_MAX_K 62
#define VCR_GRID_MAX_N 131072
#define VCR_GRID_CELLS(N) (2 * (N) + 64)   /* G(N): the cells a cloud's grid may have; the workspace is sized for it */
#define VCR_GRID_QUERIES 256               /* queries a workgroup serves, one a lane */

/* variant: 0 = the plan decides.  Otherwise it forces the order the queries are served in: 1 = in cell order (the plan's: a
 * wave's queries share their neighbourhood), 2 = in index order.  Any other value: VCR_EINVAL.
 * B < 1, a missing xyz or idx, cell negative, NaN or infinite: VCR_EINVAL.  N outside [1, 131 072], B * N >= 2^31, k outside
 * [1, 62]: VCR_EUNSUPPORTED. */
typedef struct {
  uint32_t struct_bytes;        /* sizeof(vcr_grid_knn_args) as the CALLER was compiled (see vcr_fps_args); the mandatory part
                                   ends behind idx: 0, shorter than that or longer than this library knows: VCR_EINVAL */
  const float* xyz;             /* [B,3,N] channels-first fp32, contiguous */
  int B, N, k;
  float cell;                   /* 0 = the automatic grid; a finite value > 0 forces the cells' edge */
  int* idx;                     /* [B,N,k], mandatory */
  float* d2;                    /* optional [B,N,k] */
  int variant;                  /* 0 = plan decides; otherwise forces a form (tests, benchmarks) */
} vcr_grid_knn_args;

/* Bytes of workspace vcr_grid_knn_f32 needs for these arguments; 0 for arguments the call would refuse.  The form does not
 * depend on the device: with an explicit cu_count (> 0) nothing touches one, and cu_count 0 asks for the same number.  With
 * up(v) = v rounded up to a multiple of 256 and G = VCR_GRID_CELLS(N):
 *   up(64 B) + up(4 B N) + up(4 B (G + 2)) + up(16 B N)
 * (per cloud the grid; per point its cell; per cloud a zero, a counter per cell and one for the points that are not finite;
 * per point its (x, y, z, index) in cell order). */
size_t vcr_grid_knn_workspace_bytes(const vcr_grid_knn_args*, int cu_count);
/* Asynchronous on the stream: no host synchronisation, no allocation; six launches.  workspace: device memory, 16-B aligned,
 * at least vcr_grid_knn_workspace_bytes(args, 0) bytes (VCR_EWORKSPACE below that); its contents need not be initialised. */
int    vcr_grid_knn_f32(const vcr_grid_knn_args*, void* workspace, size_t workspace_bytes, vcr_stream_t);
/* Host-only query (nothing is launched): the cell budget per cloud G(N) and the queries a workgroup serves. */
int    vcr_grid_knn_form(const vcr_grid_knn_args*, int cu_count, int* cells_per_cloud, int* queries_per_workgroup);

#ifdef __cplusplus
}
#endif
#endif

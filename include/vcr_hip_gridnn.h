/*
 * vcr_hip_gridnn.h -- scoring and refining a registration with the nearest neighbour searched on the TARGET's uniform grid and
 * CAPPED at max_dist: vcr_nn_score_f32 and the three refinements (vcr_hip_score.h, vcr_hip_refine.h,
 * vcr_hip_plane.h, vcr_hip_gicp.h) with another search in front of the same merge, fits, solves and stop test.  An extension of
 * vcr_hip.h (same library, same conventions, same error codes); it adds no symbol to that header or to its other extensions
 * and moves none of their layouts, so VCR_ABI_VERSION is unchanged.
 *
 * The definition is vcr_nn_score_f32's (include/vcr_hip_score.h) with ONE difference.  The moved source point, d2 (differences,
 * d2 = fmaf(dz, dz, fmaf(dy, dy, dx * dx)) of p - q), "the smallest d2, the LOWEST target index among equals", the inlier test
 * index >= 0 and d2 <= cap2 = max_dist * max_dist (the fp32 product), sum_d2 and its order, fitness and rmse are that header's,
 * word for word.
 *   the difference   a source point whose nearest target point is no inlier (d2 > cap2) reports nn_idx = -1, nn_d2 = +inf,
 *                    where the scan form reports the far neighbour it found.  So does a moved point that is not finite (a NaN
 *                    pose, a NaN source point) and a point without a finite candidate, as there
 * So the inliers are the same points with the same bits: inliers, sum_d2, fitness, rmse, every sum of every fit, every pose,
 * iterations and converged are bit-equal to the scan form's, and nn_idx / nn_d2 equal the scan form's after its non-inlier
 * rows are overwritten with (-1, +inf).  The result is a function of the input alone: it does not depend on the grid (the
 * automatic or a forced edge), the order the queries are served in, the batch or the run.
 *
 * How it is searched (nothing of this shows in the result).  The grid is the target's, vcr_hip_grid.h's in every respect: lo_c,
 * hi_c the fp32 minimum / maximum over the finite target points, the edge h, the cells n_c under the budget
 * VCR_GRID_CELLS(Nt), the faces face_c[j] = fmaf((float)j, h, lo_c), a target point in cell j iff face_c[j] <= x_c < face_c[j+1],
 * target points that are not finite in no cell.  The query is a moved source point x_q and may lie outside the box:
 *   query cell     per axis by the face rule; below lo_c: cell 0; at or above the last face: n_c - 1
 *   ring bound     vcr_hip_grid.h's: after ring r, per side that exists g = face - x_q (or x_q - face) >= 0, one fp32
 *                  subtraction, and the minimum of g * g over those sides
 *   outside bound  o_c = lo_c - x_q where x_q < lo_c, x_q - hi_c where x_q > hi_c, 0 otherwise; out = max_c fl(o_c * o_c).
 *                  Every target point has d2 >= out
 *   stops          after ring r, with bound = max(ring bound, out): the best d2 is STRICTLY below bound; or bound is STRICTLY
 *                  above cap2; or the grid is exhausted.  A query with out > cap2, or that is not finite, walks nothing
 *   written        (j, d2) of the best where d2 <= cap2, (-1, +inf) otherwise -- also where a candidate beyond the cap was seen
 */
#ifndef VCR_HIP_GRIDNN_H
#define VCR_HIP_GRIDNN_H

#include "vcr_hip_score.h"
#include "vcr_hip_refine.h"
#include "vcr_hip_plane.h"
#include "vcr_hip_gicp.h"
#include "vcr_hip_grid.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct {
  uint32_t struct_bytes;   /* sizeof(vcr_grid_nn_args) as the CALLER was compiled; the mandatory part is all of it today: 0,
                              shorter than that or longer than this library knows: VCR_EINVAL */
  float cell;              /* 0 = the target's automatic edge (vcr_hip_grid.h's rule); a finite value > 0 forces it; negative,
                              NaN or infinite: VCR_EINVAL */
  int order;               /* 0 = the plan decides (vcr_nn_score_grid: index order; the refinements: the source's order for
                              max_iterations >= 7, index order below); 1 = the queries are served in the cell order of the
                              SOURCE cloud (built once a call, in the source's own frame); 2 = in index order; anything
                              else: VCR_EINVAL */
} vcr_grid_nn_args;

/* Four families, each the grid sibling of the scan entry points of the same name: the scan sibling's args struct first, with
 * its meaning, limits and error codes -- its variant must be 0 (VCR_EINVAL otherwise: the scan's forms do not apply) --, then
 * the grid's.  A NULL vcr_grid_nn_args: VCR_EINVAL.
 *
 * _workspace_bytes: 0 for arguments the call would refuse; the form does not depend on the device (cu_count >= 0 is accepted
 * and ignored).  With up(v) = v rounded up to a multiple of 256, nb = ceil(Ns / 256), G(N) = VCR_GRID_CELLS(N),
 *   cloud(N) = up(64 B) + up(4 B N) + up(4 B (G(N) + 2)) + up(16 B N)                  (vcr_grid_knn_workspace_bytes')
 *   grid     = cloud(Nt), and + cloud(Ns) with order 1 (order 0: as the plan decides, see _form)
 *   vcr_nn_score_grid:        2 up(4 B Ns) + up(16 B nb) + grid
 *   vcr_refine_grid:          2 up(4 B Ns) + up(8 V B nb) + up(96 B) + up(8 B) + 2 up(4 B) + grid,  V = 17
 *   vcr_refine_plane_grid, vcr_refine_gicp_grid: the same with V = 29
 * (the scan sibling's workspace at one target split, then the grids) -- a function of (B, Ns, Nt, order) alone.
 * _f32: asynchronous on the stream: no host synchronisation, no allocation.  workspace: device memory, 16-B aligned, at least
 * _workspace_bytes (VCR_EWORKSPACE below that); its contents need not be initialised.  The grids are built once a call, in
 * front of round 0: five launches for the target, six more for the source's order.
 * _form: host-only (nothing is launched): the target's cell budget G(Nt), the order taken (1 or 2) and the queries a workgroup
 * serves. */
size_t vcr_nn_score_grid_workspace_bytes(const vcr_nn_score_args*, const vcr_grid_nn_args*, int cu_count);
int    vcr_nn_score_grid_f32(const vcr_nn_score_args*, const vcr_grid_nn_args*, void* workspace, size_t workspace_bytes, vcr_stream_t);
int    vcr_nn_score_grid_form(const vcr_nn_score_args*, const vcr_grid_nn_args*, int cu_count, int* cells_per_cloud, int* order, int* queries_per_workgroup);

size_t vcr_refine_grid_workspace_bytes(const vcr_refine_args*, const vcr_grid_nn_args*, int cu_count);
int    vcr_refine_grid_f32(const vcr_refine_args*, const vcr_grid_nn_args*, void* workspace, size_t workspace_bytes, vcr_stream_t);
int    vcr_refine_grid_form(const vcr_refine_args*, const vcr_grid_nn_args*, int cu_count, int* cells_per_cloud, int* order, int* queries_per_workgroup);

size_t vcr_refine_plane_grid_workspace_bytes(const vcr_refine_plane_args*, const vcr_grid_nn_args*, int cu_count);
int    vcr_refine_plane_grid_f32(const vcr_refine_plane_args*, const vcr_grid_nn_args*, void* workspace, size_t workspace_bytes, vcr_stream_t);
int    vcr_refine_plane_grid_form(const vcr_refine_plane_args*, const vcr_grid_nn_args*, int cu_count, int* cells_per_cloud, int* order, int* queries_per_workgroup);

size_t vcr_refine_gicp_grid_workspace_bytes(const vcr_refine_gicp_args*, const vcr_grid_nn_args*, int cu_count);
int    vcr_refine_gicp_grid_f32(const vcr_refine_gicp_args*, const vcr_grid_nn_args*, void* workspace, size_t workspace_bytes, vcr_stream_t);
int    vcr_refine_gicp_grid_form(const vcr_refine_gicp_args*, const vcr_grid_nn_args*, int cu_count, int* cells_per_cloud, int* order, int* queries_per_workgroup);

#ifdef __cplusplus
}
#endif
#endif

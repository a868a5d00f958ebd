/*
 * vcr_hip_query.h -- neighbours of ANY query positions in a cloud, searched on the cloud's uniform grid (DESIGN.md section
 * 4.28): the k nearest points, and ALL points within a radius as rows of varying length in CSR form.  What Open3D's
 * search_knn_vector_3d / search_radius_vector_3d answer for a query that is not a point of the cloud, for every query at once.
 * An extension of vcr_hip.h (same library, same conventions, same error codes); it adds no symbol to that header or to its other
 * extensions and moves none of their layouts, so VCR_ABI_VERSION is unchanged.
 *
 * The searches of vcr_hip_grid.h and vcr_hip_radius.h look a cloud's own points up among its other points: query i IS point i
 * and is excluded from its row by its index.  Here the queries are positions of their own.
 *
 * The definition.  Per cloud b the points are xyz [B,3,N] and the queries are queries [B,3,M], both fp32 channels-first.  In
 * fp32 without contraction (d2 is vcr_hip_grid.h's, word for word):
 *   finite       a point or a query is finite if its three coordinates are.  A point that is not finite is in nobody's row
 *   d2(i, j)     for a finite query i and a finite point j:  dx = x_j - q_i,  dy, dz likewise,
 *                d2 = fmaf(dz, dz, fmaf(dy, dy, dx * dx)).  Differences: a translation of BOTH clouds that is exact in fp32
 *                changes no bit.  A d2 that is +inf (overflow) is no candidate
 *   no self      a query is a position, not an index: a point that coincides with it is an ordinary candidate at d2 = 0
 *   kNN row i    the k smallest candidates under the total order (d2, j): ascending d2, the lower index among equals.
 *                idx [B,M,k] int32, d2 [B,M,k] fp32 (optional)
 *   short rows   a query that is not finite, fewer than k candidates, k > N: the remaining slots hold idx = -1 and d2 = +inf.
 *                (The self search of vcr_hip_grid.h fills them with the query's own index; a query has no index in the cloud,
 *                so this search follows vcr_hip_gridnn.h's -1.)
 *   radius row i ALL candidates with d2 <= r2, ascending in (d2, j);  r2 = radius * radius is the fp32 product, one rounding,
 *                and must be finite.  A point ON the sphere is in the row
 *   CSR          over the M queries, exactly as vcr_hip_radius.h defines it over the N points: count [B,M] int32 (the row's
 *                length n_i); row_start [B,M+1] int64, row_start[b,i] = the sum of n_i' over i' < i; total [B] int64 =
 *                row_start[b,M]; idx / d2 [B,capacity].  The rows are written for cloud b iff total[b] <= capacity: row i is
 *                then at row_start[b,i] ... row_start[b,i+1], and every slot behind total[b] holds -1 / +inf.  So does every
 *                slot of a cloud that does not fit.  count, row_start and total are written whether it fits or not
 *   count only   idx == NULL asks for the counts alone; capacity must then be 0, and d2 without idx is VCR_EINVAL
 *   every slot of every output is written by the call.  The result is a function of the two clouds and k / radius / capacity
 *   alone: it never depends on the grid (automatic or forced `cell`), the order the queries are served in, the launch form, the
 *   batch or the run.
 *
 * How it is searched (nothing of this shows in the result).  The grid is built over the POINTS, as vcr_hip_grid.h describes it:
 * bounds, cells under the budget G(N), faces, cells by comparison, Chebyshev rings, the ring bound.
 *   edge         kNN: vcr_hip_grid.h's rule (cell = 0: one point a cell of the bounding box).  Radius: cell = 0 takes h = radius
 *   query cell   per axis by the face rule, clamped: below lo_c it is cell 0, at or above the last face it is n_c - 1 (the rule
 *                of vcr_hip_gridnn.h)
 *   outside      o_c = lo_c - x_q below the box, x_q - hi_c above it, 0 inside, one fp32 subtraction an axis: no point of the
 *                cloud is nearer along axis c.  out = the largest o_c * o_c (vcr_hip_gridnn.h's outside bound)
 *   ring bound   after ring r a point not yet seen lies behind a side that exists (vcr_hip_grid.h's: face_c[q_c + r + 1] or
 *                face_c[q_c - r], with g = face - x_q or x_q - face >= 0 for a clamped cell too; a side that does not exist
 *                contributes nothing).  Its difference along c is at least m_c = max(g, o_c) and along the other axes at least
 *                m_a = o_a, and d2's expression is monotone in each (every fp32 rounding is), so the side's term is
 *                fmaf(m_z, m_z, fmaf(m_y, m_y, m_x * m_x)) and bound = the smallest term.  For a query inside the box (o = 0)
 *                every term is g * g: vcr_hip_grid.h's bound, bit for bit.  For one outside it this is what lets the walk stop
 *                after the few rings that hold its neighbours instead of crossing the grid.  bound >= out always
 *   kNN stop     after ring r, when the row's k-th d2 is STRICTLY below bound, or when the grid is exhausted
 *   radius stop  after ring r, when bound > r2 STRICTLY, or when the grid is exhausted
 *   no walk      a query that is not finite; every query of a cloud without a finite point; radius: a query with out > r2;
 *                kNN: a query with out = +inf (every d2 overflows)
 *   order        the queries are served one a lane.  Order 1: in the order of their clamped cells IN THE POINTS' GRID, by one
 *                counting sort a call (a wave's lanes then walk the same cells); order 2: in index order (no sort)
 * The radius rows are ordered by vcr_hip_radius.h's rank sort, a wave a row: its cost is QUADRATIC in a row's length.
 */
#ifndef VCR_HIP_QUERY_H
#define VCR_HIP_QUERY_H

#include "../vcr_hip.h"
#include "../vcr_hip_grid.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VCR_QUERY_MAX_N 131072             /* points a cloud, and queries a cloud */
#define VCR_QUERY_MAX_K 62
#define VCR_QUERY_CHUNK 128                /* keys of a row the ordering stages through LDS at a time */

/* variant (both structs): 0 = the plan decides the order the queries are served in; 1 = in the order of their cells in the
 * points' grid; 2 = in index order.  Any other value: VCR_EINVAL.  Both orders return the same bits.
 *
 * vcr_query_knn_*.  VCR_EINVAL: B < 1; a missing xyz, queries or idx; cell negative, NaN or infinite.  VCR_EUNSUPPORTED: N or M
 * outside [1, 131 072]; B * N >= 2^31; B * M >= 2^31; k outside [1, 62]. */
typedef struct {
  uint32_t struct_bytes;        /* sizeof(vcr_query_knn_args) as the CALLER was compiled (see vcr_fps_args); the mandatory part
                                   ends behind idx: 0, shorter than that or longer than this library knows: VCR_EINVAL */
  const float* xyz;             /* [B,3,N] channels-first fp32, contiguous: the points */
  const float* queries;         /* [B,3,M] channels-first fp32, contiguous: the positions asked about */
  int B, N, M, k;
  float cell;                   /* 0 = the automatic grid; a finite value > 0 forces the cells' edge */
  int* idx;                     /* [B,M,k], mandatory */
  float* d2;                    /* optional [B,M,k] */
  int variant;                  /* 0 = plan decides; otherwise forces the queries' order (tests, benchmarks) */
} vcr_query_knn_args;

/* vcr_query_radius_*.  VCR_EINVAL: B < 1; a missing xyz, queries, count, row_start or total; radius not finite, <= 0, or with
 * an infinite square; cell negative, NaN or infinite; capacity < 0; idx == NULL with capacity != 0; d2 without idx.
 * VCR_EUNSUPPORTED: N or M outside [1, 131 072]; B * N >= 2^31; B * M >= 2^31; B * capacity >= 2^31. */
typedef struct {
  uint32_t struct_bytes;        /* sizeof(vcr_query_radius_args) as the CALLER was compiled; the mandatory part ends behind
                                   total: 0, shorter than that or longer than this library knows: VCR_EINVAL */
  const float* xyz;             /* [B,3,N] */
  const float* queries;         /* [B,3,M] */
  int B, N, M;
  float radius;                 /* finite, > 0, radius * radius finite */
  float cell;                   /* 0 = the edge is the radius; a finite value > 0 forces the cells' edge */
  int capacity;                 /* slots of idx / d2 a cloud; 0 with idx == NULL */
  int* count;                   /* [B,M], mandatory: n_i */
  int64_t* row_start;           /* [B,M+1], mandatory */
  int64_t* total;               /* [B], mandatory */
  int* idx;                     /* optional [B,capacity] */
  float* d2;                    /* optional [B,capacity]; needs idx */
  int variant;                  /* 0 = plan decides; otherwise forces the queries' order (tests, benchmarks) */
} vcr_query_radius_args;

/* Bytes of workspace the _f32 call needs for these arguments; 0 for arguments it would refuse.  A function of (B, N, M) --
 * for the radius search (B, N, M, capacity) -- alone: neither the order nor the device enters (cu_count >= 0 is accepted and
 * ignored).  With up(v) = v rounded up to a multiple of 256 and G = VCR_GRID_CELLS(N):
 *   kNN      up(64 B) + up(4 B N) + up(4 B (G + 2)) + up(16 B N)  +  up(4 B M) + up(4 B (G + 2)) + up(16 B M)
 *   radius   the same + up(8 B capacity)
 * (the points' grid as vcr_hip_grid.h lays it out; then per query its cell, per cloud the queries' counters over the same
 * cells, per query its (x, y, z, index) in cell order; then a cloud's unordered keys, 8 bytes a slot). */
size_t vcr_query_knn_workspace_bytes(const vcr_query_knn_args*, int cu_count);
size_t vcr_query_radius_workspace_bytes(const vcr_query_radius_args*, int cu_count);
/* Asynchronous on the stream: no host synchronisation, no allocation.  Launches: the grid's five, four more for the queries'
 * order where it is 1, then the search (kNN: one; radius: the count and the offsets, and with idx the fill, the ordering and
 * the pad).  workspace: device memory, 16-B aligned, at least _workspace_bytes(args, 0) bytes (VCR_EWORKSPACE below that); its
 * contents need not be initialised.  The argument checks return before any device call. */
int    vcr_query_knn_f32(const vcr_query_knn_args*, void* workspace, size_t workspace_bytes, vcr_stream_t);
int    vcr_query_radius_f32(const vcr_query_radius_args*, void* workspace, size_t workspace_bytes, vcr_stream_t);
/* Host-only query (nothing is launched): the cell budget per cloud G(N) and the order the queries are served in (1 or 2). */
int    vcr_query_knn_form(const vcr_query_knn_args*, int cu_count, int* cells_per_cloud, int* query_order);
int    vcr_query_radius_form(const vcr_query_radius_args*, int cu_count, int* cells_per_cloud, int* query_order);

#ifdef __cplusplus
}
#endif
#endif

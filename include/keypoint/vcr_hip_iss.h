/*
 * vcr_hip_iss.h -- keypoints by Intrinsic Shape Signatures (Zhong 2009; Open3D's compute_iss_keypoints) over neighbourhoods given
 * as ragged rows: the saliency of every point from the eigenvalues of its neighbourhood's covariance, the
 * non-maximum suppression over a row, and the compaction of a cloud to its keypoints.  An extension of vcr_hip.h (same library,
 * same conventions, same error codes); it adds no symbol to that header or to its other extensions and moves none of their
 * layouts, so VCR_ABI_VERSION is unchanged.
 *
 * The rows are those of ext/vcr_hip_rows.h.  Per cloud b:
 *   idx          int32 [B,capacity]; row_start int64 [B,N+1]; total int64 [B] -- exactly what vcr_grid_radius_f32 writes, but any
 *                caller may build them.  Point i's row is idx[b, row_start[b,i] ... row_start[b,i+1]), n_i entries
 *   entry        an entry outside [0, N) reads as i, as in the fixed-width calls
 *   no radius    the saliency knows no radius and re-tests no distance: the row IS the neighbourhood
 *   served       cloud b is served iff 0 <= total[b] <= capacity, row_start[b,0] == 0, row_start[b,N] == total[b] and
 *                row_start[b,i] <= row_start[b,i+1] for every i.  No idx entry of a cloud that is not served is read.  The other
 *                clouds of the batch are unaffected
 *
 * SALIENCY (vcr_rows_iss_saliency_f32) of point i over its row of n_i entries, m = n_i + 1 (the point counts itself, as Open3D's
 * radius search returns it):
 *   d_e          = x_{row[e]} - x_i, each component subtracted in fp32 and widened to fp64
 *   terms        the nine values dx, dy, dz, dx dx, dx dy, dx dz, dy dy, dy dz, dz dz of an entry; the products are exact in fp64
 *   64 chains    chain p (p = 0 ... 63) starts at +0.0 and adds, term by term, the entries e = p, p + 64, p + 128, ... in
 *                ascending e.  Then six combining steps s = 32, 16, 8, 4, 2, 1, each v[p] = v[p] + v[p ^ s] for all p at once.
 *                IEEE addition is commutative, so after the last step every chain holds the same nine sums S_d (3), S_dd (6).
 *                THIS ORDER IS THE DEFINITION; a row shorter than 64 leaves chains at +0.0
 *   C            = S_dd / m - (S_d / m)(S_d / m)^T in fp64: mean_a = S_a / m, C_ab = S_ab / m - mean_a * mean_b (vcr_normals_f32's
 *                expressions, vcr_hip_plane.h)
 *   lambda       l0 <= l1 <= l2: the diagonal of C after vcr_normals_f32's cyclic Jacobi -- at most 16 sweeps over the pairs
 *                (0,1), (0,2), (1,2), stopping when the three off-diagonal entries are exactly zero, each rotation by the smaller
 *                root t of t^2 + 2 theta t - 1 = 0 -- sorted as there (the lowest index among equals first)
 *   eigen[i]     (0, 0, 0) where m < min_neighbors; otherwise (NaN, NaN, NaN) where an entry of C is not finite; otherwise
 *                (0, 0, 0) where all of C is zero; otherwise (l0, l1, l2)
 *   saliency[i]  l0 where m >= min_neighbors, C is finite and not all zero, l1 / l2 < gamma_21 and l0 / l1 < gamma_32 (divisions
 *                and comparisons in fp64; a NaN ratio fails); otherwise +0.0.  A negative l0 (rounding on a plane) stays negative
 *                and is never a keypoint below
 *   not served   every saliency and every eigenvalue of the cloud is NaN
 *
 * NON-MAXIMUM SUPPRESSION (vcr_rows_iss_nms_f32) over rows that may be the same or others:
 *   used         all n_i entries of row i where d2 is NULL; otherwise its leading entries e with d2[b, row_start[b,i] + e] <=
 *                r2_nm (fp32; the first entry that fails ends them), u_i of them.  vcr_grid_radius_f32's rows ascend in
 *                (d2, index), so this prefix is bit for bit the row a search at a radius r' <= r with r' * r' == r2_nm returns:
 *                one search serves the saliency and the suppression
 *   keypoint[i]  1 iff saliency[i] > 0, u_i + 1 >= min_neighbors and no used entry j (an entry outside [0, N) reads as i) has
 *                saliency[i] < saliency[j]; otherwise 0.  The comparison is strict: copies of a point keep each other, as in
 *                Open3D's IsLocalMaxima
 *   voided       a cloud that is not served, or of which ANY saliency is NaN, gets VCR_ISS_NOT_SERVED in every slot
 * The result is free of any order: every launch form returns the same bits.
 *
 * SELECTION (vcr_iss_select_f32): the points with keypoint > 0, compacted in ascending index order by the outlier filters' tail:
 * the (points, count, index) of vcr_hip_outlier.h.  A voided cloud gives count 0.
 *
 * All three are asynchronous on the stream: no host synchronisation, no allocation, no atomics.  The first two take no workspace
 * and are two launches each: the pass, and a check of row_start (and of the saliency) that voids a cloud.
 *
 * Launch forms.  The saliency has ONE form, a wave a row with lane p running chain p: another shape would be another summation
 * order, hence another definition.  The suppression has two that return the same bits:
 *   VCR_ISS_LANE   a lane a row; it stops at the first entry that ends the prefix or blocks the point
 *   VCR_ISS_WAVE   a wave a row, 64 entries a step, the prefix and the blockers by a ballot
 * vcr_rows_iss_form decides from the row length the host can see without a synchronisation, est = capacity / N: wave where
 * est >= VCR_ISS_WAVE_NMS, lane below; variant forces either.  As measured (profiles/iss_bench.txt) the
 * wave form won nowhere -- level with the lane form at 16 x 1 024 points, 1.3 to 2.2 times slower from 16 x 16 384 on, at 28 and
 * at 146 entries a row alike: a lane leaves its row at the first blocker -- so the threshold lies above every row the limits
 * allow and only variant reaches the wave form.
 */
#ifndef VCR_HIP_ISS_H
#define VCR_HIP_ISS_H

#include "../vcr_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VCR_ISS_MAX_N 131072
#define VCR_ISS_LANE 1
#define VCR_ISS_WAVE 2
#define VCR_ISS_WAVE_NMS 131072           /* est at and above which the suppression takes the wave form: no row is that long --
                                             the form won no measurement */
#define VCR_ISS_NOT_SERVED (-2)

/* The two passes: B < 1, a missing mandatory pointer (idx may be NULL where capacity == 0; eigen and d2 are optional), capacity < 0,
 * min_neighbors < 1, a gamma that is not finite and > 0, an r2_nm that is not >= 0 where d2 is given, a variant other than 0,
 * VCR_ISS_LANE or VCR_ISS_WAVE, a bad struct_bytes, xyz4 not 16-B aligned: VCR_EINVAL.  N outside [1, 131 072], B * N >= 2^31 or
 * B * capacity >= 2^31: VCR_EUNSUPPORTED. */
typedef struct {
  uint32_t struct_bytes;        /* sizeof(vcr_rows_iss_saliency_args) as the CALLER was compiled (see vcr_fps_args); the mandatory
                                   part ends behind saliency: 0, shorter than that or longer than this library knows: VCR_EINVAL */
  const float* xyz4;            /* [B,N,4] rows as vcr_rows4_f32 writes them, 16-B aligned; the fourth value is not read */
  const int* idx;               /* [B,capacity] */
  const int64_t* row_start;     /* [B,N+1] */
  const int64_t* total;         /* [B] */
  int B, N, capacity;
  int min_neighbors;            /* >= 1, held against m = n_i + 1 */
  double gamma_21, gamma_32;    /* finite and > 0 */
  double* saliency;             /* out [B,N], mandatory */
  double* eigen;                /* optional out [B,N,3]: l0, l1, l2 */
} vcr_rows_iss_saliency_args;

int vcr_rows_iss_saliency_f32(const vcr_rows_iss_saliency_args*, vcr_stream_t);

typedef struct {
  uint32_t struct_bytes;        /* every field is part of the struct: 0, shorter or longer than this library knows: VCR_EINVAL */
  const int* idx;               /* [B,capacity] */
  const int64_t* row_start;     /* [B,N+1] */
  const int64_t* total;         /* [B] */
  const double* saliency;       /* [B,N] */
  const float* d2;              /* optional [B,capacity]: the entries' squared distances, ascending inside a row */
  int B, N, capacity;
  int min_neighbors;            /* >= 1, held against u_i + 1 */
  float r2_nm;                  /* read where d2 is given: >= 0 (+inf uses every entry) */
  int variant;                  /* 0 = vcr_rows_iss_form decides; VCR_ISS_LANE / VCR_ISS_WAVE force a form (tests, benchmarks) */
  int* keypoint;                /* out [B,N]: 1 / 0, VCR_ISS_NOT_SERVED over a voided cloud */
} vcr_rows_iss_nms_args;

int vcr_rows_iss_nms_f32(const vcr_rows_iss_nms_args*, vcr_stream_t);

/* Host-only query (nothing is launched), the one place that decides: the form the suppression takes (VCR_ISS_LANE or VCR_ISS_WAVE)
 * for these numbers.  cu_count >= 0 is accepted and not used today: the rule is the row length's alone.  The limits and error
 * codes are the passes'; cu_count < 0: VCR_EINVAL.  nms_form may be NULL. */
int vcr_rows_iss_form(int B, int N, int capacity, int cu_count, int variant, int* nms_form);

/* B < 1, a missing pointer (index is optional), a bad struct_bytes, a workspace that is NULL, short or not 256-B aligned: VCR_EINVAL.
 * N outside [1, 131 072] or B * N >= 2^31: VCR_EUNSUPPORTED. */
typedef struct {
  uint32_t struct_bytes;        /* the mandatory part ends behind count */
  const float* xyz;             /* [B,3,N] channels-first */
  const int* keypoint;          /* [B,N] as vcr_rows_iss_nms_f32 wrote them: kept where > 0 */
  int B, N;
  float* points;                /* out [B,3,N]: the kept points in ascending index order, NaN behind them */
  int* count;                   /* out [B] */
  int* index;                   /* optional out [B,N]: the kept points' indices, -1 behind them */
} vcr_iss_select_args;

/* 0 for arguments vcr_iss_select_f32 refuses.  cu_count is accepted and not used today (>= 0). */
size_t vcr_iss_select_workspace_bytes(const vcr_iss_select_args*, int cu_count);
int vcr_iss_select_f32(const vcr_iss_select_args*, void* workspace, size_t workspace_bytes, vcr_stream_t);

#ifdef __cplusplus
}
#endif
#endif

/*
 * vcr_hip_rows.h -- normals and FPFH over neighbourhoods given as ragged rows: the consumers of
 * vcr_grid_radius_f32's CSR output (vcr_hip_radius.h).  vcr_normals_f32 (vcr_hip_plane.h), vcr_spfh_f32 and vcr_fpfh_f32
 * (vcr_hip_fpfh.h) take a fixed-width idx [B,N,k] with k <= 62; these three take (idx, row_start, total) instead, so a pure
 * radius neighbourhood (Open3D's KDTreeSearchParamRadius) and a hybrid one with any max_nn (KDTreeSearchParamHybrid) are served,
 * with rows of any length below N.  An extension of vcr_hip.h (same library, same conventions, same error codes); it adds no
 * symbol to that header or to its other extensions and moves none of their layouts, so VCR_ABI_VERSION is unchanged.  Public
 * headers added from here on live in include/ext/ and include their base by its relative path.
 *
 * The rows, common to all three calls.  Per cloud b:
 *   idx          int32 [B,capacity]; row_start int64 [B,N+1]; total int64 [B] -- exactly what vcr_grid_radius_f32 writes, but any
 *                caller may build them.  Point i's row is idx[b, row_start[b,i] ... row_start[b,i+1]), n_i entries
 *   L_i          min(n_i, max_nn) where max_nn > 0, n_i where max_nn == 0: point i uses the FIRST L_i entries of its row
 *   entry        an entry outside [0, N) reads as i, as in the fixed-width calls
 *   no radius    the kernels know no radius and re-test no distance: the row IS the neighbourhood
 *   served       cloud b is served iff 0 <= total[b] <= capacity, row_start[b,0] == 0, row_start[b,N] == total[b] and
 *                row_start[b,i] <= row_start[b,i+1] for every i.  A cloud that is not served (one vcr_grid_radius_f32 left as
 *                -1s because it did not fit, say) comes back with every normal, curvature and fpfh value NaN and every spfh
 *                word zero; no idx entry of it is read.  The other clouds of the batch are unaffected
 * A point's result is a function of its own rows alone -- every B, every launch form and every batch returns the same bits --
 * and every slot of every output is written.  All three are asynchronous on the stream: no host synchronisation, no allocation,
 * no workspace.  Each is two launches: the pass, and a check of row_start that voids a cloud that is not served.
 *
 * vcr_rows_normals_f32: vcr_normals_f32's definition (vcr_hip_plane.h) word for word over the m = L_i + 1 rows
 * { i } U row[0 .. L_i) -- the nine fp64 sums in the row's order, C, the Jacobi solve, the sign rule with or without a viewpoint,
 * the curvature, the non-finite cases.  One addition: L_i < 2 gives n = (0,0,1), curvature 0 (fewer than three points define no
 * plane) -- the one place where a row of one entry differs from vcr_normals_f32 at k = 1.
 *
 * vcr_rows_spfh_f32: vcr_spfh_f32's pair definition (vcr_hip_fpfh.h) word for word with "no radius", over row[0 .. L_i).  The
 * histogram is kept wider:
 *   spfh[b, i]   uint32 [3][12], 144 bytes: per group (f0, f1, f2) the counts of its 11 bins, then c_i, the number of counted
 *                pairs (the same in all three).  No count can overflow: n_i < 131 072
 *
 * vcr_rows_fpfh_f32: vcr_fpfh_f32's weighted sum word for word -- the neighbours in the row's order, the bins ascending inside a
 * neighbour, d2 in fp64 from the widened fp32 differences, a neighbour with d2 == 0, d2 not finite or c_j == 0 skipped (no
 * radius test) -- reading the 144-byte rows, c_j and c_i per group.
 *
 * Launch forms.  The normals pass is a lane a row.  The two FPFH passes have two forms that return the same bits:
 *   VCR_ROWS_LANE   a lane a row (a lane a (row, group) in the second pass): the fixed-width kernels' shape, for short rows
 *   VCR_ROWS_WAVE   a wave a row: a row's pairs are dealt to the wave's 64 lanes (the counts are integers: order-free); in the
 *                   second pass a lane a bin runs its own chain in the row's order
 * vcr_rows_form decides from the row length the host can see without a synchronisation,
 *   est = capacity / N, and min(est, max_nn) where max_nn > 0
 * wave where est >= VCR_ROWS_WAVE_SPFH (VCR_ROWS_WAVE_FPFH for the second pass), lane below.  variant forces either.  As
 * measured the first pass's wave form never lost from 24 entries a row on; the second pass's lost at
 * every length up to 330, so its threshold lies above every row the limits allow and only variant reaches it.
 */
#ifndef VCR_HIP_ROWS_H
#define VCR_HIP_ROWS_H

#include "../vcr_hip_plane.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VCR_ROWS_MAX_N 131072
#define VCR_ROWS_SPFH_WORDS 36            /* a point's histograms: three groups of 11 counts and c_i, uint32 each (144 bytes) */
#define VCR_ROWS_LANE 1
#define VCR_ROWS_WAVE 2
#define VCR_ROWS_WAVE_SPFH 24             /* est at and above which the first pass takes the wave form */
#define VCR_ROWS_WAVE_FPFH 131072         /* ... and the second pass: no row is that long -- its wave form won no measurement */

/* All three: B < 1, a missing pointer (idx may be NULL where capacity == 0; viewpoint and curvature are optional), capacity < 0,
 * max_nn < 0, a variant other than 0, VCR_ROWS_LANE or VCR_ROWS_WAVE, a bad struct_bytes, xyz4 or spfh not 16-B aligned:
 * VCR_EINVAL.  N outside [1, 131 072], B * N >= 2^31 or B * capacity >= 2^31: VCR_EUNSUPPORTED. */
typedef struct {
  uint32_t struct_bytes;        /* sizeof(vcr_rows_normals_args) as the CALLER was compiled (see vcr_fps_args); the mandatory part
                                   ends behind normals: 0, shorter than that or longer than this library knows: VCR_EINVAL */
  const float* xyz4;            /* [B,N,4] rows as vcr_rows4_f32 writes them, 16-B aligned; the fourth value is not read */
  const int* idx;               /* [B,capacity] */
  const int64_t* row_start;     /* [B,N+1] */
  const int64_t* total;         /* [B] */
  int B, N, capacity;
  int max_nn;                   /* 0: the whole row; m > 0: its first min(n_i, m) entries */
  const float* viewpoint;       /* optional [B,3], as vcr_normals_args.viewpoint */
  float* normals;               /* [B,3,N] channels-first, mandatory */
  float* curvature;             /* optional [B,N] */
} vcr_rows_normals_args;

int vcr_rows_normals_f32(const vcr_rows_normals_args*, vcr_stream_t);

typedef struct {
  uint32_t struct_bytes;        /* every field is mandatory: 0, shorter or longer than this library knows: VCR_EINVAL */
  const float* xyz4;            /* [B,N,4], 16-B aligned */
  const float* normals;         /* [B,3,N] channels-first */
  const int* idx;               /* [B,capacity] */
  const int64_t* row_start;     /* [B,N+1] */
  const int64_t* total;         /* [B] */
  int B, N, capacity, max_nn;
  int variant;                  /* 0 = vcr_rows_form decides; VCR_ROWS_LANE / VCR_ROWS_WAVE force a form (tests, benchmarks) */
  uint32_t* spfh;               /* out [B,N,3,12], 16-B aligned */
} vcr_rows_spfh_args;

int vcr_rows_spfh_f32(const vcr_rows_spfh_args*, vcr_stream_t);

typedef struct {
  uint32_t struct_bytes;        /* as above */
  const float* xyz4;            /* [B,N,4], 16-B aligned */
  const int* idx;               /* [B,capacity] */
  const int64_t* row_start;     /* [B,N+1] */
  const int64_t* total;         /* [B] */
  const uint32_t* spfh;         /* [B,N,3,12] as vcr_rows_spfh_f32 wrote them for the same rows and max_nn, 16-B aligned */
  int B, N, capacity, max_nn;
  int variant;                  /* as vcr_rows_spfh_args.variant */
  float* fpfh;                  /* out [B,33,N] channels-first */
} vcr_rows_fpfh_args;

int vcr_rows_fpfh_f32(const vcr_rows_fpfh_args*, vcr_stream_t);

/* Host-only query (nothing is launched), the one place that decides: the form each of the two FPFH passes takes (VCR_ROWS_LANE
 * or VCR_ROWS_WAVE) for these numbers.  cu_count >= 0 is accepted and not used today: the rule is the row length's alone.  The
 * limits and error codes are the calls'; cu_count < 0: VCR_EINVAL.  Either pointer may be NULL. */
int vcr_rows_form(int B, int N, int capacity, int max_nn, int cu_count, int variant, int* spfh_form, int* fpfh_form);

#ifdef __cplusplus
}
#endif
#endif

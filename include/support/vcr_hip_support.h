/*
 * vcr_hip_support.h -- normals and FPFH at M CENTRES over a SUPPORT cloud of N points: the consumers of
 * rows whose row i belongs to centre i -- any position, a point of the cloud or not -- and whose entries index the support cloud;
 * what vcr_hip_query.h's radius search writes.  vcr_hip_rows.h's three passes assume that row i belongs to point i of the same
 * cloud; these four calls drop that assumption (PCL's setInputCloud(keypoints) + setSearchSurface(cloud)).  An extension of
 * vcr_hip.h (same library, same conventions, same error codes); it adds no symbol to that header or to any other and moves none
 * of their layouts, so VCR_ABI_VERSION is unchanged.  It lives alone in include/support/ and includes its base by relative path.
 *
 * What all four calls share.  Per cloud b:
 *   support      xyz4 [B,N,4] rows, 16-B aligned, the fourth value not read; normals [B,3,N] channels-first
 *   centres      c4 [B,M,4] rows, 16-B aligned, the fourth value not read
 *   rows         idx int32 [B,capacity]; row_start int64 [B,M+1]; total int64 [B]: the CSR triple over the M centres, entries
 *                indexing the support cloud -- exactly what vcr_hip_query.h's radius search writes, but any caller may build
 *                them.  Centre i's row is idx[b, row_start[b,i] ... row_start[b,i+1])
 *   self         optional int32 [B,M]: self[b,i] = s >= 0 says "centre i IS support point s".  NULL: -1 everywhere
 *   max_nn       >= 0
 *   used entries walk row i in order.  An entry outside [0, N) is skipped and counts as nothing.  An entry equal to self[b,i]
 *                is a SELF entry; any other entry is a NEIGHBOUR entry.  The walk ends behind the max_nn-th neighbour entry (at
 *                the row's end where max_nn == 0); self entries behind that point are not used
 *   no radius    the kernels know no radius and re-test no distance: the row IS the neighbourhood
 *   served       vcr_hip_rows.h's rule with M for N: cloud b is served iff 0 <= total[b] <= capacity, row_start[b,0] == 0,
 *                row_start[b,M] == total[b] and row_start[b,i] <= row_start[b,i+1] for every i.  A cloud that is not served comes
 *                back with every normal, curvature and fpfh value NaN, every spfh word zero and nothing needed; no idx entry of
 *                it is read.  The other clouds of the batch are unaffected
 *   not finite   a centre with a NaN or infinite coordinate gets NaN normals, curvature and fpfh and zero spfh words, and needs
 *                nothing (a padded keypoint slot is NaN; vcr_hip_match.h never lets a NaN feature win)
 * A centre's result is a function of its own row alone -- every B, every launch form and every batch returns the same bits --
 * and every slot of every output is written.  All four are asynchronous on the stream: no host synchronisation, no allocation.
 * Each pass is followed by the row_start check launch of vcr_hip_rows.h's passes, which voids a cloud that is not served.
 *
 * vcr_support_normals_f32: vcr_hip_plane.h's definition word for word over the m used entries of the row, self and neighbour
 * entries alike: the differences x_j - c_i in fp32, widened; the nine fp64 sums in the row's order; the divisor m; C, the Jacobi
 * solve, the curvature and the non-finite cases unchanged; the sign rule with or without a viewpoint, taken at the centre's
 * position.  m < 3 gives n = (0,0,1), curvature 0.  One lane a centre.  Consequence: centres equal to the cloud's own points with
 * self = i and a row that holds i once return vcr_hip_rows.h's normals of the same row without i, bit for bit (the self entry's
 * differences are exact zeros).
 *
 * vcr_support_spfh_f32: vcr_hip_fpfh.h's pair definition with "no radius" for the pair (centre i with centre_normals, support
 * point j with the support's normals), over the used NEIGHBOUR entries, in vcr_hip_rows.h's 144-byte layout uint32 [3][12].  A
 * neighbour at d2 == 0 that is not the self entry is counted (bins 5, 5, 5), as everywhere.  The one call serves the centres' own
 * histograms and those of the NEEDED support points: the centres are then the needed points, self their index, the rows their
 * own rows in the support.  Two launch forms return the same bits:
 *   VCR_SUPPORT_LANE   a lane a centre: a column of LDS words a lane
 *   VCR_SUPPORT_WAVE   a wave a centre: a row's entries are dealt to the wave's 64 lanes, integer LDS atomics; the cut at max_nn
 *                      takes each entry's rank among the neighbour entries (a ballot and prefix count per 64-entry chunk)
 * vcr_support_form decides from what the host can see without a synchronisation: wave where B * M <= VCR_SUPPORT_WAVE_CENTRES
 * (too few centres for a lane each to fill the device: the wave form won every such case measured, from 11 entries a row on),
 * otherwise from est = capacity / M (and min(est, max_nn) where max_nn > 0): wave where est >= VCR_SUPPORT_WAVE_SPFH, lane
 * below; variant forces either (DESIGN.md section 4.29 holds the table).
 *
 * vcr_support_needed_f32: which support points the second pass will read.  need[b,j] = 1 iff j is a used neighbour entry of some
 * finite centre of a served cloud b.  The outputs are laid out as vcr_hip_outlier.h's filters lay out theirs: the needed points in
 * ascending index order, NaN behind the count; index -1 behind the count; and slot, the rank of point j among the needed points,
 * or -1.
 *
 * vcr_support_fpfh_f32: vcr_hip_fpfh.h's weighted sum word for word.  Per centre i and group g, the used neighbour entries j in the
 * row's order, the bins ascending inside a neighbour; d2 in fp64 from the widened fp32 differences x_j - c_i.  A neighbour is
 * skipped where d2 == 0, d2 is not finite, slot[b,j] is outside [0, R), or c == 0 in its histogram row support_spfh[b, slot[b,j]].
 * The own term comes from centre_spfh[b, i].  One lane a (centre, group); there is no wave form (in vcr_hip_rows.h's second pass
 * it lost every case measured).
 */
#ifndef VCR_HIP_SUPPORT_H
#define VCR_HIP_SUPPORT_H

#include "../vcr_hip_plane.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VCR_SUPPORT_MAX_N 131072          /* N, M and R */
#define VCR_SUPPORT_SPFH_WORDS 36         /* a histogram row: three groups of 11 counts and c, uint32 each (144 bytes) */
#define VCR_SUPPORT_LANE 1
#define VCR_SUPPORT_WAVE 2
#define VCR_SUPPORT_WAVE_SPFH 24          /* est at and above which the first pass takes the wave form */
#define VCR_SUPPORT_WAVE_CENTRES 32768    /* ... and B * M up to which it takes it at any est (as measured, section 4.29) */
#define VCR_SUPPORT_COVERAGE_PCT 0        /* the "needed" plan is taken where min(N, est M) * 100 <= this * N: as measured it won
                                             at no coverage (section 4.29), so only support="needed" reaches it */

/* All four: B < 1, a missing pointer (idx may be NULL where capacity == 0; self, viewpoint, curvature and slot are optional),
 * capacity < 0, max_nn < 0, a variant other than 0, VCR_SUPPORT_LANE or VCR_SUPPORT_WAVE, a bad struct_bytes, xyz4, c4 or a
 * histogram pointer not 16-B aligned: VCR_EINVAL.  N, M (and R) outside [1, 131 072], B * N, B * M (B * R) or B * capacity
 * >= 2^31: VCR_EUNSUPPORTED.  Argument errors return before any device call. */
typedef struct {
  uint32_t struct_bytes;        /* sizeof(vcr_support_normals_args) as the CALLER was compiled (see vcr_fps_args); the mandatory
                                   part ends behind normals: 0, shorter than that or longer than this library knows: VCR_EINVAL */
  const float* xyz4;            /* [B,N,4] the support's rows, 16-B aligned */
  const float* c4;              /* [B,M,4] the centres' rows, 16-B aligned */
  const int* idx;               /* [B,capacity] */
  const int64_t* row_start;     /* [B,M+1] */
  const int64_t* total;         /* [B] */
  const int* self;              /* optional [B,M] */
  int B, N, M, capacity;
  int max_nn;                   /* 0: the whole row; m > 0: up to and including its m-th neighbour entry */
  const float* viewpoint;       /* optional [B,3]: the normals look at it from the centre's position */
  float* normals;               /* [B,3,M] channels-first, mandatory */
  float* curvature;             /* optional [B,M] */
} vcr_support_normals_args;

int vcr_support_normals_f32(const vcr_support_normals_args*, vcr_stream_t);

typedef struct {
  uint32_t struct_bytes;        /* every field but self is mandatory: 0, shorter or longer than this library knows: VCR_EINVAL */
  const float* xyz4;            /* [B,N,4], 16-B aligned */
  const float* normals;         /* [B,3,N] the support's normals, channels-first */
  const float* c4;              /* [B,M,4], 16-B aligned */
  const float* centre_normals;  /* [B,3,M] channels-first */
  const int* idx;               /* [B,capacity] */
  const int64_t* row_start;     /* [B,M+1] */
  const int64_t* total;         /* [B] */
  const int* self;              /* optional [B,M] */
  int B, N, M, capacity, max_nn;
  int variant;                  /* 0 = vcr_support_form decides; VCR_SUPPORT_LANE / VCR_SUPPORT_WAVE force a form */
  uint32_t* spfh;               /* out [B,M,3,12], 16-B aligned */
} vcr_support_spfh_args;

int vcr_support_spfh_f32(const vcr_support_spfh_args*, vcr_stream_t);

typedef struct {
  uint32_t struct_bytes;        /* every field but self is mandatory */
  const float* xyz4;            /* [B,N,4], 16-B aligned */
  const float* c4;              /* [B,M,4], 16-B aligned */
  const int* idx;               /* [B,capacity] */
  const int64_t* row_start;     /* [B,M+1] */
  const int64_t* total;         /* [B] */
  const int* self;              /* optional [B,M] */
  int B, N, M, capacity, max_nn;
  float* points;                /* out [B,3,N] channels-first: the needed points, ascending by index; NaN behind count[b] */
  int* count;                   /* out [B] */
  int* index;                   /* out [B,N]: the needed points' indices, ascending; -1 behind count[b] */
  int* slot;                    /* out [B,N]: point j's rank among the needed points, -1 where it is not needed */
} vcr_support_needed_args;

/* The workspace (256-B aligned is enough; 16-B is asked): the marks and the per-block counts of the compaction.  0 for
 * arguments the call refuses, or cu_count < 0.  A NULL or misaligned workspace: VCR_EINVAL; a short one: VCR_EWORKSPACE. */
size_t vcr_support_needed_workspace_bytes(const vcr_support_needed_args*, int cu_count);
int vcr_support_needed_f32(const vcr_support_needed_args*, void* workspace, size_t workspace_bytes, vcr_stream_t);

typedef struct {
  uint32_t struct_bytes;        /* every field but self and slot is mandatory */
  const float* xyz4;            /* [B,N,4], 16-B aligned */
  const float* c4;              /* [B,M,4], 16-B aligned */
  const int* idx;               /* [B,capacity] */
  const int64_t* row_start;     /* [B,M+1] */
  const int64_t* total;         /* [B] */
  const int* self;              /* optional [B,M] */
  const int* slot;              /* optional [B,N]: support point j's histogram row; NULL: the identity (slot[b,j] = j) */
  const uint32_t* support_spfh; /* [B,R,3,12], 16-B aligned */
  const uint32_t* centre_spfh;  /* [B,M,3,12], 16-B aligned: the centres' own histograms, for the same rows and max_nn */
  int B, N, M, R, capacity, max_nn;
  float* fpfh;                  /* out [B,33,M] channels-first */
} vcr_support_fpfh_args;

int vcr_support_fpfh_f32(const vcr_support_fpfh_args*, vcr_stream_t);

/* Host-only query (nothing is launched), the one place that decides the first pass's form (VCR_SUPPORT_LANE or VCR_SUPPORT_WAVE)
 * for these numbers.  cu_count >= 0 is accepted and not used today: the rule is the centres' number's and the row length's.  The limits and error
 * codes are the calls'; cu_count < 0: VCR_EINVAL.  The pointer may be NULL. */
int vcr_support_form(int B, int N, int M, int capacity, int max_nn, int cu_count, int variant, int* spfh_form);

#ifdef __cplusplus
}
#endif
#endif

/*
 * vcr_hip_border.h -- the rim of a scanned surface (Open3D's compute_boundary_points, PCL's BoundaryEstimation) over neighbourhoods
 * given as ragged rows: the angle of every neighbour in the point's tangent frame, the largest angular gap
 * between neighbours that follow each other around the point, and the spreading of the flags over rows.  An extension of vcr_hip.h
 * (same library, same conventions, same error codes); it adds no symbol to that header or to its other extensions and moves none of
 * their layouts, so VCR_ABI_VERSION is unchanged.
 *
 * The rows are those of ext/vcr_hip_rows.h.  Per cloud b:
 *   idx          int32 [B,capacity]; row_start int64 [B,N+1]; total int64 [B] -- exactly what the radius search writes, but any
 *                caller may build them.  Point i's row is idx[b, row_start[b,i] ... row_start[b,i+1]), n_i entries
 *   entry        an entry outside [0, N) reads as i, as in the fixed-width calls
 *   no radius    no pass knows a radius or re-tests a distance: the row IS the neighbourhood
 *   served       cloud b is served iff 0 <= total[b] <= capacity, row_start[b,0] == 0, row_start[b,N] == total[b] and
 *                row_start[b,i] <= row_start[b,i+1] for every i.  No idx entry of a cloud that is not served is read.  The other
 *                clouds of the batch are unaffected
 *
 * FRAME of point i (vcr_border_angles_f32), all of it in fp64:
 *   n            normals[b,:,i] widened;  s = (nx*nx + ny*ny) + nz*nz
 *   no frame     where x_i or n holds a value that is not finite, or s is not > 0 and finite.  Such a point has frame 0, every
 *                slot of its row holds NaN, and the gap pass that is given `frame` writes gap NaN, flag 0 for it
 *   nh           = n * (1.0 / sqrt(s))
 *   a            the axis with the smallest |nh_a|, the lowest index among equals; e = the unit vector of axis a (0.0s and a 1.0)
 *   u, v         u = nh x e and v = nh x u, written out: u0 = nh1*e2 - nh2*e1, u1 = nh2*e0 - nh0*e2, u2 = nh0*e1 - nh1*e0 and v
 *                likewise from nh and u.  Every component is ONE difference of two products, no fused multiply-add
 * ANGLE of entry e (neighbour j) of row i:
 *   d            the three fp32 differences x_j - x_i, widened
 *   pu, pv       pu = (u0*d0 + u1*d1) + u2*d2, pv = (v0*d0 + v1*d1) + v2*d2
 *   skipped      where a component of d is not finite, where d is all zero (copies of the point, entries that read as i) or where
 *                pu == 0 and pv == 0.  A skipped slot holds NaN
 *   angle        = atan2(pv, pu) in fp64 otherwise: the ONE library call of the definition.  Everything before it and everything
 *                behind it is defined to the bit; two atan2 implementations may differ in the last places, which is why the angles
 *                are a stage of their own: the gap of GIVEN angles is exact
 *   pad          the slots behind total[b] hold NaN; so does every slot of a cloud that is not served
 *   used         with the optional d2 and r2 (the rule of NEAR below) a row is its used entries alone: the slots of the others
 *                hold NaN, and the gap pass given the same d2 and r2 reads n_i as u_i.  One search at a larger radius then
 *                serves a boundary at a smaller one
 *
 * GAP of row i (vcr_border_gap_f32) from its n_i angle slots, c of them counted (not NaN), m = n_i + 1 (the point counts itself):
 *   too few      m < min_neighbors or c == 0: gap = +0.0, flag = 0
 *   succ         of a counted angle: the smallest counted angle strictly above it (copies of an angle share theirs)
 *   gap          = max( max over the counted angles that have one of (succ - angle), (TWO_PI - a_max) + a_min ), a_max and a_min
 *                the largest and the smallest counted angle, TWO_PI the double 0x401921FB54442D18.  max is exact, so the value is
 *                free of any order: every launch form and every batch returns the same bits from the same angles.  A single
 *                angle a gives (TWO_PI - a) + a: TWO_PI itself for every a >= 0, and within one unit in the last place of it below
 *   flag         = gap > angle_threshold (radians), strict and in fp64
 *   frame        where the optional frame [B,N] is given and frame[b,i] == 0: gap = NaN, flag = 0, before anything else
 *   not served   VCR_BORDER_NOT_SERVED in every flag and NaN in every gap of the cloud
 *
 * NEAR (vcr_border_near_f32): the flags spread once over rows that may be the same or others.
 *   used         all n_i entries of row i where d2 is NULL; otherwise its leading entries e with d2[b, row_start[b,i] + e] <= r2
 *                (fp32; the first entry that fails ends them): on the radius search's rows, which ascend in (d2, index), bit for
 *                bit the row of a search at a radius r' <= r with r' * r' == r2
 *   near[i]      1 where flag[i] > 0 or a used entry's flag is > 0 (an entry outside [0, N) reads as i); otherwise 0
 *   voided       a cloud that is not served, or of which ANY flag is VCR_BORDER_NOT_SERVED, gets that value in every slot
 *
 * All three are asynchronous on the stream: no host synchronisation, no allocation, no atomics, no workspace.  Each is two
 * launches: the pass, and a check of row_start that voids a cloud (and pads the angles).  Every slot of every output is written.
 *
 * Launch forms.  The angles are a function of one entry, so any shape returns the same bits; the pass runs a wave a row: the 64
 * lanes read 64 consecutive idx entries and write 64 consecutive angles, the row of a slot needs no search through row_start, and
 * the frame is computed once a row instead of once an entry.  The gap has two forms that return the same bits:
 *   VCR_BORDER_LANE   a lane a row: for every counted angle a pass over the row for its successor
 *   VCR_BORDER_WAVE   a wave a row: 64 angles a step, the row passing through LDS in chunks of VCR_BORDER_CHUNK angles
 * vcr_border_form decides from the row length the host can see without a synchronisation, est = capacity / N: wave where
 * est >= VCR_BORDER_WAVE_GAP, lane below; variant forces either.  As measured (profiles/border_bench.txt)
 * the wave form won everywhere it was tried -- 1.3 to 3.8 times faster at 10 to 12 entries a row, 21 to 51 times at 71 to 100: a
 * lane's search for the successors is quadratic in its row and reads it uncoalesced -- so the threshold is the shortest row of
 * that measurement; below it nothing was measured and the lane form stays.
 * The spreading runs a lane a row and leaves the row at the first hit.
 */
#ifndef VCR_HIP_BORDER_H
#define VCR_HIP_BORDER_H

#include "../vcr_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VCR_BORDER_MAX_N 131072
#define VCR_BORDER_LANE 1
#define VCR_BORDER_WAVE 2
#define VCR_BORDER_CHUNK 256              /* angles of a row the wave form holds in LDS at a time */
#define VCR_BORDER_WAVE_GAP 10            /* est at and above which the gap takes the wave form: the shortest rows it was measured
                                             on, and won */
#define VCR_BORDER_NOT_SERVED (-2)        /* the value the keypoint flags use for a cloud that is not served */

/* All three passes: B < 1, a missing mandatory pointer (idx may be NULL where capacity == 0; frame and d2 are optional), capacity < 0,
 * min_neighbors < 1, an angle_threshold that is NaN, an r2 that is not >= 0 where d2 is given, a variant other than 0,
 * VCR_BORDER_LANE or VCR_BORDER_WAVE, a bad struct_bytes, xyz4 not 16-B aligned: VCR_EINVAL.  N outside [1, 131 072],
 * B * N >= 2^31 or B * capacity >= 2^31: VCR_EUNSUPPORTED. */
typedef struct {
  uint32_t struct_bytes;        /* sizeof(vcr_border_angles_args) as the CALLER was compiled; the mandatory part ends behind angle:
                                   0, shorter than that or longer than this library knows: VCR_EINVAL */
  const float* xyz4;            /* [B,N,4] rows as vcr_rows4_f32 writes them, 16-B aligned; the fourth value is not read */
  const float* normals;         /* [B,3,N] channels-first; any length (the frame normalises in fp64) */
  const int* idx;               /* [B,capacity] */
  const int64_t* row_start;     /* [B,N+1] */
  const int64_t* total;         /* [B] */
  int B, N, capacity;
  double* angle;                /* out [B,capacity], mandatory where capacity > 0 */
  int* frame;                   /* optional out [B,N]: 1 where the point has a frame, 0 where not, VCR_BORDER_NOT_SERVED voided */
  const float* d2;              /* optional [B,capacity]: the entries' squared distances, ascending inside a row */
  float r2;                     /* read where d2 is given: >= 0 (+inf uses every entry) */
} vcr_border_angles_args;

int vcr_border_angles_f32(const vcr_border_angles_args*, vcr_stream_t);

typedef struct {
  uint32_t struct_bytes;        /* every field is part of the struct: 0, shorter or longer than this library knows: VCR_EINVAL */
  const double* angle;          /* [B,capacity]: NaN in a slot that does not count (may be NULL where capacity == 0) */
  const int64_t* row_start;     /* [B,N+1] */
  const int64_t* total;         /* [B] */
  const int* frame;             /* optional [B,N] as vcr_border_angles_f32 wrote it */
  const float* d2;              /* optional [B,capacity], as the angles' */
  int B, N, capacity;
  int min_neighbors;            /* >= 1, held against m = n_i + 1 */
  double angle_threshold;       /* radians; not NaN */
  float r2;                     /* read where d2 is given: >= 0 */
  int variant;                  /* 0 = vcr_border_form decides; VCR_BORDER_LANE / VCR_BORDER_WAVE force a form (tests, benchmarks) */
  double* gap;                  /* out [B,N] */
  int* flag;                    /* out [B,N]: 1 / 0, VCR_BORDER_NOT_SERVED over a cloud that is not served */
} vcr_border_gap_args;

int vcr_border_gap_f32(const vcr_border_gap_args*, vcr_stream_t);

/* Host-only query (nothing is launched), the one place that decides: the form the gap pass takes (VCR_BORDER_LANE or
 * VCR_BORDER_WAVE) for these numbers.  cu_count >= 0 is accepted and not used today: the rule is the row length's alone.  The
 * limits and error codes are the passes'; cu_count < 0: VCR_EINVAL.  form may be NULL. */
int vcr_border_form(int B, int N, int capacity, int cu_count, int variant, int* form);

typedef struct {
  uint32_t struct_bytes;        /* every field is part of the struct */
  const int* flag;              /* [B,N] as vcr_border_gap_f32 wrote it */
  const int* idx;               /* [B,capacity] */
  const int64_t* row_start;     /* [B,N+1] */
  const int64_t* total;         /* [B] */
  const float* d2;              /* optional [B,capacity]: the entries' squared distances, ascending inside a row */
  int B, N, capacity;
  float r2;                     /* read where d2 is given: >= 0 (+inf uses every entry) */
  int* near;                    /* out [B,N]: 1 / 0, VCR_BORDER_NOT_SERVED over a voided cloud */
} vcr_border_near_args;

int vcr_border_near_f32(const vcr_border_near_args*, vcr_stream_t);

#ifdef __cplusplus
}
#endif
#endif

/*
 * vcr_hip_fpfh.h -- describing a point by its local geometry on the device: Open3D's
 * compute_fpfh_feature, the 33-bin Fast Point Feature Histogram, in two launches behind the normals (vcr_hip_plane.h).  An
 * extension of vcr_hip.h (same library, same conventions, same error codes); it adds no symbol to that header or to its other
 * extensions and moves none of their layouts, so VCR_ABI_VERSION is unchanged.
 *
 * Neither call runs a search of its own (like vcr_normals_f32): idx holds point i's k neighbours, the point itself NOT among
 * them, so Open3D's "skip the first entry" is done and its indices.size() - 1 is k.  Neither needs a workspace.  A point's
 * result is a function of its own rows alone -- every B, every launch and every batch returns the same bits -- and every slot
 * of every output is written.  Common to both, per point i and idx entry j:
 *   j               an idx entry outside [0, N) reads as i
 *   dx              (double)(x_j - x_i): the fp32 difference, widened (as in vcr_normals_f32); dy, dz likewise
 *   d2              (dx dx + dy dy) + dz dz in fp64
 *   r2              (double)(radius * radius), the product in fp32 (one rounding).  radius = 0: no radius, a plain kNN
 *                   neighbourhood; otherwise Open3D's hybrid search -- a neighbour with d2 > r2 is dropped in BOTH passes
 * Every sum of three terms below is (a + b) + c, every a b - c d is two products and one subtraction, nothing is fused, and
 * every operation is fp64 unless it says otherwise.
 *
 * vcr_spfh_f32 -- the simplified histograms.  n_i, n_j are the fp32 normals of i and j, widened.  The pair (i, j) is COUNTED iff
 * d2 is finite, all six components of n_i and n_j are finite, and d2 <= r2 where a radius is set.  For a counted pair
 * (Open3D's ComputePairFeatures with p1 = x_i, n1 = n_i, p2 = x_j, n2 = n_j):
 *   L               sqrt(d2);  L == 0 gives f = (0, 0, 0) -- still counted, as Open3D counts it: bins 5, 5, 5
 *   a1              ((n1x dx + n1y dy) + n1z dz) / L,  a2 likewise with n2
 *   swap            if |a1| < |a2|: n1 and n2 change places, d = -d, f2 = -a2; otherwise f2 = a1.  (Open3D's
 *                   acos(fabs(a1)) > acos(fabs(a2)) without the arc cosines)
 *   v               d x n1 = (dy n1z - dz n1y, dz n1x - dx n1z, dx n1y - dy n1x);  |v| = sqrt((vx vx + vy vy) + vz vz)
 *                   |v| == 0 gives f = (0, 0, 0); otherwise v = (vx / |v|, vy / |v|, vz / |v|)
 *   w               n1 x v = (n1y vz - n1z vy, n1z vx - n1x vz, n1x vy - n1y vx)
 *   f1              (vx n2x + vy n2y) + vz n2z
 *   f0              atan2((wx n2x + wy n2y) + wz n2z, (n1x n2x + n1y n2y) + n1z n2z)
 *   bins            floor((11 (f0 + pi)) / (2 pi)),  floor((11 (f1 + 1)) 0.5),  floor((11 (f2 + 1)) 0.5), each clamped to
 *                   [0, 10]; a NaN coordinate goes to bin 0 of its group and the pair still counts
 * The arc tangent is the one step whose last bit is the math library's; everything else is IEEE arithmetic.  Open3D adds
 * 100 / c_i to a bin per pair, c_i the number of counted pairs: the histogram is kept as the integer counts,
 *   spfh[b, i]      48 bytes, three groups (f0, f1, f2) of 16: bytes 0..10 the counts of the group's 11 bins, byte 11 c_i (the
 *                   same in all three), bytes 12..15 zero
 *
 * vcr_fpfh_f32 -- the weighted sum over the neighbours (Open3D's ComputeFPFHFeature with dist the squared distance).  Per
 * point i and group g, with count_p[b] and c_p the bytes of spfh[., p] for that group: the neighbours j in idx's order, the bins
 * b ascending inside a neighbour; a neighbour with d2 == 0, d2 not finite, d2 > r2 where a radius is set, or c_j == 0 is skipped:
 *   val             ((double)count_j[b] * (100.0 / (double)c_j)) / d2
 *   acc[b] += val;  sum_g += val
 * and behind the loop
 *   acc[b]          acc[b] * (100.0 / sum_g) where sum_g != 0
 *   fpfh[b, 11 g + b, i]   (float)(acc[b] + (double)count_i[b] * (100.0 / (double)c_i)), the own term 0 where c_i == 0
 */
#ifndef VCR_HIP_FPFH_H
#define VCR_HIP_FPFH_H

#include "vcr_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VCR_FPFH_MAX_K 62                 /* vcr_knn_f32's limit: VCR_EUNSUPPORTED beyond */
#define VCR_FPFH_BINS 11                  /* per group; three groups: 33 channels */
#define VCR_SPFH_ROW_BYTES 48             /* a point's histograms: three groups of 16 bytes */

/* Both calls: B < 1, N < 1, k < 1, radius negative or not finite, a missing pointer (all are mandatory), xyz4 or spfh not
 * 16-B aligned: VCR_EINVAL.  k > VCR_FPFH_MAX_K, N > 131 072 or B * N >= 2^31: VCR_EUNSUPPORTED. */
typedef struct {
  uint32_t struct_bytes;        /* sizeof(vcr_spfh_args) as the CALLER was compiled (see vcr_fps_args); every field is
                                   mandatory: 0, shorter or longer than this library knows: VCR_EINVAL */
  const float* xyz4;            /* [B,N,4] rows as vcr_rows4_f32 writes them, 16-B aligned; the fourth value is not read */
  const float* normals;         /* [B,3,N] channels-first, as vcr_normals_f32 writes them */
  const int* idx;               /* [B,N,k]: the neighbours vcr_knn_f32 wrote for C == 4 (cloud-local) */
  int B, N, k;                  /* 1 <= N <= 131 072, B N < 2^31; 1 <= k <= VCR_FPFH_MAX_K */
  float radius;                 /* 0: none; otherwise finite and > 0 */
  unsigned char* spfh;          /* out [B,N,48], 16-B aligned */
} vcr_spfh_args;

/* Asynchronous on the stream: no host synchronisation, no allocation, no workspace. */
int vcr_spfh_f32(const vcr_spfh_args*, vcr_stream_t);

typedef struct {
  uint32_t struct_bytes;        /* as above */
  const float* xyz4;            /* [B,N,4], 16-B aligned */
  const int* idx;               /* [B,N,k] */
  const unsigned char* spfh;    /* [B,N,48] as vcr_spfh_f32 wrote them for the same xyz4, idx and radius, 16-B aligned */
  int B, N, k;
  float radius;                 /* as vcr_spfh_args.radius */
  float* fpfh;                  /* out [B,33,N] channels-first */
} vcr_fpfh_args;

int vcr_fpfh_f32(const vcr_fpfh_args*, vcr_stream_t);

#ifdef __cplusplus
}
#endif
#endif

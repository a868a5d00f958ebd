/*
 * vcr_hip_fgr.h -- a pose from correspondences without trials: Fast Global Registration (Zhou, Park,
 * Koltun, ECCV 2016) as Open3D's registration_fgr_based_on_feature_matching runs it behind its matching -- the tuple test, the
 * normalisation and a fixed number of Gauss-Newton steps under a graduated robust weight.  An extension of vcr_hip.h (same
 * library, same conventions, same error codes); it adds no symbol to that header or to its other extensions and moves none of
 * their layouts, so VCR_ABI_VERSION is unchanged.
 *
 * vcr_fgr_f32 -- per cloud pair, independently of the batch (every cloud uses the same seed): the result is a function of one
 * pair's inputs alone, the same bits in every B and every batch.  All arithmetic below is fp64 unless it says fp32; a * b + c
 * is two roundings, fma(a, b, c) is one.
 *   pairs      as vcr_ransac_f32 (vcr_hip_match.h): the source indices i with 0 <= corr[i] < Nt, ascending; M is their number
 *   tuple test (tuple_scale != 0)  trials t = 0 .. min(T, 100 M) - 1; the three picks of trial t are vcr_ransac_f32's
 *              pick_j (the same mix32, the same meaning of seed).  For the pick pairs (0,1), (0,2), (1,2), ls2 and lt2 are that
 *              header's ds2 / dt2 expressions (fp32) of the two source points and of their two partners,
 *              s2 = tuple_scale * tuple_scale in fp32; the trial passes iff  s2 * ls2 < lt2 && s2 * lt2 < ls2  for all three
 *              (fp32 products, strict: a NaN fails, and a repeated pick fails through its zero edge, as in Open3D).
 *              kept: the first K = max_tuples passing trials in ascending t; tuples = min(K, passes).  The list optimised is
 *              their picks in (trial, pick) order, repeats kept: L = 3 tuples source indices (tuple_list; entries behind L are
 *              not written).  tuple_scale == 0: the list is the M pairs, L = M, tuples = 0.
 *   too few    L < 10: R = I, t = 0 (pose64 too), status 1 -- Open3D's identity.  Nothing below runs but the normalisation.
 *   sum order  `the sum over n items` below: lane l of 256 adds its items l, l + 256, ... in ascending order onto 0; the 64
 *              lanes of a wave are folded by the butterfly v += v[lane ^ o], o = 32, 16, 8, 4, 2, 1; the four waves are added
 *              in ascending order, ((w0 + w1) + w2) + w3.
 *   normalise  mean_s, mean_t: the sum over ALL Ns (Nt) points of the cloud -- not over the pairs, as Open3D -- of every
 *              coordinate widened to fp64, divided by (double)N.  For every point of both clouds, centred on its own cloud's
 *              mean, d = (double)x - mean and n2 = fma(dz, dz, fma(dy, dy, dx * dx)); scale = sqrt(the largest n2).  A point
 *              is ((double)x - mean) / scale per coordinate (a division).  A non-finite mean or scale, or scale == 0: R, t and
 *              pose64 are all NaN, status 2.
 *   loop       R = I, t = 0, mu = 1; q_c is the normalised source point of entry c of the list, p_c its normalised partner
 *              (tgt[corr[i]]).  For it = 0 .. iterations - 1:
 *     weight   r = p - q;  d2 = fma(rz, rz, fma(ry, ry, rx * rx));  w = mu / (d2 + mu);  s = w * w
 *     rows     x: J = (0, -qz, qy, -1, 0, 0), residual rx;  y: (qz, 0, -qx, 0, -1, 0), ry;  z: (-qy, qx, 0, 0, 0, -1), rz
 *     values   the upper triangle of A = s J^T J by rows, then g = s J^T r -- each s times its x, y, z row terms added in that
 *              order, structural zeros skipped:
 *                A00 = s * (qz * qz + qy * qy)   A01 = s * -(qy * qx)   A02 = s * -(qz * qx)   A03 = 0   A04 = s * -qz   A05 = s * qy
 *                A11 = s * (qz * qz + qx * qx)   A12 = s * -(qz * qy)   A13 = s * qz   A14 = 0   A15 = s * -qx
 *                A22 = s * (qy * qy + qx * qx)   A23 = s * -qy   A24 = s * qx   A25 = 0
 *                A33 = s   A34 = 0   A35 = 0   A44 = s   A45 = 0   A55 = s
 *                g0 = s * (qz * ry + -(qy * rz))   g1 = s * (-(qz * rx) + qx * rz)   g2 = s * (qy * rx + -(qx * ry))
 *                g3 = s * -rx   g4 = s * -ry   g5 = s * -rz
 *              sums [27]: each value's sum over the L entries (the structural zeros are +0)
 *     solve    A x = -g by vcr_plane_refine_f32's Cholesky with its pivot rule (a pivot at or below 1e-12 times its diagonal
 *              entry, or not finite: singular).  A singular system or a non-finite x is an identity update -- Open3D's
 *              behaviour -- and sets bit 4 (16) of status.
 *     update   otherwise Ri = Rz(x2) Ry(x1) Rx(x0), ti = (x3, x4, x5) (Open3D's TransformVector6dToMatrix4d), and with
 *              m(v)_r = fma(Ri[r][2], v2, fma(Ri[r][1], v1, Ri[r][0] * v0)):  every column of R <- m(column);
 *              t <- m(t) + ti;  every q_c <- m(q_c) + ti  (the moved copy is moved again, as Open3D moves its own)
 *     mu       decrease_mu != 0 && it % 4 == 0 && mu > mu_floor:  mu <- mu / division_factor  (at the END of the iteration)
 *   closing    pose64 = (R row-major, then scale * t + mean_t - m'(mean_s)), m' the chain above with R for Ri;
 *              R_out, t_out = pose64 rounded once to fp32.
 * Optional outputs: sums holds the last iteration's (27 zeros where none ran), mu its value after the loop (1 where none ran),
 * norm = (mean_s, mean_t, scale) is written in every case.
 * Against Open3D: hashed draws for rand(); the squared form of the edge test; the moving cloud is the source, so no closing
 * inverse; mu_floor (its maximum_correspondence_distance, which it compares with mu in normalised units too) is
 * dimensionless; use_absolute_scale is not built.
 */
#ifndef VCR_HIP_FGR_H
#define VCR_HIP_FGR_H

#include "vcr_hip_match.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VCR_FGR_MAX_ITERATIONS 1024
#define VCR_FGR_MIN_ENTRIES 10            /* L below this: the identity, status 1 */

/* B, Ns, Nt < 1, a missing src, tgt, corr, R_out or t_out, tuple_scale outside [0, 1] or NaN, tuple_trials < 1, max_tuples < 1,
 * iterations outside [0, 1024], division_factor not finite or <= 1, mu_floor not finite or <= 0: VCR_EINVAL.
 * tuple_trials > VCR_RANSAC_MAX_TRIALS, Ns or Nt > 131 072, B * max(Ns, Nt) >= 2^31 or B * tuple_trials >= 2^29:
 * VCR_EUNSUPPORTED. */
typedef struct {
  uint32_t struct_bytes;        /* sizeof(vcr_fgr_args) as the CALLER was compiled (see vcr_fps_args); the mandatory part ends
                                   behind t_out: 0, shorter than that or longer than this library knows: VCR_EINVAL */
  const float* src; const float* tgt;   /* [B,3,Ns], [B,3,Nt] channels-first fp32, contiguous */
  const int* corr;              /* [B,Ns]: the target index per source point; outside [0, Nt) = none */
  int B, Ns, Nt;
  float tuple_scale;            /* 0: no tuple test; otherwise in (0, 1] */
  int tuple_trials;             /* T: 1 ... VCR_RANSAC_MAX_TRIALS */
  int max_tuples;               /* K >= 1 */
  uint32_t seed;
  int iterations;               /* 0 ... VCR_FGR_MAX_ITERATIONS */
  int decrease_mu;
  double division_factor;       /* finite, > 1 */
  double mu_floor;              /* finite, > 0 */
  float* R_out; float* t_out;   /* [B,3,3], [B,3], mandatory */
  int* pairs; int* tuples; int* used; int* status;   /* optional [B] each: M, tuples, L, status */
  int* tuple_list;              /* optional [B,3K]: source indices, the first L of a cloud written */
  double* norm;                 /* optional [B,7]: mean_s, mean_t, scale */
  double* pose64;               /* optional [B,12]: R row-major, then t, in the caller's frame */
  double* sums;                 /* optional [B,27]: the last iteration's sums */
  double* mu;                   /* optional [B]: mu after the loop */
} vcr_fgr_args;

/* Bytes of workspace vcr_fgr_f32 needs for these arguments; 0 for arguments the call would refuse.  The form does not depend
 * on the device: with an explicit cu_count (> 0) nothing touches one, and cu_count 0 asks for the same number. */
size_t vcr_fgr_workspace_bytes(const vcr_fgr_args*, int cu_count);
/* Asynchronous on the stream: no host synchronisation, no allocation; five launches (two without the tuple test).
 * workspace: device memory, 16-B aligned, at least vcr_fgr_workspace_bytes(args, 0) bytes (VCR_EWORKSPACE below that); its
 * contents need not be initialised. */
int    vcr_fgr_f32(const vcr_fgr_args*, void* workspace, size_t workspace_bytes, vcr_stream_t);

#ifdef __cplusplus
}
#endif
#endif

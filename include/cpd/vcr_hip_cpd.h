/*
 * vcr_hip_cpd.h -- registering by soft assignment: rigid Coherent Point Drift (Myronenko & Song, PAMI
 * 2010; pycpd, probreg, MATLAB's pcregistercpd).  An isotropic Gaussian mixture sits on the moved source points, a uniform
 * component of weight w takes the target points nothing explains, and EM alternates an O(M N) soft assignment with a closed-form
 * rigid (or similarity) update -- no neighbour search, no normals, no features, no correspondence cap.  An extension of
 * vcr_hip.h (same library, same conventions, same error codes); it adds no symbol to that header or to its other extensions
 * and moves none of their layouts, so VCR_ABI_VERSION is unchanged.
 *
 * src = Y [B,3,M] moves, tgt = X [B,3,N] is fixed.  The state per cloud is fp64: R, t, s, sigma2.
 *
 * vcr_cpd_expectation_f32 -- the E-step at a state; also the loop's round.  Every bit but ONE value per pair is defined.
 *   moved source r'_ij = (float)(s * (double)R_ij), t'_c = (float)t_c; ty_c(m) = fmaf(r'[3c+2], z, fmaf(r'[3c+1], y, r'[3c] * x)) +
 *               t'[c]: vcr_hip_score.h's fp32 expression on r', t', bit for bit, written once a round to the workspace
 *   pair weight d_c = x_c(n) - ty_c(m) in fp32;  d2 = (d_0 d_0 + d_1 d_1) + d_2 d_2, no fused multiply-add;
 *               k = (float)(-1.4426950408889634 / (2.0 * sigma2)), formed in fp64;  e_mn = exp2(d2 * k), the hardware's
 *               v_exp_f32 -- the ONE value that is not spelled out.  A point with a non-finite coordinate, source (moved) or
 *               target, has e = 0 with every partner: its own row or column is zero and nobody else's bits change
 *   sums        every streamed sum has ONE association.  A tile is 256 consecutive streamed points (the last may be shorter);
 *               its partial is an fp32 chain from +0 in ascending order.  A segment is VCR_CPD_SEGMENT = 4096 consecutive
 *               streamed points; its partial is the fp64 sum of its tiles' partials ascending from +0.  The total is the fp64
 *               sum of the segment partials ascending from +0.  Every launch form stores the per-segment partials and a second
 *               launch adds them: forms differ in which workgroup takes which segments, in points per lane and in how the
 *               streamed point reaches the lanes, never in this association
 *   pass 1      streams m for each n:  S_n = sum_m e_mn;  q = 6.283185307179586 * sigma2;
 *               c = ((q * sqrt(q)) * (w / (1.0 - w))) * ((double)M / (double)N), fp64, once a cloud;  den_n = S_n + c;
 *               rden_n = 1.0 / den_n;  inv_n = (float)rden_n, or 0 where den_n == 0 (w = 0 and every weight underflowed: the
 *               point is an outlier, deliberately not CPD's "assign to the nearest");  Pt1_n = S_n * rden_n, 0 where den_n == 0
 *   pass 2      streams n for each m:  p = e_mn * inv_n in fp32;  P1_m = sum_n p;  PX_m,c = sum_n p * x_c(n), the product in
 *               fp32, the same hierarchy
 *   outputs     fp64: Pt1 [B,N], P1 [B,M], PX [B,3,M], Np [B].  Np = sum_m P1_m per 256 consecutive source points (lanes past M
 *               add zeros): the wave butterfly v_l += v_{l ^ o}, o = 32 ... 1, then the four waves ascending, then the
 *               partials ascending from +0 -- the refinements' order.  Optional e_stage [B,M,N] fp32: e_mn
 *
 * M-step (inside vcr_cpd_f32) -- one workgroup per cloud, fp64, no fused multiply-add, no atomics; every sum over points in the
 * 256-block order above; y is the ORIGINAL source point, x the target point, both widened to fp64 as they are: a non-finite
 * point reaches the sums (0 * NaN) and stops the loop with status 4 -- filter the clouds first.
 *   first       Np = sum P1;  sx_c = sum_m PX_m,c;  sy_c = sum_m P1_m * y_m,c;  mux = sx / Np;  muy = sy / Np
 *   second      yh = y - muy;  A_ij = sum_m (PX_m,i - P1_m * mux_i) * yh_m,j;  yPy = sum_m P1_m * ((yh_0^2 + yh_1^2) + yh_2^2);
 *               xPx = sum_n Pt1_n * ((xh_0^2 + xh_1^2) + xh_2^2), xh = x - mux
 *   rotation    the rigid solve's one-sided Jacobi on H = A^T and its tail (ordering, rank completion, the reflection rule that
 *               flips the vector of the smallest singular value): R = U diag(1, 1, det(U V^T)) V^T for A = U S V^T
 *   rest        trAR = sum_ij A_ij * R_ij, row-major ascending from +0;  s = trAR / yPy with scaling, 1 without;
 *               t_c = mux_c - s * ((R_c0 * muy_0 + R_c1 * muy_1) + R_c2 * muy_2);
 *               sigma2_new = ((xPx - (2.0 * s) * trAR) + (s * s) * yPy) / (3.0 * Np)
 *   taken       a state that is taken stores R and t ROUNDED to fp32 (and widened again), so the returned fp32 pose is the
 *               pose the last E-step saw; s and sigma2 stay fp64
 *
 * vcr_cpd_f32 -- the loop, one call, every round enqueued, no host synchronisation, a cloud's result independent of its batch.
 *   start       the pose given (s = 1), or the identity.  sigma2_0 given, or sum_n sum_m |x_n - T(y_m)|^2 / (3 M N) evaluated in
 *               fp64 about the two clouds' means: cx = (sum x) / N, cy = (sum ty) / M (ty the fp32 moved source),
 *               ((M * sum|x - cx|^2 + N * sum|ty - cy|^2) + (M * N) * |cx - cy|^2) / ((3 * M) * N), block order.
 *               floor = sigma2_floor, or 1e-8 * sigma2_0.  A start sigma2 that is not finite or not > 0: status 4 at once
 *   round       E-step at the state, M-step, then the stops in this order:
 *               4  a non-finite sum (Np, sx, sy); the state stays
 *               3  Np == 0; the state stays
 *               4  a non-finite sum (A, yPy, xPx) or result (R, t, s, sigma2_new); the state stays
 *               2  collapsed: sigma2_new is not > floor.  The new pose is taken and sigma2 is set to the floor
 *               0  converged: |sigma2_new - sigma2| <= tolerance * sigma2.  The new state is taken
 *               1  max_iterations M-steps done (the new state is taken)
 *   closing     after a stop that took a state one more E-step runs at it: the returned Pt1, P1, PX, Np are
 *               vcr_cpd_expectation_f32's at (R_out, t_out, scale, sigma2), bit for bit.  max_iterations + 1 E-steps are
 *               enqueued; the launches of a stopped cloud return at once through a per-cloud live word
 *   returned    R_out, t_out = the state's pose (fp32); R_ba, t_ba its inverse as vcr_refine_f32 has it (of R, t alone: the
 *               scale is returned beside them); scale, sigma2, Np fp64; iterations = M-steps done; status;
 *               trace[0] = sigma2_0, trace[k] = sigma2 after M-step k (the floor at a collapse), NaN behind the stop
 */
#ifndef VCR_HIP_CPD_H
#define VCR_HIP_CPD_H

#include "../vcr_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VCR_CPD_TILE 256
#define VCR_CPD_SEGMENT 4096
#define VCR_CPD_STATE_BYTES 256    /* per cloud, in the workspace */
#define VCR_CPD_FORMS 6            /* 1 ... 3: the streamed point through LDS tiles, 1 / 2 / 4 points a lane; 4 ... 6: through
                                      scalar loads, 1 / 2 / 4 points a lane */
#define VCR_CPD_CONVERGED 0
#define VCR_CPD_MAX_ITERATIONS 1
#define VCR_CPD_COLLAPSED 2
#define VCR_CPD_NO_MASS 3
#define VCR_CPD_NOT_FINITE 4

/* B, M, N < 1, a missing src or tgt, one of R and t without the other, w outside [0, 1) or NaN, without sigma2_dev a sigma2
 * that is not finite or not > 0 (vcr_cpd_f32: 0 = compute sigma2_0), without scale_dev a scale that is not finite or not > 0,
 * a variant that names no form, and for vcr_cpd_f32 max_iterations < 0, a tolerance or a sigma2_floor negative or NaN:
 * VCR_EINVAL.  M or N > 131 072, B * M or B * N >= 2^31, max_iterations > 2^20: VCR_EUNSUPPORTED.  _expectation_ needs Pt1,
 * P1, PX and Np and ignores what follows e_stage; vcr_cpd_f32 needs Pt1, P1, PX (its M-step reads them there), R_out and t_out
 * and takes every other output as optional.  What a DEVICE array holds cannot be refused here: a cloud whose sigma2_dev or
 * scale_dev entry is not finite or not > 0 gets no E-step -- _expectation_ writes NaN to its Pt1, P1, PX and Np (e_stage too),
 * the loop stops it with status 4 at once -- and the other clouds of the batch are served as if alone. */
typedef struct {
  uint32_t struct_bytes;        /* sizeof(vcr_cpd_args) as the CALLER was compiled; the mandatory part ends behind e_stage: 0,
                                   shorter than that or longer than this library knows: VCR_EINVAL */
  const float* src;             /* Y [B,3,M] channels-first fp32, contiguous: moves */
  const float* tgt;             /* X [B,3,N]: fixed */
  int B, M, N;
  const float* R; const float* t;   /* [B,3,3], [B,3]; both NULL = the identity */
  double sigma2;                /* the variance of every cloud ... */
  const double* sigma2_dev;     /* ... or, when given, [B] on the device: one per cloud */
  double scale;                 /* s of every cloud (_expectation_ only; the loop starts at 1) ... */
  const double* scale_dev;      /* ... or [B] on the device */
  double w;                     /* the uniform component's weight, in [0, 1) */
  int variant;                  /* 0 = the plan decides; f + 8 g: f = 1 ... VCR_CPD_FORMS forces a form (0: the plan's), g = 1
                                   forces one workgroup over all segments, g = 2 one workgroup a segment (0: the plan's).
                                   Every variant returns the same bits */
  double* Pt1;                  /* [B,N] */
  double* P1;                   /* [B,M] */
  double* PX;                   /* [B,3,M] */
  double* Np;                   /* [B] */
  float* e_stage;               /* optional [B,M,N] */
  int max_iterations;           /* M-steps */
  int with_scaling;             /* 0: rigid; otherwise a similarity */
  double tolerance;
  double sigma2_floor;          /* 0 = 1e-8 * sigma2_0 */
  float* R_out; float* t_out;   /* [B,3,3], [B,3] */
  float* R_ba; float* t_ba;     /* optional: the inverse, as vcr_refine_f32's */
  double* scale_out;            /* optional [B] */
  double* sigma2_out;           /* optional [B] */
  int* iterations; int* status; /* optional [B] each */
  double* trace;                /* optional [B, max_iterations + 1] */
} vcr_cpd_args;

/* With up(v) = v rounded up to a multiple of 256, sm = ceil(M / 4096), sn = ceil(N / 4096):
 * up(VCR_CPD_STATE_BYTES B) + up(16 B M) + up(16 B N) + up(8 B sm N) + up(32 B sn M) (the state, the moved source, the target
 * with inv_n, the per-segment partials of the two passes), the same for both calls and every variant; 0 for arguments the call
 * would refuse; with an explicit cu_count > 0 nothing touches a device. */
size_t vcr_cpd_expectation_workspace_bytes(const vcr_cpd_args*, int cu_count);
size_t vcr_cpd_workspace_bytes(const vcr_cpd_args*, int cu_count);
/* Asynchronous on the stream: no host synchronisation, no allocation, no atomic.  7 launches (_expectation_; 8 with e_stage);
 * 6 (max_iterations + 1) + 2 (vcr_cpd_f32), whose shapes depend on (B, M, N) and the form alone.  workspace: device memory, 16-B
 * aligned, at least _workspace_bytes (VCR_EWORKSPACE below that); its contents need not be initialised.  Every slot of every
 * output is written. */
int    vcr_cpd_expectation_f32(const vcr_cpd_args*, void* workspace, size_t workspace_bytes, vcr_stream_t);
int    vcr_cpd_f32(const vcr_cpd_args*, void* workspace, size_t workspace_bytes, vcr_stream_t);
/* Host-only with cu_count > 0 (0: the current device's): the form (1 ... VCR_CPD_FORMS) and the workgroups the segments of
 * pass 1 (over M) and of pass 2 (over N) are dealt to. */
int    vcr_cpd_expectation_form(const vcr_cpd_args*, int cu_count, int* form, int* splits1, int* splits2);
int    vcr_cpd_form(const vcr_cpd_args*, int cu_count, int* form, int* splits1, int* splits2);

#ifdef __cplusplus
}
#endif
#endif

/*
 * vcr_hip_mls.h -- moving least squares smoothing (PCL's MovingLeastSquares, polynomial order 1 or 2, SIMPLE projection) over
 * neighbourhoods given as ragged rows: every point is moved onto a quadratic fitted, with Gaussian weights,
 * to its neighbours' heights over the plane across its normal.  An extension of vcr_hip.h (same library, same conventions, same
 * error codes); it adds no symbol to that header or to its other extensions and moves none of their layouts, so VCR_ABI_VERSION is
 * unchanged.
 *
 * The rows.  Per cloud b:
 *   idx          int32 [B,capacity]; row_start int64 [B,N+1]; total int64 [B] -- what a radius search over the cloud itself writes,
 *                but any caller may build them.  Point i's row is idx[b, row_start[b,i] ... row_start[b,i+1]), n_i entries; a row
 *                does not hold its own point: the fit adds the point itself, m = n_i + 1
 *   entry        an entry outside [0, N) reads as i
 *   no radius    no stage knows a radius or re-tests a distance: the row IS the neighbourhood
 *   served       cloud b is served iff 0 <= total[b] <= capacity, row_start[b,0] == 0, row_start[b,N] == total[b] and
 *                row_start[b,i] <= row_start[b,i+1] for every i.  No idx entry of a cloud that is not served is read.  The other
 *                clouds of the batch are unaffected
 *   d_e          of entry e (neighbour j) of row i: the three fp32 differences x_j - x_i, widened to fp64.  An entry of which a
 *                component of d_e is not finite is SKIPPED: it adds +0.0 to every sum below and its weight is +0.0
 *   64 chains    a sum over a row: chain p (p = 0 ... 63) adds the terms of the entries p, p + 64, ... in ascending order, from +0.0;
 *                then six steps v[p] = v[p] + v[p ^ s] follow for s = 32, 16, 8, 4, 2, 1.  IEEE addition is commutative, so every
 *                chain ends with the same bits.  The definition fixes this TREE, not where a node is computed
 * Everything is fp64, one rounding an operation, no fused multiply-add.
 *
 * FRAME of point i (both stages build it alike):
 *   n            normals[b,:,i] widened;  s = (nx*nx + ny*ny) + nz*nz
 *   no frame     where x_i or n holds a value that is not finite, or s is not > 0 and finite
 *   nh           = n * (1.0 / sqrt(s))
 *   a            the axis with the smallest |nh_a|, the lowest index among equals; e = the unit vector of axis a (0.0s and a 1.0)
 *   u            = nh x e written out: u0 = nh1*e2 - nh2*e1, u1 = nh2*e0 - nh0*e2, u2 = nh0*e1 - nh1*e0.  Every component is ONE
 *                difference of two products.  |u|^2 = 1 - nh_a^2 >= 2/3: u is never zero
 *   uh           = u * (1.0 / sqrt((u0*u0 + u1*u1) + u2*u2)): u normalised as nh was
 *   v            = nh x uh, written out likewise.  nh and uh are unit and orthogonal up to rounding, so v is unit up to a few units
 *                in the last place and is NOT normalised again: this is the definition
 *
 * STAGE A (vcr_mls_weights_f32): the origin of every fit and every entry's weight.
 *   mean         S_d = the three sums of d_e over the row, in the 64 chains;  mu = S_d / m, m = n_i + 1 as a double
 *   origin       the point's projection on the plane across nh through the mean, relative to x_i:
 *                t = (mu0*nh0 + mu1*nh1) + mu2*nh2;  o = t * nh
 *   weight       q = d_e - o;  w_e = exp(-(((q0*q0 + q1*q1) + q2*q2) / h2)), h2 the double sqr_gauss_param: the ONE library call of
 *                the definition.  Everything before it and everything behind it is defined to the bit; two exp implementations may
 *                differ in the last places, which is why the weights are a stage of their own: the fit of GIVEN weights is exact
 *   w_self       the point's own weight: the same with q = -o
 *   outputs      weight float64 [B,capacity] (+0.0 in a skipped slot; NaN in every slot of a point without a frame, behind total[b]
 *                and over a cloud that is not served), origin float64 [B,N,3], w_self float64 [B,N] (NaN without a frame) and
 *                frame int32 [B,N]: 1 / 0, VCR_MLS_NOT_SERVED over a cloud that is not served.  Every slot is written
 *
 * STAGE B (vcr_mls_fit_f32): the fit, reading weight, origin, w_self and frame AS GIVEN (stage A's, or any caller's).
 *   no fit       fit = 0 where frame[b,i] == 0, the frame cannot be built, or m < min_neighbors: the point comes back with its input
 *                bits, coeffs 0.0, and its normal is nh rounded to fp32 (NaN where there is no frame)
 *   terms        of entry e:  q = d_e - o;  uu = (q0*uh0 + q1*uh1) + q2*uh2, vv likewise with v, f likewise with nh;
 *                p = (1, vv, vv*vv, uu, uu*vv, uu*uu) (PCL's term order);  wp_a = w_e * p_a
 *   sums         A_ab = sum of wp_a * p_b (a <= b, 21 of them) and r_a = sum of wp_a * f (6): each over the row in the 64 chains;
 *                then the point's own term (q = -o, the weight w_self) is added to each by ONE addition, last
 *   solve        A c = r by Cholesky, A = L L^T, column k = 0 ... 5:  t = A_kk, then t = t - L_kj*L_kj for j = 0 ... k-1 in that
 *                order;  the pivot t FAILS where it is not finite or not > A_kk * 2^-40 (A_kk as summed);  L_kk = sqrt(t);  for
 *                i = k+1 ... 5:  t = A_ik, then t = t - L_ij*L_kj for j = 0 ... k-1, L_ik = t / L_kk.  Forward, k = 0 ... 5:
 *                t = r_k, t = t - L_kj*y_j for j = 0 ... k-1, y_k = t / L_kk.  Back, k = 5 ... 0:  t = y_k, t = t - L_jk*c_j for
 *                j = k+1 ... 5 ascending, c_k = t / L_kk
 *   fit          1 (the plane alone, c = 0.0 in all six) where order == 1, m < 6 or a pivot failed; 2 otherwise
 *   point        out_a = (float)((double)x_a + (o_a + c0 * nh_a))
 *   normal       g_a = (nh_a - c3*uh_a) - c1*v_a;  (float)(g_a * (1.0 / sqrt((g0*g0 + g1*g1) + g2*g2))): the fitted surface's normal
 *                at the projected point, on the side of the input normal
 *   outputs      points float32 [B,3,N], fit int32 [B,N], and where asked normals float32 [B,3,N] and coeffs float64 [B,N,6].  A
 *                cloud that is not served gets NaN in every point, normal and coefficient and VCR_MLS_NOT_SERVED in every fit
 *
 * Both stages are asynchronous on the stream: no host synchronisation, no allocation, no atomics, no workspace.  Each is two
 * launches: the pass (a wave a row), and a check of row_start that voids a cloud (and pads the weights).
 *
 * Launch forms of stage B's combine, which return the same bits:
 *   VCR_MLS_PLAIN      every lane keeps all 27 sums through the six steps: 162 exchanges of a double
 *   VCR_MLS_TRANSPOSE  at every step a lane keeps half of its sums and hands the other half to lane p ^ s: 32 exchanges, then
 *                      27 broadcasts
 * variant 0 takes the plan's form: the transposing one, which was 1.3 to 1.4 times faster in all twelve measured cases (rows of
 * about 12 and about 100 entries; DESIGN.md section 4.34, profiles/mls_bench.txt).
 */
#ifndef VCR_HIP_MLS_H
#define VCR_HIP_MLS_H

#include "../vcr_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VCR_MLS_MAX_N 131072
#define VCR_MLS_PLAIN 1
#define VCR_MLS_TRANSPOSE 2
#define VCR_MLS_NOT_SERVED (-2)           /* the value the other row families' flags use for a cloud that is not served */
#define VCR_MLS_TERMS 6                   /* coefficients of a fit: 1, v, v^2, u, uv, u^2 */

/* Both stages: B < 1, a missing mandatory pointer (idx and weight may be NULL where capacity == 0), capacity < 0, a
 * sqr_gauss_param that is not finite and > 0, an order other than 1 or 2, min_neighbors < 1, a variant other than 0, VCR_MLS_PLAIN
 * or VCR_MLS_TRANSPOSE, a bad struct_bytes, xyz4 not 16-B aligned: VCR_EINVAL.  N outside [1, 131 072], B * N >= 2^31 or
 * B * capacity >= 2^31: VCR_EUNSUPPORTED. */
typedef struct {
  uint32_t struct_bytes;        /* sizeof(vcr_mls_weights_args) as the CALLER was compiled; every field of today is mandatory:
                                   0, shorter than that or longer than this library knows: VCR_EINVAL */
  const float* xyz4;            /* [B,N,4] rows (x, y, z and a fourth value that is not read), 16-B aligned */
  const float* normals;         /* [B,3,N] channels-first; any length (the frame normalises in fp64) */
  const int* idx;               /* [B,capacity] */
  const int64_t* row_start;     /* [B,N+1] */
  const int64_t* total;         /* [B] */
  int B, N, capacity;
  double sqr_gauss_param;       /* h2: finite and > 0 */
  double* weight;               /* out [B,capacity], mandatory where capacity > 0 */
  double* origin;               /* out [B,N,3] */
  double* w_self;               /* out [B,N] */
  int* frame;                   /* out [B,N] */
} vcr_mls_weights_args;

int vcr_mls_weights_f32(const vcr_mls_weights_args*, vcr_stream_t);

typedef struct {
  uint32_t struct_bytes;        /* the mandatory part ends behind fit: 0, shorter than that or longer than this library knows:
                                   VCR_EINVAL */
  const float* xyz4;            /* [B,N,4], 16-B aligned */
  const float* normals;         /* [B,3,N] */
  const int* idx;               /* [B,capacity] */
  const int64_t* row_start;     /* [B,N+1] */
  const int64_t* total;         /* [B] */
  const double* weight;         /* [B,capacity] as given (may be NULL where capacity == 0) */
  const double* origin;         /* [B,N,3] as given */
  const double* w_self;         /* [B,N] as given */
  const int* frame;             /* [B,N] as given: 0 = no fit */
  int B, N, capacity;
  int order;                    /* 1 = the plane alone, 2 = the quadratic */
  int min_neighbors;            /* >= 1, held against m = n_i + 1 */
  int variant;                  /* 0 = the plan; VCR_MLS_PLAIN / VCR_MLS_TRANSPOSE force a combine (tests, benchmarks) */
  float* points;                /* out [B,3,N] */
  int* fit;                     /* out [B,N]: 2 / 1 / 0, VCR_MLS_NOT_SERVED over a cloud that is not served */
  float* normals_out;           /* optional out [B,3,N] */
  double* coeffs;               /* optional out [B,N,6] */
} vcr_mls_fit_args;

int vcr_mls_fit_f32(const vcr_mls_fit_args*, vcr_stream_t);

#ifdef __cplusplus
}
#endif
#endif

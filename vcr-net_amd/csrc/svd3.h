// The 3x3 fp64 rigid solve's shared pieces: the quad one-sided Jacobi SVD (DPP sums over four lanes) and the tail on one lane
// (ordering, rank completion, R = V U^T, the reflection rule).  Included by rigid_svd.hip (the learned correspondences' solve)
// and refine.hip (the ICP step on the full clouds): one text, so both solve alike.
#pragma once
#include "common.h"

namespace {

// sum over the four lanes of a DPP quad (two butterflies on the 32-bit halves of a double); same value in every lane
__device__ __forceinline__ double quad_xor(double v, int ctrl_is_1) {
  int lo = __double2loint(v), hi = __double2hiint(v);
  if (ctrl_is_1) { lo = __builtin_amdgcn_mov_dpp(lo, 0xB1, 0xF, 0xF, true); hi = __builtin_amdgcn_mov_dpp(hi, 0xB1, 0xF, 0xF, true); }
  else { lo = __builtin_amdgcn_mov_dpp(lo, 0x4E, 0xF, 0xF, true); hi = __builtin_amdgcn_mov_dpp(hi, 0x4E, 0xF, 0xF, true); }
  return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double quad_sum(double v) {
  v += quad_xor(v, 1);                                   // lanes (0,1) (2,3)
  v += quad_xor(v, 0);                                   // + the other pair: (x0 + x1) + (x2 + x3) in every lane
  return v;
}
__device__ __forceinline__ double quad_get(double v, int lane_in_quad) {   // lane_in_quad: compile-time 0..2
  int lo = __double2loint(v), hi = __double2hiint(v);
  const int c = lane_in_quad == 0 ? 0x00 : lane_in_quad == 1 ? 0x55 : 0xAA;
  if (lane_in_quad == 0) { lo = __builtin_amdgcn_mov_dpp(lo, 0x00, 0xF, 0xF, true); hi = __builtin_amdgcn_mov_dpp(hi, 0x00, 0xF, 0xF, true); }
  else if (lane_in_quad == 1) { lo = __builtin_amdgcn_mov_dpp(lo, 0x55, 0xF, 0xF, true); hi = __builtin_amdgcn_mov_dpp(hi, 0x55, 0xF, 0xF, true); }
  else { lo = __builtin_amdgcn_mov_dpp(lo, 0xAA, 0xF, 0xF, true); hi = __builtin_amdgcn_mov_dpp(hi, 0xAA, 0xF, 0xF, true); }
  (void)c;
  return __hiloint2double(hi, lo);
}

// One-sided Jacobi sweeps on the quad: lane i < 3 holds a[0..2] = row i of A (initially H) and v[0..2] = row i of V
// (initially I); lane 3 holds zeros.  The control flow is uniform over the quad (the inner products are quad sums).
// Every test is relative to the columns' own norms: H scales with the square of the cloud size (ga with its fourth power),
// and a cloud of any size the fp32 inputs can hold must converge like a unit one.
__device__ __forceinline__ void jacobi_sweeps_quad(double (&a)[3], double (&v)[3]) {
  for (int sweep = 0; sweep < 40; ++sweep) {
    double off = 0.0;
#pragma unroll
    for (int pq = 0; pq < 3; ++pq) {
      const int p = (pq == 2) ? 1 : 0, q = (pq == 0) ? 1 : 2;
      const double al = quad_sum(a[p] * a[p]), be = quad_sum(a[q] * a[q]), ga = quad_sum(a[p] * a[q]);
      const double ab = sqrt(al) * sqrt(be);                // (not sqrt(al * be): the product can leave fp64's range)
      if (!(fabs(ga) > 1e-17 * ab)) continue;               // orthogonal already; a zero column (ab == 0) is skipped too
      off = fmax(off, fabs(ga) / ab);
      const double zeta = (be - al) / (2.0 * ga);
      const double tt = (zeta >= 0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
      const double c = 1.0 / sqrt(1.0 + tt * tt), s = c * tt;
      const double ap = a[p], aq = a[q];
      a[p] = c * ap - s * aq; a[q] = s * ap + c * aq;
      const double vp = v[p], vq = v[q];
      v[p] = c * vp - s * vq; v[q] = s * vp + c * vq;
    }
    if (off < 1e-15) break;
  }
}

// Tail of the solve on one lane, from the converged A (columns = singular vectors times singular values) and V
__device__ void svd3_finish(const double A[3][3], const double V[3][3], double R[9]) {
  double sig[3];
  int ord[3] = {0, 1, 2};
  for (int j = 0; j < 3; ++j) sig[j] = sqrt(A[0][j] * A[0][j] + A[1][j] * A[1][j] + A[2][j] * A[2][j]);
  for (int i = 0; i < 2; ++i)
    for (int j = 0; j < 2 - i; ++j)
      if (sig[ord[j]] < sig[ord[j + 1]]) { const int tmp = ord[j]; ord[j] = ord[j + 1]; ord[j + 1] = tmp; }
  double U[3][3], W[3][3];
  for (int j = 0; j < 3; ++j) {
    const int c = ord[j];
    const double inv = sig[c] > 0 ? 1.0 / sig[c] : 0.0;
    for (int i = 0; i < 3; ++i) { U[i][j] = A[i][c] * inv; W[i][j] = V[i][c]; }
  }
  // Vanishing singular values leave their left vectors undefined: complete the frame so that R is always a proper
  // rotation.  Rank 2 (coplanar pairs): u2 = u0 x u1, either sign gives the same R after the determinant rule
  // below.  Rank 1 / rank 0 (all pairs on a line / one point; happens when tiny partial clouds collapse in later
  // vcrnetIter passes): R is not unique -- LAPACK's choice in the reference is arbitrary too -- we take the
  // completion closest to the coordinate axes, and R = I for H = 0.
  const double s0 = sig[ord[0]];
  if (!(s0 > 0)) {
    for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) U[i][j] = W[i][j];
  } else {
    if (sig[ord[1]] <= 1e-12 * s0) {
      int e = 0;
      for (int i = 1; i < 3; ++i) if (fabs(U[i][0]) < fabs(U[e][0])) e = i;
      double v[3] = {0, 0, 0}, n2 = 0;
      v[e] = 1.0;
      const double d = U[e][0];
      for (int i = 0; i < 3; ++i) { v[i] -= d * U[i][0]; n2 += v[i] * v[i]; }
      const double inv = 1.0 / sqrt(n2);
      for (int i = 0; i < 3; ++i) U[i][1] = v[i] * inv;
    }
    if (sig[ord[2]] <= 1e-12 * s0) {
      U[0][2] = U[1][0] * U[2][1] - U[2][0] * U[1][1];
      U[1][2] = U[2][0] * U[0][1] - U[0][0] * U[2][1];
      U[2][2] = U[0][0] * U[1][1] - U[1][0] * U[0][1];
    }
  }
  auto build = [&]() {
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j) R[3 * i + j] = W[i][0] * U[j][0] + W[i][1] * U[j][1] + W[i][2] * U[j][2];
  };
  build();
  const double det = R[0] * (R[4] * R[8] - R[5] * R[7]) - R[1] * (R[3] * R[8] - R[5] * R[6]) +
                     R[2] * (R[3] * R[7] - R[4] * R[6]);
  if (det < 0) {
    for (int i = 0; i < 3; ++i) W[i][2] = -W[i][2];
    build();
  }
}

}  // namespace

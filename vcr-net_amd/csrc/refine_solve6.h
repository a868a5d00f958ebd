// What the six-unknown fits share behind their sums (refine_plane.hip, refine_gicp.hip): the Cholesky solve with its pivot
// rule and Open3D's TransformVector6dToMatrix4d.  One lane, registers only.
#pragma once

namespace {

constexpr double PL_PIVOT = 1e-12;                         // a Cholesky pivot at or below this times its diagonal entry: singular

// A x = -g for the symmetric A (upper triangle by rows in a21) by Cholesky, fully unrolled: registers only.  false: singular.
__device__ bool pl_solve(const double* a21, const double* g, double* x) {
  double A[6][6], L[6][6];
  int e = 0;
#pragma unroll
  for (int r = 0; r < 6; ++r)
#pragma unroll
    for (int c = r; c < 6; ++c) { A[r][c] = a21[e]; A[c][r] = a21[e]; ++e; }
  bool ok = true;
#pragma unroll
  for (int j = 0; j < 6; ++j) {
    double s = A[j][j];
#pragma unroll
    for (int k = 0; k < j; ++k) s -= L[j][k] * L[j][k];
    ok = ok && __builtin_isfinite(s) && s > PL_PIVOT * A[j][j];
    const double d = sqrt(s);
    L[j][j] = d;
#pragma unroll
    for (int i = j + 1; i < 6; ++i) {
      double v = A[i][j];
#pragma unroll
      for (int k = 0; k < j; ++k) v -= L[i][k] * L[j][k];
      L[i][j] = v / d;
    }
  }
  double y[6];
#pragma unroll
  for (int i = 0; i < 6; ++i) {                            // L y = -g
    double v = -g[i];
#pragma unroll
    for (int k = 0; k < i; ++k) v -= L[i][k] * y[k];
    y[i] = v / L[i][i];
  }
#pragma unroll
  for (int i = 5; i >= 0; --i) {                           // L^T x = y
    double v = y[i];
#pragma unroll
    for (int k = i + 1; k < 6; ++k) v -= L[k][i] * x[k];
    x[i] = v / L[i][i];
  }
  return ok;
}

// R_i = Rz(x2) Ry(x1) Rx(x0), t_i = (x3, x4, x5)
__device__ __forceinline__ void pl_euler(const double* x, double* Ri, double* ti) {
  double s0, c0, s1, c1, s2, c2;
  sincos(x[0], &s0, &c0); sincos(x[1], &s1, &c1); sincos(x[2], &s2, &c2);
  Ri[0] = c2 * c1; Ri[1] = (c2 * s1) * s0 - s2 * c0; Ri[2] = (c2 * s1) * c0 + s2 * s0;
  Ri[3] = s2 * c1; Ri[4] = (s2 * s1) * s0 + c2 * c0; Ri[5] = (s2 * s1) * c0 - c2 * s0;
  Ri[6] = -s1;     Ri[7] = c1 * s0;                  Ri[8] = c1 * c0;
  ti[0] = x[3]; ti[1] = x[4]; ti[2] = x[5];
}

}  // namespace

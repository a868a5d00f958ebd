// One point's three eigenvalues from its nine sums (include/keypoint/vcr_hip_iss.h): normals_point.h's C, its
// cyclic Jacobi and its sort, without the eigenvectors.  The rotations are nm_rotate itself: its columns of v are fed values
// nobody reads, so the compiler drops them and the diagonal keeps vcr_normals_f32's bits.
#pragma once
#include "normals_point.h"

constexpr int ISS_ZERO = 0, ISS_NOT_FINITE = 1, ISS_SOLVED = 2;

// The sums of m rows -> l0 <= l1 <= l2 (ISS_SOLVED); they are left alone where C is all zero or not finite.
__device__ __forceinline__ int iss_eigenvalues(const NmSums& s, double m, double& l0, double& l1, double& l2) {
  const double mx = s.sx / m, my = s.sy / m, mz = s.sz / m;
  double a00 = s.sxx / m - mx * mx, a01 = s.sxy / m - mx * my, a02 = s.sxz / m - mx * mz;
  double a11 = s.syy / m - my * my, a12 = s.syz / m - my * mz, a22 = s.szz / m - mz * mz;
  const bool finite = __builtin_isfinite(a00) && __builtin_isfinite(a01) && __builtin_isfinite(a02) && __builtin_isfinite(a11) &&
                      __builtin_isfinite(a12) && __builtin_isfinite(a22);
  if (!finite) return ISS_NOT_FINITE;
  if (a00 == 0. && a01 == 0. && a02 == 0. && a11 == 0. && a12 == 0. && a22 == 0.) return ISS_ZERO;
  double v0 = 0., v1 = 0., v2 = 0., v3 = 0., v4 = 0., v5 = 0.;              // (not read)
  for (int sweep = 0; sweep < NM_SWEEPS; ++sweep) {
    if (a01 == 0. && a02 == 0. && a12 == 0.) break;
    nm_rotate(a00, a11, a01, a02, a12, v0, v1, v2, v3, v4, v5);             // (0, 1): the third row is 2
    nm_rotate(a00, a22, a02, a01, a12, v0, v1, v2, v3, v4, v5);             // (0, 2): the third row is 1
    nm_rotate(a11, a22, a12, a01, a02, v0, v1, v2, v3, v4, v5);             // (1, 2): the third row is 0
  }
  const int c = (a00 <= a11 && a00 <= a22) ? 0 : (a11 <= a22 ? 1 : 2);       // the smallest, the lowest index among equals
  l0 = c == 0 ? a00 : c == 1 ? a11 : a22;
  const double o1 = c == 0 ? a11 : a00, o2 = c == 2 ? a11 : a22;            // the other two
  l1 = o1 <= o2 ? o1 : o2;
  l2 = o1 <= o2 ? o2 : o1;
  return ISS_SOLVED;
}

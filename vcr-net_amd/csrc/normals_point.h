// One point's normal from its nine sums (include/vcr_hip_plane.h): what normals.hip's lane a point and
// rows.hip's lane a row both run behind their own loop over the neighbours -- C, the cyclic Jacobi, the smallest eigenvalue's
// column, the sign rule and the curvature, in that lane's registers.
#pragma once
#include "common.h"

constexpr int NM_SWEEPS = 16;                              // a cap: the sweeps converge quadratically and stop on an exact zero

// The nine fp64 sums over a point's rows, in the order the caller adds them
struct NmSums {
  double sx = 0., sy = 0., sz = 0., sxx = 0., sxy = 0., sxz = 0., syy = 0., syz = 0., szz = 0.;
  __device__ __forceinline__ void add(const f32x4& v, const f32x4& me) {
    const double dx = (double)(v[0] - me[0]), dy = (double)(v[1] - me[1]), dz = (double)(v[2] - me[2]);
    sx += dx; sy += dy; sz += dz;                          // (the row i itself adds exact zeros: it only counts in m)
    sxx += dx * dx; sxy += dx * dy; sxz += dx * dz; syy += dy * dy; syz += dy * dz; szz += dz * dz;   // products exact
  }
};

// One Jacobi rotation that annihilates a_pq of the symmetric matrix: (app, aqq, apq) the 2 x 2 block, (arp, arq) the third
// row's entries in columns p and q, (v.p, v.q) the eigenvector columns.
__device__ __forceinline__ void nm_rotate(double& app, double& aqq, double& apq, double& arp, double& arq,
                                          double& v0p, double& v0q, double& v1p, double& v1q, double& v2p, double& v2q) {
  if (apq == 0.0) return;
  const double theta = (aqq - app) / (2.0 * apq);
  const double th2 = theta * theta;
  // the smaller root of t^2 + 2 theta t - 1 = 0; past the range of theta^2 its limit
  const double t = __builtin_isinf(th2) ? 0.5 / theta : (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(th2 + 1.0));
  const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
  app = app - t * apq; aqq = aqq + t * apq; apq = 0.0;
  const double x = arp, y = arq;
  arp = c * x - s * y; arq = s * x + c * y;
  const double a0 = v0p, b0 = v0q, a1 = v1p, b1 = v1q, a2 = v2p, b2 = v2q;
  v0p = c * a0 - s * b0; v0q = s * a0 + c * b0;
  v1p = c * a1 - s * b1; v1q = s * a1 + c * b1;
  v2p = c * a2 - s * b2; v2q = s * a2 + c * b2;
}

// The sums of m rows -> the fp32 normal (n0, n1, n2) and the curvature.  me: the point's row; vp: its cloud's viewpoint or NULL.
__device__ __forceinline__ void nm_point(const NmSums& s, double m, const f32x4& me, const float* vp, float& n0, float& n1,
                                         float& n2, float& cv) {
  const double mx = s.sx / m, my = s.sy / m, mz = s.sz / m;
  double a00 = s.sxx / m - mx * mx, a01 = s.sxy / m - mx * my, a02 = s.sxz / m - mx * mz;
  double a11 = s.syy / m - my * my, a12 = s.syz / m - my * mz, a22 = s.szz / m - mz * mz;
  const bool finite = __builtin_isfinite(a00) && __builtin_isfinite(a01) && __builtin_isfinite(a02) && __builtin_isfinite(a11) &&
                      __builtin_isfinite(a12) && __builtin_isfinite(a22);
  const bool zero = a00 == 0. && a01 == 0. && a02 == 0. && a11 == 0. && a12 == 0. && a22 == 0.;
  n0 = 0.f; n1 = 0.f; n2 = 1.f; cv = finite ? 0.f : __uint_as_float(0x7FC00000u);
  if (finite && !zero) {
    double v00 = 1., v01 = 0., v02 = 0., v10 = 0., v11 = 1., v12 = 0., v20 = 0., v21 = 0., v22 = 1.;
    for (int sweep = 0; sweep < NM_SWEEPS; ++sweep) {
      if (a01 == 0. && a02 == 0. && a12 == 0.) break;
      nm_rotate(a00, a11, a01, a02, a12, v00, v01, v10, v11, v20, v21);       // (0, 1): the third row is 2
      nm_rotate(a00, a22, a02, a01, a12, v00, v02, v10, v12, v20, v22);       // (0, 2): the third row is 1
      nm_rotate(a11, a22, a12, a01, a02, v01, v02, v11, v12, v21, v22);       // (1, 2): the third row is 0
    }
    // the eigenvalues are the diagonal; the normal is the column of the smallest (the lowest index among equals)
    const int c = (a00 <= a11 && a00 <= a22) ? 0 : (a11 <= a22 ? 1 : 2);
    const double l0 = c == 0 ? a00 : c == 1 ? a11 : a22;
    const double o1 = c == 0 ? a11 : a00, o2 = c == 2 ? a11 : a22;            // the other two
    const double l1 = o1 <= o2 ? o1 : o2, l2 = o1 <= o2 ? o2 : o1;
    double e0 = c == 0 ? v00 : c == 1 ? v01 : v02;
    double e1 = c == 0 ? v10 : c == 1 ? v11 : v12;
    double e2 = c == 0 ? v20 : c == 1 ? v21 : v22;
    const double len = sqrt((e0 * e0 + e1 * e1) + e2 * e2);                  // 1 up to the rotations' rounding
    n0 = (float)(e0 / len); n1 = (float)(e1 / len); n2 = (float)(e2 / len);
    const double tr = (l0 + l1) + l2;
    cv = tr == 0. ? 0.f : (float)(l0 / tr);
    // the sign, on the fp32 normal: towards the viewpoint; without one, or at a right angle to it, the largest component up
    double dot = 0.;
    if (vp) {
      const double w0 = (double)vp[0] - (double)me[0], w1 = (double)vp[1] - (double)me[1], w2 = (double)vp[2] - (double)me[2];
      dot = ((double)n0 * w0 + (double)n1 * w1) + (double)n2 * w2;
    }
    bool flip = dot < 0.;
    if (!(dot < 0.) && !(dot > 0.)) {                      // zero (or no viewpoint, or a NaN viewpoint)
      const float m0 = fabsf(n0), m1 = fabsf(n1), m2 = fabsf(n2);
      const float big = (m0 >= m1 && m0 >= m2) ? n0 : (m1 >= m2 ? n1 : n2);
      flip = big < 0.f;
    }
    if (flip) { n0 = -n0; n1 = -n1; n2 = -n2; }
  }
}

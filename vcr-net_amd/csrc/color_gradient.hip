// A colour gradient per point from given neighbours (include/colored/vcr_hip_colored.h):
// vcr_color_gradient_f32, what the colored refinement reads at the target.
//
// One launch, one LANE per point, as normals.hip: the header fixes the nine fp64 sums over the row in idx's order, so one lane
// sums a point's row, and the 3 x 3 Cholesky behind them runs in that lane's registers: no LDS, no scratch.  A neighbour is one
// 16-B row load and one intensity; the idx entry is checked against [0, N) before it is used.
#include "common.h"
#include "../../include/colored/vcr_hip_colored.h"

namespace {

constexpr int CG_BLOCK = 256;
constexpr int CG_MAX_N = 131072;                           // vcr_normals_f32's limit
constexpr double CG_PIVOT = 1e-12;                         // vcr_refine_plane_f32's pivot rule

struct CgArgs {
  const float* xyz4; const int* idx; int N, k; long total; // total = B N
  const float* normals; const float* intensity; float radius;   // radius = 0: no cap
  float* gradient;
};

__global__ __launch_bounds__(CG_BLOCK) void color_gradient_kernel(CgArgs p) {
  const long g = (long)blockIdx.x * CG_BLOCK + threadIdx.x;
  if (g >= p.total) return;
  const int N = p.N, k = p.k;
  const long b = g / N;
  const int i = (int)(g - b * N);
  const float* rows = p.xyz4 + (size_t)b * N * 4;
  const float* inten = p.intensity + (size_t)b * N;
  const float* nrm = p.normals + (size_t)b * 3 * N + i;
  const int* nb = p.idx + (size_t)g * k;
  const f32x4 me = ld4(rows + (size_t)i * 4);
  const double n0 = (double)nrm[0], n1 = (double)nrm[N], n2 = (double)nrm[2 * (size_t)N];
  const double Ii = (double)inten[i];
  const bool capped = p.radius > 0.f;
  const float radius2 = p.radius * p.radius;
  double s00 = 0., s01 = 0., s02 = 0., s11 = 0., s12 = 0., s22 = 0., b0 = 0., b1 = 0., b2 = 0.;
  int m = 0;
#pragma unroll 2
  for (int j = 0; j < k; ++j) {
    const int r = nb[j];
    if ((unsigned)r >= (unsigned)N || r == i) continue;
    const f32x4 q = ld4(rows + (size_t)r * 4);
    const float f0 = q.x - me.x, f1 = q.y - me.y, f2 = q.z - me.z;
    if (capped && (f0 * f0 + f1 * f1) + f2 * f2 > radius2) continue;
    const double d0 = (double)f0, d1 = (double)f1, d2 = (double)f2;
    const double dn = (d0 * n0 + d1 * n1) + d2 * n2;
    const double a0 = d0 - dn * n0, a1 = d1 - dn * n1, a2 = d2 - dn * n2;
    const double di = (double)inten[r] - Ii;
    s00 += a0 * a0; s01 += a0 * a1; s02 += a0 * a2; s11 += a1 * a1; s12 += a1 * a2; s22 += a2 * a2;
    b0 += a0 * di; b1 += a1 * di; b2 += a2 * di;
    ++m;
  }
  bool ok = m >= 3;
  ok = ok && __builtin_isfinite(s00) && __builtin_isfinite(s01) && __builtin_isfinite(s02) && __builtin_isfinite(s11) &&
       __builtin_isfinite(s12) && __builtin_isfinite(s22) && __builtin_isfinite(b0) && __builtin_isfinite(b1) && __builtin_isfinite(b2);
  const double mm = (double)m * (double)m;
  const double M00 = s00 + mm * (n0 * n0), M01 = s01 + mm * (n0 * n1), M02 = s02 + mm * (n0 * n2);
  const double M11 = s11 + mm * (n1 * n1), M12 = s12 + mm * (n1 * n2), M22 = s22 + mm * (n2 * n2);
  // M = L L^T, the pivots held to the rule; L y = S_ab; L^T x = y
  const double p0 = M00;
  ok = ok && __builtin_isfinite(p0) && p0 > CG_PIVOT * M00;
  const double l00 = sqrt(p0), l10 = M01 / l00, l20 = M02 / l00;
  const double p1 = M11 - l10 * l10;
  ok = ok && __builtin_isfinite(p1) && p1 > CG_PIVOT * M11;
  const double l11 = sqrt(p1), l21 = (M12 - l20 * l10) / l11;
  const double p2 = (M22 - l20 * l20) - l21 * l21;
  ok = ok && __builtin_isfinite(p2) && p2 > CG_PIVOT * M22;
  const double l22 = sqrt(p2);
  const double y0 = b0 / l00, y1 = (b1 - l10 * y0) / l11, y2 = ((b2 - l20 * y0) - l21 * y1) / l22;
  const double x2 = y2 / l22, x1 = (y1 - l21 * x2) / l11, x0 = ((y0 - l10 * x1) - l20 * x2) / l00;
  float* out = p.gradient + (size_t)b * 3 * N + i;
  out[0] = ok ? (float)x0 : 0.f; out[N] = ok ? (float)x1 : 0.f; out[2 * (size_t)N] = ok ? (float)x2 : 0.f;
}

}  // namespace

extern "C" int vcr_color_gradient_f32(const vcr_color_gradient_args* ua, vcr_stream_t stream) {
  vcr_color_gradient_args a;
  if (vcr_take_args(ua, &a, sizeof(a))) return VCR_EINVAL;
  if (!a.xyz4 || !a.idx || !a.normals || !a.intensity || !a.gradient || a.B < 1 || a.N < 1 || a.k < 1 || (((uintptr_t)a.xyz4) & 15))
    return VCR_EINVAL;
  if (!(a.radius >= 0.f) || a.radius == __builtin_huge_valf()) return VCR_EINVAL;
  if (a.k > VCR_NORMALS_MAX_K || a.N > CG_MAX_N || (long)a.B * a.N >= (1L << 31)) return VCR_EUNSUPPORTED;
  const long total = (long)a.B * a.N;
  const CgArgs k{a.xyz4, a.idx, a.N, a.k, total, a.normals, a.intensity, a.radius, a.gradient};
  hipLaunchKernelGGL(color_gradient_kernel, dim3((unsigned)((total + CG_BLOCK - 1) / CG_BLOCK)), dim3(CG_BLOCK), 0, (hipStream_t)stream, k);
  return VCR_LAUNCH_RC();
}

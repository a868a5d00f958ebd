// Fast Point Feature Histograms from given neighbours and normals (include/vcr_hip_fpfh.h): the two gather
// passes of Open3D's compute_fpfh_feature, vcr_spfh_f32 and vcr_fpfh_f32.  One launch each, no workspace, no LDS, no atomics.
//
//   spfh_kernel   one LANE per point, like normals_kernel: a neighbour is one 16-B row load and three normal loads, the pair
//                 feature is fp64 VALU and one atan2.  33 counters indexed by a computed bin would live in scratch; a count is at
//                 most k <= 62, so the 11 bins of a group are 8-bit fields of two 64-bit words (six words for the three groups)
//                 and an increment is one shift and two conditional adds.  The row leaves as three 16-B stores.
//   fpfh_kernel   one lane per (point, group): 11 fp64 accumulators and the group's sum, a neighbour is its 16-B row and the
//                 16-B group of its histogram.  The header's order -- neighbours in idx's order, bins ascending -- is that
//                 lane's serial order, and nothing crosses lanes.  The lanes are numbered [b][group][i], so a wave holds 64
//                 consecutive points of one group and each of its 11 stores to [B,33,N] is one contiguous run.
// Both check an idx entry against [0, N) before they use it, like normals_kernel.
#include "common.h"
#include "../../include/vcr_hip_fpfh.h"

namespace {

typedef unsigned long long u64;

constexpr int FP_BLOCK = 256;
constexpr int FP_MAX_N = 131072;                           // the kNN entry points' limit (vcr_hip.h)
constexpr int FP_BINS = VCR_FPFH_BINS;
constexpr double FP_PI = 3.14159265358979323846;
constexpr double FP_INF = __builtin_huge_val();

struct SpArgs {
  const float* xyz4; const float* normals; const int* idx; int N, k; long total;   // total = B N
  double r2;                                               // +inf without a radius
  unsigned char* spfh;
};

struct FpArgs {
  const float* xyz4; const int* idx; const unsigned char* spfh; int N, k; long total;   // total = 3 B N
  double r2;
  float* fpfh;
};

__device__ __forceinline__ bool fp_finite(float v) { return fabsf(v) < __builtin_huge_valf(); }

// floor(t) clamped to [0, 10]; a NaN goes to 0
__device__ __forceinline__ int fp_bin(double t) {
  const double f = floor(t);
  return f >= 10.0 ? 10 : (f >= 0.0 ? (int)f : 0);
}

// one more in the 8-bit field `bin` of the group's two words (bins 0..7 | bins 8..10)
__device__ __forceinline__ void fp_count(u64& lo, u64& hi, int bin) {
  const u64 one = 1ull << ((bin & 7) << 3);
  lo += bin < 8 ? one : 0ull;
  hi += bin < 8 ? 0ull : one;
}

__global__ __launch_bounds__(FP_BLOCK) void spfh_kernel(SpArgs p) {
  const long g = (long)blockIdx.x * FP_BLOCK + threadIdx.x;
  if (g >= p.total) return;
  const int N = p.N, k = p.k;
  const long b = g / N;
  const int i = (int)(g - b * N);
  const float* rows = p.xyz4 + (size_t)b * N * 4;
  const float* nrm = p.normals + (size_t)b * 3 * N;
  const int* nb = p.idx + (size_t)g * k;
  const f32x4 me = ld4(rows + (size_t)i * 4);
  const float m0 = nrm[i], m1 = nrm[N + i], m2 = nrm[2 * (size_t)N + i];
  const bool me_ok = fp_finite(m0) && fp_finite(m1) && fp_finite(m2);
  const double r2 = p.r2;
  u64 a_lo = 0, a_hi = 0, b_lo = 0, b_hi = 0, c_lo = 0, c_hi = 0;      // the groups of f0, f1, f2
  unsigned c = 0;
  for (int j = 0; j < k; ++j) {
    int r = nb[j];
    r = (unsigned)r < (unsigned)N ? r : i;                 // an entry outside [0, N) reads as the row itself
    const f32x4 q = ld4(rows + (size_t)r * 4);
    const float o0 = nrm[r], o1 = nrm[N + r], o2 = nrm[2 * (size_t)N + r];
    double dx = (double)(q[0] - me[0]), dy = (double)(q[1] - me[1]), dz = (double)(q[2] - me[2]);
    const double d2 = (dx * dx + dy * dy) + dz * dz;
    if (!(me_ok && fp_finite(o0) && fp_finite(o1) && fp_finite(o2) && d2 < FP_INF && d2 <= r2)) continue;   // not counted
    double n1x = (double)m0, n1y = (double)m1, n1z = (double)m2, n2x = (double)o0, n2y = (double)o1, n2z = (double)o2;
    const double L = sqrt(d2);
    const double a1 = ((n1x * dx + n1y * dy) + n1z * dz) / L, a2 = ((n2x * dx + n2y * dy) + n2z * dz) / L;
    double f2 = a1;
    if (fabs(a1) < fabs(a2)) {                             // the smaller angle's normal leads
      double t;
      t = n1x; n1x = n2x; n2x = t;
      t = n1y; n1y = n2y; n2y = t;
      t = n1z; n1z = n2z; n2z = t;
      dx = -dx; dy = -dy; dz = -dz;
      f2 = -a2;
    }
    double vx = dy * n1z - dz * n1y, vy = dz * n1x - dx * n1z, vz = dx * n1y - dy * n1x;
    const double vn = sqrt((vx * vx + vy * vy) + vz * vz);
    const bool zero = L == 0.0 || vn == 0.0;
    vx = vx / vn; vy = vy / vn; vz = vz / vn;
    const double wx = n1y * vz - n1z * vy, wy = n1z * vx - n1x * vz, wz = n1x * vy - n1y * vx;
    double f1 = (vx * n2x + vy * n2y) + vz * n2z;
    double f0 = atan2((wx * n2x + wy * n2y) + wz * n2z, (n1x * n2x + n1y * n2y) + n1z * n2z);
    if (zero) { f0 = 0.0; f1 = 0.0; f2 = 0.0; }
    fp_count(a_lo, a_hi, fp_bin((11.0 * (f0 + FP_PI)) / (2.0 * FP_PI)));
    fp_count(b_lo, b_hi, fp_bin((11.0 * (f1 + 1.0)) * 0.5));
    fp_count(c_lo, c_hi, fp_bin((11.0 * (f2 + 1.0)) * 0.5));
    ++c;
  }
  uint4* out = reinterpret_cast<uint4*>(p.spfh + (size_t)g * VCR_SPFH_ROW_BYTES);
  const unsigned top = c << 24;                            // byte 11 of a group: the counted pairs
  out[0] = make_uint4((unsigned)a_lo, (unsigned)(a_lo >> 32), (unsigned)a_hi | top, 0u);
  out[1] = make_uint4((unsigned)b_lo, (unsigned)(b_lo >> 32), (unsigned)b_hi | top, 0u);
  out[2] = make_uint4((unsigned)c_lo, (unsigned)(c_lo >> 32), (unsigned)c_hi | top, 0u);
}

// byte `bin` of a group's 16
__device__ __forceinline__ unsigned fp_byte(const uint4& h, int bin) {
  const unsigned w = bin < 4 ? h.x : (bin < 8 ? h.y : h.z);
  return (w >> ((bin & 3) << 3)) & 0xFFu;
}

__global__ __launch_bounds__(FP_BLOCK) void fpfh_kernel(FpArgs p) {
  const long t = (long)blockIdx.x * FP_BLOCK + threadIdx.x;
  if (t >= p.total) return;
  const int N = p.N, k = p.k;
  const long bg = t / N;                                   // (cloud, group)
  const int i = (int)(t - bg * N);
  const long b = bg / 3;
  const int grp = (int)(bg - b * 3);
  const float* rows = p.xyz4 + (size_t)b * N * 4;
  const unsigned char* sp = p.spfh + (size_t)b * N * VCR_SPFH_ROW_BYTES + grp * 16;
  const int* nb = p.idx + ((size_t)b * N + i) * k;
  const f32x4 me = ld4(rows + (size_t)i * 4);
  const uint4 own = *reinterpret_cast<const uint4*>(sp + (size_t)i * VCR_SPFH_ROW_BYTES);
  const double r2 = p.r2;
  double acc[FP_BINS];
#pragma unroll
  for (int h = 0; h < FP_BINS; ++h) acc[h] = 0.0;
  double sum = 0.0;
  for (int j = 0; j < k; ++j) {
    int r = nb[j];
    r = (unsigned)r < (unsigned)N ? r : i;                 // an entry outside [0, N) reads as the row itself: d2 = 0, skipped
    const f32x4 q = ld4(rows + (size_t)r * 4);
    const uint4 hj = *reinterpret_cast<const uint4*>(sp + (size_t)r * VCR_SPFH_ROW_BYTES);
    const double dx = (double)(q[0] - me[0]), dy = (double)(q[1] - me[1]), dz = (double)(q[2] - me[2]);
    const double d2 = (dx * dx + dy * dy) + dz * dz;
    const unsigned cj = hj.z >> 24;
    if (!(d2 > 0.0 && d2 < FP_INF && d2 <= r2) || cj == 0u) continue;
    const double s = 100.0 / (double)cj;
#pragma unroll
    for (int h = 0; h < FP_BINS; ++h) {
      const double val = ((double)fp_byte(hj, h) * s) / d2;
      acc[h] += val;
      sum += val;
    }
  }
  const double scale = 100.0 / sum;
  const unsigned ci = own.z >> 24;
  const double so = 100.0 / (double)ci;
  float* out = p.fpfh + ((size_t)b * 33 + (size_t)grp * FP_BINS) * N + i;
#pragma unroll
  for (int h = 0; h < FP_BINS; ++h) {
    const double a = sum != 0.0 ? acc[h] * scale : acc[h];
    const double mine = ci != 0u ? (double)fp_byte(own, h) * so : 0.0;
    out[(size_t)h * N] = (float)(a + mine);
  }
}

// What both entry points ask of (xyz4, idx, spfh, B, N, k, radius); the last output goes by its own name
int fp_check(const void* xyz4, const void* idx, const void* spfh, const void* other, int B, int N, int k, float radius) {
  if (!xyz4 || !idx || !spfh || !other || B < 1 || N < 1 || k < 1) return VCR_EINVAL;
  if ((((uintptr_t)xyz4) & 15) || (((uintptr_t)spfh) & 15)) return VCR_EINVAL;
  if (!(radius >= 0.f) || radius == __builtin_huge_valf()) return VCR_EINVAL;                 // negative, NaN, +inf
  if (k > VCR_FPFH_MAX_K || N > FP_MAX_N || (long)B * N >= (1L << 31)) return VCR_EUNSUPPORTED;
  return VCR_OK;
}

double fp_r2(float radius) {
  const float r2 = radius * radius;                        // fp32: one rounding
  return radius == 0.f ? FP_INF : (double)r2;
}

}  // namespace

extern "C" int vcr_spfh_f32(const vcr_spfh_args* ua, vcr_stream_t stream) {
  vcr_spfh_args a;
  if (vcr_take_args(ua, &a, sizeof(vcr_spfh_args))) return VCR_EINVAL;
  const int e = fp_check(a.xyz4, a.idx, a.spfh, a.normals, a.B, a.N, a.k, a.radius);
  if (e) return e;
  const long total = (long)a.B * a.N;
  const SpArgs k{a.xyz4, a.normals, a.idx, a.N, a.k, total, fp_r2(a.radius), a.spfh};
  hipLaunchKernelGGL(spfh_kernel, dim3((unsigned)((total + FP_BLOCK - 1) / FP_BLOCK)), dim3(FP_BLOCK), 0, (hipStream_t)stream, k);
  return VCR_LAUNCH_RC();
}

extern "C" int vcr_fpfh_f32(const vcr_fpfh_args* ua, vcr_stream_t stream) {
  vcr_fpfh_args a;
  if (vcr_take_args(ua, &a, sizeof(vcr_fpfh_args))) return VCR_EINVAL;
  const int e = fp_check(a.xyz4, a.idx, a.spfh, a.fpfh, a.B, a.N, a.k, a.radius);
  if (e) return e;
  const long total = 3L * a.B * a.N;                       // < 3 * 2^31 lanes: at most 25 165 824 workgroups
  const FpArgs k{a.xyz4, a.idx, a.spfh, a.N, a.k, total, fp_r2(a.radius), a.fpfh};
  hipLaunchKernelGGL(fpfh_kernel, dim3((unsigned)((total + FP_BLOCK - 1) / FP_BLOCK)), dim3(FP_BLOCK), 0, (hipStream_t)stream, k);
  return VCR_LAUNCH_RC();
}

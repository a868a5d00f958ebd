// What the consumers of ragged rows share (DESIGN sections 4.23, 4.29), written once for rows.hip (row i belongs to point i of the
// same cloud) and support.hip (row i belongs to centre i, its entries index a support cloud): how a row is read, the pair of the
// simplified histogram and its bins, and the check behind every pass that voids a cloud that is not served.
//   rw_row            a row's first entry and length where 0 <= row_start[i] <= row_start[i+1] <= total <= capacity, nothing else
//   rw_pair, rw_bin   vcr_spfh_f32's pair (i, j) without a radius, in fp64, and floor() clamped to the eleven bins
//   rows_void_kernel  a thread per (row_start[i], row_start[i+1]) pair; a workgroup that finds the cloud not served fills ALL of
//                     that cloud's outputs (NaN, or zero words).  Several may; they write the same values.  It runs behind the
//                     pass because a pass cannot know of another row's fault.
#pragma once
#include "common.h"
#include "../../include/ext/vcr_hip_rows.h"

namespace {

typedef long long i64;

constexpr int RW_BLOCK = 256;
constexpr int RW_WAVES = RW_BLOCK / 64;                    // rows a workgroup of a wave form serves
constexpr int RW_BINS = 11;
constexpr int RW_WORDS = VCR_ROWS_SPFH_WORDS;              // 3 x (11 + 1)
constexpr double RW_PI = 3.14159265358979323846;
constexpr double RW_INF = __builtin_huge_val();

// N: the number of ROWS (row_start is [B,N+1]); what an entry may index is the caller's to check
struct RwRows { const int* idx; const i64* row_start; const i64* total; int N, capacity, max_nn; };

// per cloud: n0 floats of f0 and n1 of f1 become NaN, nz words of z zero (a NULL pointer: nothing)
struct RwVoid { const i64* row_start; const i64* total; int N, capacity; long nblk; float* f0; long n0; float* f1; long n1; unsigned* z; long nz; };

__device__ __forceinline__ float rw_nan() { return __uint_as_float(0x7FC00000u); }
__device__ __forceinline__ bool rw_finite(float v) { return fabsf(v) < __builtin_huge_valf(); }

// Row i of cloud b: its first entry and L_i.  false (and L = 0) where the row cannot be read: the cloud is then not served.
__device__ __forceinline__ bool rw_row(const RwRows& r, long b, int i, const int*& nb, int& L) {
  const i64 tot = r.total[b];
  const i64* rs = r.row_start + (size_t)b * ((size_t)r.N + 1) + i;
  const i64 s = rs[0], e = rs[1];
  const bool ok = tot >= 0 && tot <= (i64)r.capacity && s >= 0 && s <= e && e <= tot;
  const i64 n = e - s;                                     // <= capacity: an int
  L = ok ? (int)(r.max_nn > 0 && n > (i64)r.max_nn ? (i64)r.max_nn : n) : 0;
  nb = r.idx + (size_t)b * r.capacity + (ok ? s : 0);
  return ok;
}

// floor(t) clamped to [0, 10]; a NaN goes to 0
__device__ __forceinline__ int rw_bin(double t) {
  const double f = floor(t);
  return f >= 10.0 ? 10 : (f >= 0.0 ? (int)f : 0);
}

// vcr_spfh_f32's pair (i, j) without a radius: false where it is not counted, otherwise the three bins.  me / q the two rows,
// (m0, m1, m2) / (o0, o1, o2) the two fp32 normals, me_ok: n_i is finite.
__device__ __forceinline__ bool rw_pair(const f32x4& me, float m0, float m1, float m2, bool me_ok, const f32x4& q, float o0, float o1,
                                        float o2, int& b0, int& b1, int& b2) {
  double dx = (double)(q[0] - me[0]), dy = (double)(q[1] - me[1]), dz = (double)(q[2] - me[2]);
  const double d2 = (dx * dx + dy * dy) + dz * dz;
  if (!(me_ok && rw_finite(o0) && rw_finite(o1) && rw_finite(o2) && d2 < RW_INF)) return false;
  double n1x = (double)m0, n1y = (double)m1, n1z = (double)m2, n2x = (double)o0, n2y = (double)o1, n2z = (double)o2;
  const double L = sqrt(d2);
  const double a1 = ((n1x * dx + n1y * dy) + n1z * dz) / L, a2 = ((n2x * dx + n2y * dy) + n2z * dz) / L;
  double f2 = a1;
  if (fabs(a1) < fabs(a2)) {                               // the smaller angle's normal leads
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
  b0 = rw_bin((11.0 * (f0 + RW_PI)) / (2.0 * RW_PI));
  b1 = rw_bin((11.0 * (f1 + 1.0)) * 0.5);
  b2 = rw_bin((11.0 * (f2 + 1.0)) * 0.5);
  return true;
}

__global__ __launch_bounds__(RW_BLOCK) void rows_void_kernel(RwVoid p) {
  const long b = (long)blockIdx.x / p.nblk;
  const long i = ((long)blockIdx.x - b * p.nblk) * RW_BLOCK + threadIdx.x;      // the pair (i, i + 1)
  const int N = p.N;
  bool bad = false;
  if (i < N) {
    const i64* rs = p.row_start + (size_t)b * ((size_t)N + 1) + i;
    const i64 s = rs[0], e = rs[1], tot = p.total[b];
    bad = s > e || (i == 0 && (s != 0 || tot < 0 || tot > (i64)p.capacity)) || (i == N - 1 && e != tot);
  }
  if (!__syncthreads_or(bad)) return;
  // not served: all of the cloud's outputs, by this workgroup (and by any other that found a fault: the same values)
  const float nan = rw_nan();
  if (p.f0) for (long j = threadIdx.x; j < p.n0; j += RW_BLOCK) p.f0[(size_t)b * p.n0 + j] = nan;
  if (p.f1) for (long j = threadIdx.x; j < p.n1; j += RW_BLOCK) p.f1[(size_t)b * p.n1 + j] = nan;
  if (p.z) for (long j = threadIdx.x; j < p.nz; j += RW_BLOCK) p.z[(size_t)b * p.nz + j] = 0u;
}

unsigned rw_blocks(long items, int per_block) { return (unsigned)((items + per_block - 1) / per_block); }

int rw_void(const RwRows& r, int B, float* f0, long n0, float* f1, long n1, unsigned* z, long nz, hipStream_t s) {
  const long nblk = ((long)r.N + RW_BLOCK - 1) / RW_BLOCK;
  const RwVoid v{r.row_start, r.total, r.N, r.capacity, nblk, f0, n0, f1, n1, z, nz};
  hipLaunchKernelGGL(rows_void_kernel, dim3((unsigned)(nblk * B)), dim3(RW_BLOCK), 0, s, v);
  return VCR_LAUNCH_RC();
}

}  // namespace

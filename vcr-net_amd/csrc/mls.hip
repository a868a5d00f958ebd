// Moving least squares over ragged rows (include/smooth/vcr_hip_mls.h): vcr_mls_weights_f32 and
// vcr_mls_fit_f32.  No atomics, no workspace, no allocation, no LDS in the two passes.
//
//   mls_weights_kernel   one WAVE per row, lane p the header's chain p.  Every lane builds the row's frame (the same arithmetic on
//                        the same values); the lanes read 64 consecutive idx entries a step, each gathers its neighbour's 16-byte
//                        row and adds the three differences to its own sums; six exchanges with lane p ^ s give every lane the
//                        mean, hence the origin; a second pass over the row writes 64 consecutive weights a step (the one exp)
//   mls_fit_kernel<T>    one WAVE per row: 27 fp64 sums a lane (a statically indexed array: registers), the combine, the point's
//                        own term, then the 6 x 6 Cholesky fully unrolled, alike in every lane; lane 0 stores.
//                        T = false: every sum goes through the six exchanges (162 of a double).  T = true: the transposing
//                        combine -- at step s a lane keeps the half of its sums its bit s names and hands the other half to lane
//                        p ^ s, 16 + 8 + 4 + 2 + 1 exchanges, one more for the last step, and lane 2k ends with sum k, which 27
//                        broadcasts hand round.  v[p] + v[p ^ s] and v[p ^ s] + v[p] are the same IEEE sum and after step s the
//                        lanes p and p ^ s agree, so the tree is the header's and the bits are the plain form's
//   mls_void_kernel      behind either pass: a thread per (row_start[i], row_start[i+1]) pair; a workgroup that finds the cloud not
//                        served fills ALL of that cloud's outputs.  Several may; they write the same values.  Behind the weights
//                        it also writes NaN to the slots behind total[b], which no row owns
// A pass reads a row only where 0 <= row_start[i] <= row_start[i+1] <= total <= capacity, so no idx or weight slot outside the
// cloud's capacity is touched whatever row_start holds; an idx entry is checked against [0, N) before it is used.
#include "common.h"
#include "../../include/smooth/vcr_hip_mls.h"

namespace {

typedef long long i64;

constexpr int ML_BLOCK = 256;
constexpr int ML_WAVES = ML_BLOCK / 64;                    // rows a workgroup serves
constexpr int ML_SUMS = 27;                                // 21 of A (a <= b, row by row) and 6 of r
// The combine variant 0 takes: the transposing one was x1.3 to x1.4 faster in all twelve measured cases, beyond the blocks'
// spread in each (profiles/mls_bench.txt)
constexpr int ML_PLAN = VCR_MLS_TRANSPOSE;

struct MlRows { const int* idx; const i64* row_start; const i64* total; int N, capacity; };

struct MlWts { MlRows r; const float* xyz4; const float* normals; long total; double h2; double* weight; double* origin;
               double* w_self; int* frame; };
struct MlFit { MlRows r; const float* xyz4; const float* normals; const double* weight; const double* origin; const double* w_self;
               const int* frame; long total; int order, min_neighbors; float* points; int* fit; float* normals_out; double* coeffs; };
// per cloud: nd[k] doubles of d[k] and nf floats of f[k] become NaN, nk ints of k VCR_MLS_NOT_SERVED (a NULL pointer: nothing);
// pad: the capacity's slots behind total become NaN in a served cloud
struct MlVoid { const i64* row_start; const i64* total; int N, capacity; long nblk; double* d0; long n0; double* d1; long n1;
                double* d2; long n2; float* f0; float* f1; long nf; int* k; long nk; double* pad; };

__device__ __forceinline__ double ml_nan() { return __longlong_as_double(0x7FF8000000000000LL); }
__device__ __forceinline__ bool ml_finite(double v) { return __builtin_fabs(v) < __builtin_huge_val(); }      // false for a NaN
__device__ __forceinline__ double ml_xor(double v, int s) { return __shfl_xor(v, s, 64); }

// Row i of cloud b: its first slot in the cloud's capacity and n_i.  false (and n = 0) where the row cannot be read.
__device__ __forceinline__ bool ml_row(const MlRows& r, long b, int i, i64& first, int& n) {
  const i64 tot = r.total[b];
  const i64* rs = r.row_start + (size_t)b * ((size_t)r.N + 1) + i;
  const i64 s = rs[0], e = rs[1];
  const bool ok = tot >= 0 && tot <= (i64)r.capacity && s >= 0 && s <= e && e <= tot;
  n = ok ? (int)(e - s) : 0;                               // <= capacity: an int
  first = ok ? s : 0;
  return ok;
}

// The header's FRAME: nh, uh and v (NaN where there is none)
struct MlFrame { double h0, h1, h2, u0, u1, u2, v0, v1, v2; bool ok; };

__device__ __forceinline__ MlFrame ml_frame(const f32x4& me, const float* nr, int N) {
  MlFrame f;
  const double n0 = (double)nr[0], n1 = (double)nr[N], n2 = (double)nr[2 * (size_t)N];
  const double s = (n0 * n0 + n1 * n1) + n2 * n2;
  f.ok = ml_finite((double)me.x) && ml_finite((double)me.y) && ml_finite((double)me.z) && ml_finite(n0) && ml_finite(n1) &&
         ml_finite(n2) && s > 0. && ml_finite(s);
  const double inv = 1.0 / sqrt(s);
  f.h0 = n0 * inv; f.h1 = n1 * inv; f.h2 = n2 * inv;
  const double a0 = __builtin_fabs(f.h0), a1 = __builtin_fabs(f.h1), a2 = __builtin_fabs(f.h2);
  int ax = 0;                                              // the smallest |nh_a|, the lowest index among equals
  double am = a0;
  if (a1 < am) { ax = 1; am = a1; }
  if (a2 < am) ax = 2;
  const double e0 = ax == 0 ? 1.0 : 0.0, e1 = ax == 1 ? 1.0 : 0.0, e2 = ax == 2 ? 1.0 : 0.0;
  const double u0 = f.h1 * e2 - f.h2 * e1, u1 = f.h2 * e0 - f.h0 * e2, u2 = f.h0 * e1 - f.h1 * e0;
  const double iu = 1.0 / sqrt((u0 * u0 + u1 * u1) + u2 * u2);
  f.u0 = u0 * iu; f.u1 = u1 * iu; f.u2 = u2 * iu;
  f.v0 = f.h1 * f.u2 - f.h2 * f.u1; f.v1 = f.h2 * f.u0 - f.h0 * f.u2; f.v2 = f.h0 * f.u1 - f.h1 * f.u0;
  if (!f.ok) f.h0 = f.h1 = f.h2 = f.u0 = f.u1 = f.u2 = f.v0 = f.v1 = f.v2 = ml_nan();
  return f;
}

__global__ __launch_bounds__(ML_BLOCK) void mls_weights_kernel(MlWts p) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const long g = (long)blockIdx.x * ML_WAVES + w;          // the wave's row
  if (g >= p.total) return;                                // the whole wave leaves (no barrier below)
  const int N = p.r.N;
  const long b = g / N;
  const int i = (int)(g - b * N);
  const float* rows = p.xyz4 + (size_t)b * N * 4;
  i64 first;
  int L;
  const bool ok = ml_row(p.r, b, i, first, L);
  const f32x4 me = ld4(rows + (size_t)i * 4);
  const MlFrame f = ml_frame(me, p.normals + (size_t)b * 3 * N + i, N);
  const int* nb = p.r.idx + (size_t)b * p.r.capacity + first;
  double s0 = 0., s1 = 0., s2 = 0.;                        // chain `lane`: +0.0, then the entries lane, lane + 64, ...
  for (int e = lane; e < L; e += 64) {
    int r = nb[e];
    r = (unsigned)r < (unsigned)N ? r : i;                 // an entry outside [0, N) reads as the row itself
    const f32x4 q = ld4(rows + (size_t)r * 4);
    const double d0 = (double)(q.x - me.x), d1 = (double)(q.y - me.y), d2 = (double)(q.z - me.z);
    const bool fin = ml_finite(d0) && ml_finite(d1) && ml_finite(d2);
    s0 = s0 + (fin ? d0 : 0.); s1 = s1 + (fin ? d1 : 0.); s2 = s2 + (fin ? d2 : 0.);
  }
#pragma unroll
  for (int st = 32; st >= 1; st >>= 1) {                   // v[p] = v[p] + v[p ^ st]
    const double x = ml_xor(s0, st), y = ml_xor(s1, st), z = ml_xor(s2, st);
    s0 = s0 + x; s1 = s1 + y; s2 = s2 + z;
  }
  // the same in every lane from here on
  const double m = (double)(L + 1);
  const double mu0 = s0 / m, mu1 = s1 / m, mu2 = s2 / m;
  const double t = (mu0 * f.h0 + mu1 * f.h1) + mu2 * f.h2;
  const double o0 = t * f.h0, o1 = t * f.h1, o2 = t * f.h2;
  double* out = p.weight + (size_t)b * p.r.capacity + first;
  for (int e = lane; e < L; e += 64) {
    int r = nb[e];
    r = (unsigned)r < (unsigned)N ? r : i;
    const f32x4 q = ld4(rows + (size_t)r * 4);
    const double d0 = (double)(q.x - me.x), d1 = (double)(q.y - me.y), d2 = (double)(q.z - me.z);
    const bool fin = ml_finite(d0) && ml_finite(d1) && ml_finite(d2);
    const double q0 = d0 - o0, q1 = d1 - o1, q2 = d2 - o2;
    const double we = exp(-(((q0 * q0 + q1 * q1) + q2 * q2) / p.h2));
    out[e] = f.ok ? (fin ? we : 0.) : ml_nan();
  }
  if (lane == 0) {
    const double ws = exp(-(((o0 * o0 + o1 * o1) + o2 * o2) / p.h2));          // q = -o: the squares are o's
    double* og = p.origin + (size_t)g * 3;
    const bool has = ok && f.ok;
    og[0] = has ? o0 : ml_nan(); og[1] = has ? o1 : ml_nan(); og[2] = has ? o2 : ml_nan();
    p.w_self[g] = has ? ws : ml_nan();
    p.frame[g] = ok ? (f.ok ? 1 : 0) : VCR_MLS_NOT_SERVED;
  }
}

// The 27 terms of one entry added to the lane's sums: A row by row (a <= b), then r
__device__ __forceinline__ void ml_add(double (&acc)[32], double w, double uu, double vv, double f) {
  const double p[6] = {1.0, vv, vv * vv, uu, uu * vv, uu * uu};
  double wp[6];
#pragma unroll
  for (int a = 0; a < 6; ++a) wp[a] = w * p[a];
  int k = 0;
#pragma unroll
  for (int a = 0; a < 6; ++a)
#pragma unroll
    for (int c = a; c < 6; ++c) { acc[k] = acc[k] + wp[a] * p[c]; ++k; }
#pragma unroll
  for (int a = 0; a < 6; ++a) acc[21 + a] = acc[21 + a] + wp[a] * f;
}

// Where A_ab (a <= b) sits among the sums
__device__ __forceinline__ constexpr int ml_at(int a, int b) { return a * 6 - a * (a - 1) / 2 + (b - a); }

template <bool TRANSPOSE>
__global__ __launch_bounds__(ML_BLOCK) void mls_fit_kernel(MlFit p) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const long g = (long)blockIdx.x * ML_WAVES + w;          // the wave's row
  if (g >= p.total) return;                                // the whole wave leaves (no barrier below)
  const int N = p.r.N;
  const long b = g / N;
  const int i = (int)(g - b * N);
  const float* rows = p.xyz4 + (size_t)b * N * 4;
  i64 first;
  int L;
  const bool ok = ml_row(p.r, b, i, first, L);
  const f32x4 me = ld4(rows + (size_t)i * 4);
  const MlFrame f = ml_frame(me, p.normals + (size_t)b * 3 * N + i, N);
  const bool fitted = f.ok && p.frame[g] != 0 && L + 1 >= p.min_neighbors;
  const bool quad = fitted && p.order == 2 && L + 1 >= VCR_MLS_TERMS;          // (wave-uniform, like everything that bounds a loop)
  const double* og = p.origin + (size_t)g * 3;
  const double o0 = og[0], o1 = og[1], o2 = og[2];
  double c[6] = {0., 0., 0., 0., 0., 0.};
  int fit = fitted ? 1 : 0;
  if (quad) {
    const int* nb = p.r.idx + (size_t)b * p.r.capacity + first;
    const double* wt = p.weight + (size_t)b * p.r.capacity + first;
    double acc[32];                                        // (every index below is a constant once unrolled: registers)
#pragma unroll
    for (int k = 0; k < 32; ++k) acc[k] = 0.;
    for (int e = lane; e < L; e += 64) {
      int r = nb[e];
      r = (unsigned)r < (unsigned)N ? r : i;               // an entry outside [0, N) reads as the row itself
      const f32x4 x = ld4(rows + (size_t)r * 4);
      const double d0 = (double)(x.x - me.x), d1 = (double)(x.y - me.y), d2 = (double)(x.z - me.z);
      const bool fin = ml_finite(d0) && ml_finite(d1) && ml_finite(d2);
      const double q0 = d0 - o0, q1 = d1 - o1, q2 = d2 - o2;
      const double uu = (q0 * f.u0 + q1 * f.u1) + q2 * f.u2, vv = (q0 * f.v0 + q1 * f.v1) + q2 * f.v2;
      const double ff = (q0 * f.h0 + q1 * f.h1) + q2 * f.h2;
      // a skipped entry adds +0.0 to every sum: w = +0.0 on the terms of (1, 0, 0, 0, 0, 0) and f = 0
      ml_add(acc, fin ? wt[e] : 0., fin ? uu : 0., fin ? vv : 0., fin ? ff : 0.);
    }
    if (TRANSPOSE) {
#pragma unroll
      for (int h = 16; h >= 1; h >>= 1) {                  // the step s = 2h: slot k keeps k or k + h, as the lane's bit s says
        const bool up = (lane & (2 * h)) != 0;
#pragma unroll
        for (int k = 0; k < h; ++k) {
          const double keep = up ? acc[k + h] : acc[k], send = up ? acc[k] : acc[k + h];
          acc[k] = keep + ml_xor(send, 2 * h);
        }
      }
      acc[0] = acc[0] + ml_xor(acc[0], 1);                 // lane p now holds sum p >> 1, combined over all 64 chains
      const double mine = acc[0];
#pragma unroll
      for (int k = 0; k < ML_SUMS; ++k) acc[k] = __shfl(mine, 2 * k, 64);
    } else {
#pragma unroll
      for (int st = 32; st >= 1; st >>= 1)
#pragma unroll
        for (int k = 0; k < ML_SUMS; ++k) acc[k] = acc[k] + ml_xor(acc[k], st);
    }
    // the same in every lane from here on: the point's own term, by one addition a sum, last
    {
      const double q0 = -o0, q1 = -o1, q2 = -o2;
      const double uu = (q0 * f.u0 + q1 * f.u1) + q2 * f.u2, vv = (q0 * f.v0 + q1 * f.v1) + q2 * f.v2;
      const double ff = (q0 * f.h0 + q1 * f.h1) + q2 * f.h2;
      ml_add(acc, p.w_self[g], uu, vv, ff);
    }
    // A = L L^T in the textbook column order
    double Lm[6][6];
    bool failed = false;
    const double tiny = 0x1p-40;
#pragma unroll
    for (int k = 0; k < 6; ++k) {
      const double akk = acc[ml_at(k, k)];
      double t = akk;
#pragma unroll
      for (int j = 0; j < k; ++j) t = t - Lm[k][j] * Lm[k][j];
      failed = failed || !(ml_finite(t) && t > akk * tiny);
      Lm[k][k] = sqrt(t);
#pragma unroll
      for (int r = k + 1; r < 6; ++r) {
        double s = acc[ml_at(k, r)];
#pragma unroll
        for (int j = 0; j < k; ++j) s = s - Lm[r][j] * Lm[k][j];
        Lm[r][k] = s / Lm[k][k];
      }
    }
    double y[6], x[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) {
      double t = acc[21 + k];
#pragma unroll
      for (int j = 0; j < k; ++j) t = t - Lm[k][j] * y[j];
      y[k] = t / Lm[k][k];
    }
#pragma unroll
    for (int k = 5; k >= 0; --k) {
      double t = y[k];
#pragma unroll
      for (int j = k + 1; j < 6; ++j) t = t - Lm[j][k] * x[j];
      x[k] = t / Lm[k][k];
    }
    if (!failed) {
      fit = 2;
#pragma unroll
      for (int k = 0; k < 6; ++k) c[k] = x[k];
    }
  }
  if (lane != 0) return;
  const double nan = ml_nan();
  float x0 = me.x, x1 = me.y, x2 = me.z;                   // fit 0: the input's bits
  double g0 = f.h0, g1 = f.h1, g2 = f.h2;                  // ... and nh rounded (NaN where there is no frame)
  if (fitted) {
    x0 = (float)((double)me.x + (o0 + c[0] * f.h0));
    x1 = (float)((double)me.y + (o1 + c[0] * f.h1));
    x2 = (float)((double)me.z + (o2 + c[0] * f.h2));
    g0 = (f.h0 - c[3] * f.u0) - c[1] * f.v0;
    g1 = (f.h1 - c[3] * f.u1) - c[1] * f.v1;
    g2 = (f.h2 - c[3] * f.u2) - c[1] * f.v2;
    const double ig = 1.0 / sqrt((g0 * g0 + g1 * g1) + g2 * g2);
    g0 = g0 * ig; g1 = g1 * ig; g2 = g2 * ig;
  }
  float* pt = p.points + (size_t)b * 3 * N + i;
  pt[0] = ok ? x0 : (float)nan; pt[N] = ok ? x1 : (float)nan; pt[2 * (size_t)N] = ok ? x2 : (float)nan;
  p.fit[g] = ok ? fit : VCR_MLS_NOT_SERVED;
  if (p.normals_out) {
    float* no = p.normals_out + (size_t)b * 3 * N + i;
    no[0] = ok ? (float)g0 : (float)nan; no[N] = ok ? (float)g1 : (float)nan; no[2 * (size_t)N] = ok ? (float)g2 : (float)nan;
  }
  if (p.coeffs) {
    double* co = p.coeffs + (size_t)g * 6;
#pragma unroll
    for (int k = 0; k < 6; ++k) co[k] = ok ? c[k] : nan;
  }
}

__global__ __launch_bounds__(ML_BLOCK) void mls_void_kernel(MlVoid p) {
  const long b = (long)blockIdx.x / p.nblk;
  const long blk = (long)blockIdx.x - b * p.nblk;
  const long i = blk * ML_BLOCK + threadIdx.x;             // the pair (i, i + 1)
  const int N = p.N;
  const i64 tot = p.total[b];
  bool bad = false;
  if (i < N) {
    const i64* rs = p.row_start + (size_t)b * ((size_t)N + 1) + i;
    const i64 s = rs[0], e = rs[1];
    bad = s > e || (i == 0 && (s != 0 || tot < 0 || tot > (i64)p.capacity)) || (i == N - 1 && e != tot);
  }
  const double nan = ml_nan();
  if (!__syncthreads_or(bad)) {
    // served as far as this workgroup sees: its share of the slots no row owns (a cloud another workgroup voids gets NaN there too)
    if (p.pad && tot >= 0 && tot <= (i64)p.capacity)
      for (i64 j = tot + i; j < (i64)p.capacity; j += p.nblk * ML_BLOCK) p.pad[(size_t)b * p.capacity + j] = nan;
    return;
  }
  // voided: all of the cloud's outputs, by this workgroup (and by any other that found a fault: the same values)
  if (p.d0) for (long j = threadIdx.x; j < p.n0; j += ML_BLOCK) p.d0[(size_t)b * p.n0 + j] = nan;
  if (p.d1) for (long j = threadIdx.x; j < p.n1; j += ML_BLOCK) p.d1[(size_t)b * p.n1 + j] = nan;
  if (p.d2) for (long j = threadIdx.x; j < p.n2; j += ML_BLOCK) p.d2[(size_t)b * p.n2 + j] = nan;
  if (p.f0) for (long j = threadIdx.x; j < p.nf; j += ML_BLOCK) p.f0[(size_t)b * p.nf + j] = (float)nan;
  if (p.f1) for (long j = threadIdx.x; j < p.nf; j += ML_BLOCK) p.f1[(size_t)b * p.nf + j] = (float)nan;
  if (p.k) for (long j = threadIdx.x; j < p.nk; j += ML_BLOCK) p.k[(size_t)b * p.nk + j] = VCR_MLS_NOT_SERVED;
}

// What both stages ask of the numbers
int ml_numbers(int B, int N, int capacity) {
  if (B < 1 || capacity < 0) return VCR_EINVAL;
  if (N < 1 || N > VCR_MLS_MAX_N || (long)B * N >= (1L << 31) || (long)B * capacity >= (1L << 31)) return VCR_EUNSUPPORTED;
  return VCR_OK;
}

unsigned ml_blocks(long items, int per_block) { return (unsigned)((items + per_block - 1) / per_block); }

int ml_void(const MlRows& r, int B, const MlVoid& lists, hipStream_t s) {
  MlVoid v = lists;
  v.row_start = r.row_start; v.total = r.total; v.N = r.N; v.capacity = r.capacity;
  v.nblk = ((long)r.N + ML_BLOCK - 1) / ML_BLOCK;
  hipLaunchKernelGGL(mls_void_kernel, dim3((unsigned)(v.nblk * B)), dim3(ML_BLOCK), 0, s, v);
  return VCR_LAUNCH_RC();
}

}  // namespace

extern "C" int vcr_mls_weights_f32(const vcr_mls_weights_args* ua, vcr_stream_t stream) {
  vcr_mls_weights_args a;
  if (vcr_take_args(ua, &a, sizeof(vcr_mls_weights_args))) return VCR_EINVAL;
  if (!a.xyz4 || !a.normals || !a.row_start || !a.total || !a.origin || !a.w_self || !a.frame) return VCR_EINVAL;
  if ((!a.idx || !a.weight) && a.capacity != 0) return VCR_EINVAL;
  if ((((uintptr_t)a.xyz4) & 15) || !(a.sqr_gauss_param > 0. && a.sqr_gauss_param < __builtin_huge_val())) return VCR_EINVAL;
  const int e = ml_numbers(a.B, a.N, a.capacity);
  if (e) return e;
  const long total = (long)a.B * a.N;
  const MlRows r{a.idx, (const i64*)a.row_start, (const i64*)a.total, a.N, a.capacity};
  const MlWts k{r, a.xyz4, a.normals, total, a.sqr_gauss_param, a.weight, a.origin, a.w_self, a.frame};
  hipLaunchKernelGGL(mls_weights_kernel, dim3(ml_blocks(total, ML_WAVES)), dim3(ML_BLOCK), 0, (hipStream_t)stream, k);
  const int rc = VCR_LAUNCH_RC();
  if (rc) return rc;
  MlVoid v{};
  v.d0 = a.weight; v.n0 = a.capacity; v.d1 = a.origin; v.n1 = 3L * a.N; v.d2 = a.w_self; v.n2 = a.N;
  v.k = a.frame; v.nk = a.N; v.pad = a.weight;
  return ml_void(r, a.B, v, (hipStream_t)stream);
}

extern "C" int vcr_mls_fit_f32(const vcr_mls_fit_args* ua, vcr_stream_t stream) {
  vcr_mls_fit_args a;
  if (vcr_take_args(ua, &a, offsetof(vcr_mls_fit_args, normals_out))) return VCR_EINVAL;
  if (!a.xyz4 || !a.normals || !a.row_start || !a.total || !a.origin || !a.w_self || !a.frame || !a.points || !a.fit) return VCR_EINVAL;
  if ((!a.idx || !a.weight) && a.capacity != 0) return VCR_EINVAL;
  if ((((uintptr_t)a.xyz4) & 15) || (a.order != 1 && a.order != 2) || a.min_neighbors < 1) return VCR_EINVAL;
  if (a.variant != 0 && a.variant != VCR_MLS_PLAIN && a.variant != VCR_MLS_TRANSPOSE) return VCR_EINVAL;
  const int e = ml_numbers(a.B, a.N, a.capacity);
  if (e) return e;
  const long total = (long)a.B * a.N;
  const MlRows r{a.idx, (const i64*)a.row_start, (const i64*)a.total, a.N, a.capacity};
  const MlFit k{r, a.xyz4, a.normals, a.weight, a.origin, a.w_self, a.frame, total, a.order, a.min_neighbors, a.points, a.fit,
                a.normals_out, a.coeffs};
  if ((a.variant ? a.variant : ML_PLAN) == VCR_MLS_TRANSPOSE)
    hipLaunchKernelGGL(mls_fit_kernel<true>, dim3(ml_blocks(total, ML_WAVES)), dim3(ML_BLOCK), 0, (hipStream_t)stream, k);
  else
    hipLaunchKernelGGL(mls_fit_kernel<false>, dim3(ml_blocks(total, ML_WAVES)), dim3(ML_BLOCK), 0, (hipStream_t)stream, k);
  const int rc = VCR_LAUNCH_RC();
  if (rc) return rc;
  MlVoid v{};
  v.d0 = a.coeffs; v.n0 = 6L * a.N; v.f0 = a.points; v.f1 = a.normals_out; v.nf = 3L * a.N; v.k = a.fit; v.nk = a.N;
  return ml_void(r, a.B, v, (hipStream_t)stream);
}

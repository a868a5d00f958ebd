// Boundary points over ragged rows (include/border/vcr_hip_border.h): vcr_border_angles_f32,
// vcr_border_gap_f32 with the host-only vcr_border_form, and vcr_border_near_f32.  No atomics, no workspace, no allocation.
//
//   border_angles_kernel    one WAVE per row: every lane builds the row's frame (the same arithmetic on the same values), then
//                           the lanes read 64 consecutive idx entries a step, each gathers its neighbour's 16-byte row and writes
//                           its slot's angle.  An angle is a function of its entry alone: the shape decides nothing but the time
//   border_gap_lane_kernel  one lane per row: for every counted angle a pass over the row for the smallest angle above it
//   border_gap_wave_kernel  one workgroup of ONE wave per row (csr_rows.h's ordering kernel is the pattern): 64 angles a step, each
//                           lane looking for its angle's successor in the row, which passes through LDS in chunks of BD_CHUNK;
//                           the largest difference, the largest and the smallest angle and the count are combined over the wave
//                           by exchanges.  max and min are exact, so both forms return the same bits
//   border_near_kernel      one lane per row: it leaves at the first entry that ends the d2 prefix or carries a flag
//   border_void_kernel      behind every pass, iss.hip's shape: a thread per (row_start[i], row_start[i+1]) pair (and, behind the
//                           spreading, per flag); a workgroup that finds the cloud not served fills ALL of that cloud's outputs.
//                           Several may; they write the same values.  Behind the angles it also writes NaN to the slots behind
//                           total[b], which no row owns
// A pass reads a row only where 0 <= row_start[i] <= row_start[i+1] <= total <= capacity, so no idx, d2 or angle slot outside the
// cloud's capacity is touched whatever row_start holds; an idx entry is checked against [0, N) before it is used.
#include "common.h"
#include "../../include/border/vcr_hip_border.h"

namespace {

typedef long long i64;

constexpr int BD_BLOCK = 256;
constexpr int BD_WAVES = BD_BLOCK / 64;                    // rows a workgroup of the angles' wave form serves
constexpr int BD_CHUNK = VCR_BORDER_CHUNK;                 // angles of a row in LDS at a time
static_assert(BD_CHUNK % 64 == 0, "a wave stages a chunk in whole passes");

struct BdRows { const int* idx; const i64* row_start; const i64* total; int N, capacity; };

struct BdAng { BdRows r; const float* xyz4; const float* normals; const float* d2; float r2; long total; double* angle;
               int* frame; };
struct BdGap { BdRows r; const double* angle; const int* frame; const float* d2; float r2; long total; int min_neighbors;
               double threshold; double* gap; int* flag; };
struct BdNear { BdRows r; const int* flag; const float* d2; long total; float r2; int* near; };
// per cloud: n0 doubles of d0 become NaN and nk ints of k (and of k1) VCR_BORDER_NOT_SERVED (a NULL pointer: nothing); flg: a
// VCR_BORDER_NOT_SERVED in it voids the cloud too; pad: the capacity's slots behind total become NaN in a served cloud
struct BdVoid { const i64* row_start; const i64* total; int N, capacity; long nblk; const int* flg; double* d0; long n0; int* k;
                int* k1; long nk; double* pad; };

__device__ __forceinline__ double bd_nan() { return __longlong_as_double(0x7FF8000000000000LL); }
__device__ __forceinline__ double bd_two_pi() { return __longlong_as_double(0x401921FB54442D18LL); }
__device__ __forceinline__ bool bd_finite(double v) { return __builtin_fabs(v) < __builtin_huge_val(); }      // false for a NaN

// Row i of cloud b: its first slot in the cloud's capacity and n_i.  false (and n = 0) where the row cannot be read.
__device__ __forceinline__ bool bd_row(const BdRows& r, long b, int i, i64& first, int& n) {
  const i64 tot = r.total[b];
  const i64* rs = r.row_start + (size_t)b * ((size_t)r.N + 1) + i;
  const i64 s = rs[0], e = rs[1];
  const bool ok = tot >= 0 && tot <= (i64)r.capacity && s >= 0 && s <= e && e <= tot;
  n = ok ? (int)(e - s) : 0;                               // <= capacity: an int
  first = ok ? s : 0;
  return ok;
}

// The used entries of a row of L: all of them where dd is NULL, otherwise the leading ones with dd[e] <= r2.  By one lane ...
__device__ __forceinline__ int bd_used_lane(const float* dd, int L, float r2) {
  if (!dd) return L;
  int u = 0;
  while (u < L && dd[u] <= r2) ++u;
  return u;
}

// ... and by a wave, 64 entries a step: the first lane whose entry fails ends them (the same number in every lane)
__device__ __forceinline__ int bd_used_wave(const float* dd, int L, float r2, int lane) {
  if (!dd) return L;
  for (int base = 0; base < L; base += 64) {
    const int e = base + lane;
    const unsigned long long fm = __ballot(e < L && !(dd[e] <= r2));
    if (fm) return base + __ffsll((long long)fm) - 1;
  }
  return L;
}

__global__ __launch_bounds__(BD_BLOCK) void border_angles_kernel(BdAng p) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const long g = (long)blockIdx.x * BD_WAVES + w;          // the wave's row
  if (g >= p.total) return;                                // the whole wave leaves (no barrier below)
  const int N = p.r.N;
  const long b = g / N;
  const int i = (int)(g - b * N);
  const float* rows = p.xyz4 + (size_t)b * N * 4;
  i64 first;
  int L;
  const bool ok = bd_row(p.r, b, i, first, L);
  const f32x4 me = ld4(rows + (size_t)i * 4);
  const float* nr = p.normals + (size_t)b * 3 * N + i;
  const double n0 = (double)nr[0], n1 = (double)nr[N], n2 = (double)nr[2 * (size_t)N];
  const double s = (n0 * n0 + n1 * n1) + n2 * n2;
  const bool framed = bd_finite((double)me.x) && bd_finite((double)me.y) && bd_finite((double)me.z) && bd_finite(n0) &&
                      bd_finite(n1) && bd_finite(n2) && s > 0. && bd_finite(s);
  if (lane == 0 && p.frame) p.frame[g] = ok ? (framed ? 1 : 0) : VCR_BORDER_NOT_SERVED;
  if (L == 0) return;                                      // (wave-uniform)
  const double inv = 1.0 / sqrt(s);
  const double h0 = n0 * inv, h1 = n1 * inv, h2 = n2 * inv;
  const double a0 = __builtin_fabs(h0), a1 = __builtin_fabs(h1), a2 = __builtin_fabs(h2);
  int ax = 0;                                              // the smallest |nh_a|, the lowest index among equals
  double am = a0;
  if (a1 < am) { ax = 1; am = a1; }
  if (a2 < am) ax = 2;
  const double e0 = ax == 0 ? 1.0 : 0.0, e1 = ax == 1 ? 1.0 : 0.0, e2 = ax == 2 ? 1.0 : 0.0;
  const double u0 = h1 * e2 - h2 * e1, u1 = h2 * e0 - h0 * e2, u2 = h0 * e1 - h1 * e0;
  const double v0 = h1 * u2 - h2 * u1, v1 = h2 * u0 - h0 * u2, v2 = h0 * u1 - h1 * u0;
  const int* nb = p.r.idx + (size_t)b * p.r.capacity + first;
  double* out = p.angle + (size_t)b * p.r.capacity + first;
  const int U = bd_used_wave(p.d2 ? p.d2 + (size_t)b * p.r.capacity + first : nullptr, L, p.r2, lane);
  for (int e = lane; e < L; e += 64) {
    int r = nb[e];
    r = (unsigned)r < (unsigned)N ? r : i;                 // an entry outside [0, N) reads as the row itself
    const f32x4 q = ld4(rows + (size_t)r * 4);
    const double d0 = (double)(q.x - me.x), d1 = (double)(q.y - me.y), d2 = (double)(q.z - me.z);
    const double pu = (u0 * d0 + u1 * d1) + u2 * d2, pv = (v0 * d0 + v1 * d1) + v2 * d2;
    const bool skip = !framed || e >= U || !(bd_finite(d0) && bd_finite(d1) && bd_finite(d2)) ||
                      (d0 == 0. && d1 == 0. && d2 == 0.) || (pu == 0. && pv == 0.);
    out[e] = skip ? bd_nan() : atan2(pv, pu);
  }
}

// What a row's angles come to: the largest difference to a successor (-1 where no angle has one), the extremes and the count
struct BdAcc { double diff, hi, lo; int c; };

__device__ __forceinline__ void bd_store(const BdGap& p, long g, bool ok, int L, const BdAcc& a) {
  double gap = 0.;
  int flag = 0;
  if (L + 1 >= p.min_neighbors && a.c > 0) {
    const double wrap = (bd_two_pi() - a.hi) + a.lo;
    gap = a.diff > wrap ? a.diff : wrap;
    flag = gap > p.threshold ? 1 : 0;
  }
  if (p.frame && p.frame[g] == 0) { gap = bd_nan(); flag = 0; }
  p.gap[g] = ok ? gap : bd_nan();
  p.flag[g] = ok ? flag : VCR_BORDER_NOT_SERVED;
}

__global__ __launch_bounds__(BD_BLOCK) void border_gap_lane_kernel(BdGap p) {
  const long g = (long)blockIdx.x * BD_BLOCK + threadIdx.x;
  if (g >= p.total) return;
  const int N = p.r.N;
  const long b = g / N;
  const int i = (int)(g - b * N);
  i64 first;
  int L;
  const bool ok = bd_row(p.r, b, i, first, L);
  BdAcc a{-1., 0., 0., 0};
  L = bd_used_lane(p.d2 ? p.d2 + (size_t)b * p.r.capacity + first : nullptr, L, p.r2);
  if (L + 1 >= p.min_neighbors) {
    const double* ang = p.angle + (size_t)b * p.r.capacity + first;
    for (int e = 0; e < L; ++e) {
      const double x = ang[e];
      if (x != x) continue;
      a.hi = a.c == 0 || x > a.hi ? x : a.hi;
      a.lo = a.c == 0 || x < a.lo ? x : a.lo;
      ++a.c;
      double succ = __builtin_huge_val();
      for (int f = 0; f < L; ++f) {
        const double y = ang[f];
        succ = y > x && y < succ ? y : succ;               // (a NaN fails y > x)
      }
      const double d = succ - x;
      a.diff = succ < __builtin_huge_val() && d > a.diff ? d : a.diff;
    }
  }
  bd_store(p, g, ok, L, a);
}

__global__ __launch_bounds__(64) void border_gap_wave_kernel(BdGap p) {
  __shared__ double chunk[BD_CHUNK];
  const int lane = threadIdx.x;
  const long g = blockIdx.x;                               // the workgroup's row
  const int N = p.r.N;
  const long b = g / N;
  const int i = (int)(g - b * N);
  i64 first;
  int L;
  const bool ok = bd_row(p.r, b, i, first, L);             // (workgroup-uniform, and so is everything that bounds a loop)
  const double inf = __builtin_huge_val();
  double diff = -1., hi = -inf, lo = inf;
  int c = 0;
  L = bd_used_wave(p.d2 ? p.d2 + (size_t)b * p.r.capacity + first : nullptr, L, p.r2, lane);
  if (L + 1 >= p.min_neighbors) {
    const double* ang = p.angle + (size_t)b * p.r.capacity + first;
    for (int e0 = 0; e0 < L; e0 += 64) {
      const int e = e0 + lane;
      const double x = e < L ? ang[e] : bd_nan();
      double succ = inf;
      for (int c0 = 0; c0 < L; c0 += BD_CHUNK) {
        const int m = L - c0 < BD_CHUNK ? L - c0 : BD_CHUNK;
        __syncthreads();                                   // the previous chunk has been read
        for (int f = lane; f < m; f += 64) chunk[f] = ang[c0 + f];
        __syncthreads();
        for (int f = 0; f < m; ++f) {                      // one address for every lane: broadcast reads
          const double y = chunk[f];
          succ = y > x && y < succ ? y : succ;
        }
      }
      if (x == x) {
        hi = x > hi ? x : hi;
        lo = x < lo ? x : lo;
        ++c;
        const double d = succ - x;
        diff = succ < inf && d > diff ? d : diff;
      }
    }
#pragma unroll
    for (int st = 32; st >= 1; st >>= 1) {
      const double od = __shfl_xor(diff, st, 64), oh = __shfl_xor(hi, st, 64), ol = __shfl_xor(lo, st, 64);
      c += __shfl_xor(c, st, 64);
      diff = od > diff ? od : diff;
      hi = oh > hi ? oh : hi;
      lo = ol < lo ? ol : lo;
    }
  }
  if (lane == 0) bd_store(p, g, ok, L, BdAcc{diff, hi, lo, c});
}

__global__ __launch_bounds__(BD_BLOCK) void border_near_kernel(BdNear p) {
  const long g = (long)blockIdx.x * BD_BLOCK + threadIdx.x;
  if (g >= p.total) return;
  const int N = p.r.N;
  const long b = g / N;
  const int i = (int)(g - b * N);
  i64 first;
  int L;
  const bool ok = bd_row(p.r, b, i, first, L);
  const int* flg = p.flag + (size_t)b * N;
  int hit = flg[i] > 0;
  if (!hit) {
    const int* nb = p.r.idx + (size_t)b * p.r.capacity + first;
    const float* dd = p.d2 ? p.d2 + (size_t)b * p.r.capacity + first : nullptr;
    for (int e = 0; e < L; ++e) {
      if (dd && !(dd[e] <= p.r2)) break;                   // the prefix ends
      int r = nb[e];
      r = (unsigned)r < (unsigned)N ? r : i;
      if (flg[r] > 0) { hit = 1; break; }
    }
  }
  p.near[g] = ok ? hit : VCR_BORDER_NOT_SERVED;
}

__global__ __launch_bounds__(BD_BLOCK) void border_void_kernel(BdVoid p) {
  const long b = (long)blockIdx.x / p.nblk;
  const long blk = (long)blockIdx.x - b * p.nblk;
  const long i = blk * BD_BLOCK + threadIdx.x;             // the pair (i, i + 1)
  const int N = p.N;
  const i64 tot = p.total[b];
  bool bad = false;
  if (i < N) {
    const i64* rs = p.row_start + (size_t)b * ((size_t)N + 1) + i;
    const i64 s = rs[0], e = rs[1];
    bad = s > e || (i == 0 && (s != 0 || tot < 0 || tot > (i64)p.capacity)) || (i == N - 1 && e != tot);
    if (p.flg) bad = bad || p.flg[(size_t)b * N + i] == VCR_BORDER_NOT_SERVED;
  }
  const double nan = bd_nan();
  if (!__syncthreads_or(bad)) {
    // served as far as this workgroup sees: its share of the slots no row owns (a cloud another workgroup voids gets NaN there too)
    if (p.pad && tot >= 0 && tot <= (i64)p.capacity)
      for (i64 j = tot + i; j < (i64)p.capacity; j += p.nblk * BD_BLOCK) p.pad[(size_t)b * p.capacity + j] = nan;
    return;
  }
  // voided: all of the cloud's outputs, by this workgroup (and by any other that found a fault: the same values)
  if (p.d0) for (long j = threadIdx.x; j < p.n0; j += BD_BLOCK) p.d0[(size_t)b * p.n0 + j] = nan;
  if (p.k) for (long j = threadIdx.x; j < p.nk; j += BD_BLOCK) p.k[(size_t)b * p.nk + j] = VCR_BORDER_NOT_SERVED;
  if (p.k1) for (long j = threadIdx.x; j < p.nk; j += BD_BLOCK) p.k1[(size_t)b * p.nk + j] = VCR_BORDER_NOT_SERVED;
}

// What the three passes and the form query ask of the numbers
int bd_numbers(int B, int N, int capacity, int variant) {
  if (B < 1 || capacity < 0) return VCR_EINVAL;
  if (variant != 0 && variant != VCR_BORDER_LANE && variant != VCR_BORDER_WAVE) return VCR_EINVAL;
  if (N < 1 || N > VCR_BORDER_MAX_N || (long)B * N >= (1L << 31) || (long)B * capacity >= (1L << 31)) return VCR_EUNSUPPORTED;
  return VCR_OK;
}

// THE one place that decides the gap's form: the row length the host can see
int bd_form(int N, int capacity, int variant) {
  if (variant) return variant;
  return (long)capacity / N >= VCR_BORDER_WAVE_GAP ? VCR_BORDER_WAVE : VCR_BORDER_LANE;
}

unsigned bd_blocks(long items, int per_block) { return (unsigned)((items + per_block - 1) / per_block); }

int bd_void(const BdRows& r, int B, const int* flg, double* d0, long n0, int* k, int* k1, long nk, double* pad, hipStream_t s) {
  const long nblk = ((long)r.N + BD_BLOCK - 1) / BD_BLOCK;
  const BdVoid v{r.row_start, r.total, r.N, r.capacity, nblk, flg, d0, n0, k, k1, nk, pad};
  hipLaunchKernelGGL(border_void_kernel, dim3((unsigned)(nblk * B)), dim3(BD_BLOCK), 0, s, v);
  return VCR_LAUNCH_RC();
}

}  // namespace

extern "C" int vcr_border_form(int B, int N, int capacity, int cu_count, int variant, int* form) {
  if (cu_count < 0) return VCR_EINVAL;
  const int e = bd_numbers(B, N, capacity, variant);
  if (e) return e;
  if (form) *form = bd_form(N, capacity, variant);
  return VCR_OK;
}

extern "C" int vcr_border_angles_f32(const vcr_border_angles_args* ua, vcr_stream_t stream) {
  vcr_border_angles_args a;
  if (vcr_take_args(ua, &a, offsetof(vcr_border_angles_args, frame))) return VCR_EINVAL;
  if (!a.xyz4 || !a.normals || !a.row_start || !a.total || ((!a.idx || !a.angle) && a.capacity != 0)) return VCR_EINVAL;
  if ((((uintptr_t)a.xyz4) & 15) || (a.d2 && !(a.r2 >= 0.f))) return VCR_EINVAL;
  const int e = bd_numbers(a.B, a.N, a.capacity, 0);
  if (e) return e;
  const long total = (long)a.B * a.N;
  const BdRows r{a.idx, (const i64*)a.row_start, (const i64*)a.total, a.N, a.capacity};
  const BdAng k{r, a.xyz4, a.normals, a.d2, a.r2, total, a.angle, a.frame};
  hipLaunchKernelGGL(border_angles_kernel, dim3(bd_blocks(total, BD_WAVES)), dim3(BD_BLOCK), 0, (hipStream_t)stream, k);
  const int rc = VCR_LAUNCH_RC();
  return rc ? rc : bd_void(r, a.B, nullptr, a.angle, a.capacity, a.frame, nullptr, a.N, a.angle, (hipStream_t)stream);
}

extern "C" int vcr_border_gap_f32(const vcr_border_gap_args* ua, vcr_stream_t stream) {
  vcr_border_gap_args a;
  if (vcr_take_args(ua, &a, sizeof(vcr_border_gap_args))) return VCR_EINVAL;
  if (!a.row_start || !a.total || !a.gap || !a.flag || (!a.angle && a.capacity != 0)) return VCR_EINVAL;
  if (a.min_neighbors < 1 || a.angle_threshold != a.angle_threshold || (a.d2 && !(a.r2 >= 0.f))) return VCR_EINVAL;
  const int e = bd_numbers(a.B, a.N, a.capacity, a.variant);
  if (e) return e;
  const long total = (long)a.B * a.N;
  const BdRows r{nullptr, (const i64*)a.row_start, (const i64*)a.total, a.N, a.capacity};
  const BdGap k{r, a.angle, a.frame, a.d2, a.r2, total, a.min_neighbors, a.angle_threshold, a.gap, a.flag};
  if (bd_form(a.N, a.capacity, a.variant) == VCR_BORDER_WAVE)
    hipLaunchKernelGGL(border_gap_wave_kernel, dim3((unsigned)total), dim3(64), 0, (hipStream_t)stream, k);
  else
    hipLaunchKernelGGL(border_gap_lane_kernel, dim3(bd_blocks(total, BD_BLOCK)), dim3(BD_BLOCK), 0, (hipStream_t)stream, k);
  const int rc = VCR_LAUNCH_RC();
  return rc ? rc : bd_void(r, a.B, nullptr, a.gap, a.N, a.flag, nullptr, a.N, nullptr, (hipStream_t)stream);
}

extern "C" int vcr_border_near_f32(const vcr_border_near_args* ua, vcr_stream_t stream) {
  vcr_border_near_args a;
  if (vcr_take_args(ua, &a, sizeof(vcr_border_near_args))) return VCR_EINVAL;
  if (!a.flag || !a.row_start || !a.total || !a.near || (!a.idx && a.capacity != 0)) return VCR_EINVAL;
  if (a.d2 && !(a.r2 >= 0.f)) return VCR_EINVAL;
  const int e = bd_numbers(a.B, a.N, a.capacity, 0);
  if (e) return e;
  const long total = (long)a.B * a.N;
  const BdRows r{a.idx, (const i64*)a.row_start, (const i64*)a.total, a.N, a.capacity};
  const BdNear k{r, a.flag, a.d2, total, a.r2, a.near};
  hipLaunchKernelGGL(border_near_kernel, dim3(bd_blocks(total, BD_BLOCK)), dim3(BD_BLOCK), 0, (hipStream_t)stream, k);
  const int rc = VCR_LAUNCH_RC();
  return rc ? rc : bd_void(r, a.B, a.flag, nullptr, 0, a.near, nullptr, a.N, nullptr, (hipStream_t)stream);
}

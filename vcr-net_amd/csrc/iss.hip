// ISS keypoints over ragged rows (include/keypoint/vcr_hip_iss.h): vcr_rows_iss_saliency_f32,
// vcr_rows_iss_nms_f32, the host-only vcr_rows_iss_form, and vcr_iss_select_f32, which hands the keypoint flags to the outlier
// filters' tail (outlier.hip).  No floating-point atomics, no LDS, no workspace in the two passes.
//
//   iss_saliency_kernel   one WAVE per row, lane p the header's chain p: the lanes read 64 consecutive idx entries a step, each
//                         gathers its neighbour's 16-byte row and adds the nine terms to its own sums.  The six combining steps
//                         are 64-bit exchanges with lane p ^ s (s = 32 ... 1); a + b and b + a are the same IEEE sum, so every
//                         lane ends with the same nine values and runs the same Jacobi on them (iss_point.h); lane 0 stores.
//   iss_nms_lane_kernel   one lane per row: it leaves at the first entry that ends the d2 prefix or blocks the point
//   iss_nms_wave_kernel   one wave per row, 64 entries a step: the prefix's end and the blockers are two ballots
//   iss_void_kernel       behind either pass, rows.hip's shape: a thread per (row_start[i], row_start[i+1]) pair (and, behind the
//                         suppression, per saliency); a workgroup that finds the cloud not served (or a NaN saliency) fills ALL
//                         of that cloud's outputs.  Several may; they write the same values.
// A pass reads a row only where 0 <= row_start[i] <= row_start[i+1] <= total <= capacity, so no idx or d2 slot outside the cloud's
// capacity is touched whatever row_start holds; an idx entry is checked against [0, N) before it is used.
#include "common.h"
#include "iss_point.h"
#include "outlier_flags.h"
#include "../../include/keypoint/vcr_hip_iss.h"

namespace {

typedef long long i64;

constexpr int IS_BLOCK = 256;
constexpr int IS_WAVES = IS_BLOCK / 64;                    // rows a workgroup of a wave form serves

struct IsRows { const int* idx; const i64* row_start; const i64* total; int N, capacity; };

struct IsSal { IsRows r; const float* xyz4; long total; int min_neighbors; double g21, g32; double* saliency; double* eigen; };
struct IsNms { IsRows r; const double* saliency; const float* d2; long total; int min_neighbors; float r2; int* keypoint; };
// per cloud: n0 doubles of d0 and n1 of d1 become NaN, nk ints of k VCR_ISS_NOT_SERVED (a NULL pointer: nothing); sal: a NaN in it
// voids the cloud too
struct IsVoid { const i64* row_start; const i64* total; int N, capacity; long nblk; const double* sal; double* d0; long n0;
                double* d1; long n1; int* k; long nk; };

__device__ __forceinline__ double is_nan() { return __longlong_as_double(0x7FF8000000000000LL); }

// Row i of cloud b: its first slot in the cloud's capacity and n_i.  false (and n = 0) where the row cannot be read.
__device__ __forceinline__ bool is_row(const IsRows& r, long b, int i, i64& first, int& n) {
  const i64 tot = r.total[b];
  const i64* rs = r.row_start + (size_t)b * ((size_t)r.N + 1) + i;
  const i64 s = rs[0], e = rs[1];
  const bool ok = tot >= 0 && tot <= (i64)r.capacity && s >= 0 && s <= e && e <= tot;
  n = ok ? (int)(e - s) : 0;                               // <= capacity: an int
  first = ok ? s : 0;
  return ok;
}

__device__ __forceinline__ double is_xor(double v, int s) { return __shfl_xor(v, s, 64); }

__global__ __launch_bounds__(IS_BLOCK) void iss_saliency_kernel(IsSal p) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const long g = (long)blockIdx.x * IS_WAVES + w;          // the wave's row
  if (g >= p.total) return;                                // the whole wave leaves (no barrier below)
  const int N = p.r.N;
  const long b = g / N;
  const int i = (int)(g - b * N);
  const float* rows = p.xyz4 + (size_t)b * N * 4;
  i64 first;
  int L;
  const bool ok = is_row(p.r, b, i, first, L);
  const int* nb = p.r.idx + (size_t)b * p.r.capacity + first;
  const f32x4 me = ld4(rows + (size_t)i * 4);
  NmSums s;                                                // chain `lane`: +0.0, then the entries lane, lane + 64, ...
#pragma unroll 2
  for (int e = lane; e < L; e += 64) {
    int r = nb[e];
    r = (unsigned)r < (unsigned)N ? r : i;                 // an entry outside [0, N) reads as the row itself
    s.add(ld4(rows + (size_t)r * 4), me);
  }
#pragma unroll
  for (int st = 32; st >= 1; st >>= 1) {                   // v[p] = v[p] + v[p ^ st], all nine, all p at once
    const double x = is_xor(s.sx, st), y = is_xor(s.sy, st), z = is_xor(s.sz, st);
    const double xx = is_xor(s.sxx, st), xy = is_xor(s.sxy, st), xz = is_xor(s.sxz, st);
    const double yy = is_xor(s.syy, st), yz = is_xor(s.syz, st), zz = is_xor(s.szz, st);
    s.sx = s.sx + x; s.sy = s.sy + y; s.sz = s.sz + z;
    s.sxx = s.sxx + xx; s.sxy = s.sxy + xy; s.sxz = s.sxz + xz;
    s.syy = s.syy + yy; s.syz = s.syz + yz; s.szz = s.szz + zz;
  }
  // the same in every lane from here on
  double l0 = 0., l1 = 0., l2 = 0., sal = 0.;
  if (L + 1 >= p.min_neighbors) {
    const int how = iss_eigenvalues(s, (double)(L + 1), l0, l1, l2);
    if (how == ISS_NOT_FINITE) l0 = l1 = l2 = is_nan();
    if (how == ISS_SOLVED && l1 / l2 < p.g21 && l0 / l1 < p.g32) sal = l0;
  }
  if (!ok) l0 = l1 = l2 = sal = is_nan();
  if (lane == 0) {
    p.saliency[g] = sal;
    if (p.eigen) {
      double* o = p.eigen + (size_t)g * 3;
      o[0] = l0; o[1] = l1; o[2] = l2;
    }
  }
}

__global__ __launch_bounds__(IS_BLOCK) void iss_nms_lane_kernel(IsNms p) {
  const long g = (long)blockIdx.x * IS_BLOCK + threadIdx.x;
  if (g >= p.total) return;
  const int N = p.r.N;
  const long b = g / N;
  const int i = (int)(g - b * N);
  i64 first;
  int L;
  const bool ok = is_row(p.r, b, i, first, L);
  const double* sal = p.saliency + (size_t)b * N;
  const double si = sal[i];
  int kp = 0;
  if (si > 0. && L + 1 >= p.min_neighbors) {               // (u_i <= n_i; a row that cannot be read has L = 0 and is voided)
    const int* nb = p.r.idx + (size_t)b * p.r.capacity + first;
    const float* dd = p.d2 ? p.d2 + (size_t)b * p.r.capacity + first : nullptr;
    int u = 0;
    bool blocked = false;
    for (; u < L; ++u) {
      if (dd && !(dd[u] <= p.r2)) break;                   // the prefix ends
      int r = nb[u];
      r = (unsigned)r < (unsigned)N ? r : i;
      if (si < sal[r]) { blocked = true; break; }
    }
    kp = !blocked && u + 1 >= p.min_neighbors;
  }
  p.keypoint[g] = ok ? kp : VCR_ISS_NOT_SERVED;
}

__global__ __launch_bounds__(IS_BLOCK) void iss_nms_wave_kernel(IsNms p) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const long g = (long)blockIdx.x * IS_WAVES + w;          // the wave's row
  if (g >= p.total) return;                                // the whole wave leaves (no barrier below)
  const int N = p.r.N;
  const long b = g / N;
  const int i = (int)(g - b * N);
  i64 first;
  int L;
  const bool ok = is_row(p.r, b, i, first, L);
  const double* sal = p.saliency + (size_t)b * N;
  const double si = sal[i];
  int kp = 0;
  if (si > 0. && L + 1 >= p.min_neighbors) {               // wave-uniform
    const int* nb = p.r.idx + (size_t)b * p.r.capacity + first;
    const float* dd = p.d2 ? p.d2 + (size_t)b * p.r.capacity + first : nullptr;
    int u = 0;
    bool blocked = false;
    for (int base = 0; base < L; base += 64) {
      const int e = base + lane;
      const bool in = e < L;
      const bool fail = in && dd && !(dd[e] <= p.r2);
      const unsigned long long fm = __ballot(fail);
      const int end = fm ? __ffsll((long long)fm) - 1 : 64;                    // the first lane behind the prefix
      const bool used = in && lane < end;
      bool blk = false;
      if (used) {
        int r = nb[e];
        r = (unsigned)r < (unsigned)N ? r : i;
        blk = si < sal[r];
      }
      if (__ballot(blk)) { blocked = true; break; }
      u += __popcll(__ballot(used));
      if (fm) break;
    }
    kp = !blocked && u + 1 >= p.min_neighbors;
  }
  if (lane == 0) p.keypoint[g] = ok ? kp : VCR_ISS_NOT_SERVED;
}

__global__ __launch_bounds__(IS_BLOCK) void iss_void_kernel(IsVoid p) {
  const long b = (long)blockIdx.x / p.nblk;
  const long i = ((long)blockIdx.x - b * p.nblk) * IS_BLOCK + threadIdx.x;       // the pair (i, i + 1)
  const int N = p.N;
  bool bad = false;
  if (i < N) {
    const i64* rs = p.row_start + (size_t)b * ((size_t)N + 1) + i;
    const i64 s = rs[0], e = rs[1], tot = p.total[b];
    bad = s > e || (i == 0 && (s != 0 || tot < 0 || tot > (i64)p.capacity)) || (i == N - 1 && e != tot);
    if (p.sal) {
      const double v = p.sal[(size_t)b * N + i];
      bad = bad || v != v;
    }
  }
  if (!__syncthreads_or(bad)) return;
  // voided: all of the cloud's outputs, by this workgroup (and by any other that found a fault: the same values)
  const double nan = is_nan();
  if (p.d0) for (long j = threadIdx.x; j < p.n0; j += IS_BLOCK) p.d0[(size_t)b * p.n0 + j] = nan;
  if (p.d1) for (long j = threadIdx.x; j < p.n1; j += IS_BLOCK) p.d1[(size_t)b * p.n1 + j] = nan;
  if (p.k) for (long j = threadIdx.x; j < p.nk; j += IS_BLOCK) p.k[(size_t)b * p.nk + j] = VCR_ISS_NOT_SERVED;
}

// What the two passes and the form query ask of the numbers
int is_numbers(int B, int N, int capacity, int variant) {
  if (B < 1 || capacity < 0) return VCR_EINVAL;
  if (variant != 0 && variant != VCR_ISS_LANE && variant != VCR_ISS_WAVE) return VCR_EINVAL;
  if (N < 1 || N > VCR_ISS_MAX_N || (long)B * N >= (1L << 31) || (long)B * capacity >= (1L << 31)) return VCR_EUNSUPPORTED;
  return VCR_OK;
}

// THE one place that decides the suppression's form: the row length the host can see
int is_form(int N, int capacity, int variant) {
  if (variant) return variant;
  return (long)capacity / N >= VCR_ISS_WAVE_NMS ? VCR_ISS_WAVE : VCR_ISS_LANE;
}

unsigned is_blocks(long items, int per_block) { return (unsigned)((items + per_block - 1) / per_block); }

int is_void(const IsRows& r, int B, const double* sal, double* d0, long n0, double* d1, long n1, int* k, long nk, hipStream_t s) {
  const long nblk = ((long)r.N + IS_BLOCK - 1) / IS_BLOCK;
  const IsVoid v{r.row_start, r.total, r.N, r.capacity, nblk, sal, d0, n0, d1, n1, k, nk};
  hipLaunchKernelGGL(iss_void_kernel, dim3((unsigned)(nblk * B)), dim3(IS_BLOCK), 0, s, v);
  return VCR_LAUNCH_RC();
}

int sl_take(const vcr_iss_select_args* user, vcr_iss_select_args* mine) {
  return vcr_take_args(user, mine, offsetof(vcr_iss_select_args, index));
}

int sl_check(const vcr_iss_select_args& a) {
  if (!a.xyz || !a.keypoint || !a.points || !a.count || a.B < 1) return VCR_EINVAL;
  if (a.N < 1 || a.N > VCR_ISS_MAX_N || (long)a.B * a.N >= (1L << 31)) return VCR_EUNSUPPORTED;
  return VCR_OK;
}

// workspace: blkcnt [B nblk], the tail's block counts
size_t sl_bytes(int B, int N) {
  const size_t nblk = ((size_t)N + IS_BLOCK - 1) / IS_BLOCK;
  return ((size_t)B * nblk * 4 + 255) & ~(size_t)255;
}

}  // namespace

extern "C" int vcr_rows_iss_form(int B, int N, int capacity, int cu_count, int variant, int* nms_form) {
  if (cu_count < 0) return VCR_EINVAL;
  const int e = is_numbers(B, N, capacity, variant);
  if (e) return e;
  if (nms_form) *nms_form = is_form(N, capacity, variant);
  return VCR_OK;
}

extern "C" int vcr_rows_iss_saliency_f32(const vcr_rows_iss_saliency_args* ua, vcr_stream_t stream) {
  vcr_rows_iss_saliency_args a;
  if (vcr_take_args(ua, &a, offsetof(vcr_rows_iss_saliency_args, eigen))) return VCR_EINVAL;
  if (!a.xyz4 || !a.row_start || !a.total || !a.saliency || (!a.idx && a.capacity != 0)) return VCR_EINVAL;
  if (((uintptr_t)a.xyz4) & 15) return VCR_EINVAL;
  if (a.min_neighbors < 1 || !(__builtin_isfinite(a.gamma_21) && a.gamma_21 > 0.) || !(__builtin_isfinite(a.gamma_32) && a.gamma_32 > 0.))
    return VCR_EINVAL;
  const int e = is_numbers(a.B, a.N, a.capacity, 0);
  if (e) return e;
  const long total = (long)a.B * a.N;
  const IsRows r{a.idx, (const i64*)a.row_start, (const i64*)a.total, a.N, a.capacity};
  const IsSal k{r, a.xyz4, total, a.min_neighbors, a.gamma_21, a.gamma_32, a.saliency, a.eigen};
  hipLaunchKernelGGL(iss_saliency_kernel, dim3(is_blocks(total, IS_WAVES)), dim3(IS_BLOCK), 0, (hipStream_t)stream, k);
  const int rc = VCR_LAUNCH_RC();
  return rc ? rc : is_void(r, a.B, nullptr, a.saliency, a.N, a.eigen, 3L * a.N, nullptr, 0, (hipStream_t)stream);
}

extern "C" int vcr_rows_iss_nms_f32(const vcr_rows_iss_nms_args* ua, vcr_stream_t stream) {
  vcr_rows_iss_nms_args a;
  if (vcr_take_args(ua, &a, sizeof(vcr_rows_iss_nms_args))) return VCR_EINVAL;
  if (!a.row_start || !a.total || !a.saliency || !a.keypoint || (!a.idx && a.capacity != 0)) return VCR_EINVAL;
  if (a.min_neighbors < 1 || (a.d2 && !(a.r2_nm >= 0.f))) return VCR_EINVAL;
  const int e = is_numbers(a.B, a.N, a.capacity, a.variant);
  if (e) return e;
  const long total = (long)a.B * a.N;
  const IsRows r{a.idx, (const i64*)a.row_start, (const i64*)a.total, a.N, a.capacity};
  const IsNms k{r, a.saliency, a.d2, total, a.min_neighbors, a.r2_nm, a.keypoint};
  if (is_form(a.N, a.capacity, a.variant) == VCR_ISS_WAVE)
    hipLaunchKernelGGL(iss_nms_wave_kernel, dim3(is_blocks(total, IS_WAVES)), dim3(IS_BLOCK), 0, (hipStream_t)stream, k);
  else
    hipLaunchKernelGGL(iss_nms_lane_kernel, dim3(is_blocks(total, IS_BLOCK)), dim3(IS_BLOCK), 0, (hipStream_t)stream, k);
  const int rc = VCR_LAUNCH_RC();
  return rc ? rc : is_void(r, a.B, a.saliency, nullptr, 0, nullptr, 0, a.keypoint, a.N, (hipStream_t)stream);
}

extern "C" size_t vcr_iss_select_workspace_bytes(const vcr_iss_select_args* ua, int cu_count) {
  vcr_iss_select_args a;
  if (sl_take(ua, &a) || cu_count < 0 || sl_check(a)) return 0;
  return sl_bytes(a.B, a.N);
}

extern "C" int vcr_iss_select_f32(const vcr_iss_select_args* ua, void* workspace, size_t workspace_bytes, vcr_stream_t stream) {
  vcr_iss_select_args a;
  if (sl_take(ua, &a)) return VCR_EINVAL;
  const int e = sl_check(a);
  if (e) return e;
  if (!workspace || (((uintptr_t)workspace) & 255) || workspace_bytes < sl_bytes(a.B, a.N)) return VCR_EINVAL;
  return outlier_compact_flags(a.keypoint, a.xyz, a.B, a.N, reinterpret_cast<int*>(workspace), a.points, a.count, a.index,
                               (hipStream_t)stream);
}

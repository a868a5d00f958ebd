// Normals and FPFH over ragged rows (include/ext/vcr_hip_rows.h): vcr_rows_normals_f32, vcr_rows_spfh_f32,
// vcr_rows_fpfh_f32 -- normals.hip's and fpfh.hip's definitions with the neighbourhood taken from (idx, row_start, total), the
// CSR rows vcr_grid_radius_f32 writes, instead of idx [B,N,k].  No workspace, no floating-point atomics, no tree reduction.
//
//   rows_normals_kernel     one LANE per row, normals_kernel's shape: the nine sums are ordered, so a row is one lane's; the
//                           arithmetic behind the sums is normals_point.h, shared with normals.hip.
//   rows_spfh_lane_kernel   one lane per row, spfh_kernel's shape.  A count may reach 131 071, so the 33 counters do not pack
//                           into registers as spfh_kernel's bytes do: they are a column of LDS words the lane owns
//                           (cnt[bin][thread]: consecutive lanes, consecutive banks, no atomics).
//   rows_spfh_wave_kernel   one WAVE per row: lane l takes the pairs l, l + 64, ...; the counts are integers, so the order is
//                           free -- the lanes add into the wave's 33 LDS words with integer LDS atomics.  36 lanes store the row.
//   rows_fpfh_lane_kernel   one lane per (row, group), fpfh_kernel's shape and lane numbering, reading 48-byte groups.
//   rows_fpfh_wave_kernel   one wave per row, a lane a BIN: lane 11 g + b runs acc[b] of group g in the row's order.  The wave
//                           takes 64 neighbours at a time -- lane l loads entry l, its row and its d2 -- and then walks them in
//                           order, every lane reading the neighbour's index and d2 from lane t.  sum_g adds the group's eleven
//                           values of a neighbour, bins ascending: each lane of the group fetches them from the lanes that
//                           computed them (the same bits as its own formula would give) and runs the whole chain itself, so
//                           no lane waits for three others that divide eleven times.
//   rows_void_kernel        behind every pass: a thread per (row_start[i], row_start[i+1]) pair; a workgroup that finds the
//                           cloud not served fills ALL of that cloud's outputs (NaN, or zero words).  Several may; they write
//                           the same values.  It runs behind the pass because a pass cannot know of another row's fault.
// A pass reads a row only where 0 <= row_start[i] <= row_start[i+1] <= total <= capacity, so no idx slot outside the cloud's
// capacity is touched whatever row_start holds; an idx entry is checked against [0, N) before it is used.
// The row's bounds, the pair arithmetic and the void kernel are rows_pair.h's, shared with support.hip.
#include "rows_pair.h"
#include "normals_point.h"

namespace {

struct RwNormals { RwRows r; const float* xyz4; long total; const float* view; float* normals; float* curv; };   // total = B N
struct RwSpfh { RwRows r; const float* xyz4; const float* normals; long total; unsigned* spfh; };
struct RwFpfh { RwRows r; const float* xyz4; const unsigned* spfh; long total; float* fpfh; };

__global__ __launch_bounds__(RW_BLOCK) void rows_normals_kernel(RwNormals p) {
  const long g = (long)blockIdx.x * RW_BLOCK + threadIdx.x;
  if (g >= p.total) return;
  const int N = p.r.N;
  const long b = g / N;
  const int i = (int)(g - b * N);
  const float* rows = p.xyz4 + (size_t)b * N * 4;
  const int* nb;
  int L;
  const bool ok = rw_row(p.r, b, i, nb, L);
  const f32x4 me = ld4(rows + (size_t)i * 4);
  float n0 = 0.f, n1 = 0.f, n2 = 1.f, cv = 0.f;            // L < 2: fewer than three points define no plane
  if (L >= 2) {
    NmSums s;
#pragma unroll 4
    for (int j = 0; j < L; ++j) {
      int r = nb[j];
      r = (unsigned)r < (unsigned)N ? r : i;               // an entry outside [0, N) reads as the row itself
      s.add(ld4(rows + (size_t)r * 4), me);
    }
    nm_point(s, (double)(L + 1), me, p.view ? p.view + (size_t)b * 3 : nullptr, n0, n1, n2, cv);
  }
  if (!ok) n0 = n1 = n2 = cv = rw_nan();
  float* out = p.normals + (size_t)b * 3 * N + i;
  out[0] = n0; out[N] = n1; out[2 * (size_t)N] = n2;
  if (p.curv) p.curv[g] = cv;
}

__global__ __launch_bounds__(RW_BLOCK) void rows_spfh_lane_kernel(RwSpfh p) {
  __shared__ unsigned cnt[3 * RW_BINS][RW_BLOCK];          // a column a lane: its own 33 counters
  const int tid = threadIdx.x;
  const long g = (long)blockIdx.x * RW_BLOCK + tid;
  if (g >= p.total) return;                                // (no barrier below: a lane touches its own column alone)
  const int N = p.r.N;
  const long b = g / N;
  const int i = (int)(g - b * N);
  const float* rows = p.xyz4 + (size_t)b * N * 4;
  const float* nrm = p.normals + (size_t)b * 3 * N;
  const int* nb;
  int L;
  rw_row(p.r, b, i, nb, L);                                // (a row that cannot be read is empty: zero words)
#pragma unroll
  for (int h = 0; h < 3 * RW_BINS; ++h) cnt[h][tid] = 0u;
  const f32x4 me = ld4(rows + (size_t)i * 4);
  const float m0 = nrm[i], m1 = nrm[N + i], m2 = nrm[2 * (size_t)N + i];
  const bool me_ok = rw_finite(m0) && rw_finite(m1) && rw_finite(m2);
  unsigned c = 0;
  for (int j = 0; j < L; ++j) {
    int r = nb[j];
    r = (unsigned)r < (unsigned)N ? r : i;                 // an entry outside [0, N) reads as the row itself
    const f32x4 q = ld4(rows + (size_t)r * 4);
    int b0, b1, b2;
    if (!rw_pair(me, m0, m1, m2, me_ok, q, nrm[r], nrm[N + r], nrm[2 * (size_t)N + r], b0, b1, b2)) continue;
    cnt[b0][tid] += 1u;
    cnt[RW_BINS + b1][tid] += 1u;
    cnt[2 * RW_BINS + b2][tid] += 1u;
    ++c;
  }
  uint4* out = reinterpret_cast<uint4*>(p.spfh + (size_t)g * RW_WORDS);
#pragma unroll
  for (int grp = 0; grp < 3; ++grp) {
    const int o = grp * RW_BINS;
    out[3 * grp] = make_uint4(cnt[o][tid], cnt[o + 1][tid], cnt[o + 2][tid], cnt[o + 3][tid]);
    out[3 * grp + 1] = make_uint4(cnt[o + 4][tid], cnt[o + 5][tid], cnt[o + 6][tid], cnt[o + 7][tid]);
    out[3 * grp + 2] = make_uint4(cnt[o + 8][tid], cnt[o + 9][tid], cnt[o + 10][tid], c);
  }
}

__global__ __launch_bounds__(RW_BLOCK) void rows_spfh_wave_kernel(RwSpfh p) {
  __shared__ unsigned cnt[RW_WAVES][3 * RW_BINS + 3];      // a wave's 33 counters, then c_i
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const long g = (long)blockIdx.x * RW_WAVES + w;          // the wave's row
  const bool live = g < p.total;
  if (lane < 3 * RW_BINS + 3) cnt[w][lane] = 0u;
  __syncthreads();
  if (live) {
    const int N = p.r.N;
    const long b = g / N;
    const int i = (int)(g - b * N);
    const float* rows = p.xyz4 + (size_t)b * N * 4;
    const float* nrm = p.normals + (size_t)b * 3 * N;
    const int* nb;
    int L;
    rw_row(p.r, b, i, nb, L);
    const f32x4 me = ld4(rows + (size_t)i * 4);
    const float m0 = nrm[i], m1 = nrm[N + i], m2 = nrm[2 * (size_t)N + i];
    const bool me_ok = rw_finite(m0) && rw_finite(m1) && rw_finite(m2);
    unsigned c = 0;
    for (int j = lane; j < L; j += 64) {
      int r = nb[j];
      r = (unsigned)r < (unsigned)N ? r : i;
      const f32x4 q = ld4(rows + (size_t)r * 4);
      int b0, b1, b2;
      if (!rw_pair(me, m0, m1, m2, me_ok, q, nrm[r], nrm[N + r], nrm[2 * (size_t)N + r], b0, b1, b2)) continue;
      atomicAdd(&cnt[w][b0], 1u);                          // integer LDS atomics: the counts do not depend on the order
      atomicAdd(&cnt[w][RW_BINS + b1], 1u);
      atomicAdd(&cnt[w][2 * RW_BINS + b2], 1u);
      ++c;
    }
    if (c) atomicAdd(&cnt[w][3 * RW_BINS], c);
  }
  __syncthreads();
  if (live && lane < RW_WORDS) {
    const int grp = lane / 12, s = lane - grp * 12;
    p.spfh[(size_t)g * RW_WORDS + lane] = s == RW_BINS ? cnt[w][3 * RW_BINS] : cnt[w][grp * RW_BINS + s];
  }
}

__global__ __launch_bounds__(RW_BLOCK) void rows_fpfh_lane_kernel(RwFpfh p) {
  const long t = (long)blockIdx.x * RW_BLOCK + threadIdx.x;
  if (t >= p.total) return;                                // total = 3 B N
  const int N = p.r.N;
  const long bg = t / N;                                   // (cloud, group)
  const int i = (int)(t - bg * N);
  const long b = bg / 3;
  const int grp = (int)(bg - b * 3);
  const float* rows = p.xyz4 + (size_t)b * N * 4;
  const unsigned* sp = p.spfh + (size_t)b * N * RW_WORDS + grp * 12;
  const int* nb;
  int L;
  const bool ok = rw_row(p.r, b, i, nb, L);
  const f32x4 me = ld4(rows + (size_t)i * 4);
  double acc[RW_BINS];
#pragma unroll
  for (int h = 0; h < RW_BINS; ++h) acc[h] = 0.0;
  double sum = 0.0;
  for (int j = 0; j < L; ++j) {
    int r = nb[j];
    r = (unsigned)r < (unsigned)N ? r : i;                 // an entry outside [0, N) reads as the row itself: d2 = 0, skipped
    const f32x4 q = ld4(rows + (size_t)r * 4);
    const uint4* hp = reinterpret_cast<const uint4*>(sp + (size_t)r * RW_WORDS);
    const uint4 h0 = hp[0], h1 = hp[1], h2 = hp[2];
    const double dx = (double)(q[0] - me[0]), dy = (double)(q[1] - me[1]), dz = (double)(q[2] - me[2]);
    const double d2 = (dx * dx + dy * dy) + dz * dz;
    const unsigned cj = h2.w;
    if (!(d2 > 0.0 && d2 < RW_INF) || cj == 0u) continue;
    const unsigned hj[RW_BINS] = {h0.x, h0.y, h0.z, h0.w, h1.x, h1.y, h1.z, h1.w, h2.x, h2.y, h2.z};
    const double s = 100.0 / (double)cj;
#pragma unroll
    for (int h = 0; h < RW_BINS; ++h) {
      const double val = ((double)hj[h] * s) / d2;
      acc[h] += val;
      sum += val;
    }
  }
  const uint4* op = reinterpret_cast<const uint4*>(sp + (size_t)i * RW_WORDS);
  const uint4 o0 = op[0], o1 = op[1], o2 = op[2];
  const unsigned own[RW_BINS] = {o0.x, o0.y, o0.z, o0.w, o1.x, o1.y, o1.z, o1.w, o2.x, o2.y, o2.z};
  const unsigned ci = o2.w;
  const double scale = 100.0 / sum;
  const double so = 100.0 / (double)ci;
  float* out = p.fpfh + ((size_t)b * 33 + (size_t)grp * RW_BINS) * N + i;
#pragma unroll
  for (int h = 0; h < RW_BINS; ++h) {
    const double a = sum != 0.0 ? acc[h] * scale : acc[h];
    const double mine = ci != 0u ? (double)own[h] * so : 0.0;
    out[(size_t)h * N] = ok ? (float)(a + mine) : rw_nan();
  }
}

__global__ __launch_bounds__(RW_BLOCK) void rows_fpfh_wave_kernel(RwFpfh p) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const long g = (long)blockIdx.x * RW_WAVES + w;          // the wave's row
  if (g >= p.total) return;                                // total = B N; the whole wave leaves (no barrier below)
  const int N = p.r.N;
  const long b = g / N;
  const int i = (int)(g - b * N);
  const bool mine = lane < 3 * RW_BINS;                    // lanes 33 .. 63 shadow lane 0 and store nothing
  const int grp = mine ? lane / RW_BINS : 0, bin = mine ? lane - grp * RW_BINS : 0;
  const float* rows = p.xyz4 + (size_t)b * N * 4;
  const unsigned* sp = p.spfh + (size_t)b * N * RW_WORDS + grp * 12;
  const int* nb;
  int L;
  const bool ok = rw_row(p.r, b, i, nb, L);
  const f32x4 me = ld4(rows + (size_t)i * 4);
  double acc = 0.0, sum = 0.0;
  for (int base = 0; base < L; base += 64) {
    int r = i;
    double d2l = 0.0;
    if (base + lane < L) {                                 // lane l: the chunk's entry l, its row and its d2
      r = nb[base + lane];
      r = (unsigned)r < (unsigned)N ? r : i;               // an entry outside [0, N) reads as the row itself: d2 = 0, skipped
      const f32x4 q = ld4(rows + (size_t)r * 4);
      const double dx = (double)(q[0] - me[0]), dy = (double)(q[1] - me[1]), dz = (double)(q[2] - me[2]);
      d2l = (dx * dx + dy * dy) + dz * dz;
    }
    const int n = L - base < 64 ? L - base : 64;
    for (int t = 0; t < n; ++t) {                         // the row's order; (rj, d2) are the same in every lane
      const int rj = __shfl(r, t, 64);
      const double d2 = __shfl(d2l, t, 64);
      if (!(d2 > 0.0 && d2 < RW_INF)) continue;
      const unsigned* hj = sp + (size_t)rj * RW_WORDS;
      const unsigned cj = hj[RW_BINS], count = hj[bin];
      const bool use = cj != 0u;                           // per group: the same in the lanes a value is fetched from
      const double s = 100.0 / (double)cj;
      const double val = ((double)count * s) / d2;
      if (use) acc += val;
#pragma unroll
      for (int h = 0; h < RW_BINS; ++h) {                  // sum_g: the group's eleven values, bins ascending
        const double v = __shfl(val, grp * RW_BINS + h, 64);
        if (use) sum += v;
      }
    }
  }
  const unsigned* own = sp + (size_t)i * RW_WORDS;
  const unsigned ci = own[RW_BINS];
  const double a = sum != 0.0 ? acc * (100.0 / sum) : acc;
  const double self = ci != 0u ? (double)own[bin] * (100.0 / (double)ci) : 0.0;
  if (mine) p.fpfh[((size_t)b * 33 + lane) * N + i] = ok ? (float)(a + self) : rw_nan();
}

// What the three entry points and the form query ask of the numbers
int rw_numbers(int B, int N, int capacity, int max_nn, int variant) {
  if (B < 1 || capacity < 0 || max_nn < 0) return VCR_EINVAL;
  if (variant != 0 && variant != VCR_ROWS_LANE && variant != VCR_ROWS_WAVE) return VCR_EINVAL;
  if (N < 1 || N > VCR_ROWS_MAX_N || (long)B * N >= (1L << 31) || (long)B * capacity >= (1L << 31)) return VCR_EUNSUPPORTED;
  return VCR_OK;
}

// ... and of the pointers: `out` the mandatory output, a16 the two that must be 16-B aligned (either may be NULL: not asked)
int rw_check(const void* xyz4, const void* idx, const void* row_start, const void* total, const void* out, const void* a16, int B,
             int N, int capacity, int max_nn, int variant) {
  if (!xyz4 || !row_start || !total || !out || (!idx && capacity != 0)) return VCR_EINVAL;
  if ((((uintptr_t)xyz4) & 15) || (((uintptr_t)a16) & 15)) return VCR_EINVAL;
  return rw_numbers(B, N, capacity, max_nn, variant);
}

// THE one place that decides a pass's form: the row length the host can see
int rw_form(int N, int capacity, int max_nn, int variant, int threshold) {
  if (variant) return variant;
  long est = (long)capacity / N;
  if (max_nn > 0 && est > max_nn) est = max_nn;
  return est >= threshold ? VCR_ROWS_WAVE : VCR_ROWS_LANE;
}

}  // namespace

extern "C" int vcr_rows_form(int B, int N, int capacity, int max_nn, int cu_count, int variant, int* spfh_form, int* fpfh_form) {
  if (cu_count < 0) return VCR_EINVAL;
  const int e = rw_numbers(B, N, capacity, max_nn, variant);
  if (e) return e;
  if (spfh_form) *spfh_form = rw_form(N, capacity, max_nn, variant, VCR_ROWS_WAVE_SPFH);
  if (fpfh_form) *fpfh_form = rw_form(N, capacity, max_nn, variant, VCR_ROWS_WAVE_FPFH);
  return VCR_OK;
}

extern "C" int vcr_rows_normals_f32(const vcr_rows_normals_args* ua, vcr_stream_t stream) {
  vcr_rows_normals_args a;
  if (vcr_take_args(ua, &a, offsetof(vcr_rows_normals_args, curvature))) return VCR_EINVAL;
  const int e = rw_check(a.xyz4, a.idx, a.row_start, a.total, a.normals, nullptr, a.B, a.N, a.capacity, a.max_nn, 0);
  if (e) return e;
  const long total = (long)a.B * a.N;
  const RwRows r{a.idx, (const i64*)a.row_start, (const i64*)a.total, a.N, a.capacity, a.max_nn};
  const RwNormals k{r, a.xyz4, total, a.viewpoint, a.normals, a.curvature};
  hipLaunchKernelGGL(rows_normals_kernel, dim3(rw_blocks(total, RW_BLOCK)), dim3(RW_BLOCK), 0, (hipStream_t)stream, k);
  const int rc = VCR_LAUNCH_RC();
  return rc ? rc : rw_void(r, a.B, a.normals, 3L * a.N, a.curvature, a.N, nullptr, 0, (hipStream_t)stream);
}

extern "C" int vcr_rows_spfh_f32(const vcr_rows_spfh_args* ua, vcr_stream_t stream) {
  vcr_rows_spfh_args a;
  if (vcr_take_args(ua, &a, sizeof(vcr_rows_spfh_args))) return VCR_EINVAL;
  const int e = rw_check(a.xyz4, a.idx, a.row_start, a.total, a.spfh, a.spfh, a.B, a.N, a.capacity, a.max_nn, a.variant);
  if (e) return e;
  if (!a.normals) return VCR_EINVAL;
  const long total = (long)a.B * a.N;
  const RwRows r{a.idx, (const i64*)a.row_start, (const i64*)a.total, a.N, a.capacity, a.max_nn};
  const RwSpfh k{r, a.xyz4, a.normals, total, a.spfh};
  if (rw_form(a.N, a.capacity, a.max_nn, a.variant, VCR_ROWS_WAVE_SPFH) == VCR_ROWS_WAVE)
    hipLaunchKernelGGL(rows_spfh_wave_kernel, dim3(rw_blocks(total, RW_WAVES)), dim3(RW_BLOCK), 0, (hipStream_t)stream, k);
  else
    hipLaunchKernelGGL(rows_spfh_lane_kernel, dim3(rw_blocks(total, RW_BLOCK)), dim3(RW_BLOCK), 0, (hipStream_t)stream, k);
  const int rc = VCR_LAUNCH_RC();
  return rc ? rc : rw_void(r, a.B, nullptr, 0, nullptr, 0, a.spfh, (long)RW_WORDS * a.N, (hipStream_t)stream);
}

extern "C" int vcr_rows_fpfh_f32(const vcr_rows_fpfh_args* ua, vcr_stream_t stream) {
  vcr_rows_fpfh_args a;
  if (vcr_take_args(ua, &a, sizeof(vcr_rows_fpfh_args))) return VCR_EINVAL;
  const int e = rw_check(a.xyz4, a.idx, a.row_start, a.total, a.fpfh, a.spfh, a.B, a.N, a.capacity, a.max_nn, a.variant);
  if (e) return e;
  if (!a.spfh) return VCR_EINVAL;
  const long total = (long)a.B * a.N;
  const RwRows r{a.idx, (const i64*)a.row_start, (const i64*)a.total, a.N, a.capacity, a.max_nn};
  if (rw_form(a.N, a.capacity, a.max_nn, a.variant, VCR_ROWS_WAVE_FPFH) == VCR_ROWS_WAVE) {
    const RwFpfh k{r, a.xyz4, a.spfh, total, a.fpfh};
    hipLaunchKernelGGL(rows_fpfh_wave_kernel, dim3(rw_blocks(total, RW_WAVES)), dim3(RW_BLOCK), 0, (hipStream_t)stream, k);
  } else {
    const RwFpfh k{r, a.xyz4, a.spfh, 3 * total, a.fpfh};  // < 3 * 2^31 lanes: at most 25 165 824 workgroups
    hipLaunchKernelGGL(rows_fpfh_lane_kernel, dim3(rw_blocks(3 * total, RW_BLOCK)), dim3(RW_BLOCK), 0, (hipStream_t)stream, k);
  }
  const int rc = VCR_LAUNCH_RC();
  return rc ? rc : rw_void(r, a.B, a.fpfh, 33L * a.N, nullptr, 0, nullptr, 0, (hipStream_t)stream);
}

// Normals and FPFH at M centres over a support cloud of N points (include/support/vcr_hip_support.h):
// vcr_support_normals_f32, vcr_support_spfh_f32, vcr_support_needed_f32, vcr_support_fpfh_f32 -- rows.hip's passes with row i
// belonging to CENTRE i (c4) and its entries indexing the SUPPORT (xyz4).  The row's bounds, the pair arithmetic and the check
// behind every pass are rows_pair.h's; the normal from the nine sums is normals_point.h's; the compaction of the needed points
// is outlier_tail.h's (wg_scan.h's rank and offsets).  No floating-point atomics, no tree reduction.
//
//   support_normals_kernel     one lane a centre: the nine sums over the used entries in the row's order, self entries included
//   support_spfh_lane_kernel   one lane a centre over the used NEIGHBOUR entries; the 33 counters a column of LDS words a lane
//   support_spfh_wave_kernel   one wave a centre, 64 entries at a time: an entry's rank among the neighbour entries is the
//                              running base + the prefix count of the chunk's ballot, so the cut at max_nn needs no serial walk;
//                              the counts are integers, the lanes add them with LDS atomics
//   support_zero_kernel        the marks' zeros (a kernel, not a memset: graph capture keeps to kernel nodes)
//   support_mark_kernel        one lane a centre: need[b, j] = 1 for its used neighbour entries -- plain stores of the value 1;
//                              several lanes may write the same word
//   support_slot_kernel        one lane a support point: its rank among the needed (the block's offset + the ballot rank), or -1
//   support_fpfh_kernel        one lane a (centre, group), rows_fpfh_lane_kernel's shape; a neighbour's histogram row is
//                              support_spfh[slot[j]], the own term centre_spfh[i]
// A pass reads a row only where 0 <= row_start[i] <= row_start[i+1] <= total <= capacity, so no idx slot outside the cloud's
// capacity is touched whatever row_start holds; an idx entry is checked against [0, N) and a slot against [0, R) before use.
#include "rows_pair.h"
#include "normals_point.h"
#include "outlier_tail.h"
#include "../../include/support/vcr_hip_support.h"

static_assert(VCR_SUPPORT_SPFH_WORDS == VCR_ROWS_SPFH_WORDS, "one histogram layout");
static_assert(RW_BLOCK == NN_BLOCK, "the compaction's workgroup");

namespace {

// r: the rows of the M centres (r.N = M, r.max_nn = 0: the cut is taken here, on neighbour entries); N: the support's size
struct SpRows { RwRows r; int N, max_nn; const int* self; const float* c4; const float* xyz4; };

struct SpNormals { SpRows s; long total; const float* view; float* normals; float* curv; };              // total = B M
struct SpSpfh { SpRows s; const float* normals; const float* cnormals; long total; unsigned* spfh; };
struct SpMark { SpRows s; long total; int* need; };
struct SpSlot { const int* need; const int* blkcnt; int N, nblk; int* slot; };
struct SpFpfh { SpRows s; const int* slot; const unsigned* sspfh; const unsigned* cspfh; int R; long total; float* fpfh; };

__device__ __forceinline__ bool sp_finite(const f32x4& c) { return rw_finite(c[0]) && rw_finite(c[1]) && rw_finite(c[2]); }

// Centre i of cloud b: its row (empty where the centre is not finite), its position, its self index.  -> the row can be read
__device__ __forceinline__ bool sp_centre(const SpRows& s, long b, int i, const int*& nb, int& L, f32x4& c, bool& fin, int& self) {
  const bool ok = rw_row(s.r, b, i, nb, L);
  const size_t g = (size_t)b * s.r.N + i;
  c = ld4(s.c4 + g * 4);
  fin = sp_finite(c);
  self = s.self ? s.self[g] : -1;
  if (!fin) L = 0;
  return ok;
}

__global__ __launch_bounds__(RW_BLOCK) void support_normals_kernel(SpNormals p) {
  const long g = (long)blockIdx.x * RW_BLOCK + threadIdx.x;
  if (g >= p.total) return;
  const int M = p.s.r.N, N = p.s.N, cut = p.s.max_nn;
  const long b = g / M;
  const int i = (int)(g - b * M);
  const float* rows = p.s.xyz4 + (size_t)b * N * 4;
  const int* nb;
  int L, self;
  f32x4 c;
  bool fin;
  const bool ok = sp_centre(p.s, b, i, nb, L, c, fin, self);
  NmSums s;
  int m = 0, taken = 0;
  for (int j = 0; j < L; ++j) {
    const int e = nb[j];
    if ((unsigned)e >= (unsigned)N) continue;              // skipped: it counts as nothing
    s.add(ld4(rows + (size_t)e * 4), c);
    ++m;
    if (e != self && ++taken == cut) break;                // behind the max_nn-th neighbour entry (cut == 0: never)
  }
  float n0 = 0.f, n1 = 0.f, n2 = 1.f, cv = 0.f;            // m < 3: fewer than three points define no plane
  if (m >= 3) nm_point(s, (double)m, c, p.view ? p.view + (size_t)b * 3 : nullptr, n0, n1, n2, cv);
  if (!ok || !fin) n0 = n1 = n2 = cv = rw_nan();
  float* out = p.normals + (size_t)b * 3 * M + i;
  out[0] = n0; out[M] = n1; out[2 * (size_t)M] = n2;
  if (p.curv) p.curv[g] = cv;
}

__global__ __launch_bounds__(RW_BLOCK) void support_spfh_lane_kernel(SpSpfh p) {
  __shared__ unsigned cnt[3 * RW_BINS][RW_BLOCK];          // a column a lane: its own 33 counters
  const int tid = threadIdx.x;
  const long g = (long)blockIdx.x * RW_BLOCK + tid;
  if (g >= p.total) return;                                // (no barrier below: a lane touches its own column alone)
  const int M = p.s.r.N, N = p.s.N, cut = p.s.max_nn;
  const long b = g / M;
  const int i = (int)(g - b * M);
  const float* rows = p.s.xyz4 + (size_t)b * N * 4;
  const float* nrm = p.normals + (size_t)b * 3 * N;
  const float* cn = p.cnormals + (size_t)b * 3 * M;
  const int* nb;
  int L, self;
  f32x4 c;
  bool fin;
  sp_centre(p.s, b, i, nb, L, c, fin, self);               // (a row that cannot be read is empty: zero words)
#pragma unroll
  for (int h = 0; h < 3 * RW_BINS; ++h) cnt[h][tid] = 0u;
  const float m0 = cn[i], m1 = cn[M + i], m2 = cn[2 * (size_t)M + i];
  const bool me_ok = rw_finite(m0) && rw_finite(m1) && rw_finite(m2);
  unsigned n = 0;
  int taken = 0;
  for (int j = 0; j < L; ++j) {
    const int e = nb[j];
    if ((unsigned)e >= (unsigned)N || e == self) continue;
    const f32x4 q = ld4(rows + (size_t)e * 4);
    int b0, b1, b2;
    if (rw_pair(c, m0, m1, m2, me_ok, q, nrm[e], nrm[N + e], nrm[2 * (size_t)N + e], b0, b1, b2)) {
      cnt[b0][tid] += 1u;
      cnt[RW_BINS + b1][tid] += 1u;
      cnt[2 * RW_BINS + b2][tid] += 1u;
      ++n;
    }
    if (++taken == cut) break;
  }
  uint4* out = reinterpret_cast<uint4*>(p.spfh + (size_t)g * RW_WORDS);
#pragma unroll
  for (int grp = 0; grp < 3; ++grp) {
    const int o = grp * RW_BINS;
    out[3 * grp] = make_uint4(cnt[o][tid], cnt[o + 1][tid], cnt[o + 2][tid], cnt[o + 3][tid]);
    out[3 * grp + 1] = make_uint4(cnt[o + 4][tid], cnt[o + 5][tid], cnt[o + 6][tid], cnt[o + 7][tid]);
    out[3 * grp + 2] = make_uint4(cnt[o + 8][tid], cnt[o + 9][tid], cnt[o + 10][tid], n);
  }
}

__global__ __launch_bounds__(RW_BLOCK) void support_spfh_wave_kernel(SpSpfh p) {
  __shared__ unsigned cnt[RW_WAVES][3 * RW_BINS + 3];      // a wave's 33 counters, then c_i
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const long g = (long)blockIdx.x * RW_WAVES + w;          // the wave's centre
  const bool live = g < p.total;
  if (lane < 3 * RW_BINS + 3) cnt[w][lane] = 0u;
  __syncthreads();
  if (live) {
    const int M = p.s.r.N, N = p.s.N, cut = p.s.max_nn;
    const long b = g / M;
    const int i = (int)(g - b * M);
    const float* rows = p.s.xyz4 + (size_t)b * N * 4;
    const float* nrm = p.normals + (size_t)b * 3 * N;
    const float* cn = p.cnormals + (size_t)b * 3 * M;
    const int* nb;
    int L, self;
    f32x4 c;
    bool fin;
    sp_centre(p.s, b, i, nb, L, c, fin, self);
    const float m0 = cn[i], m1 = cn[M + i], m2 = cn[2 * (size_t)M + i];
    const bool me_ok = rw_finite(m0) && rw_finite(m1) && rw_finite(m2);
    unsigned n = 0;
    int base = 0;                                          // neighbour entries in front of this chunk (wave-uniform)
    for (int j0 = 0; j0 < L && (cut == 0 || base < cut); j0 += 64) {
      const int j = j0 + lane;
      const int e = j < L ? nb[j] : -1;
      const bool nbr = (unsigned)e < (unsigned)N && e != self;
      const unsigned long long bal = __ballot(nbr);
      const int rank = base + __popcll(bal & ((1ull << lane) - 1ull));
      base += __popcll(bal);
      if (nbr && (cut == 0 || rank < cut)) {               // (the ballot above is the round's one wave operation)
        const f32x4 q = ld4(rows + (size_t)e * 4);
        int b0, b1, b2;
        if (rw_pair(c, m0, m1, m2, me_ok, q, nrm[e], nrm[N + e], nrm[2 * (size_t)N + e], b0, b1, b2)) {
          atomicAdd(&cnt[w][b0], 1u);                      // integer LDS atomics: the counts do not depend on the order
          atomicAdd(&cnt[w][RW_BINS + b1], 1u);
          atomicAdd(&cnt[w][2 * RW_BINS + b2], 1u);
          ++n;
        }
      }
    }
    if (n) atomicAdd(&cnt[w][3 * RW_BINS], n);
  }
  __syncthreads();
  if (live && lane < RW_WORDS) {
    const int grp = lane / 12, s = lane - grp * 12;
    p.spfh[(size_t)g * RW_WORDS + lane] = s == RW_BINS ? cnt[w][3 * RW_BINS] : cnt[w][grp * RW_BINS + s];
  }
}

__global__ __launch_bounds__(RW_BLOCK) void support_zero_kernel(int* p, long n) {
  const long g = (long)blockIdx.x * RW_BLOCK + threadIdx.x;
  if (g < n) p[g] = 0;
}

__global__ __launch_bounds__(RW_BLOCK) void support_mark_kernel(SpMark p) {
  const long g = (long)blockIdx.x * RW_BLOCK + threadIdx.x;
  if (g >= p.total) return;
  const int M = p.s.r.N, N = p.s.N, cut = p.s.max_nn;
  const long b = g / M;
  const int i = (int)(g - b * M);
  const int* nb;
  int L, self;
  f32x4 c;
  bool fin;
  sp_centre(p.s, b, i, nb, L, c, fin, self);
  int* need = p.need + (size_t)b * N;
  int taken = 0;
  for (int j = 0; j < L; ++j) {
    const int e = nb[j];
    if ((unsigned)e >= (unsigned)N || e == self) continue;
    need[e] = 1;
    if (++taken == cut) break;
  }
}

__global__ __launch_bounds__(RW_BLOCK) void support_slot_kernel(SpSlot p) {
  __shared__ int wcnt[RW_BLOCK / 64];
  const int t = threadIdx.x;
  const int b = (int)(blockIdx.x / (unsigned)p.nblk), blk = (int)(blockIdx.x % (unsigned)p.nblk);
  const int i = blk * RW_BLOCK + t;
  const size_t row = (size_t)b * p.N;
  const bool keep = i < p.N && p.need[row + i] > 0;
  int kept;
  const int rank = wg_rank(keep, t, wcnt, &kept);
  if (i < p.N) p.slot[row + i] = keep ? p.blkcnt[(size_t)b * p.nblk + blk] + rank : -1;
}

__global__ __launch_bounds__(RW_BLOCK) void support_fpfh_kernel(SpFpfh p) {
  const long t = (long)blockIdx.x * RW_BLOCK + threadIdx.x;
  if (t >= p.total) return;                                // total = 3 B M
  const int M = p.s.r.N, N = p.s.N, cut = p.s.max_nn, R = p.R;
  const long bg = t / M;                                   // (cloud, group)
  const int i = (int)(t - bg * M);
  const long b = bg / 3;
  const int grp = (int)(bg - b * 3);
  const float* rows = p.s.xyz4 + (size_t)b * N * 4;
  const unsigned* sp = p.sspfh + (size_t)b * R * RW_WORDS + grp * 12;
  const int* slot = p.slot ? p.slot + (size_t)b * N : nullptr;
  const int* nb;
  int L, self;
  f32x4 c;
  bool fin;
  const bool ok = sp_centre(p.s, b, i, nb, L, c, fin, self);
  double acc[RW_BINS];
#pragma unroll
  for (int h = 0; h < RW_BINS; ++h) acc[h] = 0.0;
  double sum = 0.0;
  int taken = 0;
  for (int j = 0; j < L; ++j) {
    const int e = nb[j];
    if ((unsigned)e >= (unsigned)N || e == self) continue;
    const bool last = ++taken == cut;
    const int r = slot ? slot[e] : e;
    if ((unsigned)r < (unsigned)R) {
      const f32x4 q = ld4(rows + (size_t)e * 4);
      const uint4* hp = reinterpret_cast<const uint4*>(sp + (size_t)r * RW_WORDS);
      const uint4 h0 = hp[0], h1 = hp[1], h2 = hp[2];
      const double dx = (double)(q[0] - c[0]), dy = (double)(q[1] - c[1]), dz = (double)(q[2] - c[2]);
      const double d2 = (dx * dx + dy * dy) + dz * dz;
      const unsigned cj = h2.w;
      if (d2 > 0.0 && d2 < RW_INF && cj != 0u) {
        const unsigned hj[RW_BINS] = {h0.x, h0.y, h0.z, h0.w, h1.x, h1.y, h1.z, h1.w, h2.x, h2.y, h2.z};
        const double s = 100.0 / (double)cj;
#pragma unroll
        for (int h = 0; h < RW_BINS; ++h) {
          const double val = ((double)hj[h] * s) / d2;
          acc[h] += val;
          sum += val;
        }
      }
    }
    if (last) break;
  }
  const uint4* op = reinterpret_cast<const uint4*>(p.cspfh + ((size_t)b * M + i) * RW_WORDS + grp * 12);
  const uint4 o0 = op[0], o1 = op[1], o2 = op[2];
  const unsigned own[RW_BINS] = {o0.x, o0.y, o0.z, o0.w, o1.x, o1.y, o1.z, o1.w, o2.x, o2.y, o2.z};
  const unsigned ci = o2.w;
  const double scale = 100.0 / sum;
  const double so = 100.0 / (double)ci;
  float* out = p.fpfh + ((size_t)b * 33 + (size_t)grp * RW_BINS) * M + i;
#pragma unroll
  for (int h = 0; h < RW_BINS; ++h) {
    const double a = sum != 0.0 ? acc[h] * scale : acc[h];
    const double mine = ci != 0u ? (double)own[h] * so : 0.0;
    out[(size_t)h * M] = ok && fin ? (float)(a + mine) : rw_nan();
  }
}

// What the entry points and the form query ask of the numbers (R: the histogram rows of the second pass, M elsewhere)
int sp_numbers(int B, int N, int M, int R, int capacity, int max_nn, int variant) {
  if (B < 1 || capacity < 0 || max_nn < 0) return VCR_EINVAL;
  if (variant != 0 && variant != VCR_SUPPORT_LANE && variant != VCR_SUPPORT_WAVE) return VCR_EINVAL;
  const int lim = VCR_SUPPORT_MAX_N;
  if (N < 1 || N > lim || M < 1 || M > lim || R < 1 || R > lim) return VCR_EUNSUPPORTED;
  const long top = 1L << 31;
  if ((long)B * N >= top || (long)B * M >= top || (long)B * R >= top || (long)B * capacity >= top) return VCR_EUNSUPPORTED;
  return VCR_OK;
}

// ... and of the pointers every call takes: `out` the mandatory output, a16 one more that must be 16-B aligned (or NULL)
int sp_check(const void* xyz4, const void* c4, const void* idx, const void* row_start, const void* total, const void* out,
             const void* a16, int B, int N, int M, int R, int capacity, int max_nn, int variant) {
  if (!xyz4 || !c4 || !row_start || !total || !out || (!idx && capacity != 0)) return VCR_EINVAL;
  if ((((uintptr_t)xyz4) & 15) || (((uintptr_t)c4) & 15) || (((uintptr_t)a16) & 15)) return VCR_EINVAL;
  return sp_numbers(B, N, M, R, capacity, max_nn, variant);
}

// THE one place that decides the first pass's form: the number of centres and the row length the host can see
int sp_form(int B, int M, int capacity, int max_nn, int variant) {
  if (variant) return variant;
  if ((long)B * M <= VCR_SUPPORT_WAVE_CENTRES) return VCR_SUPPORT_WAVE;     // a lane a centre would leave most of the device idle
  long est = (long)capacity / M;
  if (max_nn > 0 && est > max_nn) est = max_nn;
  return est >= VCR_SUPPORT_WAVE_SPFH ? VCR_SUPPORT_WAVE : VCR_SUPPORT_LANE;
}

template <class A>
SpRows sp_rows(const A& a) {
  return SpRows{RwRows{a.idx, (const i64*)a.row_start, (const i64*)a.total, a.M, a.capacity, 0}, a.N, a.max_nn, a.self, a.c4, a.xyz4};
}

size_t sp_up(size_t v) { return (v + 255) & ~(size_t)255; }

struct SpNeedPlan { int nblk; size_t blk_off, bytes; };    // workspace: need int [B,N] | blkcnt int [B,nblk]

int sp_need_plan(const vcr_support_needed_args& a, SpNeedPlan* p) {
  const int e = sp_check(a.xyz4, a.c4, a.idx, a.row_start, a.total, a.points, nullptr, a.B, a.N, a.M, 1, a.capacity, a.max_nn, 0);
  if (e) return e;
  if (!a.count || !a.index || !a.slot) return VCR_EINVAL;
  p->nblk = (a.N + NN_BLOCK - 1) / NN_BLOCK;
  p->blk_off = sp_up(sizeof(int) * (size_t)a.B * a.N);
  p->bytes = p->blk_off + sp_up(sizeof(int) * (size_t)a.B * p->nblk);
  return VCR_OK;
}

}  // namespace

extern "C" int vcr_support_form(int B, int N, int M, int capacity, int max_nn, int cu_count, int variant, int* spfh_form) {
  if (cu_count < 0) return VCR_EINVAL;
  const int e = sp_numbers(B, N, M, 1, capacity, max_nn, variant);
  if (e) return e;
  if (spfh_form) *spfh_form = sp_form(B, M, capacity, max_nn, variant);
  return VCR_OK;
}

extern "C" int vcr_support_normals_f32(const vcr_support_normals_args* ua, vcr_stream_t stream) {
  vcr_support_normals_args a;
  if (vcr_take_args(ua, &a, offsetof(vcr_support_normals_args, curvature))) return VCR_EINVAL;
  const int e = sp_check(a.xyz4, a.c4, a.idx, a.row_start, a.total, a.normals, nullptr, a.B, a.N, a.M, 1, a.capacity, a.max_nn, 0);
  if (e) return e;
  const long total = (long)a.B * a.M;
  const SpRows s = sp_rows(a);
  const SpNormals k{s, total, a.viewpoint, a.normals, a.curvature};
  hipLaunchKernelGGL(support_normals_kernel, dim3(rw_blocks(total, RW_BLOCK)), dim3(RW_BLOCK), 0, (hipStream_t)stream, k);
  const int rc = VCR_LAUNCH_RC();
  return rc ? rc : rw_void(s.r, a.B, a.normals, 3L * a.M, a.curvature, a.M, nullptr, 0, (hipStream_t)stream);
}

extern "C" int vcr_support_spfh_f32(const vcr_support_spfh_args* ua, vcr_stream_t stream) {
  vcr_support_spfh_args a;
  if (vcr_take_args(ua, &a, sizeof(vcr_support_spfh_args))) return VCR_EINVAL;
  const int e = sp_check(a.xyz4, a.c4, a.idx, a.row_start, a.total, a.spfh, a.spfh, a.B, a.N, a.M, 1, a.capacity, a.max_nn, a.variant);
  if (e) return e;
  if (!a.normals || !a.centre_normals) return VCR_EINVAL;
  const long total = (long)a.B * a.M;
  const SpRows s = sp_rows(a);
  const SpSpfh k{s, a.normals, a.centre_normals, total, a.spfh};
  if (sp_form(a.B, a.M, a.capacity, a.max_nn, a.variant) == VCR_SUPPORT_WAVE)
    hipLaunchKernelGGL(support_spfh_wave_kernel, dim3(rw_blocks(total, RW_WAVES)), dim3(RW_BLOCK), 0, (hipStream_t)stream, k);
  else
    hipLaunchKernelGGL(support_spfh_lane_kernel, dim3(rw_blocks(total, RW_BLOCK)), dim3(RW_BLOCK), 0, (hipStream_t)stream, k);
  const int rc = VCR_LAUNCH_RC();
  return rc ? rc : rw_void(s.r, a.B, nullptr, 0, nullptr, 0, a.spfh, (long)RW_WORDS * a.M, (hipStream_t)stream);
}

extern "C" size_t vcr_support_needed_workspace_bytes(const vcr_support_needed_args* ua, int cu_count) {
  vcr_support_needed_args a;
  SpNeedPlan p;
  if (vcr_take_args(ua, &a, sizeof(vcr_support_needed_args)) || cu_count < 0) return 0;
  return sp_need_plan(a, &p) ? 0 : p.bytes;
}

extern "C" int vcr_support_needed_f32(const vcr_support_needed_args* ua, void* workspace, size_t workspace_bytes,
                                      vcr_stream_t stream) {
  vcr_support_needed_args a;
  if (vcr_take_args(ua, &a, sizeof(vcr_support_needed_args))) return VCR_EINVAL;
  SpNeedPlan p;
  const int e = sp_need_plan(a, &p);
  if (e) return e;
  if (!workspace || (((uintptr_t)workspace) & 15)) return VCR_EINVAL;
  if (workspace_bytes < p.bytes) return VCR_EWORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  unsigned char* w = reinterpret_cast<unsigned char*>(workspace);
  int* need = reinterpret_cast<int*>(w);
  int* blkcnt = reinterpret_cast<int*>(w + p.blk_off);
  const long points = (long)a.B * a.N, centres = (long)a.B * a.M;
  const SpRows s = sp_rows(a);
  hipLaunchKernelGGL(support_zero_kernel, dim3(rw_blocks(points, RW_BLOCK)), dim3(RW_BLOCK), 0, st, need, points);
  int rc = VCR_LAUNCH_RC();
  if (rc) return rc;
  const SpMark mk{s, centres, need};
  hipLaunchKernelGGL(support_mark_kernel, dim3(rw_blocks(centres, RW_BLOCK)), dim3(RW_BLOCK), 0, st, mk);
  if ((rc = VCR_LAUNCH_RC())) return rc;
  if ((rc = rw_void(s.r, a.B, nullptr, 0, nullptr, 0, reinterpret_cast<unsigned*>(need), a.N, st))) return rc;   // not served: nothing needed
  OlTail tl{};
  tl.cnt = need; tl.nb_points = 0;                         // keep: need > 0
  tl.rows = a.xyz4;
  tl.N = a.N; tl.nblk = p.nblk; tl.blkcnt = blkcnt;
  tl.points = a.points; tl.count = a.count; tl.index = a.index;
  const unsigned point_grid = (unsigned)((long)a.B * p.nblk);
  hipLaunchKernelGGL(outlier_mark_kernel, dim3(point_grid), dim3(NN_BLOCK), 0, st, tl);
  if ((rc = VCR_LAUNCH_RC())) return rc;
  if ((rc = ol_compact(tl, a.B, point_grid, st))) return rc;
  const SpSlot sl{need, blkcnt, a.N, p.nblk, a.slot};
  hipLaunchKernelGGL(support_slot_kernel, dim3(point_grid), dim3(RW_BLOCK), 0, st, sl);
  return VCR_LAUNCH_RC();
}

extern "C" int vcr_support_fpfh_f32(const vcr_support_fpfh_args* ua, vcr_stream_t stream) {
  vcr_support_fpfh_args a;
  if (vcr_take_args(ua, &a, sizeof(vcr_support_fpfh_args))) return VCR_EINVAL;
  const int e = sp_check(a.xyz4, a.c4, a.idx, a.row_start, a.total, a.fpfh, a.support_spfh, a.B, a.N, a.M, a.R, a.capacity, a.max_nn, 0);
  if (e) return e;
  if (!a.support_spfh || !a.centre_spfh || (((uintptr_t)a.centre_spfh) & 15)) return VCR_EINVAL;
  const long total = (long)a.B * a.M;
  const SpRows s = sp_rows(a);
  const SpFpfh k{s, a.slot, a.support_spfh, a.centre_spfh, a.R, 3 * total, a.fpfh};   // < 3 * 2^31 lanes
  hipLaunchKernelGGL(support_fpfh_kernel, dim3(rw_blocks(3 * total, RW_BLOCK)), dim3(RW_BLOCK), 0, (hipStream_t)stream, k);
  const int rc = VCR_LAUNCH_RC();
  return rc ? rc : rw_void(s.r, a.B, a.fpfh, 33L * a.M, nullptr, 0, nullptr, 0, (hipStream_t)stream);
}

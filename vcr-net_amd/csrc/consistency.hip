// A pose from mostly wrong correspondences (include/consistency/vcr_hip_consistency.h): pairwise
// length-consistency voting over vcr_ransac_f32's pair list.  Fourteen launches, no host synchronisation, no atomics:
//   consistency_pairs_kernel   (its body: corr_pairs.h, shared with ransac.hip and fgr.hip) the pair list, gathered ONCE into
//                              32-B rows (sx, sy, sz, source index | tx, ty, tz, 0); M behind them.
//   consistency_degree_kernel<Q, PRE>  the hot path, M^2 tests: 256 lanes x Q pairs per lane, their two points in registers,
//                              against one of the S segments of the SAME list.  The streamed row's address is the same for every
//                              lane of the workgroup (blockIdx and the loop counter alone), so it arrives through SCALAR loads
//                              and the differences take it as their scalar operand -- featnn_scan_kernel's shape: no LDS, no
//                              barrier.  Per test two fmaf chains, two correctly rounded square roots (the definition), four
//                              compares; the count stays in the lane.  PRE: the same decision from the raw hardware roots
//                              wherever the rounding cannot matter (cs_compatible_pre); the plan takes it from two pairs a
//                              lane.  Segments are cut from M on the device, the grid from Ns on the host; a workgroup whose
//                              pairs lie behind M leaves at once.
//   consistency_merge_kernel   one lane per pair position: the S partial counts added (integers: any S, any Q, the same bits),
//                              deg in the source's numbering, and the sort's key 0x1FFFF - deg beside the position as its value
//                              (0x3FFFF behind M: such slots sort last).
//   rs_hist / rs_scan / rs_scatter (radix_sort.h) twice: the stable sort of the 18-bit keys in two passes of 9 bits.
//   consistency_kept_kernel    one lane per rank: the first P = min(M, keep) positions' rows gathered to [keep][8], kept.
//   consistency_adj_kernel     one wave per rank r, the lane as the column: per 64 columns one test a lane and one ballot; lane w
//                              keeps word w and the row leaves as one coalesced store.  A row of 4096 bits is one word a lane.
//   consistency_seed_kernel    one workgroup per seed r: its four waves share the columns c set in adj[r] -- one &, one 64-bit
//                              popcount a lane and a wave sum each -- into w[r][.] in LDS; the row's maximum; the members' bits
//                              by ballot; then wave 0 runs the rigid step on the members: lane l is chain l of the header's sum
//                              order, the butterfly leaves the fifteen sums in every lane, svd3.h's quad Jacobi and tail -- the
//                              text of every solve of the library -- and the fp32 pose.
//   consistency_count_kernel   one LANE per seed, its pose in twelve registers, over one segment of 1024 of ALL M rows, which
//                              arrive through scalar loads (ransac_count_kernel's loop and its expressions: rs_d2 of
//                              corr_pairs.h); the segments' counts are added by the last launch.
//   consistency_best_kernel    one workgroup per cloud: ransac_best_kernel's 64-bit key over the seeds, and the outputs.
// Every result is a function of the cloud alone; all writes are plain vector stores.
#include "seg_scan.h"
#include "corr_pairs.h"
#include "radix_sort.h"
#include "svd3.h"
#include "../../include/consistency/vcr_hip_consistency.h"

namespace {

constexpr int CS_MAX_SPLITS = 128;
constexpr int CS_MIN_SEGMENT = 64;                         // the plan cuts no segment shorter than this (a forced split may)
constexpr int CS_FILL_PER_CU = 16;                         // workgroups per CU the plan cuts the work into, where it can
constexpr SegLimits CS_LIMITS{CS_MIN_SEGMENT, CS_FILL_PER_CU, CS_MAX_SPLITS};
constexpr int CS_BITS = 9, CS_E = 4, CS_R = 1 << CS_BITS;  // the sort: two passes cover the 18-bit key
constexpr int CS_SORT_PASSES = 2;
constexpr int CS_MAX_KEEP = VCR_CONSISTENCY_MAX_KEEP;
constexpr int CS_COUNT_SEG = 1024;                         // rows of the pair list a count workgroup takes
constexpr unsigned CS_KEY_TOP = 0x1FFFFu, CS_KEY_NONE = 0x3FFFFu;
constexpr int CS_VARIANT_PRETEST_ON = 0x10, CS_VARIANT_PRETEST_OFF = 0x20, CS_VARIANT_PRETEST = 0x30;
constexpr int CS_PLAN_PRETEST_FROM_Q = 2;                  // the plan runs the pre-test from this many pairs a lane (cs_plan)
static_assert(RS_MAX_N - 1 <= (int)CS_KEY_TOP, "a degree fits the key");

__global__ __launch_bounds__(RS_BLOCK) void consistency_pairs_kernel(RsPairs p) { rs_pairs_body(p); }

// compatible(a, b) of the header from the two rows' points; the caller excludes a == b
__device__ __forceinline__ bool cs_compatible(const f32x4& sa, const f32x4& ta, const f32x4& sb, const f32x4& tb, float tau,
                                              float min_len2) {
  const float ds2 = rs_len2(sa, sb), dt2 = rs_len2(ta, tb);
  const float ds = __builtin_sqrtf(ds2), dt = __builtin_sqrtf(dt2);    // (correctly rounded: the build gives no licence)
  return fabsf(ds - dt) <= tau && ds2 >= min_len2 && dt2 >= min_len2;  // a NaN fails
}

// The same decision behind a pre-test: a correctly rounded square root is v_sqrt_f32 and a dozen
// instructions of correction, twice a test, and almost no test needs them.  Let a', b' be the RAW instruction's roots (within
// 1 ulp for arguments of 2^-96 and above), t = |a' - b'| and band = 2^-20 (a' + b').  The definition's roots lie within 1.5 ulp
// of a', b' and the two subtractions round by 2^-24 of their results, so the definition's |ds - dt| lies within
// 2.5 x 2^-23 (a' + b') = 0.32 band of t; the roundings of tau -+ band are below 2^-24 (tau + band), which the rest of the
// band covers wherever a' + b' >= tau / 10 -- and below that t <= a' + b' lies under both limits.  Hence
//   t <= tau - band   is compatible whatever the roundings,   !(t <= tau + band)   is not (a NaN lands here),
// and only a test between the two -- about one in 10^6 on lengths spread over a unit cube --, or with an argument below 2^-96
// (zero included: two pairs that share a point), runs the definition's expression -- then for all Q pairs of its lane, behind
// one branch a streamed row.  The length floor reads ds2, dt2 as before.
template <int Q>
__device__ __forceinline__ void cs_compatible_pre(const f32x4 (&sa)[Q], const f32x4 (&ta)[Q], const f32x4& sb, const f32x4& tb,
                                                  float tau, float min_len2, bool (&ok)[Q]) {
  float ds2[Q], dt2[Q];
  bool unsure = false;
#pragma unroll
  for (int q = 0; q < Q; ++q) {
    ds2[q] = rs_len2(sa[q], sb); dt2[q] = rs_len2(ta[q], tb);
    const float a = __builtin_amdgcn_sqrtf(ds2[q]), b = __builtin_amdgcn_sqrtf(dt2[q]);
    const float t = fabsf(a - b), band = 0x1p-20f * (a + b);
    ok[q] = t <= tau - band;
    unsure = unsure || (ok[q] != (t <= tau + band)) || fminf(ds2[q], dt2[q]) < 0x1p-96f;
  }
  if (unsure) {                                            // ONE branch a row, rare, skipped by a wave none of whose lanes needs it
#pragma unroll
    for (int q = 0; q < Q; ++q) ok[q] = fabsf(__builtin_sqrtf(ds2[q]) - __builtin_sqrtf(dt2[q])) <= tau;
  }
#pragma unroll
  for (int q = 0; q < Q; ++q) ok[q] = ok[q] && ds2[q] >= min_len2 && dt2[q] >= min_len2;
}

struct CsDegree {
  const float* rows; const int* M;                         // [B][Ns][8], [B]
  int B, Ns, S, nblk;                                      // nblk: workgroups per cloud and segment = ceil(Ns / (256 Q))
  float tau, min_len2;
  int* part;                                               // [S][B][Ns]
};

template <int Q, bool PRE>
__global__ __launch_bounds__(RS_BLOCK) void consistency_degree_kernel(CsDegree p) {
  const int t = threadIdx.x;
  int s, blk, b;
  seg_workgroup(blockIdx.x, p.S, p.nblk, &s, &blk, &b);
  const int M = p.M[b];
  if (blk * (RS_BLOCK * Q) >= M) return;                   // (workgroup-uniform) its pairs lie behind the list's end
  const float* __restrict__ rows = p.rows + (size_t)b * p.Ns * 8;      // (workgroup-uniform, like j below: scalar loads)

  f32x4 sa[Q], ta[Q];
  int at[Q], cnt[Q];
#pragma unroll
  for (int q = 0; q < Q; ++q) {
    at[q] = blk * (RS_BLOCK * Q) + q * RS_BLOCK + t;
    const int c = at[q] < M ? at[q] : M - 1;               // a lane without a pair scans a copy of the last one, stores nothing
    sa[q] = ld4(rows + (size_t)c * 8);
    ta[q] = ld4(rows + (size_t)c * 8 + 4);
    cnt[q] = 0;
  }
  int lo, hi;
  seg_range(s, (M + p.S - 1) / p.S, M, &lo, &hi);          // the segments are cut from M: Ns sized the grid alone
  const float tau = p.tau, min_len2 = p.min_len2;
  for (int j = lo; j < hi; ++j) {
    const float* __restrict__ r = rows + (size_t)j * 8;
    const f32x4 sb = {r[0], r[1], r[2], 0.f}, tb = {r[4], r[5], r[6], 0.f};
    bool ok[Q];
    if (PRE) {
      cs_compatible_pre<Q>(sa, ta, sb, tb, tau, min_len2, ok);
    } else {
#pragma unroll
      for (int q = 0; q < Q; ++q) ok[q] = cs_compatible(sa[q], ta[q], sb, tb, tau, min_len2);
    }
#pragma unroll
    for (int q = 0; q < Q; ++q) cnt[q] += (ok[q] && j != at[q]) ? 1 : 0;
  }
  const size_t out = ((size_t)s * p.B + b) * (size_t)p.Ns;
#pragma unroll
  for (int q = 0; q < Q; ++q)
    if (at[q] < M) p.part[out + at[q]] = cnt[q];
}

struct CsMerge {
  const int* part; const float* rows; const int* M; const int* corr;
  int B, Ns, Nt, S; long total;                            // total = B Ns
  int* deg;                                                // optional [B][Ns]
  rs_u64* key; unsigned* val; int* npass;                  // the sort's buffer 0, [B][Ns] each; [B]
};

__global__ __launch_bounds__(RS_BLOCK) void consistency_merge_kernel(CsMerge p) {
  const long g = (long)blockIdx.x * RS_BLOCK + threadIdx.x;
  if (g >= p.total) return;
  const long b = g / p.Ns;
  const int n = (int)(g - b * p.Ns);
  const int M = p.M[b];
  unsigned key = CS_KEY_NONE;
  if (n < M) {
    int d = 0;
    for (int s = 0; s < p.S; ++s) d += p.part[((size_t)s * p.B + b) * (size_t)p.Ns + n];
    key = CS_KEY_TOP - (unsigned)d;                        // d <= M - 1 < 2^17
    if (p.deg) p.deg[b * p.Ns + __float_as_int(p.rows[(size_t)g * 8 + 3])] = d;
  }
  if (p.deg && !((unsigned)p.corr[g] < (unsigned)p.Nt)) p.deg[g] = -1;   // (a point is a pair or not: the two writes never meet)
  p.key[g] = key;
  p.val[g] = (unsigned)n;
  if (n == 0) p.npass[b] = CS_SORT_PASSES;
}

struct CsKept {
  const unsigned* order; const float* rows; const int* M;  // the sorted positions [B][Ns]
  int Ns, keep; long total;                                // total = B keep
  float* krows; int* kept;                                 // [B][keep][8]; optional [B][keep]
};

__global__ __launch_bounds__(RS_BLOCK) void consistency_kept_kernel(CsKept p) {
  const long g = (long)blockIdx.x * RS_BLOCK + threadIdx.x;
  if (g >= p.total) return;
  const long b = g / p.keep;
  const int r = (int)(g - b * p.keep);
  const int M = p.M[b], P = M < p.keep ? M : p.keep;
  int src = -1;
  if (r < P) {
    const unsigned pos = p.order[(size_t)b * p.Ns + r];    // < M: the slots behind M sort last
    const float* row = p.rows + ((size_t)b * p.Ns + pos) * 8;
    const f32x4 s4 = ld4(row), t4 = ld4(row + 4);
    st4(p.krows + (size_t)g * 8, s4);
    st4(p.krows + (size_t)g * 8 + 4, t4);
    src = __float_as_int(s4[3]);
  }
  if (p.kept) p.kept[g] = src;
}

struct CsAdj {
  const float* krows; const int* M;
  int keep, W; long total;                                 // W = keep / 64; total = B keep (waves)
  float tau, min_len2;
  rs_u64* adj;                                             // [B][keep][W]
};

__global__ __launch_bounds__(RS_BLOCK) void consistency_adj_kernel(CsAdj p) {
  const int lane = threadIdx.x & 63;
  const long g = (long)blockIdx.x * WG_WAVES + (threadIdx.x >> 6);     // (b, r): total is a multiple of WG_WAVES
  if (g >= p.total) return;
  const long b = g / p.keep;
  const int r = (int)(g - b * p.keep);
  const int M = p.M[b], P = M < p.keep ? M : p.keep;
  const float* krows = p.krows + (size_t)b * p.keep * 8;
  rs_u64 mine = 0ull;
  if (r < P) {                                             // (wave-uniform)
    const f32x4 sa = ld4(krows + (size_t)r * 8), ta = ld4(krows + (size_t)r * 8 + 4);
    for (int w = 0; w * 64 < P; ++w) {
      const int c = w * 64 + lane;
      bool ok = false;
      if (c < P && c != r) ok = cs_compatible(sa, ta, ld4(krows + (size_t)c * 8), ld4(krows + (size_t)c * 8 + 4), p.tau, p.min_len2);
      const rs_u64 word = __ballot(ok);
      mine = lane == w ? word : mine;
    }
  }
  if (lane < p.W) p.adj[(size_t)g * p.W + lane] = mine;
}

struct CsSeed {
  const float* krows; const int* M; const rs_u64* adj;
  int keep, W, seeds;
  float ratio;
  int* status; float* pose;                                // [B][seeds], [B][seeds][12]
  int* members; rs_u64* member;                            // optional [B][seeds], [B][seeds][W]
};

__global__ __launch_bounds__(RS_BLOCK) void consistency_seed_kernel(CsSeed p) {
  __shared__ rs_u64 sadj[CS_MAX_KEEP / 64], smem[CS_MAX_KEEP / 64];
  __shared__ int sw[CS_MAX_KEEP];
  __shared__ int wred[WG_WAVES];
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const int b = (int)(blockIdx.x / (unsigned)p.seeds), r = (int)(blockIdx.x % (unsigned)p.seeds);
  const int M = p.M[b], P = M < p.keep ? M : p.keep, W = p.W;
  const size_t slot = (size_t)b * p.seeds + r;
  float Pz[12] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (r >= P) {                                            // (workgroup-uniform) a slot behind the seeds
    if (t < W && p.member) p.member[slot * W + t] = 0ull;
    if (t == 0) {
      p.status[slot] = 1;
      if (p.members) p.members[slot] = 0;
      for (int e = 0; e < 12; ++e) p.pose[slot * 12 + e] = 0.f;
    }
    return;
  }
  const rs_u64* adj = p.adj + (size_t)b * p.keep * W;
  if (t < W) sadj[t] = adj[(size_t)r * W + t];
  __syncthreads();
  // second order: w[r][c] for the columns c set in adj[r], a wave a column
  const rs_u64 mine = lane < W ? sadj[lane] : 0ull;
  for (int c0 = wv * 4; c0 < P; c0 += 4 * WG_WAVES) {      // (wave-uniform) four columns a trip: their rows in flight together
    rs_u64 other[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int c = c0 + u;
      const bool on = c < P && ((sadj[c >> 6] >> (c & 63)) & 1ull) && lane < W;    // (c < keep: inside sadj)
      other[u] = on ? adj[(size_t)c * W + lane] : 0ull;
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      int v = __popcll(mine & other[u]);
#pragma unroll
      for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
      if (lane == 0 && c0 + u < P) sw[c0 + u] = v;
    }
  }
  __syncthreads();
  int wmax = 0;
  for (int c = t; c < P; c += RS_BLOCK) wmax = sw[c] > wmax ? sw[c] : wmax;
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) { const int u = __shfl_xor(wmax, o, 64); wmax = u > wmax ? u : wmax; }
  if (lane == 0) wred[wv] = wmax;
  __syncthreads();
  for (int k = 0; k < WG_WAVES; ++k) wmax = wred[k] > wmax ? wred[k] : wmax;
  const float floor_w = p.ratio * (float)wmax;             // fp32: one rounding
  for (int w = wv; w < W; w += WG_WAVES) {
    const int c = w * 64 + lane;
    const bool in = c == r || (c < P && ((sadj[w] >> lane) & 1ull) && (float)sw[c] >= floor_w);
    const rs_u64 word = __ballot(in);
    if (lane == 0) smem[w] = word;
  }
  __syncthreads();
  if (wv != 0) return;
  int n = lane < W ? __popcll(smem[lane]) : 0;
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) n += __shfl_xor(n, o, 64);
  if (lane < W && p.member) p.member[slot * W + lane] = smem[lane];
  if (lane == 0 && p.members) p.members[slot] = n;
  int status = 1;
  if (n >= 3) {                                            // (wave-uniform) the rigid step on the members: lane l = chain l
    const float* krows = p.krows + (size_t)b * p.keep * 8;
    double Sp[3] = {0., 0., 0.}, Sq[3] = {0., 0., 0.}, Spq[9] = {0., 0., 0., 0., 0., 0., 0., 0., 0.};
    for (int w = 0; w * 64 < P; ++w) {
      if (!((smem[w] >> lane) & 1ull)) continue;
      const float* row = krows + (size_t)(w * 64 + lane) * 8;
      const f32x4 s4 = ld4(row), q4 = ld4(row + 4);
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        Sp[i] += (double)s4[i];
        Sq[i] += (double)q4[i];
#pragma unroll
        for (int j = 0; j < 3; ++j) Spq[3 * i + j] += (double)s4[i] * (double)q4[j];
      }
    }
    bool finite = true;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
      for (int o = 32; o >= 1; o >>= 1) { Sp[i] += __shfl_xor(Sp[i], o, 64); Sq[i] += __shfl_xor(Sq[i], o, 64); }
      finite = finite && __builtin_isfinite(Sp[i]) && __builtin_isfinite(Sq[i]);
    }
#pragma unroll
    for (int e = 0; e < 9; ++e) {
#pragma unroll
      for (int o = 32; o >= 1; o >>= 1) Spq[e] += __shfl_xor(Spq[e], o, 64);
      finite = finite && __builtin_isfinite(Spq[e]);
    }
    const double inv_n = 1.0 / (double)n;
    double H[9];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j) H[3 * i + j] = Spq[3 * i + j] - (Sp[i] * Sq[j]) * inv_n;
    const int li = lane & 3;                               // every quad of the wave holds the same sums and solves alike
    double a[3], v[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      a[j] = li == 0 ? H[j] : li == 1 ? H[3 + j] : li == 2 ? H[6 + j] : 0.0;
      v[j] = li == j ? 1.0 : 0.0;
    }
    jacobi_sweeps_quad(a, v);
    double A[3][3], V[3][3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {                          // gather the rows (lane i of the quad = row i)
      A[0][j] = quad_get(a[j], 0); A[1][j] = quad_get(a[j], 1); A[2][j] = quad_get(a[j], 2);
      V[0][j] = quad_get(v[j], 0); V[1][j] = quad_get(v[j], 1); V[2][j] = quad_get(v[j], 2);
    }
    if (lane != 0) return;
    double R[9];
    svd3_finish(A, V, R);
    const double nan = __builtin_nan("");
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      const double tr = Sq[i] * inv_n - (R[3 * i] * (Sp[0] * inv_n) + R[3 * i + 1] * (Sp[1] * inv_n) + R[3 * i + 2] * (Sp[2] * inv_n));
      Pz[9 + i] = (float)(finite ? tr : nan);
    }
#pragma unroll
    for (int e = 0; e < 9; ++e) Pz[e] = (float)(finite ? R[e] : nan);
    bool ok = true;
#pragma unroll
    for (int e = 0; e < 12; ++e) ok = ok && __builtin_isfinite(Pz[e]);
    status = ok ? 0 : 3;
  }
  if (lane != 0) return;
  p.status[slot] = status;
#pragma unroll
  for (int e = 0; e < 12; ++e) p.pose[slot * 12 + e] = Pz[e];
}

struct CsCount {
  const float* rows; const int* M; const int* status; const float* pose;
  int Ns, seeds, nsb, nseg;                                // nsb = ceil(seeds / 64), nseg = ceil(Ns / CS_COUNT_SEG)
  float max_d2;
  int* part;                                               // [B][nseg][seeds]
};

__global__ __launch_bounds__(64) void consistency_count_kernel(CsCount p) {
  const unsigned k = blockIdx.x % (unsigned)p.nseg, rest = blockIdx.x / (unsigned)p.nseg;
  const int sb = (int)(rest % (unsigned)p.nsb), b = (int)(rest / (unsigned)p.nsb);
  const int r = sb * 64 + (int)threadIdx.x;
  if (r >= p.seeds) return;
  const size_t slot = (size_t)b * p.seeds + r;
  const int M = p.M[b];
  int count = 0;
  if (p.status[slot] == 0) {
    float P[12];
#pragma unroll
    for (int e = 0; e < 12; ++e) P[e] = p.pose[slot * 12 + e];
    const float* __restrict__ rows = p.rows + (size_t)b * p.Ns * 8;    // (workgroup-uniform, like j: scalar loads)
    const int lo = (int)k * CS_COUNT_SEG, hi = lo + CS_COUNT_SEG < M ? lo + CS_COUNT_SEG : M;
    for (int j = lo; j < hi; ++j) {
      const float* __restrict__ row = rows + (size_t)j * 8;
      count += rs_d2(P, row[0], row[1], row[2], row[4], row[5], row[6]) <= p.max_d2 ? 1 : 0;
    }
  }
  p.part[((size_t)b * p.nseg + k) * p.seeds + r] = count;
}

struct CsBest {
  const int* status; const float* pose; const int* part;
  int seeds, nseg;
  float* R_out; float* t_out; int* best_seed; int* inliers; int* seed_inliers;
};

__global__ __launch_bounds__(RS_BLOCK) void consistency_best_kernel(CsBest p) {
  __shared__ u64 wbest[WG_WAVES];
  const int t = threadIdx.x, b = blockIdx.x;
  u64 key = 0;                                             // a valid seed's key is above 0xFFFFF000
  for (int i = t; i < p.seeds; i += RS_BLOCK) {
    const size_t slot = (size_t)b * p.seeds + i;
    int c = -1;
    if (p.status[slot] == 0) {
      c = 0;
      for (int k = 0; k < p.nseg; ++k) c += p.part[((size_t)b * p.nseg + k) * p.seeds + i];
    }
    if (p.seed_inliers) p.seed_inliers[slot] = c;
    const u64 kk = c >= 0 ? ((u64)(unsigned)c << 32) | (u64)(0xFFFFFFFFu - (unsigned)i) : 0ull;
    key = kk > key ? kk : key;
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    const u64 other = __shfl_xor(key, o, 64);
    key = other > key ? other : key;
  }
  if ((t & 63) == 0) wbest[t >> 6] = key;
  __syncthreads();
  if (t != 0) return;
  for (int w = 1; w < WG_WAVES; ++w) key = wbest[w] > key ? wbest[w] : key;
  float P[12] = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f};
  int best = -1, inl = 0;
  if (key != 0ull) {
    best = (int)(0xFFFFFFFFu - (unsigned)(key & 0xFFFFFFFFull));
    inl = (int)(key >> 32);
    const float* pose = p.pose + ((size_t)b * p.seeds + best) * 12;
    for (int e = 0; e < 12; ++e) P[e] = pose[e];
  }
  for (int e = 0; e < 9; ++e) p.R_out[(size_t)b * 9 + e] = P[e];
  for (int e = 0; e < 3; ++e) p.t_out[(size_t)b * 3 + e] = P[9 + e];
  if (p.best_seed) p.best_seed[b] = best;
  if (p.inliers) p.inliers[b] = inl;
}

// How one call runs: cs_plan() validates the arguments and decides the degree pass's form from them and the CU count, and it
// is the only place that does.
struct CsPlan {
  int Q; bool pretest; SegSplit scan;
  int W, nt, nsb, nseg;
  size_t rows, M, zeroed, npass, part, key0, key1, val0, val1, hist, tot, krows, adj, status, pose, cpart, bytes;
};

int cs_plan(const vcr_consistency_args& a, int cu, CsPlan* p) {
  *p = CsPlan{};
  if (!a.src || !a.tgt || !a.corr || a.B < 1 || a.Ns < 1 || a.Nt < 1) return VCR_EINVAL;
  if (a.stop_after < 0 || a.stop_after > 2 || (a.stop_after == 0 && (!a.R_out || !a.t_out))) return VCR_EINVAL;
  const float inf = __builtin_huge_valf();
  if (!(a.tau >= 0.f) || a.tau == inf || !(a.max_dist >= 0.f) || a.max_dist == inf) return VCR_EINVAL;     // negative, NaN, +inf
  if (!(a.min_length >= 0.f) || a.min_length == inf || !(a.ratio >= 0.f && a.ratio <= 1.f)) return VCR_EINVAL;
  if (a.keep < 64 || a.keep > CS_MAX_KEEP || (a.keep & 63) || a.seeds < 1 || a.seeds > a.keep) return VCR_EINVAL;
  int fq, fs;
  const int fp = a.variant & CS_VARIANT_PRETEST;            // this file's two bits beside VCR_NN_SCORE_VARIANT's fields
  if (fp == CS_VARIANT_PRETEST || seg_variant(a.variant & ~CS_VARIANT_PRETEST, SEG_Q_124, CS_LIMITS, &fq, &fs)) return VCR_EINVAL;

  const int Nmax = a.Ns > a.Nt ? a.Ns : a.Nt;
  if (a.Ns > RS_MAX_N || a.Nt > RS_MAX_N || (long)a.B * Nmax >= (1L << 31) || (long)a.B * a.keep >= (1L << 30))
    return VCR_EUNSUPPORTED;                               // (B keep < 2^30: the grids by rank and by seed stay below 2^31)
  // The form is featnn_scan_kernel's rule (profiles/consistency_bench.txt has every form at three shapes): the most pairs per
  // lane that leave `fill` workgroups within reach -- they amortise the scalar loads of a streamed row --, then the streamed
  // side cut until the workgroups exist.  Ns stands for M, which only the device knows.
  p->Q = fq ? fq : seg_fills(a.B, a.Ns, a.Ns, 4, cu, CS_LIMITS) ? 4 : seg_fills(a.B, a.Ns, a.Ns, 2, cu, CS_LIMITS) ? 2 : 1;
  // The pre-test (cs_compatible_pre) costs one branch a streamed row: measured, it takes the degree pass to x0.61-x0.67 of
  // the plain form's time at two and four pairs a lane (16 x 16 384 and 131 072 pairs) and to x1.18-x1.40 at one, where a row
  // is a single test.  So the plan runs it from two pairs a lane.
  p->pretest = fp == CS_VARIANT_PRETEST_ON || (fp != CS_VARIANT_PRETEST_OFF && p->Q >= CS_PLAN_PRETEST_FROM_Q);
  const int e = seg_split(a.B, a.Ns, a.Ns, p->Q, fs, cu, CS_LIMITS, &p->scan);
  if (e) return e;
  p->W = a.keep / 64;
  p->nt = (a.Ns + WG_BLOCK * CS_E - 1) / (WG_BLOCK * CS_E);
  p->nsb = (a.seeds + 63) / 64;
  p->nseg = (a.Ns + CS_COUNT_SEG - 1) / CS_COUNT_SEG;
  const size_t BN = (size_t)a.B * a.Ns, BK = (size_t)a.B * a.keep, BS = (size_t)a.B * a.seeds;
  p->rows = 0;
  p->M = ws_up(BN * 32);
  p->zeroed = p->M + ws_up((size_t)a.B * 4);
  p->npass = p->zeroed + ws_up((size_t)a.B * 4);
  p->part = p->npass + ws_up((size_t)a.B * 4);
  p->key0 = p->part + ws_up((size_t)p->scan.S * BN * 4);
  p->key1 = p->key0 + ws_up(BN * 8);
  p->val0 = p->key1 + ws_up(BN * 8);
  p->val1 = p->val0 + ws_up(BN * 4);
  p->hist = p->val1 + ws_up(BN * 4);
  p->tot = p->hist + ws_up((size_t)a.B * p->nt * CS_R * 4);
  p->krows = p->tot + ws_up((size_t)a.B * CS_R * 4);
  p->adj = p->krows + ws_up(BK * 32);
  p->status = p->adj + (a.adj ? 0 : ws_up(BK * p->W * 8));
  p->pose = p->status + (a.seed_status ? 0 : ws_up(BS * 4));
  p->cpart = p->pose + (a.seed_pose ? 0 : ws_up(BS * 48));
  p->bytes = p->cpart + ws_up((size_t)a.B * p->nseg * a.seeds * 4);
  return VCR_OK;
}

unsigned cs_grid(long lanes) { return (unsigned)((lanes + RS_BLOCK - 1) / RS_BLOCK); }         // lanes < 2^31

int cs_take(const vcr_consistency_args* user, vcr_consistency_args* mine) {
  return vcr_take_args(user, mine, offsetof(vcr_consistency_args, best_seed));
}

}  // namespace

extern "C" int vcr_consistency_form(const vcr_consistency_args* ua, int cu_count, int* pairs_per_lane, int* splits, int* pretest) {
  vcr_consistency_args a;
  CsPlan p;
  if (cs_take(ua, &a) || cu_count < 0) return VCR_EINVAL;
  const int e = cs_plan(a, cu_count ? cu_count : vcr_cu_count(), &p);
  if (e) return e;
  if (pairs_per_lane) *pairs_per_lane = p.Q;
  if (splits) *splits = p.scan.S;
  if (pretest) *pretest = p.pretest ? 1 : 0;
  return VCR_OK;
}

extern "C" size_t vcr_consistency_workspace_bytes(const vcr_consistency_args* ua, int cu_count) {
  vcr_consistency_args a;
  CsPlan p;
  if (cs_take(ua, &a) || cu_count < 0) return 0;
  return cs_plan(a, cu_count ? cu_count : vcr_cu_count(), &p) ? 0 : p.bytes;
}

extern "C" int vcr_consistency_f32(const vcr_consistency_args* ua, void* workspace, size_t workspace_bytes, vcr_stream_t stream) {
  vcr_consistency_args a;
  if (cs_take(ua, &a)) return VCR_EINVAL;
  CsPlan p;
  int e = cs_plan(a, 1, &p);                               // the argument checks need no device
  if (e) return e;
  if (!workspace || (((uintptr_t)workspace) & 15)) return VCR_EINVAL;
  vcr_stream_scope scope_(stream);
  e = cs_plan(a, vcr_cu_count(), &p);
  if (e) return e;
  if (workspace_bytes < p.bytes) return VCR_EWORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  unsigned char* w = reinterpret_cast<unsigned char*>(workspace);
  float* rows = reinterpret_cast<float*>(w + p.rows);
  int* M = reinterpret_cast<int*>(w + p.M);
  int* npass = reinterpret_cast<int*>(w + p.npass);
  int* part = reinterpret_cast<int*>(w + p.part);
  const int B = a.B, Ns = a.Ns;
  const float min_len2 = a.min_length * a.min_length;      // fp32: one rounding
  const float max_d2 = a.max_dist * a.max_dist;

  const RsPairs pr{a.src, a.tgt, a.corr, Ns, a.Nt, rows, M, reinterpret_cast<int*>(w + p.zeroed), a.pairs};
  hipLaunchKernelGGL(consistency_pairs_kernel, dim3((unsigned)B), dim3(RS_BLOCK), 0, s, pr);
  if ((e = VCR_LAUNCH_RC())) return e;
  const CsDegree dg{rows, M, B, Ns, p.scan.S, p.scan.nblk, a.tau, min_len2, part};
  switch (p.Q * 2 + (p.pretest ? 1 : 0)) {
    case 9: hipLaunchKernelGGL((consistency_degree_kernel<4, true>), dim3(p.scan.grid), dim3(RS_BLOCK), 0, s, dg); break;
    case 8: hipLaunchKernelGGL((consistency_degree_kernel<4, false>), dim3(p.scan.grid), dim3(RS_BLOCK), 0, s, dg); break;
    case 5: hipLaunchKernelGGL((consistency_degree_kernel<2, true>), dim3(p.scan.grid), dim3(RS_BLOCK), 0, s, dg); break;
    case 4: hipLaunchKernelGGL((consistency_degree_kernel<2, false>), dim3(p.scan.grid), dim3(RS_BLOCK), 0, s, dg); break;
    case 3: hipLaunchKernelGGL((consistency_degree_kernel<1, true>), dim3(p.scan.grid), dim3(RS_BLOCK), 0, s, dg); break;
    default: hipLaunchKernelGGL((consistency_degree_kernel<1, false>), dim3(p.scan.grid), dim3(RS_BLOCK), 0, s, dg); break;
  }
  if ((e = VCR_LAUNCH_RC())) return e;
  RsSort rs{};
  rs.keys[0] = reinterpret_cast<rs_u64*>(w + p.key0); rs.keys[1] = reinterpret_cast<rs_u64*>(w + p.key1);
  rs.vals[0] = reinterpret_cast<unsigned*>(w + p.val0); rs.vals[1] = reinterpret_cast<unsigned*>(w + p.val1);
  rs.hist = reinterpret_cast<int*>(w + p.hist); rs.tot = reinterpret_cast<int*>(w + p.tot);
  rs.npass = npass; rs.N = Ns; rs.nt = p.nt;
  const CsMerge mg{part, rows, M, a.corr, B, Ns, a.Nt, p.scan.S, (long)B * Ns, a.deg, rs.keys[0], rs.vals[0], npass};
  hipLaunchKernelGGL(consistency_merge_kernel, dim3(cs_grid(mg.total)), dim3(RS_BLOCK), 0, s, mg);
  if ((e = VCR_LAUNCH_RC())) return e;
  if (a.stop_after == 1) return VCR_OK;

  const dim3 block(WG_BLOCK), tiles((unsigned)((long)B * p.nt)), digits((unsigned)((long)B * ((CS_R + WG_BLOCK - 1) / WG_BLOCK)));
  for (int pass = 0; pass < CS_SORT_PASSES; ++pass) {      // (radix_sort.h's pass; rs_sort_launch would run the 64 bits' eight)
    hipLaunchKernelGGL((rs_hist_kernel<CS_BITS, CS_E>), tiles, block, 0, s, rs, pass);
    if ((e = VCR_LAUNCH_RC())) return e;
    hipLaunchKernelGGL((rs_scan_kernel<CS_BITS>), digits, block, 0, s, rs, pass);
    if ((e = VCR_LAUNCH_RC())) return e;
    hipLaunchKernelGGL((rs_scatter_kernel<CS_BITS, CS_E>), tiles, block, 0, s, rs, pass);
    if ((e = VCR_LAUNCH_RC())) return e;
  }
  static_assert(CS_SORT_PASSES % 2 == 0, "the sorted order ends in buffer 0");
  float* krows = reinterpret_cast<float*>(w + p.krows);
  const CsKept kp{rs.vals[0], rows, M, Ns, a.keep, (long)B * a.keep, krows, a.kept};
  hipLaunchKernelGGL(consistency_kept_kernel, dim3(cs_grid(kp.total)), dim3(RS_BLOCK), 0, s, kp);
  if ((e = VCR_LAUNCH_RC())) return e;
  if (a.stop_after == 2) return VCR_OK;

  rs_u64* adj = a.adj ? reinterpret_cast<rs_u64*>(a.adj) : reinterpret_cast<rs_u64*>(w + p.adj);
  const CsAdj ad{krows, M, a.keep, p.W, (long)B * a.keep, a.tau, min_len2, adj};
  hipLaunchKernelGGL(consistency_adj_kernel, dim3((unsigned)(ad.total / WG_WAVES)), dim3(RS_BLOCK), 0, s, ad);
  if ((e = VCR_LAUNCH_RC())) return e;
  int* status = a.seed_status ? a.seed_status : reinterpret_cast<int*>(w + p.status);
  float* pose = a.seed_pose ? a.seed_pose : reinterpret_cast<float*>(w + p.pose);
  const CsSeed sd{krows, M, adj, a.keep, p.W, a.seeds, a.ratio, status, pose, a.seed_members, reinterpret_cast<rs_u64*>(a.member)};
  hipLaunchKernelGGL(consistency_seed_kernel, dim3((unsigned)((long)B * a.seeds)), dim3(RS_BLOCK), 0, s, sd);
  if ((e = VCR_LAUNCH_RC())) return e;
  int* cpart = reinterpret_cast<int*>(w + p.cpart);
  const CsCount ct{rows, M, status, pose, Ns, a.seeds, p.nsb, p.nseg, max_d2, cpart};
  hipLaunchKernelGGL(consistency_count_kernel, dim3((unsigned)((long)B * p.nsb * p.nseg)), dim3(64), 0, s, ct);
  if ((e = VCR_LAUNCH_RC())) return e;
  const CsBest bs{status, pose, cpart, a.seeds, p.nseg, a.R_out, a.t_out, a.best_seed, a.inliers, a.seed_inliers};
  hipLaunchKernelGGL(consistency_best_kernel, dim3((unsigned)B), dim3(RS_BLOCK), 0, s, bs);
  return VCR_LAUNCH_RC();
}

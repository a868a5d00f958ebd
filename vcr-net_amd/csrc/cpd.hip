// include/cpd/vcr_hip_cpd.h: rigid Coherent Point Drift -- the soft assignment of every source point to
// every target point (two streamed M x N passes of one hardware exp2 a pair), the closed-form rigid / similarity update, and
// the EM loop in one call.
//   cpd_init_kernel             one workgroup per cloud: the start pose, sigma2 (given, or the header's sigma2_0 in block order),
//                               the floor, the derived fp32 constants, the trace's first word
//   cpd_move_kernel             one lane per source point: the moved point as a 16-B record, +inf where it is not finite
//   cpd_pass_kernel<P2,SC,PPL>  P2 = false: a lane holds PPL target points and streams the moved source -> S_n per segment;
//                               P2 = true: a lane holds PPL moved source points and streams (x, inv_n) -> P1, PX per segment.
//                               SC = false: the streamed tile of 256 records goes through LDS (nn_scan.h's way); SC = true:
//                               every record is a scalar load (featnn.hip's way).  The sum hierarchy is the same text in all
//   cpd_col_kernel              one lane per target point: the segments ascending -> Pt1, and (x, inv_n) as a 16-B record
//   cpd_row_kernel              one lane per source point: the segments ascending -> P1, PX
//   cpd_np_kernel               (expectation) one workgroup per cloud: Np in the refinements' order
//   cpd_stage_kernel            (expectation, tests) e_mn
//   cpd_step_kernel             (the loop) one workgroup per cloud: the M-step's sums in block order, the rigid solve's Jacobi,
//                               the stops, the next state
//   cpd_finish_kernel           (the loop) the outputs from the state
// All stores are plain vector stores; there is no atomic.
#include "seg_scan.h"
#include "svd3.h"
#include "../../include/cpd/vcr_hip_cpd.h"

namespace {

constexpr int CP_BLOCK = 256;
constexpr int CP_TILE = VCR_CPD_TILE;
constexpr int CP_SEG = VCR_CPD_SEGMENT;
constexpr int CP_MAX_N = 131072;
constexpr double CP_LOG2E = 1.4426950408889634;
constexpr double CP_2PI = 6.283185307179586;

struct CpState {                                           // per cloud, in the workspace
  double R[9], t[3], s, sigma2;                            // the state: the E-step sees its fp32 rounding
  double c, floor, np;
  float rt[12];                                            // (float)(s R), (float)t
  float k;                                                 // (float)(-log2(e) / (2 sigma2))
  int live;                                                // 1: running; 2: stopped, the closing E-step is due; 0: done
  int iterations, status;
  double pad[7];
};
static_assert(sizeof(CpState) == VCR_CPD_STATE_BYTES, "the header documents the state's size");

__device__ __forceinline__ double cp_nan() { return __longlong_as_double(0x7FF8000000000000ll); }
__device__ __forceinline__ bool cp_finite3(float x, float y, float z) {
  return __builtin_isfinite(x) && __builtin_isfinite(y) && __builtin_isfinite(z);
}

// What the E-step reads of a state, from its fp64 words (one lane)
__device__ void cp_derive(CpState& s, double w, int M, int N) {
  for (int i = 0; i < 9; ++i) s.rt[i] = (float)(s.s * s.R[i]);
  for (int i = 0; i < 3; ++i) s.rt[9 + i] = (float)s.t[i];
  s.k = (float)(-CP_LOG2E / (2.0 * s.sigma2));
  const double q = CP_2PI * s.sigma2;
  s.c = ((q * sqrt(q)) * (w / (1.0 - w))) * ((double)M / (double)N);
}

__device__ __forceinline__ void cp_moved(const float* r, float x, float y, float z, float* pc) {
#pragma unroll
  for (int c = 0; c < 3; ++c) pc[c] = fmaf(r[3 * c + 2], z, fmaf(r[3 * c + 1], y, r[3 * c] * x)) + r[9 + c];
}

// The refinements' order over `count` points by one workgroup of 256: per 256 consecutive points the wave butterfly, the four
// waves ascending, the partials ascending from +0.  value(i, v) fills the NV values of point i.  Every thread calls this; the
// totals are in tot[] behind a barrier.  red is [2][4][NV].
template <int NV, class F>
__device__ __forceinline__ void cp_block_sums(int count, F value, double* tot, double* red) {
  const int t = threadIdx.x;
  const int nblk = (count + CP_BLOCK - 1) / CP_BLOCK;
  double run = 0.;
  for (int blk = 0; blk < nblk; ++blk) {
    double v[NV];
    const int i = blk * CP_BLOCK + t;
    if (i < count) value(i, v);
    else
#pragma unroll
      for (int e = 0; e < NV; ++e) v[e] = 0.;
    double* buf = red + (size_t)(blk & 1) * 4 * NV;
#pragma unroll
    for (int e = 0; e < NV; ++e) {
      double x = v[e];
#pragma unroll
      for (int o = 32; o >= 1; o >>= 1) x += __shfl_xor(x, o, 64);
      if ((t & 63) == 0) buf[(t >> 6) * NV + e] = x;
    }
    __syncthreads();
    if (t < NV) run = run + (((buf[t] + buf[NV + t]) + buf[2 * NV + t]) + buf[3 * NV + t]);
  }
  __syncthreads();
  if (t < NV) tot[t] = run;
  __syncthreads();
}

// ------------------------------------------------------------------------------------------------------------------ the start

struct CpInit {
  const float* src; const float* tgt; int B, M, N; const float* R; const float* t;
  double sigma2; const double* sigma2_dev; double scale; const double* scale_dev; double w, sigma2_floor;
  int loop, max_iterations;
  CpState* st; double* trace; double* Pt1; double* P1; double* PX;
};

__global__ __launch_bounds__(CP_BLOCK) void cpd_init_kernel(CpInit p) {
  __shared__ double tot[4], red[2 * 4 * 3];
  const int b = blockIdx.x, th = threadIdx.x, M = p.M, N = p.N;
  CpState& s = p.st[b];
  double R[9] = {1., 0., 0., 0., 1., 0., 0., 0., 1.}, tt[3] = {0., 0., 0.};
  if (p.R) {
    for (int i = 0; i < 9; ++i) R[i] = (double)p.R[(size_t)b * 9 + i];
    for (int i = 0; i < 3; ++i) tt[i] = (double)p.t[(size_t)b * 3 + i];
  }
  const double sc = p.loop ? 1.0 : p.scale_dev ? p.scale_dev[b] : p.scale;
  double s2 = p.sigma2_dev ? p.sigma2_dev[b] : p.sigma2;
  if (p.loop && !p.sigma2_dev && p.sigma2 == 0.) {         // sigma2_0 about the two means (workgroup-uniform branch)
    float r[12];
    for (int i = 0; i < 9; ++i) r[i] = (float)(sc * R[i]);
    for (int i = 0; i < 3; ++i) r[9 + i] = (float)tt[i];
    const float* x = p.tgt + (size_t)b * 3 * N;
    const float* y = p.src + (size_t)b * 3 * M;
    auto moved = [&](int i, double* v) {
      float pc[3];
      cp_moved(r, y[i], y[M + i], y[2 * (size_t)M + i], pc);
      for (int c = 0; c < 3; ++c) v[c] = (double)pc[c];
    };
    cp_block_sums<3>(N, [&](int i, double* v) { for (int c = 0; c < 3; ++c) v[c] = (double)x[(size_t)c * N + i]; }, tot, red);
    const double cx[3] = {tot[0] / (double)N, tot[1] / (double)N, tot[2] / (double)N};
    __syncthreads();
    cp_block_sums<3>(M, moved, tot, red);
    const double cy[3] = {tot[0] / (double)M, tot[1] / (double)M, tot[2] / (double)M};
    __syncthreads();
    cp_block_sums<1>(N, [&](int i, double* v) {
      const double a = (double)x[i] - cx[0], c = (double)x[N + i] - cx[1], d = (double)x[2 * (size_t)N + i] - cx[2];
      v[0] = (a * a + c * c) + d * d;
    }, tot, red);
    const double sxx = tot[0];
    __syncthreads();
    cp_block_sums<1>(M, [&](int i, double* v) {
      double q[3];
      moved(i, q);
      const double a = q[0] - cy[0], c = q[1] - cy[1], d = q[2] - cy[2];
      v[0] = (a * a + c * c) + d * d;
    }, tot, red);
    const double syy = tot[0];
    const double d0 = cx[0] - cy[0], d1 = cx[1] - cy[1], d2 = cx[2] - cy[2];
    const double dm = (double)M, dn = (double)N;
    s2 = ((dm * sxx + dn * syy) + (dm * dn) * ((d0 * d0 + d1 * d1) + d2 * d2)) / ((3.0 * dm) * dn);
  }
  const bool ok = __builtin_isfinite(s2) && s2 > 0. && __builtin_isfinite(sc) && sc > 0.;   // (a device array may hold anything)
  if (th == 0) {
    for (int i = 0; i < 9; ++i) s.R[i] = R[i];
    for (int i = 0; i < 3; ++i) s.t[i] = tt[i];
    s.s = sc; s.sigma2 = s2;
    s.floor = p.sigma2_floor > 0. ? p.sigma2_floor : 1e-8 * s2;
    s.np = ok ? 0. : cp_nan();
    s.iterations = 0;
    s.status = ok ? VCR_CPD_MAX_ITERATIONS : VCR_CPD_NOT_FINITE;
    s.live = ok ? 1 : 0;
    cp_derive(s, p.w, M, N);
    if (p.trace) p.trace[(size_t)b * (p.max_iterations + 1)] = s2;
  }
  if (p.trace) for (int i = 1 + th; i <= p.max_iterations; i += CP_BLOCK) p.trace[(size_t)b * (p.max_iterations + 1) + i] = cp_nan();
  if (!ok) {                                               // no E-step will run for this cloud: its outputs say so (Np follows P1)
    for (int i = th; i < N; i += CP_BLOCK) p.Pt1[(size_t)b * N + i] = cp_nan();
    for (int i = th; i < M; i += CP_BLOCK) p.P1[(size_t)b * M + i] = cp_nan();
    for (int i = th; i < 3 * M; i += CP_BLOCK) p.PX[(size_t)b * 3 * M + i] = cp_nan();
  }
}

// ---------------------------------------------------------------------------------------------------------------- the E-step

struct CpMove { const float* src; int B, M; const CpState* st; float4* ty; };

__global__ __launch_bounds__(CP_BLOCK) void cpd_move_kernel(CpMove p) {
  const long i = (long)blockIdx.x * CP_BLOCK + threadIdx.x;
  if (i >= (long)p.B * p.M) return;
  const int b = (int)(i / p.M), m = (int)(i % p.M), M = p.M;
  const CpState& s = p.st[b];
  if (!s.live) return;
  const float* y = p.src + (size_t)b * 3 * M;
  float r[12], pc[3];
#pragma unroll
  for (int e = 0; e < 12; ++e) r[e] = s.rt[e];
  cp_moved(r, y[m], y[M + m], y[2 * (size_t)M + m], pc);
  const float inf = __builtin_huge_valf();
  p.ty[i] = cp_finite3(pc[0], pc[1], pc[2]) ? make_float4(pc[0], pc[1], pc[2], 0.f) : make_float4(inf, inf, inf, 0.f);
}

struct CpPass {
  const float* tgt;                                        // pass 1's own points: [B,3,N] as the caller gave them
  const float4* own4;                                      // pass 2's own points: the moved source records
  const float4* stream;                                    // [B][Ns] records: the moved source (pass 1), (x, inv_n) (pass 2)
  int No, Ns, nblk, nseg, splits, per;                     // own and streamed points a cloud; own blocks; segments; their deal
  const CpState* st;
  double* part;                                            // pass 1 [B][nseg][No]; pass 2 [B][nseg][4][No]
};

template <bool P2, int PPL>
__device__ __forceinline__ void cp_pair(const float4 q, const float (&ox)[PPL], const float (&oy)[PPL], const float (&oz)[PPL], float k,
                                        float (&acc)[PPL][P2 ? 4 : 1]) {
#pragma unroll
  for (int j = 0; j < PPL; ++j) {
    // d = x - ty: the target is the streamed record in pass 2 and the lane's own point in pass 1
    const float d0 = P2 ? q.x - ox[j] : ox[j] - q.x, d1 = P2 ? q.y - oy[j] : oy[j] - q.y, d2 = P2 ? q.z - oz[j] : oz[j] - q.z;
    const float dd = (d0 * d0 + d1 * d1) + d2 * d2;
    const float e = __builtin_amdgcn_exp2f(dd * k);
    if constexpr (P2) {
      const float pr = e * q.w;
      acc[j][0] = acc[j][0] + pr;
      acc[j][1] = acc[j][1] + pr * q.x;
      acc[j][2] = acc[j][2] + pr * q.y;
      acc[j][3] = acc[j][3] + pr * q.z;
    } else {
      acc[j][0] = acc[j][0] + e;
    }
  }
}

// One streamed record by a scalar load: the records were written by an earlier launch and nothing in this one writes them, so
// they are read through the constant address space -- with a workgroup-uniform address that is an s_load_dwordx4 into SGPRs,
// which the lanes' subtractions take as scalar operands.  (A plain load of a uniform address stays a per-lane vector load
// here: the per-segment store of the partials keeps the compiler from proving the records invariant.)
typedef const f32x4 __attribute__((address_space(4))) cp_const4;
__device__ __forceinline__ float4 cp_scalar(const float4* q) {
  const f32x4 v = *(cp_const4*)(q);
  return make_float4(v[0], v[1], v[2], v[3]);
}

template <bool P2, bool SC, int PPL>
__global__ __launch_bounds__(CP_BLOCK) void cpd_pass_kernel(CpPass p) {
  constexpr int NV = P2 ? 4 : 1;
  __shared__ float4 tile[SC ? 1 : CP_TILE];
  const int t = threadIdx.x;
  int id = (int)blockIdx.x;
  const int sp = id % p.splits;
  id /= p.splits;
  const int blk = id % p.nblk, b = id / p.nblk;
  const CpState& st = p.st[b];
  if (!st.live) return;                                    // (workgroup-uniform: a stopped cloud)
  const float k = st.k;
  const int No = p.No, Ns = p.Ns;
  float ox[PPL], oy[PPL], oz[PPL];
#pragma unroll
  for (int j = 0; j < PPL; ++j) {
    int o = (blk * PPL + j) * CP_BLOCK + t;
    o = o < No ? o : No - 1;                               // (lanes past the end repeat the last point and store nothing)
    if constexpr (P2) {
      const float4 v = p.own4[(size_t)b * No + o];
      ox[j] = v.x; oy[j] = v.y; oz[j] = v.z;
    } else {
      const float* x = p.tgt + (size_t)b * 3 * No;
      ox[j] = x[o]; oy[j] = x[No + o]; oz[j] = x[2 * (size_t)No + o];
    }
  }
  const float4* sq = p.stream + (size_t)b * Ns;             // (workgroup-uniform, like every index into it with SC)
  const int seg1 = (sp + 1) * p.per < p.nseg ? (sp + 1) * p.per : p.nseg;
  for (int seg = sp * p.per; seg < seg1; ++seg) {
    double sacc[PPL][NV];
#pragma unroll
    for (int j = 0; j < PPL; ++j)
#pragma unroll
      for (int v = 0; v < NV; ++v) sacc[j][v] = 0.;
    const int end = (seg + 1) * CP_SEG < Ns ? (seg + 1) * CP_SEG : Ns;
    for (int base = seg * CP_SEG; base < end; base += CP_TILE) {
      const int cnt = end - base < CP_TILE ? end - base : CP_TILE;
      if constexpr (!SC) {
        __syncthreads();                                   // (the tile before this one has been read by every lane)
        if (t < cnt) tile[t] = sq[base + t];
        __syncthreads();
      }
      float acc[PPL][NV];
#pragma unroll
      for (int j = 0; j < PPL; ++j)
#pragma unroll
        for (int v = 0; v < NV; ++v) acc[j][v] = 0.f;
      if (cnt == CP_TILE) {
#pragma unroll 8
        for (int i = 0; i < CP_TILE; ++i) cp_pair<P2, PPL>(SC ? cp_scalar(sq + base + i) : tile[i], ox, oy, oz, k, acc);
      } else {
        for (int i = 0; i < cnt; ++i) cp_pair<P2, PPL>(SC ? cp_scalar(sq + base + i) : tile[i], ox, oy, oz, k, acc);
      }
#pragma unroll
      for (int j = 0; j < PPL; ++j)
#pragma unroll
        for (int v = 0; v < NV; ++v) sacc[j][v] = sacc[j][v] + (double)acc[j][v];
    }
    double* part = p.part + ((size_t)b * p.nseg + seg) * NV * No;
#pragma unroll
    for (int j = 0; j < PPL; ++j) {
      const int o = (blk * PPL + j) * CP_BLOCK + t;
      if (o < No)
#pragma unroll
        for (int v = 0; v < NV; ++v) part[(size_t)v * No + o] = sacc[j][v];
    }
  }
}

struct CpCol { const float* tgt; int B, N, nseg; const CpState* st; const double* part; double* Pt1; float4* xr; };

__global__ __launch_bounds__(CP_BLOCK) void cpd_col_kernel(CpCol p) {
  const long i = (long)blockIdx.x * CP_BLOCK + threadIdx.x;
  if (i >= (long)p.B * p.N) return;
  const int b = (int)(i / p.N), n = (int)(i % p.N), N = p.N;
  const CpState& s = p.st[b];
  if (!s.live) return;
  const float* x = p.tgt + (size_t)b * 3 * N;
  const float x0 = x[n], x1 = x[N + n], x2 = x[2 * (size_t)N + n];
  const bool fin = cp_finite3(x0, x1, x2);
  double S = 0.;
  for (int g = 0; g < p.nseg; ++g) S = S + p.part[((size_t)b * p.nseg + g) * N + n];
  if (!fin) S = 0.;
  const double den = S + s.c;
  const double rden = 1.0 / den;
  const bool live = fin && den != 0.;
  p.Pt1[i] = live ? S * rden : 0.;
  p.xr[i] = fin ? make_float4(x0, x1, x2, live ? (float)rden : 0.f) : make_float4(0.f, 0.f, 0.f, 0.f);
}

struct CpRow { int B, M, nseg; const CpState* st; const double* part; double* P1; double* PX; };

__global__ __launch_bounds__(CP_BLOCK) void cpd_row_kernel(CpRow p) {
  const long i = (long)blockIdx.x * CP_BLOCK + threadIdx.x;
  if (i >= (long)p.B * p.M) return;
  const int b = (int)(i / p.M), m = (int)(i % p.M), M = p.M;
  if (!p.st[b].live) return;
  double a[4] = {0., 0., 0., 0.};
  for (int g = 0; g < p.nseg; ++g) {
    const double* part = p.part + ((size_t)b * p.nseg + g) * 4 * M;
#pragma unroll
    for (int v = 0; v < 4; ++v) a[v] = a[v] + part[(size_t)v * M + m];
  }
  p.P1[i] = a[0];
#pragma unroll
  for (int c = 0; c < 3; ++c) p.PX[((size_t)b * 3 + c) * M + m] = a[1 + c];
}

struct CpNp { int M; const double* P1; double* Np; };

__global__ __launch_bounds__(CP_BLOCK) void cpd_np_kernel(CpNp p) {
  __shared__ double tot[1], red[2 * 4];
  const int b = blockIdx.x;
  const double* P1 = p.P1 + (size_t)b * p.M;
  cp_block_sums<1>(p.M, [&](int i, double* v) { v[0] = P1[i]; }, tot, red);
  if (threadIdx.x == 0) p.Np[b] = tot[0];
}

struct CpStage { const float* tgt; const float4* ty; int B, M, N; const CpState* st; float* e; };

__global__ __launch_bounds__(CP_BLOCK) void cpd_stage_kernel(CpStage p) {
  const size_t i = (size_t)blockIdx.x * CP_BLOCK + threadIdx.x;
  const size_t MN = (size_t)p.M * p.N;
  if (i >= (size_t)p.B * MN) return;
  const int b = (int)(i / MN), m = (int)((i % MN) / p.N), n = (int)(i % p.N), N = p.N;
  if (!p.st[b].live) { p.e[i] = __builtin_nanf(""); return; }   // (a cloud the start refused: nothing was moved)
  const float* x = p.tgt + (size_t)b * 3 * N;
  const float4 q = p.ty[(size_t)b * p.M + m];
  const float x0 = x[n], x1 = x[N + n], x2 = x[2 * (size_t)N + n];
  const float d0 = x0 - q.x, d1 = x1 - q.y, d2 = x2 - q.z;
  const float dd = (d0 * d0 + d1 * d1) + d2 * d2;
  const float e = __builtin_amdgcn_exp2f(dd * p.st[b].k);
  p.e[i] = cp_finite3(x0, x1, x2) && cp_finite3(q.x, q.y, q.z) ? e : 0.f;
}

// ----------------------------------------------------------------------------------------------------------------- the M-step

struct CpStep {
  const float* src; const float* tgt; int M, N, max_iterations, with_scaling; double tolerance, w;
  const double* Pt1; const double* P1; const double* PX; CpState* st; double* trace;
};

__global__ __launch_bounds__(CP_BLOCK) void cpd_step_kernel(CpStep p) {
  __shared__ double tot[10], red[2 * 4 * 10];
  const int b = blockIdx.x, th = threadIdx.x, M = p.M, N = p.N;
  CpState& s = p.st[b];
  const int live = s.live, done = s.iterations;            // (read by every lane before lane 0 writes: barriers follow)
  if (!live) return;
  const double* P1 = p.P1 + (size_t)b * M;
  const double* PX = p.PX + (size_t)b * 3 * M;
  const double* Pt1 = p.Pt1 + (size_t)b * N;
  const float* y = p.src + (size_t)b * 3 * M;
  const float* x = p.tgt + (size_t)b * 3 * N;
  if (live == 2 || done >= p.max_iterations) {             // the closing E-step (or the only one) has run: its Np, and the end
    cp_block_sums<1>(M, [&](int i, double* v) { v[0] = P1[i]; }, tot, red);
    if (th == 0) { s.np = tot[0]; s.live = 0; }
    return;
  }
  cp_block_sums<7>(M, [&](int i, double* v) {
    const double p1 = P1[i];
    v[0] = p1;
    for (int c = 0; c < 3; ++c) { v[1 + c] = PX[(size_t)c * M + i]; v[4 + c] = p1 * (double)y[(size_t)c * M + i]; }
  }, tot, red);
  bool finite = true;
  for (int e = 0; e < 7; ++e) finite = finite && __builtin_isfinite(tot[e]);
  const double Np = tot[0];
  if (th == 0) s.np = Np;
  if (!finite || Np == 0.) {                               // (workgroup-uniform: tot is shared)
    if (th == 0) { s.live = 0; s.status = !finite ? VCR_CPD_NOT_FINITE : VCR_CPD_NO_MASS; }
    return;
  }
  const double mux[3] = {tot[1] / Np, tot[2] / Np, tot[3] / Np}, muy[3] = {tot[4] / Np, tot[5] / Np, tot[6] / Np};
  __syncthreads();
  cp_block_sums<10>(M, [&](int i, double* v) {
    const double p1 = P1[i];
    const double yh[3] = {(double)y[i] - muy[0], (double)y[M + i] - muy[1], (double)y[2 * (size_t)M + i] - muy[2]};
    for (int r = 0; r < 3; ++r) {
      const double a = PX[(size_t)r * M + i] - p1 * mux[r];
      for (int c = 0; c < 3; ++c) v[3 * r + c] = a * yh[c];
    }
    v[9] = p1 * ((yh[0] * yh[0] + yh[1] * yh[1]) + yh[2] * yh[2]);
  }, tot, red);
  double A[9];
  for (int e = 0; e < 9; ++e) A[e] = tot[e];
  const double yPy = tot[9];
  __syncthreads();
  cp_block_sums<1>(N, [&](int i, double* v) {
    const double xh[3] = {(double)x[i] - mux[0], (double)x[N + i] - mux[1], (double)x[2 * (size_t)N + i] - mux[2]};
    v[0] = Pt1[i] * ((xh[0] * xh[0] + xh[1] * xh[1]) + xh[2] * xh[2]);
  }, tot, red);
  const double xPx = tot[0];
  if (th >= 64) return;                                    // wave 0 finishes; its first quad runs the Jacobi sweeps together
  for (int e = 0; e < 9; ++e) finite = finite && __builtin_isfinite(A[e]);
  finite = finite && __builtin_isfinite(yPy) && __builtin_isfinite(xPx);
  if (!finite) {                                           // (wave-uniform)
    if (th == 0) { s.live = 0; s.status = VCR_CPD_NOT_FINITE; }
    return;
  }
  const int li = th & 3;
  double a[3], v[3];
#pragma unroll
  for (int j = 0; j < 3; ++j) {                            // H = A^T: lane i of the quad holds row i of H = column i of A
    a[j] = li == 0 ? A[3 * j] : li == 1 ? A[3 * j + 1] : li == 2 ? A[3 * j + 2] : 0.0;
    v[j] = li == j ? 1.0 : 0.0;
  }
  jacobi_sweeps_quad(a, v);
  double Aq[3][3], Vq[3][3];
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    Aq[0][j] = quad_get(a[j], 0); Aq[1][j] = quad_get(a[j], 1); Aq[2][j] = quad_get(a[j], 2);
    Vq[0][j] = quad_get(v[j], 0); Vq[1][j] = quad_get(v[j], 1); Vq[2][j] = quad_get(v[j], 2);
  }
  if (th != 0) return;
  double Rn[9], tn[3];
  svd3_finish(Aq, Vq, Rn);
  double trAR = 0.;
  for (int e = 0; e < 9; ++e) trAR = trAR + A[e] * Rn[e];
  const double sn = p.with_scaling ? trAR / yPy : 1.0;
  for (int c = 0; c < 3; ++c) tn[c] = mux[c] - sn * ((Rn[3 * c] * muy[0] + Rn[3 * c + 1] * muy[1]) + Rn[3 * c + 2] * muy[2]);
  const double s2n = ((xPx - (2.0 * sn) * trAR) + (sn * sn) * yPy) / (3.0 * Np);
  bool good = __builtin_isfinite(sn) && __builtin_isfinite(s2n);
  for (int e = 0; e < 9; ++e) good = good && __builtin_isfinite(Rn[e]);
  for (int c = 0; c < 3; ++c) good = good && __builtin_isfinite(tn[c]);
  if (!good) { s.live = 0; s.status = VCR_CPD_NOT_FINITE; return; }
  const double s2 = s.sigma2;
  for (int e = 0; e < 9; ++e) s.R[e] = (double)(float)Rn[e];
  for (int c = 0; c < 3; ++c) s.t[c] = (double)(float)tn[c];
  s.s = sn;
  s.iterations = done + 1;
  s.live = 2;                                              // every stop below took a state: the closing E-step is due
  if (!(s2n > s.floor)) { s.sigma2 = s.floor; s.status = VCR_CPD_COLLAPSED; }
  else {
    s.sigma2 = s2n;
    if (fabs(s2n - s2) <= p.tolerance * s2) s.status = VCR_CPD_CONVERGED;
    else if (done + 1 >= p.max_iterations) s.status = VCR_CPD_MAX_ITERATIONS;
    else s.live = 1;
  }
  cp_derive(s, p.w, M, N);
  if (p.trace) p.trace[(size_t)b * (p.max_iterations + 1) + done + 1] = s.sigma2;
}

struct CpFinish {
  const CpState* st; int B;
  float* R_out; float* t_out; float* R_ba; float* t_ba; double* scale; double* sigma2; double* Np; int* iterations; int* status;
};

__global__ __launch_bounds__(CP_BLOCK) void cpd_finish_kernel(CpFinish p) {
  const int b = blockIdx.x * CP_BLOCK + threadIdx.x;
  if (b >= p.B) return;
  const CpState& s = p.st[b];
  float r[12];
  for (int i = 0; i < 9; ++i) r[i] = (float)s.R[i];
  for (int i = 0; i < 3; ++i) r[9 + i] = (float)s.t[i];
  for (int i = 0; i < 9; ++i) p.R_out[(size_t)b * 9 + i] = r[i];
  for (int i = 0; i < 3; ++i) p.t_out[(size_t)b * 3 + i] = r[9 + i];
  for (int i = 0; i < 3; ++i) {                            // the refinements' inverse (pose_step_kernel's expression)
    if (p.R_ba) for (int j = 0; j < 3; ++j) p.R_ba[(size_t)b * 9 + i * 3 + j] = r[j * 3 + i];
    if (p.t_ba) p.t_ba[(size_t)b * 3 + i] = -fmaf(r[6 + i], r[11], fmaf(r[3 + i], r[10], r[i] * r[9]));
  }
  if (p.scale) p.scale[b] = s.s;
  if (p.sigma2) p.sigma2[b] = s.sigma2;
  if (p.Np) p.Np[b] = s.np;
  if (p.iterations) p.iterations[b] = s.iterations;
  if (p.status) p.status[b] = s.status;
}

// --------------------------------------------------------------------------------------------------------------------- host

int cp_take(const vcr_cpd_args* user, vcr_cpd_args* mine) { return vcr_take_args(user, mine, offsetof(vcr_cpd_args, max_iterations)); }

struct CpPlan {
  int form, ppl, scalar;                                   // 1 ... 6; points a lane; the streamed record by scalar loads
  int sm, sn;                                              // segments of pass 1 (over M) and of pass 2 (over N)
  int nblk1, nblk2, splits1, splits2, per1, per2;
  size_t state, ty, xr, part1, part2, bytes;
};

// One pass' deal: `nseg` segments of a cloud over `splits` workgroups of `per` consecutive segments each
void cp_deal(int wgs, int nseg, int cu, int g, int* splits, int* per) {
  int want = g == 1 ? 1 : g == 2 ? nseg : (int)((2L * cu + wgs - 1) / wgs);   // two workgroups a CU before the deal stops
  want = want < 1 ? 1 : want > nseg ? nseg : want;
  *per = (nseg + want - 1) / want;
  *splits = (nseg + *per - 1) / *per;
}

int cp_plan(const vcr_cpd_args& a, bool loop, int cu, CpPlan* p) {
  *p = CpPlan{};
  if (a.B < 1 || a.M < 1 || a.N < 1 || !a.src || !a.tgt || (a.R == nullptr) != (a.t == nullptr)) return VCR_EINVAL;
  if (!(a.w >= 0. && a.w < 1.)) return VCR_EINVAL;
  const bool s2ok = __builtin_isfinite(a.sigma2) && a.sigma2 > 0.;
  if (!a.sigma2_dev && !s2ok && !(loop && a.sigma2 == 0.)) return VCR_EINVAL;
  if (!loop && !a.scale_dev && !(__builtin_isfinite(a.scale) && a.scale > 0.)) return VCR_EINVAL;
  const int f = a.variant & 7, g = a.variant >> 3;
  if (a.variant < 0 || f > VCR_CPD_FORMS || g > 2) return VCR_EINVAL;
  if (!loop && (!a.Pt1 || !a.P1 || !a.PX || !a.Np)) return VCR_EINVAL;
  if (loop && (!a.R_out || !a.t_out || !a.Pt1 || !a.P1 || !a.PX || a.max_iterations < 0 || !(a.tolerance >= 0.) || !(a.sigma2_floor >= 0.) ||
               a.sigma2_floor == __builtin_huge_val()))
    return VCR_EINVAL;
  if (a.M > CP_MAX_N || a.N > CP_MAX_N || (long)a.B * a.M >= (1L << 31) || (long)a.B * a.N >= (1L << 31) ||
      (loop && a.max_iterations > (1 << 20)))
    return VCR_EUNSUPPORTED;
  p->sm = (a.M + CP_SEG - 1) / CP_SEG;
  p->sn = (a.N + CP_SEG - 1) / CP_SEG;
  if (f) { p->scalar = f > 3; p->ppl = 1 << ((f - 1) % 3); }
  else {
    // Measured (profiles/cpd_bench.txt, every form forced at three shapes): the fastest form at each shape is an LDS one -- the
    // scalar loads' best is x0.84 of its rate at 16 x 1 024 and x0.96 ... x0.98 at the two large shapes, although at one point
    // a lane (and at two at 131 072) the scalar loads are even or a little ahead there -- so the plan takes the LDS tile.  More points a lane
    // amortise the tile's reads (4 a lane takes x0.83 of 1 a lane's time at 1 x 131 072) but leave fewer workgroups (x2.4 of
    // its time at 16 x 1 024, where 1 a lane fills a quarter of the chip): the most points a lane at which both passes still
    // have a workgroup a CU to deal out
    p->scalar = 0;
    p->ppl = 1;
    for (int q = 4; q >= 2; q >>= 1) {
      const long w1 = (long)a.B * ((a.N + CP_BLOCK * q - 1) / (CP_BLOCK * q)) * p->sm;
      const long w2 = (long)a.B * ((a.M + CP_BLOCK * q - 1) / (CP_BLOCK * q)) * p->sn;
      if ((w1 < w2 ? w1 : w2) >= cu) { p->ppl = q; break; }
    }
  }
  p->form = (p->scalar ? 3 : 0) + (p->ppl == 4 ? 3 : p->ppl);
  p->nblk1 = (a.N + CP_BLOCK * p->ppl - 1) / (CP_BLOCK * p->ppl);
  p->nblk2 = (a.M + CP_BLOCK * p->ppl - 1) / (CP_BLOCK * p->ppl);
  cp_deal(a.B * p->nblk1, p->sm, cu, g, &p->splits1, &p->per1);
  cp_deal(a.B * p->nblk2, p->sn, cu, g, &p->splits2, &p->per2);
  const size_t B = (size_t)a.B;
  p->state = 0;
  p->ty = p->state + ws_up(B * sizeof(CpState));
  p->xr = p->ty + ws_up(B * a.M * 16);
  p->part1 = p->xr + ws_up(B * a.N * 16);
  p->part2 = p->part1 + ws_up(B * p->sm * a.N * 8);
  p->bytes = p->part2 + ws_up(B * p->sn * a.M * 32);
  return VCR_OK;
}

int cp_form(const vcr_cpd_args* ua, bool loop, int cu_count, int* form, int* splits1, int* splits2) {
  vcr_cpd_args a;
  CpPlan p;
  if (cp_take(ua, &a) || cu_count < 0) return VCR_EINVAL;
  int e = cp_plan(a, loop, cu_count > 0 ? cu_count : 256, &p);  // (the refusals first: they need no device)
  if (e) return e;
  if (cu_count == 0 && (e = cp_plan(a, loop, vcr_cu_count(), &p))) return e;
  if (form) *form = p.form;
  if (splits1) *splits1 = p.splits1;
  if (splits2) *splits2 = p.splits2;
  return VCR_OK;
}

size_t cp_bytes(const vcr_cpd_args* ua, bool loop, int cu_count) {
  vcr_cpd_args a;
  CpPlan p;
  if (cp_take(ua, &a) || cu_count < 0) return 0;
  return cp_plan(a, loop, 256, &p) ? 0 : p.bytes;          // (the sizes do not depend on the CU count)
}

unsigned cp_grid(long lanes) { return (unsigned)((lanes + CP_BLOCK - 1) / CP_BLOCK); }

template <bool P2>
int cp_launch_pass(const CpPlan& pl, const CpPass& ps, unsigned grid, hipStream_t s) {
#define CP_CASE(SC, PPL)                                                                                    \
  if (pl.scalar == (SC ? 1 : 0) && pl.ppl == PPL) {                                                         \
    hipLaunchKernelGGL((cpd_pass_kernel<P2, SC, PPL>), dim3(grid), dim3(CP_BLOCK), 0, s, ps);               \
    return VCR_LAUNCH_RC();                                                                                 \
  }
  CP_CASE(false, 1) CP_CASE(false, 2) CP_CASE(false, 4) CP_CASE(true, 1) CP_CASE(true, 2) CP_CASE(true, 4)
#undef CP_CASE
  return VCR_EINVAL;
}

struct CpWork { CpState* st; float4* ty; float4* xr; double* part1; double* part2; };

// One E-step at the state: five launches
int cp_expect(const vcr_cpd_args& a, const CpPlan& p, const CpWork& w, double* Pt1, double* P1, double* PX, hipStream_t s) {
  int e;
  hipLaunchKernelGGL(cpd_move_kernel, dim3(cp_grid((long)a.B * a.M)), dim3(CP_BLOCK), 0, s, CpMove{a.src, a.B, a.M, w.st, w.ty});
  if ((e = VCR_LAUNCH_RC())) return e;
  const CpPass p1{a.tgt, nullptr, w.ty, a.N, a.M, p.nblk1, p.sm, p.splits1, p.per1, w.st, w.part1};
  if ((e = cp_launch_pass<false>(p, p1, (unsigned)((long)a.B * p.nblk1 * p.splits1), s))) return e;
  hipLaunchKernelGGL(cpd_col_kernel, dim3(cp_grid((long)a.B * a.N)), dim3(CP_BLOCK), 0, s,
                     CpCol{a.tgt, a.B, a.N, p.sm, w.st, w.part1, Pt1, w.xr});
  if ((e = VCR_LAUNCH_RC())) return e;
  const CpPass p2{nullptr, w.ty, w.xr, a.M, a.N, p.nblk2, p.sn, p.splits2, p.per2, w.st, w.part2};
  if ((e = cp_launch_pass<true>(p, p2, (unsigned)((long)a.B * p.nblk2 * p.splits2), s))) return e;
  hipLaunchKernelGGL(cpd_row_kernel, dim3(cp_grid((long)a.B * a.M)), dim3(CP_BLOCK), 0, s, CpRow{a.B, a.M, p.sn, w.st, w.part2, P1, PX});
  return VCR_LAUNCH_RC();
}

int cp_run(const vcr_cpd_args* ua, bool loop, void* workspace, size_t workspace_bytes, vcr_stream_t stream) {
  vcr_stream_scope scope(stream);
  vcr_cpd_args a;
  if (cp_take(ua, &a)) return VCR_EINVAL;
  CpPlan p;
  int e = cp_plan(a, loop, 256, &p);                       // (the refusals first: they need no device)
  if (e) return e;
  if (!workspace || (((uintptr_t)workspace) & 15)) return VCR_EINVAL;
  if (workspace_bytes < p.bytes) return VCR_EWORKSPACE;
  if ((e = cp_plan(a, loop, vcr_cu_count(), &p))) return e;
  hipStream_t s = (hipStream_t)stream;
  unsigned char* wsp = reinterpret_cast<unsigned char*>(workspace);
  const CpWork w{reinterpret_cast<CpState*>(wsp + p.state), reinterpret_cast<float4*>(wsp + p.ty), reinterpret_cast<float4*>(wsp + p.xr),
                 reinterpret_cast<double*>(wsp + p.part1), reinterpret_cast<double*>(wsp + p.part2)};
  double* Pt1 = a.Pt1; double* P1 = a.P1; double* PX = a.PX;   // (the M-step reads them where the caller gets them)
  const CpInit in{a.src, a.tgt, a.B, a.M, a.N, a.R, a.t, a.sigma2, a.sigma2_dev, a.scale, a.scale_dev, a.w, loop ? a.sigma2_floor : 0.,
                  loop ? 1 : 0, loop ? a.max_iterations : 0, w.st, loop ? a.trace : nullptr, Pt1, P1, PX};
  hipLaunchKernelGGL(cpd_init_kernel, dim3((unsigned)a.B), dim3(CP_BLOCK), 0, s, in);
  if ((e = VCR_LAUNCH_RC())) return e;
  if (!loop) {
    if ((e = cp_expect(a, p, w, Pt1, P1, PX, s))) return e;
    hipLaunchKernelGGL(cpd_np_kernel, dim3((unsigned)a.B), dim3(CP_BLOCK), 0, s, CpNp{a.M, P1, a.Np});
    if ((e = VCR_LAUNCH_RC())) return e;
    if (a.e_stage) {
      const size_t total = (size_t)a.B * a.M * a.N;
      if ((total + CP_BLOCK - 1) / CP_BLOCK > 0x7FFFFFFFull) return VCR_EUNSUPPORTED;
      hipLaunchKernelGGL(cpd_stage_kernel, dim3((unsigned)((total + CP_BLOCK - 1) / CP_BLOCK)), dim3(CP_BLOCK), 0, s,
                         CpStage{a.tgt, w.ty, a.B, a.M, a.N, w.st, a.e_stage});
      if ((e = VCR_LAUNCH_RC())) return e;
    }
    return VCR_OK;
  }
  for (int round = 0; round <= a.max_iterations; ++round) {
    if ((e = cp_expect(a, p, w, Pt1, P1, PX, s))) return e;
    const CpStep sp{a.src, a.tgt, a.M, a.N, a.max_iterations, a.with_scaling, a.tolerance, a.w, Pt1, P1, PX, w.st, a.trace};
    hipLaunchKernelGGL(cpd_step_kernel, dim3((unsigned)a.B), dim3(CP_BLOCK), 0, s, sp);
    if ((e = VCR_LAUNCH_RC())) return e;
  }
  const CpFinish fn{w.st, a.B, a.R_out, a.t_out, a.R_ba, a.t_ba, a.scale_out, a.sigma2_out, a.Np, a.iterations, a.status};
  hipLaunchKernelGGL(cpd_finish_kernel, dim3(cp_grid(a.B)), dim3(CP_BLOCK), 0, s, fn);
  return VCR_LAUNCH_RC();
}

}  // namespace

extern "C" size_t vcr_cpd_expectation_workspace_bytes(const vcr_cpd_args* a, int cu_count) { return cp_bytes(a, false, cu_count); }
extern "C" size_t vcr_cpd_workspace_bytes(const vcr_cpd_args* a, int cu_count) { return cp_bytes(a, true, cu_count); }
extern "C" int vcr_cpd_expectation_form(const vcr_cpd_args* a, int cu_count, int* form, int* splits1, int* splits2) {
  return cp_form(a, false, cu_count, form, splits1, splits2);
}
extern "C" int vcr_cpd_form(const vcr_cpd_args* a, int cu_count, int* form, int* splits1, int* splits2) {
  return cp_form(a, true, cu_count, form, splits1, splits2);
}
extern "C" int vcr_cpd_expectation_f32(const vcr_cpd_args* a, void* workspace, size_t workspace_bytes, vcr_stream_t stream) {
  return cp_run(a, false, workspace, workspace_bytes, stream);
}
extern "C" int vcr_cpd_f32(const vcr_cpd_args* a, void* workspace, size_t workspace_bytes, vcr_stream_t stream) {
  return cp_run(a, true, workspace, workspace_bytes, stream);
}

// include/ndt/vcr_hip_ndt.h: the Normal Distributions Transform -- a voxel map of Gaussians, the score of a
// scan with its gradient and Hessian, and Levenberg-Marquardt on it.
//   vcr_voxel_sort_f32          the voxels, their member lists and counts (voxel_sort.hip), into this call's workspace
//   ndt_origin_kernel           one workgroup per cloud: the fp32 minimum over the finite points -> origin (the grid's expression)
//   ndt_clear_kernel            every table word to "empty"
//   ndt_stats_kernel            one lane per voxel slot: mean, two-pass covariance, the normals' Jacobi sweeps, the eigenvalue
//                               floor, inv_cov, valid; the voxel's key enters the table by a 64-bit compare-and-swap
//   ndt_pose_kernel             the caller's pose into the per-cloud state
//   ndt_round_kernel            one lane per source point: the moved point, its cell, up to seven lookups, the 29 fp64 values of
//                               the header in cell order; the workgroup's 256 points reduced in the refinements' order
//   ndt_sums_kernel             (derivatives) one workgroup per cloud: the partials ascending -> score, hits, g, H
//   ndt_step_kernel             (the loop) one workgroup per cloud: the partials ascending, the Levenberg-Marquardt
//                               bookkeeping of the header in one lane, the next trial pose
//   ndt_finish_kernel           (the loop) the outputs from the state
// All stores are plain vector stores; the compare-and-swap of the table is the one atomic.
#include "seg_scan.h"
#include "normals_point.h"
#include "refine_solve6.h"
#include "../../include/ndt/vcr_hip_ndt.h"

namespace {

typedef unsigned long long nd_u64;
constexpr int ND_BLOCK = 256;
constexpr int ND_MAX_N = 131072;
constexpr int ND_VALUES = VCR_NDT_VALUES;
constexpr nd_u64 ND_EMPTY = ~0ull;
constexpr nd_u64 ND_HASH = 0x9E3779B97F4A7C15ull;
constexpr double ND_CELLS = (double)VCR_VOXEL_MAX_CELLS;

struct NdState {                                           // per cloud, in the workspace
  double pose[12];                                         // the accepted pose: R row-major, t
  double trial[12];                                        // the pose of the trial in flight: a round evaluates its fp32 rounding
  double v[ND_VALUES];                                     // the accepted f, hits, g, H
  double lambda, nu;
  double x[6];                                             // the step of the trial in flight
  int live, go, iterations, trials, converged, status;
};
static_assert(sizeof(NdState) == VCR_NDT_STATE_BYTES, "the header documents the state's size");

__host__ __device__ inline int nd_log2_slots(int V) {      // T = 2^this is the smallest power of two >= 2 V + 2
  int l = 1;
  while ((1L << l) < 2L * V + 2) ++l;
  return l;
}

__device__ __forceinline__ double nd_nan() { return __longlong_as_double(0x7FF8000000000000ll); }
__device__ __forceinline__ bool nd_finite3(float x, float y, float z) {
  return __builtin_isfinite(x) && __builtin_isfinite(y) && __builtin_isfinite(z);
}

// ------------------------------------------------------------------------------------------------------------------ the map

struct NdOrigin { const float* tgt; int Nt; float h; double* origin; };

__global__ __launch_bounds__(ND_BLOCK) void ndt_origin_kernel(NdOrigin p) {
  __shared__ float red[ND_BLOCK][3];
  __shared__ int any[ND_BLOCK];
  const int b = blockIdx.x, t = threadIdx.x;
  const float* x = p.tgt + (size_t)b * 3 * p.Nt;
  const float inf = __builtin_huge_valf();
  float lo[3] = {inf, inf, inf};
  int seen = 0;
  for (int i = t; i < p.Nt; i += ND_BLOCK) {
    const float a = x[i], c = x[p.Nt + i], d = x[2 * (size_t)p.Nt + i];
    if (nd_finite3(a, c, d)) { lo[0] = a < lo[0] ? a : lo[0]; lo[1] = c < lo[1] ? c : lo[1]; lo[2] = d < lo[2] ? d : lo[2]; seen = 1; }
  }
  for (int c = 0; c < 3; ++c) red[t][c] = lo[c];
  any[t] = seen;
  __syncthreads();
  if (t < 3) {                                             // (a minimum does not depend on its order; -0.0 and +0.0 give one origin)
    float m = inf;
    int s = 0;
    for (int i = 0; i < ND_BLOCK; ++i) { m = red[i][t] < m ? red[i][t] : m; s |= any[i]; }
    p.origin[(size_t)b * 3 + t] = s ? (double)m - 0.5 * (double)p.h : nd_nan();
  }
}

struct NdClear { nd_u64* keys; int* vals; long total; };

__global__ __launch_bounds__(ND_BLOCK) void ndt_clear_kernel(NdClear p) {
  const long i = (long)blockIdx.x * ND_BLOCK + threadIdx.x;
  if (i < p.total) { p.keys[i] = ND_EMPTY; p.vals[i] = -1; }
}

struct NdStats {
  const float* tgt; int B, Nt, slots; float h; int min_points; double min_eig_ratio;
  const int* members; const int* voxel_start; const int* voxel_points; const int* count; const double* origin;
  double* mean; double* inv_cov; int* valid; nd_u64* keys; int* vals;
};

__global__ __launch_bounds__(ND_BLOCK) void ndt_stats_kernel(NdStats p) {
  const long i = (long)blockIdx.x * ND_BLOCK + threadIdx.x;
  if (i >= (long)p.B * p.Nt) return;
  const int b = (int)(i / p.Nt), v = (int)(i % p.Nt), Nt = p.Nt;
  double* mean = p.mean + (size_t)b * 3 * Nt;
  double* A = p.inv_cov + (size_t)b * 6 * Nt;
  const int M = p.count[b] < Nt ? p.count[b] : Nt;         // (the grid's count; at most Nt, so 2 M + 2 <= slots)
  double mu[3] = {nd_nan(), nd_nan(), nd_nan()}, a6[6];
  for (int e = 0; e < 6; ++e) a6[e] = nd_nan();
  int ok = 0;
  const int n = v < M ? p.voxel_points[(size_t)b * Nt + v] : 0;
  const int s0 = v < M ? p.voxel_start[(size_t)b * Nt + v] : 0;
  if (n >= 1 && s0 >= 0 && (long)s0 + n <= Nt) {           // (the sort's lists; the range is checked, not trusted)
    const float* x = p.tgt + (size_t)b * 3 * Nt;
    const int* mem = p.members + (size_t)b * Nt + s0;
    int m0 = mem[0];
    m0 = m0 < 0 ? 0 : m0 >= Nt ? Nt - 1 : m0;
    double sx = (double)x[m0], sy = (double)x[Nt + m0], sz = (double)x[2 * (size_t)Nt + m0];
    for (int k = 1; k < n; ++k) {
      int m = mem[k];
      m = m < 0 ? 0 : m >= Nt ? Nt - 1 : m;
      sx = sx + (double)x[m]; sy = sy + (double)x[Nt + m]; sz = sz + (double)x[2 * (size_t)Nt + m];
    }
    const double dn = (double)n;
    mu[0] = sx / dn; mu[1] = sy / dn; mu[2] = sz / dn;
    // the voxel's key from its first member's cell (the grid's expression); the table takes every voxel
    const double h = (double)p.h;
    const double* og = p.origin + (size_t)b * 3;
    const nd_u64 cx = (nd_u64)floor(((double)x[m0] - og[0]) / h), cy = (nd_u64)floor(((double)x[Nt + m0] - og[1]) / h),
                 cz = (nd_u64)floor(((double)x[2 * (size_t)Nt + m0] - og[2]) / h);
    const nd_u64 key = cx | cy << 21 | cz << 42;
    const int lg = nd_log2_slots(M);
    const unsigned mask = (1u << lg) - 1u;
    nd_u64* keys = p.keys + (size_t)b * p.slots;
    unsigned slot = (unsigned)((key * ND_HASH) >> (64 - lg));
    for (unsigned probe = 0; probe <= mask; ++probe) {     // (2 M + 2 <= T <= slots: an empty word exists)
      const nd_u64 was = atomicCAS(keys + slot, ND_EMPTY, key);
      if (was == ND_EMPTY) { p.vals[(size_t)b * p.slots + slot] = v; break; }
      slot = (slot + 1u) & mask;
    }
    if (n >= p.min_points) {
      double cxx = 0., cxy = 0., cxz = 0., cyy = 0., cyz = 0., czz = 0.;
      for (int k = 0; k < n; ++k) {
        int m = mem[k];
        m = m < 0 ? 0 : m >= Nt ? Nt - 1 : m;
        const double dx = (double)x[m] - mu[0], dy = (double)x[Nt + m] - mu[1], dz = (double)x[2 * (size_t)Nt + m] - mu[2];
        cxx = cxx + dx * dx; cxy = cxy + dx * dy; cxz = cxz + dx * dz; cyy = cyy + dy * dy; cyz = cyz + dy * dz; czz = czz + dz * dz;
      }
      const double d1 = (double)(n - 1);
      double a00 = cxx / d1, a01 = cxy / d1, a02 = cxz / d1, a11 = cyy / d1, a12 = cyz / d1, a22 = czz / d1;
      const bool finite = __builtin_isfinite(a00) && __builtin_isfinite(a01) && __builtin_isfinite(a02) && __builtin_isfinite(a11) &&
                          __builtin_isfinite(a12) && __builtin_isfinite(a22);
      const bool zero = a00 == 0. && a01 == 0. && a02 == 0. && a11 == 0. && a12 == 0. && a22 == 0.;
      if (finite && !zero) {
        double v00 = 1., v01 = 0., v02 = 0., v10 = 0., v11 = 1., v12 = 0., v20 = 0., v21 = 0., v22 = 1.;
        for (int sweep = 0; sweep < NM_SWEEPS; ++sweep) {    // nm_point's sweeps, word for word
          if (a01 == 0. && a02 == 0. && a12 == 0.) break;
          nm_rotate(a00, a11, a01, a02, a12, v00, v01, v10, v11, v20, v21);
          nm_rotate(a00, a22, a02, a01, a12, v00, v02, v10, v12, v20, v22);
          nm_rotate(a11, a22, a12, a01, a02, v01, v02, v11, v12, v21, v22);
        }
        double lmax = a00 > a11 ? a00 : a11;
        lmax = lmax > a22 ? lmax : a22;
        if (lmax > 0.) {
          const double fl = p.min_eig_ratio * lmax;
          const double i0 = 1.0 / (a00 < fl ? fl : a00), i1 = 1.0 / (a11 < fl ? fl : a11), i2 = 1.0 / (a22 < fl ? fl : a22);
          const double V[3][3] = {{v00, v01, v02}, {v10, v11, v12}, {v20, v21, v22}};
          int e = 0;
          bool fin = true;
          for (int r = 0; r < 3; ++r)
            for (int c = r; c < 3; ++c) {
              const double s = ((V[r][0] * i0) * V[c][0] + (V[r][1] * i1) * V[c][1]) + (V[r][2] * i2) * V[c][2];
              a6[e++] = s;
              fin = fin && __builtin_isfinite(s);
            }
          ok = fin ? 1 : 0;
          if (!fin) for (int k = 0; k < 6; ++k) a6[k] = nd_nan();
        }
      }
    }
  }
  for (int c = 0; c < 3; ++c) mean[(size_t)c * Nt + v] = mu[c];
  for (int e = 0; e < 6; ++e) A[(size_t)e * Nt + v] = a6[e];
  p.valid[(size_t)b * Nt + v] = ok;
}

// ---------------------------------------------------------------------------------------------------------------- the round

struct NdRound {
  const float* src; int B, Ns, Nt, slots, nblk, neighbors; float h; double d2;
  const double* mean; const double* inv_cov; const int* valid; const int* count; const double* origin;
  const nd_u64* keys; const int* vals;
  NdState* st;
  double* part;                                            // [B][nblk][ND_VALUES]
  double* e_stage; int* voxel_stage;
};

// The voxel of a cell key, -1 for a miss: what the probe finds does not depend on the order the voxels entered in.
__device__ __forceinline__ int nd_lookup(const nd_u64* keys, const int* vals, int lg, nd_u64 key) {
  const unsigned mask = (1u << lg) - 1u;
  unsigned slot = (unsigned)((key * ND_HASH) >> (64 - lg));
  for (unsigned probe = 0; probe <= mask; ++probe) {
    const nd_u64 k = keys[slot];
    if (k == key) return vals[slot];
    if (k == ND_EMPTY) return -1;
    slot = (slot + 1u) & mask;
  }
  return -1;
}

// J_a . v of the header's chart at the point P
template <int A>
__device__ __forceinline__ double nd_jdot(const double* v, const double* P) {
  if constexpr (A == 0) return v[2] * P[1] - v[1] * P[2];
  else if constexpr (A == 1) return v[0] * P[2] - v[2] * P[0];
  else if constexpr (A == 2) return v[1] * P[0] - v[0] * P[1];
  else return v[A - 3];
}

template <int A>
struct NdRow {                                             // row A of the upper triangle: H_AB for B = A ... 5, statically indexed
  template <int Bc>
  static __device__ __forceinline__ void cols(double* H, const double* u, const double (*AJ)[3], const double* rAS, const double* P,
                                             double w, double nd2) {
    if constexpr (Bc < 6) {
      constexpr int e = A * 6 - (A * (A - 1)) / 2 + (Bc - A);   // the entry's place in the upper triangle by rows
      const double jaj = nd_jdot<Bc>(AJ[A], P);
      double inner = nd2 * (u[A] * u[Bc]) + jaj;
      if constexpr (Bc < 3) {
        constexpr int s = A == 0 ? Bc : A == 1 ? 2 + Bc : 5;   // rAS: 00, 01, 02, 11, 12, 22
        inner = inner + rAS[s];
      }
      H[e] = H[e] + w * inner;
      cols<Bc + 1>(H, u, AJ, rAS, P, w, nd2);
    }
  }
};

template <int A>
__device__ __forceinline__ void nd_fill(double* u, double (*AJ)[3], const double* Ar, const double (*Am)[3], const double* P) {
  if constexpr (A < 6) {
    u[A] = nd_jdot<A>(Ar, P);
    for (int i = 0; i < 3; ++i) AJ[A][i] = nd_jdot<A>(Am[i], P);
    nd_fill<A + 1>(u, AJ, Ar, Am, P);
  }
}

template <int A>
__device__ __forceinline__ void nd_rows(double* H, const double* u, const double (*AJ)[3], const double* rAS, const double* P, double w,
                                        double nd2) {
  if constexpr (A < 6) {
    NdRow<A>::template cols<A>(H, u, AJ, rAS, P, w, nd2);
    nd_rows<A + 1>(H, u, AJ, rAS, P, w, nd2);
  }
}

__global__ __launch_bounds__(ND_BLOCK) void ndt_round_kernel(NdRound p) {
  __shared__ double red[ND_BLOCK / 64][ND_VALUES];
  const int t = threadIdx.x;
  const int b = (int)(blockIdx.x / (unsigned)p.nblk), blk = (int)(blockIdx.x % (unsigned)p.nblk);
  const NdState& st = p.st[b];
  if (!st.live || !st.go) return;                          // (workgroup-uniform: a stopped cloud, a spent trial)
  const int n = blk * ND_BLOCK + t, Ns = p.Ns, Nt = p.Nt;
  double acc[ND_VALUES];
#pragma unroll
  for (int e = 0; e < ND_VALUES; ++e) acc[e] = 0.;
  const int M = p.count[b];
  if (n < Ns) {
    const float* sx = p.src + (size_t)b * 3 * Ns;
    float r[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) r[i] = (float)st.trial[i];
    const float x = sx[n], y = sx[Ns + n], z = sx[2 * (size_t)Ns + n];
    float pc[3];
    for (int c = 0; c < 3; ++c) pc[c] = fmaf(r[3 * c + 2], z, fmaf(r[3 * c + 1], y, r[3 * c] * x)) + r[9 + c];
    const double P[3] = {(double)pc[0], (double)pc[1], (double)pc[2]};
    const double h = (double)p.h;
    const double* og = p.origin + (size_t)b * 3;
    const double c0 = floor((P[0] - og[0]) / h), c1 = floor((P[1] - og[1]) / h), c2 = floor((P[2] - og[2]) / h);
    // (a NaN or infinite coordinate, and a NaN origin, fail the comparisons)
    const bool inside = M > 0 && M <= Nt && c0 >= 0. && c0 < ND_CELLS && c1 >= 0. && c1 < ND_CELLS && c2 >= 0. && c2 < ND_CELLS;
    const long cell0 = inside ? (long)c0 : 0, cell1 = inside ? (long)c1 : 0, cell2 = inside ? (long)c2 : 0;
    const int lg = nd_log2_slots(inside ? M : 0);
    const nd_u64* keys = p.keys + (size_t)b * p.slots;
    const int* vals = p.vals + (size_t)b * p.slots;
    const double* mean = p.mean + (size_t)b * 3 * Nt;
    const double* inv = p.inv_cov + (size_t)b * 6 * Nt;
    const double d2 = p.d2, nd2 = -d2, nd2h = -(d2 * 0.5);
    const size_t so = ((size_t)b * Ns + n) * 7;
    bool hit = false;
    for (int k = 0; k < 7; ++k) {                          // own, -x, +x, -y, +y, -z, +z
      int v = -1;
      if (inside && k < p.neighbors) {
        const int axis = (k - 1) >> 1;                     // (-1 for the own cell: no axis moves)
        const long step = k == 0 ? 0 : (k & 1) ? -1 : 1;
        const long q0 = cell0 + (axis == 0 ? step : 0), q1 = cell1 + (axis == 1 ? step : 0), q2 = cell2 + (axis == 2 ? step : 0);
        const long moved = axis == 0 ? q0 : axis == 1 ? q1 : q2;           // (the own cell is inside)
        if (moved >= 0 && moved < (long)VCR_VOXEL_MAX_CELLS) {
          v = nd_lookup(keys, vals, lg, (nd_u64)q0 | (nd_u64)q1 << 21 | (nd_u64)q2 << 42);
          if (v < 0 || v >= M || !p.valid[(size_t)b * Nt + v]) v = -1;      // (v < M <= Nt: the gathers below stay inside)
        }
      }
      double e = nd_nan();
      if (v >= 0) {
        hit = true;
        const double a00 = inv[v], a01 = inv[(size_t)Nt + v], a02 = inv[2 * (size_t)Nt + v], a11 = inv[3 * (size_t)Nt + v],
                     a12 = inv[4 * (size_t)Nt + v], a22 = inv[5 * (size_t)Nt + v];
        const double Am[3][3] = {{a00, a01, a02}, {a01, a11, a12}, {a02, a12, a22}};
        const double r0 = P[0] - mean[v], r1 = P[1] - mean[(size_t)Nt + v], r2 = P[2] - mean[2 * (size_t)Nt + v];
        double Ar[3];
        for (int i = 0; i < 3; ++i) Ar[i] = (Am[i][0] * r0 + Am[i][1] * r1) + Am[i][2] * r2;
        const double q = (r0 * Ar[0] + r1 * Ar[1]) + r2 * Ar[2];
        e = exp(nd2h * q);
        const double w = d2 * e;
        double u[6], AJ[6][3];
        nd_fill<0>(u, AJ, Ar, Am, P);
        const double rAS[6] = {-(Ar[1] * P[1] + Ar[2] * P[2]), Ar[0] * P[1], Ar[0] * P[2], -(Ar[0] * P[0] + Ar[2] * P[2]), Ar[1] * P[2],
                               -(Ar[0] * P[0] + Ar[1] * P[1])};
        acc[0] = acc[0] - e;
#pragma unroll
        for (int a = 0; a < 6; ++a) acc[2 + a] = acc[2 + a] + w * u[a];
        nd_rows<0>(acc + 8, u, AJ, rAS, P, w, nd2);
      }
      if (p.e_stage) p.e_stage[so + k] = e;
      if (p.voxel_stage) p.voxel_stage[so + k] = v;
    }
    acc[1] = hit ? 1. : 0.;
  }
#pragma unroll
  for (int e = 0; e < ND_VALUES; ++e) {                    // the refinements' order: the wave butterfly, then the four waves
    double v = acc[e];
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    if ((t & 63) == 0) red[t >> 6][e] = v;
  }
  __syncthreads();
  if (t < ND_VALUES) {
    double s = red[0][t];
    for (int w = 1; w < ND_BLOCK / 64; ++w) s += red[w][t];
    p.part[((size_t)b * p.nblk + blk) * ND_VALUES + t] = s;
  }
}

// A cloud's partials ascending from +0, one lane per value: the totals in LDS behind a barrier (every thread calls this)
__device__ __forceinline__ const double* nd_total(const double* part, int nblk) {
  __shared__ double tot[ND_VALUES];
  const int t = threadIdx.x;
  if (t < ND_VALUES) {
    double acc = 0.;
    for (int i = 0; i < nblk; ++i) acc += part[(size_t)i * ND_VALUES + t];
    tot[t] = acc;
  }
  __syncthreads();
  return tot;
}

struct NdPose { const float* R; const float* t; int B; NdState* st; };

__global__ __launch_bounds__(ND_BLOCK) void ndt_pose_kernel(NdPose p) {
  const int b = blockIdx.x * ND_BLOCK + threadIdx.x;
  if (b >= p.B) return;
  NdState& s = p.st[b];
  float r[12] = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f};
  if (p.R) {
    for (int i = 0; i < 9; ++i) r[i] = p.R[(size_t)b * 9 + i];
    for (int i = 0; i < 3; ++i) r[9 + i] = p.t[(size_t)b * 3 + i];
  }
  for (int i = 0; i < 12; ++i) { s.trial[i] = (double)r[i]; s.pose[i] = (double)r[i]; }
  s.live = 1; s.go = 1; s.iterations = 0; s.trials = 0; s.converged = 0; s.status = VCR_NDT_MAX_TRIALS;
  s.lambda = 0.; s.nu = 2.;
  for (int i = 0; i < 6; ++i) s.x[i] = 0.;
}

struct NdSums { const double* part; int nblk; double* score; int* hits; double* g; double* H; };

__global__ __launch_bounds__(64) void ndt_sums_kernel(NdSums p) {
  const int b = blockIdx.x, t = threadIdx.x;
  const double* v = nd_total(p.part + (size_t)b * p.nblk * ND_VALUES, p.nblk);
  if (t == 0) { p.score[b] = v[0]; p.hits[b] = (int)v[1]; }
  if (t >= 2 && t < 8) p.g[(size_t)b * 6 + t - 2] = v[t];
  if (t >= 8 && t < ND_VALUES) p.H[(size_t)b * 21 + t - 8] = v[t];
}

// ----------------------------------------------------------------------------------------------------------------- the loop

struct NdStep {
  const double* part; int nblk, round, max_iterations, max_trials; double rot_epsilon, trans_epsilon;
  NdState* st; double* trace;
};

// The next trial from the state (one lane): the solve, the pivot rule, the trial pose
__device__ void nd_propose(NdState& s) {
  double a21[21], g[6], x[6];
  for (int e = 0; e < 21; ++e) a21[e] = s.v[8 + e];
  a21[0] += s.lambda; a21[6] += s.lambda; a21[11] += s.lambda; a21[15] += s.lambda; a21[18] += s.lambda; a21[20] += s.lambda;
  for (int a = 0; a < 6; ++a) g[a] = s.v[2 + a];
  bool ok = pl_solve(a21, g, x);
  for (int a = 0; a < 6; ++a) ok = ok && __builtin_isfinite(x[a]);
  if (!ok) { s.lambda = s.lambda * s.nu; s.nu = s.nu * 2.0; s.go = 0; return; }
  double Ri[9], ti[3];
  pl_euler(x, Ri, ti);
  const double* R = s.pose;
  const double* tt = s.pose + 9;
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) s.trial[i * 3 + j] = (Ri[i * 3] * R[j] + Ri[i * 3 + 1] * R[3 + j]) + Ri[i * 3 + 2] * R[6 + j];
    s.trial[9 + i] = ((Ri[i * 3] * tt[0] + Ri[i * 3 + 1] * tt[1]) + Ri[i * 3 + 2] * tt[2]) + ti[i];
  }
  for (int a = 0; a < 6; ++a) s.x[a] = x[a];
  s.go = 1;
}

__global__ __launch_bounds__(64) void ndt_step_kernel(NdStep p) {
  const int b = blockIdx.x, t = threadIdx.x;
  NdState& s = p.st[b];
  const int live = s.live, went = s.go;                    // (read by every lane before lane 0 writes: a barrier follows)
  const double* v = nd_total(p.part + (size_t)b * p.nblk * ND_VALUES, p.nblk);
  if (t != 0) return;
  double* trace = p.trace ? p.trace + (size_t)b * (p.max_trials + 1) + p.round : nullptr;
  if (trace) *trace = nd_nan();
  if (!live) return;
  if (p.round > 0) s.trials += 1;
  if (p.round == 0 || went) {
    bool finite = true;
    for (int e = 0; e < ND_VALUES; ++e) finite = finite && __builtin_isfinite(v[e]);
    const bool few = v[1] < 3.0;
    if (p.round == 0) {
      for (int e = 0; e < ND_VALUES; ++e) s.v[e] = v[e];
      double m = 0.;
      const int dg[6] = {8, 14, 19, 23, 26, 28};
      for (int a = 0; a < 6; ++a) m = fabs(v[dg[a]]) > m ? fabs(v[dg[a]]) : m;
      s.lambda = 1e-5 * m; s.nu = 2.0;
      if (trace) *trace = v[0];
    }
    if (!finite || few) { s.live = 0; s.status = !finite ? VCR_NDT_NOT_FINITE : VCR_NDT_NO_HITS; return; }
    if (p.round > 0) {
      if (v[0] < s.v[0]) {
        for (int i = 0; i < 12; ++i) s.pose[i] = s.trial[i];
        for (int e = 0; e < ND_VALUES; ++e) s.v[e] = v[e];
        s.iterations += 1;
        s.lambda = s.lambda * (1.0 / 3.0); s.nu = 2.0;
        if (trace) *trace = v[0];
        double mr = 0., mt = 0.;
        for (int a = 0; a < 3; ++a) { mr = fabs(s.x[a]) > mr ? fabs(s.x[a]) : mr; mt = fabs(s.x[3 + a]) > mt ? fabs(s.x[3 + a]) : mt; }
        if (mr < p.rot_epsilon && mt < p.trans_epsilon) { s.live = 0; s.converged = 1; s.status = VCR_NDT_CONVERGED; return; }
      } else {
        s.lambda = s.lambda * s.nu; s.nu = s.nu * 2.0;
      }
    }
  }
  if (s.iterations >= p.max_iterations) { s.live = 0; s.status = VCR_NDT_MAX_ITERATIONS; return; }
  if (p.round >= p.max_trials) { s.live = 0; s.status = VCR_NDT_MAX_TRIALS; return; }
  nd_propose(s);
}

struct NdFinish {
  const NdState* st; int B, Ns; double d1;
  float* R_out; float* t_out; float* R_ba; float* t_ba; double* score; double* probability; int* hits; double* g; double* H;
  int* iterations; int* trials; int* converged; int* status;
};

__global__ __launch_bounds__(ND_BLOCK) void ndt_finish_kernel(NdFinish p) {
  const int b = blockIdx.x * ND_BLOCK + threadIdx.x;
  if (b >= p.B) return;
  const NdState& s = p.st[b];
  float r[12];
  for (int i = 0; i < 12; ++i) r[i] = (float)s.pose[i];
  for (int i = 0; i < 9; ++i) p.R_out[(size_t)b * 9 + i] = r[i];
  for (int i = 0; i < 3; ++i) p.t_out[(size_t)b * 3 + i] = r[9 + i];
  for (int i = 0; i < 3; ++i) {                            // the refinements' inverse (pose_step_kernel's expression)
    if (p.R_ba) for (int j = 0; j < 3; ++j) p.R_ba[(size_t)b * 9 + i * 3 + j] = r[j * 3 + i];
    if (p.t_ba) p.t_ba[(size_t)b * 3 + i] = -fmaf(r[6 + i], r[11], fmaf(r[3 + i], r[10], r[i] * r[9]));
  }
  if (p.score) p.score[b] = s.v[0];
  if (p.probability) p.probability[b] = ((-p.d1) * (-s.v[0])) / (double)p.Ns;
  if (p.hits) p.hits[b] = (int)s.v[1];
  if (p.g) for (int a = 0; a < 6; ++a) p.g[(size_t)b * 6 + a] = s.v[2 + a];
  if (p.H) for (int e = 0; e < 21; ++e) p.H[(size_t)b * 21 + e] = s.v[8 + e];
  if (p.iterations) p.iterations[b] = s.iterations;
  if (p.trials) p.trials[b] = s.trials;
  if (p.converged) p.converged[b] = s.converged;
  if (p.status) p.status[b] = s.status;
}

// --------------------------------------------------------------------------------------------------------------------- host

int nd_slots(int Nt) { return Nt < 1 || Nt > ND_MAX_N ? 0 : 1 << nd_log2_slots(Nt); }

struct NdMapPlan { vcr_voxel_args va; vcr_voxel_sort_args sa; size_t points, members, start, sort, bytes; int slots; };

int nd_map_plan(const vcr_ndt_map_args& a, bool building, NdMapPlan* p) {
  *p = NdMapPlan{};
  if (a.B < 1 || a.Nt < 1 || !a.mean || !a.inv_cov || !a.valid || !a.count || !a.origin || !a.table_keys || !a.table_vals)
    return VCR_EINVAL;
  if (!(a.resolution > 0.f) || a.resolution == __builtin_huge_valf()) return VCR_EINVAL;
  if (building && (!a.tgt || !a.voxel_points || a.min_points < 3 || !(a.min_eig_ratio > 0. && a.min_eig_ratio <= 1.))) return VCR_EINVAL;
  if (a.Nt > ND_MAX_N || (long)a.B * a.Nt >= (1L << 31)) return VCR_EUNSUPPORTED;
  p->slots = nd_slots(a.Nt);
  if (!building) return VCR_OK;
  const size_t BN = (size_t)a.B * a.Nt;
  p->points = 0;
  p->members = p->points + ws_up(BN * 12);
  p->start = p->members + ws_up(BN * 4);
  p->sort = p->start + ws_up(BN * 4);
  p->va = vcr_voxel_args{};
  p->va.struct_bytes = (uint32_t)sizeof(vcr_voxel_args);
  p->va.xyz = a.tgt; p->va.B = a.B; p->va.N = a.Nt; p->va.voxel_size = a.resolution;
  p->va.points = reinterpret_cast<float*>((uintptr_t)256);     // (placeholders: the sizes do not look at them)
  p->va.count = a.count; p->va.voxel_points = a.voxel_points;
  p->sa = vcr_voxel_sort_args{};
  p->sa.struct_bytes = (uint32_t)sizeof(vcr_voxel_sort_args);
  p->sa.members = reinterpret_cast<int*>((uintptr_t)256); p->sa.voxel_start = reinterpret_cast<int*>((uintptr_t)256);
  const size_t sort = vcr_voxel_sort_workspace_bytes(&p->va, &p->sa, 1);
  if (!sort) return VCR_EINVAL;
  p->bytes = p->sort + sort;
  return VCR_OK;
}

int nd_map_take(const vcr_ndt_map_args* user, vcr_ndt_map_args* mine) { return vcr_take_args(user, mine, sizeof(vcr_ndt_map_args)); }
int nd_take(const vcr_ndt_args* user, vcr_ndt_args* mine) { return vcr_take_args(user, mine, offsetof(vcr_ndt_args, max_iterations)); }

struct NdPlan { int nblk, launches, slots; size_t state, part, bytes; };

int nd_plan(const vcr_ndt_map_args& m, const vcr_ndt_args& a, bool loop, NdPlan* p) {
  *p = NdPlan{};
  NdMapPlan mp;
  const int e = nd_map_plan(m, false, &mp);
  if (e) return e;
  if (!a.src || a.Ns < 1 || (a.neighbors != 1 && a.neighbors != 7) || (a.R == nullptr) != (a.t == nullptr)) return VCR_EINVAL;
  if (!__builtin_isfinite(a.d1) || !__builtin_isfinite(a.d2) || !(a.d2 > 0.) || a.variant < 0 || a.variant > 1) return VCR_EINVAL;
  if (!loop && (!a.score || !a.hits || !a.g || !a.H)) return VCR_EINVAL;
  if (loop && (!a.R_out || !a.t_out || a.max_iterations < 0 || a.max_trials < 0 || !(a.rot_epsilon >= 0.) || !(a.trans_epsilon >= 0.)))
    return VCR_EINVAL;
  if (a.Ns > ND_MAX_N || (long)m.B * a.Ns >= (1L << 31) || (loop && a.max_trials > (1 << 20))) return VCR_EUNSUPPORTED;
  p->slots = mp.slots;
  p->nblk = (a.Ns + ND_BLOCK - 1) / ND_BLOCK;
  p->launches = loop ? 2 * (a.max_trials + 1) + 2 : 3;
  p->state = 0;
  p->part = ws_up((size_t)m.B * sizeof(NdState));
  p->bytes = p->part + ws_up((size_t)m.B * p->nblk * ND_VALUES * sizeof(double));
  return VCR_OK;
}

int nd_form(const vcr_ndt_map_args* um, const vcr_ndt_args* ua, bool loop, int cu_count, int* lanes, int* nblk, int* launches) {
  vcr_ndt_map_args m;
  vcr_ndt_args a;
  NdPlan p;
  if (nd_map_take(um, &m) || nd_take(ua, &a) || cu_count < 0) return VCR_EINVAL;
  const int e = nd_plan(m, a, loop, &p);
  if (e) return e;
  if (lanes) *lanes = 1;
  if (nblk) *nblk = p.nblk;
  if (launches) *launches = p.launches;
  return VCR_OK;
}

size_t nd_bytes(const vcr_ndt_map_args* um, const vcr_ndt_args* ua, bool loop, int cu_count) {
  vcr_ndt_map_args m;
  vcr_ndt_args a;
  NdPlan p;
  if (nd_map_take(um, &m) || nd_take(ua, &a) || cu_count < 0) return 0;
  return nd_plan(m, a, loop, &p) ? 0 : p.bytes;
}

NdRound nd_round(const vcr_ndt_map_args& m, const vcr_ndt_args& a, const NdPlan& p, NdState* st, double* part) {
  return NdRound{a.src, m.B, a.Ns, m.Nt, p.slots, p.nblk, a.neighbors, m.resolution, a.d2, m.mean, m.inv_cov, m.valid, m.count, m.origin,
                 reinterpret_cast<const nd_u64*>(m.table_keys), m.table_vals, st, part, a.e_stage, a.voxel_stage};
}

unsigned nd_grid(long lanes) { return (unsigned)((lanes + ND_BLOCK - 1) / ND_BLOCK); }

}  // namespace

extern "C" int vcr_ndt_table_slots(int Nt) { return nd_slots(Nt); }

extern "C" int vcr_ndt_map_form(const vcr_ndt_map_args* ua, int cu_count, int* lanes_per_voxel, int* table_slots) {
  vcr_ndt_map_args a;
  NdMapPlan p;
  if (nd_map_take(ua, &a) || cu_count < 0) return VCR_EINVAL;
  const int e = nd_map_plan(a, true, &p);
  if (e) return e;
  if (lanes_per_voxel) *lanes_per_voxel = 1;
  if (table_slots) *table_slots = p.slots;
  return VCR_OK;
}

extern "C" size_t vcr_ndt_map_workspace_bytes(const vcr_ndt_map_args* ua, int cu_count) {
  vcr_ndt_map_args a;
  NdMapPlan p;
  if (nd_map_take(ua, &a) || cu_count < 0) return 0;
  return nd_map_plan(a, true, &p) ? 0 : p.bytes;
}

extern "C" int vcr_ndt_map_f32(const vcr_ndt_map_args* ua, void* workspace, size_t workspace_bytes, vcr_stream_t stream) {
  vcr_ndt_map_args a;
  if (nd_map_take(ua, &a)) return VCR_EINVAL;
  NdMapPlan p;
  int e = nd_map_plan(a, true, &p);
  if (e) return e;
  if (!workspace || (((uintptr_t)workspace) & 15)) return VCR_EINVAL;
  if (workspace_bytes < p.bytes) return VCR_EWORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  unsigned char* w = reinterpret_cast<unsigned char*>(workspace);
  p.va.points = reinterpret_cast<float*>(w + p.points);
  p.sa.members = reinterpret_cast<int*>(w + p.members);
  p.sa.voxel_start = reinterpret_cast<int*>(w + p.start);
  if ((e = vcr_voxel_sort_f32(&p.va, &p.sa, w + p.sort, p.bytes - p.sort, stream))) return e;
  const NdOrigin og{a.tgt, a.Nt, a.resolution, a.origin};
  hipLaunchKernelGGL(ndt_origin_kernel, dim3((unsigned)a.B), dim3(ND_BLOCK), 0, s, og);
  if ((e = VCR_LAUNCH_RC())) return e;
  const NdClear cl{reinterpret_cast<nd_u64*>(a.table_keys), a.table_vals, (long)a.B * p.slots};
  hipLaunchKernelGGL(ndt_clear_kernel, dim3(nd_grid(cl.total)), dim3(ND_BLOCK), 0, s, cl);
  if ((e = VCR_LAUNCH_RC())) return e;
  const NdStats sp{a.tgt, a.B, a.Nt, p.slots, a.resolution, a.min_points, a.min_eig_ratio, p.sa.members, p.sa.voxel_start, a.voxel_points,
                   a.count, a.origin, a.mean, a.inv_cov, a.valid, reinterpret_cast<nd_u64*>(a.table_keys), a.table_vals};
  hipLaunchKernelGGL(ndt_stats_kernel, dim3(nd_grid((long)a.B * a.Nt)), dim3(ND_BLOCK), 0, s, sp);
  return VCR_LAUNCH_RC();
}

extern "C" size_t vcr_ndt_derivatives_workspace_bytes(const vcr_ndt_map_args* m, const vcr_ndt_args* a, int cu_count) {
  return nd_bytes(m, a, false, cu_count);
}
extern "C" size_t vcr_ndt_workspace_bytes(const vcr_ndt_map_args* m, const vcr_ndt_args* a, int cu_count) {
  return nd_bytes(m, a, true, cu_count);
}
extern "C" int vcr_ndt_derivatives_form(const vcr_ndt_map_args* m, const vcr_ndt_args* a, int cu_count, int* lanes, int* nblk, int* launches) {
  return nd_form(m, a, false, cu_count, lanes, nblk, launches);
}
extern "C" int vcr_ndt_form(const vcr_ndt_map_args* m, const vcr_ndt_args* a, int cu_count, int* lanes, int* nblk, int* launches) {
  return nd_form(m, a, true, cu_count, lanes, nblk, launches);
}

extern "C" int vcr_ndt_derivatives_f32(const vcr_ndt_map_args* um, const vcr_ndt_args* ua, void* workspace, size_t workspace_bytes,
                                       vcr_stream_t stream) {
  vcr_ndt_map_args m;
  vcr_ndt_args a;
  if (nd_map_take(um, &m) || nd_take(ua, &a)) return VCR_EINVAL;
  NdPlan p;
  int e = nd_plan(m, a, false, &p);
  if (e) return e;
  if (!workspace || (((uintptr_t)workspace) & 15)) return VCR_EINVAL;
  if (workspace_bytes < p.bytes) return VCR_EWORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  unsigned char* w = reinterpret_cast<unsigned char*>(workspace);
  NdState* st = reinterpret_cast<NdState*>(w + p.state);
  double* part = reinterpret_cast<double*>(w + p.part);
  hipLaunchKernelGGL(ndt_pose_kernel, dim3(nd_grid(m.B)), dim3(ND_BLOCK), 0, s, NdPose{a.R, a.t, m.B, st});
  if ((e = VCR_LAUNCH_RC())) return e;
  hipLaunchKernelGGL(ndt_round_kernel, dim3((unsigned)((long)m.B * p.nblk)), dim3(ND_BLOCK), 0, s, nd_round(m, a, p, st, part));
  if ((e = VCR_LAUNCH_RC())) return e;
  hipLaunchKernelGGL(ndt_sums_kernel, dim3((unsigned)m.B), dim3(64), 0, s, NdSums{part, p.nblk, a.score, a.hits, a.g, a.H});
  return VCR_LAUNCH_RC();
}

extern "C" int vcr_ndt_f32(const vcr_ndt_map_args* um, const vcr_ndt_args* ua, void* workspace, size_t workspace_bytes,
                           vcr_stream_t stream) {
  vcr_ndt_map_args m;
  vcr_ndt_args a;
  if (nd_map_take(um, &m) || nd_take(ua, &a)) return VCR_EINVAL;
  NdPlan p;
  int e = nd_plan(m, a, true, &p);
  if (e) return e;
  if (!workspace || (((uintptr_t)workspace) & 15)) return VCR_EINVAL;
  if (workspace_bytes < p.bytes) return VCR_EWORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  unsigned char* w = reinterpret_cast<unsigned char*>(workspace);
  NdState* st = reinterpret_cast<NdState*>(w + p.state);
  double* part = reinterpret_cast<double*>(w + p.part);
  hipLaunchKernelGGL(ndt_pose_kernel, dim3(nd_grid(m.B)), dim3(ND_BLOCK), 0, s, NdPose{a.R, a.t, m.B, st});
  if ((e = VCR_LAUNCH_RC())) return e;
  vcr_ndt_args stages = a;                                 // the staged outputs are the derivative call's: the loop's rounds write none
  stages.e_stage = nullptr; stages.voxel_stage = nullptr;
  const NdRound rd = nd_round(m, stages, p, st, part);
  for (int round = 0; round <= a.max_trials; ++round) {
    hipLaunchKernelGGL(ndt_round_kernel, dim3((unsigned)((long)m.B * p.nblk)), dim3(ND_BLOCK), 0, s, rd);
    if ((e = VCR_LAUNCH_RC())) return e;
    const NdStep sp{part, p.nblk, round, a.max_iterations, a.max_trials, a.rot_epsilon, a.trans_epsilon, st, a.trace};
    hipLaunchKernelGGL(ndt_step_kernel, dim3((unsigned)m.B), dim3(64), 0, s, sp);
    if ((e = VCR_LAUNCH_RC())) return e;
  }
  const NdFinish fn{st, m.B, a.Ns, a.d1, a.R_out, a.t_out, a.R_ba, a.t_ba, a.score, a.probability, a.hits, a.g, a.H,
                    a.iterations, a.trials, a.converged, a.status};
  hipLaunchKernelGGL(ndt_finish_kernel, dim3(nd_grid(m.B)), dim3(ND_BLOCK), 0, s, fn);
  return VCR_LAUNCH_RC();
}

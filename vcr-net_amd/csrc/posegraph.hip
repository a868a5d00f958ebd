// Pose-graph optimisation (include/posegraph/vcr_hip_posegraph.h): Levenberg-Marquardt with a line
// process over the uncertain edges and the pruning pass, the whole loop of a graph in ONE launch by ONE workgroup -- the manner
// of fgr_solve_kernel.  Decisions are taken by lane 0 and read by all from LDS behind a barrier, so every barrier is reached by
// every lane.  fp64 throughout, no atomic, no fma (the build has -ffp-contract=off): tests/posegraph_restated.py repeats the
// edge terms operation by operation.
#include "common.h"
#include "refine_solve6.h"
#include "../../include/posegraph/vcr_hip_posegraph.h"

namespace {

constexpr int PG_BLOCK = 256, PG_WAVES = PG_BLOCK / 64;
constexpr int PG_EW = 29;                                  // doubles an edge: W's upper triangle by rows (21), g (6), q, s
constexpr int PG_Q = 27, PG_S = 28;
constexpr int PG_LDS_LIMIT = 160 * 1024;                   // an MI355X CU's LDS, all of which one workgroup may take
constexpr int PG_LDS_GRANULE = 1280;                       // what gfx950 allocates LDS in (320 dwords: LLVM's target description)
constexpr int PG_STATIC_LDS = 4096;                        // the kernel's static __shared__ below, rounded up

enum { CD_LAMBDA, CD_NU, CD_RES, CD_MU, CD_DENOM, CD_SUM, CD_N };
enum { CI_STOP, CI_ACCEPT, CI_FAIL, CI_CONV, CI_N };        // CI_STOP: 0 go on, 1 the pass ends, 2 the call ends

struct PgParams {
  int K, E, anchor, prune, max_it, max_lm;
  double mcd2, thr, mri, mrri, mrt, mres, lsf;
  const double* R; const double* t; const int* src; const int* dst; const double* Re; const double* te; const double* info;
  const int* unc;
  double* Hg; double* Lg; double* ed; int* st; int* inc;    // the workspace, per-graph strides below
  size_t nbd;                                               // doubles of a packed H
  double* R_out; double* t_out; double* weight; int* kept; double* residual; int* iterations; int* converged;
  int* trials; double* H; double* b; double* residual0; double* l0; double* delta0; double* lambda0;
};

__host__ __device__ constexpr int pg_blk(int i, int j) { return i * (i + 1) / 2 + j; }       // block (i, j), j <= i, of the packed lower triangle
__host__ __device__ constexpr int pg_wi(int r, int c) {                                       // W[r][c] in the upper triangle by rows
  return r <= c ? r * 6 - r * (r - 1) / 2 + (c - r) : c * 6 - c * (c - 1) / 2 + (r - c);
}

__device__ __forceinline__ double pg_dot3(double a0, double b0, double a1, double b1, double a2, double b2) {
  return (a0 * b0 + a1 * b1) + a2 * b2;
}

// The sum of one term an edge in ASCENDING EDGE INDEX, whatever lane computed it: 256 terms at a time go through LDS and lane 0
// adds them in order (a blank's term is +0).  Every lane returns the sum.
template <class F>
__device__ __forceinline__ double pg_edge_sum(int E, int t, double* chunk, double* wsum, F term) {
  double a = 0.;                                            // (lane 0's)
  for (int base = 0; base < E; base += PG_BLOCK) {
    const int e = base + t;
    chunk[t] = e < E ? term(e) : 0.;
    __syncthreads();
    if (t == 0) {
      const int n = E - base < PG_BLOCK ? E - base : PG_BLOCK;
      for (int i = 0; i < n; ++i) a += chunk[i];
    }
    __syncthreads();
  }
  if (t == 0) wsum[0] = a;
  __syncthreads();
  a = wsum[0];
  __syncthreads();                                          // wsum[0] is free again
  return a;
}

__device__ __forceinline__ double pg_nanmax(double a, double b) { return a != a ? a : b != b ? b : (a > b ? a : b); }

__device__ __forceinline__ double pg_wg_max(double v, int t, double* wsum) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v = pg_nanmax(v, __shfl_xor(v, o, 64));
  __syncthreads();
  if ((t & 63) == 0) wsum[t >> 6] = v;
  __syncthreads();
  return pg_nanmax(pg_nanmax(wsum[0], wsum[1]), pg_nanmax(wsum[2], wsum[3]));
}

// vec6 of (M, tM): the inverse of pl_euler
__device__ __forceinline__ void pg_vec6(const double* M, const double* tM, double* r) {
  const double sy = sqrt(M[0] * M[0] + M[3] * M[3]);
  if (sy > 1e-6) {
    r[0] = atan2(M[7], M[8]); r[1] = atan2(-M[6], sy); r[2] = atan2(M[3], M[0]);
  } else {
    r[0] = atan2(-M[5], M[4]); r[1] = atan2(-M[6], sy); r[2] = 0.;
  }
  r[3] = tM[0]; r[4] = tM[1]; r[5] = tM[2];
}

// The edge's M = X^-1 T_dst^-1 T_src from the poses Ps, Pd (R row-major, then t): RP = R_e^T R_d^T, RM = RP R_s,
// tM = R_e^T (R_d^T (t_s - t_d) - t_e)
__device__ __forceinline__ void pg_edge_m(const double* Ps, const double* Pd, const double* Re, const double* te, double* RP,
                                          double* RM, double* tM) {
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j)
      RP[3 * i + j] = pg_dot3(Re[i], Pd[3 * j], Re[3 + i], Pd[3 * j + 1], Re[6 + i], Pd[3 * j + 2]);
  const double w0 = Ps[9] - Pd[9], w1 = Ps[10] - Pd[10], w2 = Ps[11] - Pd[11];
  double v[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) v[k] = pg_dot3(Pd[k], w0, Pd[3 + k], w1, Pd[6 + k], w2) - te[k];
#pragma unroll
  for (int i = 0; i < 3; ++i) tM[i] = pg_dot3(Re[i], v[0], Re[3 + i], v[1], Re[6 + i], v[2]);
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j)
      RM[3 * i + j] = pg_dot3(RP[3 * i], Ps[j], RP[3 * i + 1], Ps[3 + j], RP[3 * i + 2], Ps[6 + j]);
}

__device__ __forceinline__ double pg_dot6(const double* a, const double* b) {
  return ((((a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]) + a[3] * b[3]) + a[4] * b[4]) + a[5] * b[5];
}

// q = r^T info r of edge e at the poses P (LDS)
__device__ __forceinline__ double pg_edge_q(const double* P, int s, int d, const double* Re, const double* te, const double* info) {
  double Ps[12], Pd[12], RP[9], RM[9], tM[3], r[6], u[6];
#pragma unroll
  for (int k = 0; k < 12; ++k) { Ps[k] = P[12 * s + k]; Pd[k] = P[12 * d + k]; }
  pg_edge_m(Ps, Pd, Re, te, RP, RM, tM);
  pg_vec6(RM, tM, r);
#pragma unroll
  for (int p = 0; p < 6; ++p) {
    double row[6];
#pragma unroll
    for (int c = 0; c < 6; ++c) row[c] = info[6 * p + c];
    u[p] = pg_dot6(row, r);
  }
  return pg_dot6(r, u);
}

// The linearisation of edge e at the poses P: W = J^T info J (upper triangle), g = J^T info r, q; J = J_src.  Written to ed
// (field v of edge e at ed[v * E + e]).
__device__ __forceinline__ double pg_edge_lin(const double* P, int s, int d, const double* Re, const double* te, const double* info,
                                              double* ed, int E, int e) {
  double Ps[12], Pd[12], RP[9], RM[9], tM[3], r[6];
#pragma unroll
  for (int k = 0; k < 12; ++k) { Ps[k] = P[12 * s + k]; Pd[k] = P[12 * d + k]; }
  pg_edge_m(Ps, Pd, Re, te, RP, RM, tM);
  pg_vec6(RM, tM, r);
  double J[6][6];                                           // J[p][k]: component p of lin6, generator k
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int k1 = (k + 1) % 3, k2 = (k + 2) % 3;
    double N[9];                                            // R_P [e_k]x R_s
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j) N[3 * i + j] = RP[3 * i + k2] * Ps[3 * k1 + j] - RP[3 * i + k1] * Ps[3 * k2 + j];
    J[0][k] = (N[7] - N[5]) * 0.5; J[1][k] = (N[2] - N[6]) * 0.5; J[2][k] = (N[3] - N[1]) * 0.5;
#pragma unroll
    for (int i = 0; i < 3; ++i) J[3 + i][k] = RP[3 * i + k2] * Ps[9 + k1] - RP[3 * i + k1] * Ps[9 + k2];
#pragma unroll
    for (int i = 0; i < 3; ++i) { J[i][3 + k] = 0.; J[3 + i][3 + k] = RP[3 * i + k]; }
  }
  double L[6][6];
#pragma unroll
  for (int p = 0; p < 6; ++p)
#pragma unroll
    for (int c = 0; c < 6; ++c) L[p][c] = info[6 * p + c];
  double u[6];
#pragma unroll
  for (int p = 0; p < 6; ++p) u[p] = pg_dot6(L[p], r);
  const double q = pg_dot6(r, u);
#pragma unroll
  for (int k = 0; k < 6; ++k) {
    double col[6];
#pragma unroll
    for (int p = 0; p < 6; ++p) col[p] = J[p][k];
    ed[(size_t)(21 + k) * E + e] = pg_dot6(col, u);         // g_k
    double c[6];                                            // info J[:, k]
#pragma unroll
    for (int p = 0; p < 6; ++p) c[p] = pg_dot6(L[p], col);
#pragma unroll
    for (int k0 = 0; k0 <= k; ++k0) {
      double col0[6];
#pragma unroll
      for (int p = 0; p < 6; ++p) col0[p] = J[p][k0];
      ed[(size_t)pg_wi(k0, k) * E + e] = pg_dot6(col0, c);
    }
  }
  ed[(size_t)PG_Q * E + e] = q;
  return q;
}

// (R, t) <- euler(x) (R, t)
__device__ __forceinline__ void pg_step(const double* x, const double* Pi, double* Po) {
  double Ri[9], ti[3];
  pl_euler(x, Ri, ti);
#pragma unroll
  for (int r = 0; r < 3; ++r) {
#pragma unroll
    for (int c = 0; c < 3; ++c) Po[3 * r + c] = pg_dot3(Ri[3 * r], Pi[c], Ri[3 * r + 1], Pi[3 + c], Ri[3 * r + 2], Pi[6 + c]);
    Po[9 + r] = pg_dot3(Ri[3 * r], Pi[9], Ri[3 * r + 1], Pi[10], Ri[3 * r + 2], Pi[11]) + ti[r];
  }
}

// |vec6(T)|^2 of a pose, its six squares added in order
__device__ __forceinline__ double pg_x2(const double* Pi) {
  double r[6];
  pg_vec6(Pi, Pi + 9, r);
  return pg_dot6(r, r);
}

template <int FORM>
__global__ __launch_bounds__(PG_BLOCK) void posegraph_kernel(PgParams p) {
  extern __shared__ __attribute__((aligned(16))) double dyn[];
  __shared__ double wsum[PG_WAVES];
  __shared__ double chunk[PG_BLOCK];
  __shared__ int cflag[PG_BLOCK];
  __shared__ double cd[CD_N];
  __shared__ int ci[CI_N];
  const int t = threadIdx.x, K = p.K, E = p.E;
  const size_t g = blockIdx.x;
  double* P = dyn;                                          // [K][12] the poses
  double* Pn = P + 12 * K;                                  // [K][12] the trial poses
  double* bv = Pn + 12 * K;                                 // [6K]
  double* yv = bv + 6 * K;                                  // [6K] the right side, then y, then d
  double* xn = yv + 6 * K;                                  // [K] |vec6(T_i)|^2
  int* off = reinterpret_cast<int*>(xn + K);                // [K + 1] the incidence lists' starts
  double* Hg = p.Hg + g * p.nbd;
  double* L;
  if (FORM == VCR_POSEGRAPH_FORM_LDS) L = reinterpret_cast<double*>(off + ((K + 2) & ~1));
  else L = p.Lg + g * p.nbd;
  double* ed = p.ed + g * (size_t)PG_EW * E;
  int* st = p.st + g * E;                                   // bit 0: no blank; bit 1: uncertain; bit 2: no blank at entry
  int* inc = p.inc + g * 2 * (size_t)E;
  const int* src = p.src + g * E;
  const int* dst = p.dst + g * E;
  const double* Re = p.Re + g * 9 * (size_t)E;
  const double* te = p.te + g * 3 * (size_t)E;
  const double* info = p.info + g * 36 * (size_t)E;
  const int nb = K * (K + 1) / 2;

  // ---- the poses, the edges' status, the incidence lists (once a call, in edge order: a node a lane)
  for (int i = t; i < K; i += PG_BLOCK) {
#pragma unroll
    for (int k = 0; k < 9; ++k) P[12 * i + k] = p.R[(g * K + i) * 9 + k];
#pragma unroll
    for (int k = 0; k < 3; ++k) P[12 * i + 9 + k] = p.t[(g * K + i) * 3 + k];
  }
  for (int e = t; e < E; e += PG_BLOCK) {
    const int s = src[e], d = dst[e];
    const bool valid = s >= 0 && s < K && d >= 0 && d < K && s != d;
    st[e] = valid ? (5 | (p.unc[g * E + e] ? 2 : 0)) : 0;
  }
  if (t < CI_N) ci[t] = 0;
  if (t < 2) { p.iterations[g * 2 + t] = 0; if (p.trials) p.trials[g * 2 + t] = 0; }
  __syncthreads();
  for (int i = t; i < K; i += PG_BLOCK) {
    xn[i] = pg_x2(P + 12 * i);
    int n = 0;
    for (int e = 0; e < E; ++e)
      if ((st[e] & 1) && (src[e] == i || dst[e] == i)) ++n;
    off[i + 1] = n;
  }
  __syncthreads();
  if (t == 0) {
    off[0] = 0;
    for (int i = 0; i < K; ++i) off[i + 1] += off[i];
  }
  __syncthreads();
  for (int i = t; i < K; i += PG_BLOCK) {
    int n = off[i];
    for (int e = 0; e < E; ++e)
      if ((st[e] & 1) && (src[e] == i || dst[e] == i)) inc[n++] = e;
  }
  __syncthreads();

  double res_first = 0.;
  int conv = 0;
  const int passes = p.prune && p.max_it > 0 ? 2 : 1;        // (no iteration: one linearisation, nothing is pruned)
  for (int pass = 0; pass < passes; ++pass) {
    // ---- mu: the mean of info[5][5] over the uncertain edges, added in edge order (256 at a time through LDS)
    if (t == 0) { cd[CD_SUM] = 0.; ci[CI_CONV] = 0; }
    {
      int n = 0;                                            // (lane 0's)
      for (int base = 0; base < E; base += PG_BLOCK) {
        const int e = base + t;
        const bool in = e < E && (st[e] & 3) == 3;
        cflag[t] = in ? 1 : 0;
        chunk[t] = in ? info[(size_t)e * 36 + 35] : 0.;
        __syncthreads();
        if (t == 0) {
          double a = cd[CD_SUM];
          for (int i = 0; i < PG_BLOCK; ++i)
            if (cflag[i]) { a += chunk[i]; ++n; }
          cd[CD_SUM] = a;
        }
        __syncthreads();
      }
      if (t == 0) cd[CD_MU] = n > 0 ? p.mcd2 * (cd[CD_SUM] / (double)n) : 0.;
    }
    __syncthreads();
    const double mu = cd[CD_MU];

    int outer = 0, ntrials = 0, stop = 0, lm = 0;
    bool first_build = true, need_build = true;
    // A step of this loop: (re)build l, H, b at P where a trial was taken, then one trial.  outer, lm, stop and need_build are
    // the same in every lane: they follow from LDS words read behind a barrier.
    while (true) {
      if (need_build) {
        // ---- linearise: an edge a lane
        const double res_built = pg_edge_sum(E, t, chunk, wsum, [&](int e) {
          const int f = st[e];
          if (!(f & 1)) return 0.;
          const double q = pg_edge_lin(P, src[e], dst[e], Re + (size_t)e * 9, te + (size_t)e * 3, info + (size_t)e * 36, ed, E, e);
          double s = 1., pen = 0.;
          if (f & 2) {
            s = mu / (mu + q);
            pen = mu * ((s - 1.) * (s - 1.));
          }
          ed[(size_t)PG_S * E + e] = s;
          return (s * s) * q + pen;
        });
        for (int i = t; i < nb * 36; i += PG_BLOCK) Hg[i] = 0.;
        __syncthreads();                                      // ed and the zeros are visible
        // ---- assemble: entry v of node a's block row a lane, its edges in ascending order
        for (int it = t; it < K * 42; it += PG_BLOCK) {
          const int a = it / 42, v = it % 42;
          const bool anchor = a == p.anchor;
          double acc = 0.;
          if (v < 36) {
            const int wi = pg_wi(v / 6, v % 6);
            for (int n = off[a]; n < off[a + 1]; ++n) {
              const int e = inc[n];
              if (!(st[e] & 1)) continue;
              const double s = ed[(size_t)PG_S * E + e];
              const double term = (s * s) * ed[(size_t)wi * E + e];
              acc += term;
              const int sa = src[e], o = sa == a ? dst[e] : sa;
              if (o < a && !anchor && o != p.anchor) Hg[(size_t)pg_blk(a, o) * 36 + v] -= term;
            }
            Hg[(size_t)pg_blk(a, a) * 36 + v] = anchor ? (v % 7 == 0 ? 1. : 0.) : acc;
          } else {
            const int c = v - 36;
            for (int n = off[a]; n < off[a + 1]; ++n) {
              const int e = inc[n];
              if (!(st[e] & 1)) continue;
              const double s = ed[(size_t)PG_S * E + e];
              const double term = (s * s) * ed[(size_t)(21 + c) * E + e];
              acc = src[e] == a ? acc - term : acc + term;
            }
            bv[6 * a + c] = anchor ? 0. : acc;
          }
        }
        __syncthreads();
        if (first_build) {
          // ---- lambda = 1e-5 max diag(H); the optional outputs of the initial linearisation
          double m = -__builtin_huge_val();
          for (int i = t; i < 6 * K; i += PG_BLOCK) m = pg_nanmax(m, Hg[(size_t)pg_blk(i / 6, i / 6) * 36 + (i % 6) * 7]);
          m = pg_wg_max(m, t, wsum);
          if (t == 0) {
            cd[CD_LAMBDA] = 1e-5 * m; cd[CD_NU] = 2.; cd[CD_RES] = res_built;
            if (pass == 0 && p.lambda0) p.lambda0[g] = 1e-5 * m;
            if (pass == 0 && p.residual0) p.residual0[g] = res_built;
          }
          if (pass == 0) {
            res_first = res_built;
            if (p.H)
              for (size_t i = t; i < (size_t)36 * K * K; i += PG_BLOCK) {
                const int row = (int)(i / (6 * K)), col = (int)(i % (6 * K));
                const int bi = row / 6, bj = col / 6, r = row % 6, c = col % 6;
                p.H[g * 36 * K * K + i] = bi >= bj ? Hg[(size_t)pg_blk(bi, bj) * 36 + r * 6 + c] : Hg[(size_t)pg_blk(bj, bi) * 36 + c * 6 + r];
              }
            if (p.b)
              for (int i = t; i < 6 * K; i += PG_BLOCK) p.b[g * 6 * K + i] = bv[i];
            if (p.l0)
              for (int e = t; e < E; e += PG_BLOCK) {
                const double s = (st[e] & 1) ? ed[(size_t)PG_S * E + e] : __builtin_nan("");
                p.l0[g * E + e] = s * s;
              }
          }
          first_build = false;
        } else if (t == 0) {
          // ---- behind a taken trial: the right-term test; the outer iteration ends, and with it comes the residual test
          double m = 0.;
          for (int i = 0; i < 6 * K; ++i) m = fmax(m, fabs(bv[i]));
          if (m <= p.mrt || cd[CD_RES] < p.mres) { ci[CI_STOP] = 1; ci[CI_CONV] = 1; }
        }
        __syncthreads();
        stop = ci[CI_STOP];
        need_build = false;
        lm = 0;
        if (stop) break;
      }
      if (lm == 0) {                                        // an outer iteration begins
        if (outer >= p.max_it) break;
        ++outer;
      }
      int taken = 0;
      if (lm < p.max_lm) {
        ++lm;
        ++ntrials;
        const double lambda = cd[CD_LAMBDA];
        // H + lambda I into the factor's place, b into the right side's
        for (int i = 0; i < K; ++i)
          for (int it = t; it < 36 * (i + 1); it += PG_BLOCK) {
            const size_t at = (size_t)pg_blk(i, 0) * 36 + it;
            const double h = Hg[at];
            L[at] = (it / 36 == i && (it % 36) % 7 == 0) ? h + lambda : h;
          }
        for (int i = t; i < 6 * K; i += PG_BLOCK) yv[i] = bv[i];
        __syncthreads();
        // ---- right-looking block Cholesky, the right side as one more block row: three barriers a block column
        for (int j = 0; j < K; ++j) {
          double* D = L + (size_t)pg_blk(j, j) * 36;
          if (t == 0) {
            double A[6][6], F[6][6];
#pragma unroll
            for (int r = 0; r < 6; ++r)
#pragma unroll
              for (int c = 0; c <= r; ++c) A[r][c] = D[6 * r + c];
            bool ok = true;
#pragma unroll
            for (int c = 0; c < 6; ++c) {
              double s = A[c][c];
#pragma unroll
              for (int k = 0; k < c; ++k) s -= F[c][k] * F[c][k];
              const double orig = Hg[(size_t)pg_blk(j, j) * 36 + 7 * c] + lambda;
              ok = ok && __builtin_isfinite(s) && s > PL_PIVOT * orig;
              const double d = sqrt(s);
              F[c][c] = d;
#pragma unroll
              for (int r = c + 1; r < 6; ++r) {
                double v = A[r][c];
#pragma unroll
                for (int k = 0; k < c; ++k) v -= F[r][k] * F[c][k];
                F[r][c] = v / d;
              }
            }
#pragma unroll
            for (int r = 0; r < 6; ++r)
#pragma unroll
              for (int c = 0; c <= r; ++c) D[6 * r + c] = F[r][c];
            if (!ok) ci[CI_FAIL] = 1;
          }
          __syncthreads();
          if (ci[CI_FAIL]) break;                           // (uniform: read behind the barrier)
          const int n = K - 1 - j;                          // block rows below
          // the column's blocks: x L_jj^T = a, a row a lane; the last item is the right side's segment j
          for (int it = t; it < 6 * n + 1; it += PG_BLOCK) {
            double* row = it < 6 * n ? L + (size_t)pg_blk(j + 1 + it / 6, j) * 36 + 6 * (it % 6) : yv + 6 * j;
            double x[6];
#pragma unroll
            for (int c = 0; c < 6; ++c) {
              double v = row[c];
#pragma unroll
              for (int k = 0; k < c; ++k) v -= x[k] * D[6 * c + k];
              x[c] = v / D[7 * c];
            }
#pragma unroll
            for (int c = 0; c < 6; ++c) row[c] = x[c];
          }
          __syncthreads();
          // the trailing update: row r of block (i, k), j < k <= i, a lane; then the right side's segments below
          const int nt = n * (n + 1) / 2 * 6;
          for (int it = t; it < nt + 6 * n; it += PG_BLOCK) {
            if (it < nt) {
              const int q = it / 6, r = it % 6;
              int ii = (int)((sqrtf(8.f * (float)q + 1.f) - 1.f) * 0.5f);
              while (ii * (ii + 1) / 2 > q) --ii;
              while ((ii + 1) * (ii + 2) / 2 <= q) ++ii;
              const int kk = q - ii * (ii + 1) / 2;         // 0 <= kk <= ii < n
              const double* Li = L + (size_t)pg_blk(j + 1 + ii, j) * 36 + 6 * r;
              const double* Lk = L + (size_t)pg_blk(j + 1 + kk, j) * 36;
              double* A = L + (size_t)pg_blk(j + 1 + ii, j + 1 + kk) * 36 + 6 * r;
              double a[6];
#pragma unroll
              for (int m = 0; m < 6; ++m) a[m] = Li[m];
#pragma unroll
              for (int c = 0; c < 6; ++c) A[c] -= pg_dot6(a, Lk + 6 * c);
            } else {
              const int k = (it - nt) / 6, c = (it - nt) % 6;
              const double* Lk = L + (size_t)pg_blk(j + 1 + k, j) * 36 + 6 * c;
              yv[6 * (j + 1 + k) + c] -= pg_dot6(Lk, yv + 6 * j);
            }
          }
          __syncthreads();
        }
        // ---- L^T d = y, from the last block row up: two barriers a block row
        if (!ci[CI_FAIL])
          for (int i = K - 1; i >= 0; --i) {
            const double* D = L + (size_t)pg_blk(i, i) * 36;
            if (t == 0) {
              double x[6];
#pragma unroll
              for (int c = 5; c >= 0; --c) {
                double v = yv[6 * i + c];
#pragma unroll
                for (int k = c + 1; k < 6; ++k) v -= D[6 * k + c] * x[k];
                x[c] = v / D[7 * c];
              }
#pragma unroll
              for (int c = 0; c < 6; ++c) yv[6 * i + c] = x[c];
            }
            __syncthreads();
            for (int it = t; it < 6 * i; it += PG_BLOCK) {
              const int jj = it / 6, c = it % 6;
              const double* B = L + (size_t)pg_blk(i, jj) * 36;
              double a = B[c] * yv[6 * i];
#pragma unroll
              for (int m = 1; m < 6; ++m) a += B[6 * m + c] * yv[6 * i + m];
              yv[6 * jj + c] -= a;
            }
            __syncthreads();
          }
        // ---- lane 0: the solve's outcome and the increment test
        if (t == 0) {
          int s = 0;
          if (ci[CI_FAIL]) {
            s = 2;
          } else {
            double nd2 = 0., nx2 = 0., den = 0.;
            for (int i = 0; i < 6 * K; ++i) {
              const double d = yv[i];
              nd2 += d * d;
              den += d * (lambda * d + bv[i]);
            }
            for (int i = 0; i < K; ++i) nx2 += xn[i];
            cd[CD_DENOM] = den + 1e-3;
            if (!__builtin_isfinite(nd2)) s = 2;
            else if (sqrt(nd2) <= p.mri * (sqrt(nx2) + p.mri)) { s = 1; ci[CI_CONV] = 1; }
          }
          ci[CI_STOP] = s;
        }
        __syncthreads();
        stop = ci[CI_STOP];
        if (pass == 0 && ntrials == 1 && p.delta0 && stop != 2)
          for (int i = t; i < 6 * K; i += PG_BLOCK) p.delta0[g * 6 * K + i] = yv[i];
        if (stop) break;
        // ---- the trial poses and their residual under the l in force
        for (int i = t; i < K; i += PG_BLOCK) pg_step(yv + 6 * i, P + 12 * i, Pn + 12 * i);
        __syncthreads();
        const double res_new = pg_edge_sum(E, t, chunk, wsum, [&](int e) {
          const int f = st[e];
          if (!(f & 1)) return 0.;
          const double q = pg_edge_q(Pn, src[e], dst[e], Re + (size_t)e * 9, te + (size_t)e * 3, info + (size_t)e * 36);
          const double s = ed[(size_t)PG_S * E + e];
          const double pen = (f & 2) ? mu * ((s - 1.) * (s - 1.)) : 0.;
          return (s * s) * q + pen;
        });
        if (t == 0) {
          const double res = cd[CD_RES];
          const double rho = (res - res_new) / cd[CD_DENOM];
          int acc = 0;
          if (rho > 0.) {
            acc = 1;
            cd[CD_RES] = res_new;
            if (sqrt(res) - sqrt(res_new) < p.mrri * sqrt(res)) { ci[CI_STOP] = 1; ci[CI_CONV] = 1; }
            const double c = 2. * rho - 1.;
            const double alpha = 1. - (c * c) * c;
            cd[CD_LAMBDA] = lambda * (p.lsf > alpha ? p.lsf : alpha);
            cd[CD_NU] = 2.;
          } else {
            cd[CD_LAMBDA] = lambda * cd[CD_NU];
            cd[CD_NU] = cd[CD_NU] * 2.;
          }
          ci[CI_ACCEPT] = acc;
        }
        __syncthreads();
        taken = ci[CI_ACCEPT];
        stop = ci[CI_STOP];
        if (taken) {
          for (int i = t; i < K; i += PG_BLOCK) {
#pragma unroll
            for (int k = 0; k < 12; ++k) P[12 * i + k] = Pn[12 * i + k];
            xn[i] = pg_x2(Pn + 12 * i);
          }
        }
        __syncthreads();
      }
      if (stop) break;
      if (taken) {
        need_build = true;                                  // the next step rebuilds, tests and begins an outer iteration
      } else if (lm >= p.max_lm) {                          // the trials are used up: the system stands, the outer iteration ends
        if (t == 0 && cd[CD_RES] < p.mres) { ci[CI_STOP] = 1; ci[CI_CONV] = 1; }
        __syncthreads();
        stop = ci[CI_STOP];
        lm = 0;
        if (stop) break;
      }
    }
    conv = ci[CI_CONV];
    if (t == 0) { p.iterations[g * 2 + pass] = outer; if (p.trials) p.trials[g * 2 + pass] = ntrials; }
    __syncthreads();
    if (stop == 2) break;                                   // a singular or non-finite system ends the call
    if (pass + 1 < passes) {
      for (int e = t; e < E; e += PG_BLOCK) {
        const int f = st[e];
        if ((f & 3) == 3) {
          const double s = ed[(size_t)PG_S * E + e];
          if (s * s < p.thr) st[e] = f & ~1;
        }
      }
      if (t == 0) ci[CI_STOP] = 0;
      __syncthreads();
    }
  }
  // ---- closing
  for (int i = t; i < K; i += PG_BLOCK) {
#pragma unroll
    for (int k = 0; k < 9; ++k) p.R_out[(g * K + i) * 9 + k] = P[12 * i + k];
#pragma unroll
    for (int k = 0; k < 3; ++k) p.t_out[(g * K + i) * 3 + k] = P[12 * i + 9 + k];
  }
  for (int e = t; e < E; e += PG_BLOCK) {
    const int f = st[e];
    const double s = (f & 4) ? ed[(size_t)PG_S * E + e] : __builtin_nan("");
    p.weight[g * E + e] = s * s;
    p.kept[g * E + e] = f & 1;
  }
  if (t == 0) {
    p.residual[g * 2] = res_first;
    p.residual[g * 2 + 1] = cd[CD_RES];
    p.converged[g] = conv;
  }
}

struct PgPlan { size_t H, L, ed, st, inc, bytes, nbd; int form, lds; };

inline size_t pg_up(size_t n) { return (n + 255) & ~(size_t)255; }

int pg_lds_bytes(int K, bool factor) {
  size_t n = (size_t)(12 * 2 + 6 * 2 + 1) * K * 8 + (size_t)((K + 2) & ~1) * 4;
  if (factor) n += (size_t)K * (K + 1) / 2 * 36 * 8;
  return (int)n;
}

bool pg_fits(int K) {
  const int total = pg_lds_bytes(K, true) + PG_STATIC_LDS;
  return (total + PG_LDS_GRANULE - 1) / PG_LDS_GRANULE * PG_LDS_GRANULE <= PG_LDS_LIMIT;
}

int pg_plan(const vcr_posegraph_args& a, PgPlan* p) {
  *p = PgPlan{};
  if (a.G < 1 || a.K < 1 || a.E < 0 || !a.R || !a.t || !a.R_out || !a.t_out || !a.residual || !a.iterations || !a.converged)
    return VCR_EINVAL;
  if (a.E > 0 && (!a.src || !a.dst || !a.R_edge || !a.t_edge || !a.information || !a.uncertain || !a.weight || !a.kept)) return VCR_EINVAL;
  const double inf = __builtin_huge_val();
  auto bad = [inf](double v) { return !(v >= 0.) || v == inf; };          // NaN, negative, +inf
  if (bad(a.max_correspondence_distance) || bad(a.edge_prune_threshold)) return VCR_EINVAL;
  if (a.max_iteration < 0 || a.max_iteration_lm < 0 || a.max_iteration > VCR_POSEGRAPH_MAX_TRIALS || a.max_iteration_lm > VCR_POSEGRAPH_MAX_TRIALS ||
      (long)a.max_iteration * a.max_iteration_lm > VCR_POSEGRAPH_MAX_TRIALS)
    return VCR_EINVAL;
  if (!(a.min_relative_increment >= 0.) || !(a.min_relative_residual_increment >= 0.) || !(a.min_right_term >= 0.) || !(a.min_residual >= 0.))
    return VCR_EINVAL;
  if (!(a.lower_scale_factor > 0.) || a.lower_scale_factor == inf || !(a.upper_scale_factor > 0.) || a.upper_scale_factor == inf) return VCR_EINVAL;
  if (a.variant < 0 || a.variant > 2) return VCR_EINVAL;
  if (a.K > VCR_POSEGRAPH_MAX_NODES || a.E > VCR_POSEGRAPH_MAX_EDGES || (long)a.G * (a.E > 1 ? a.E : 1) >= (1L << 31)) return VCR_EUNSUPPORTED;
  if (a.anchor < 0 || a.anchor >= a.K) return VCR_EINVAL;
  const bool fits = pg_fits(a.K);
  if (a.variant == VCR_POSEGRAPH_FORM_LDS && !fits) return VCR_EINVAL;
  p->form = a.variant ? a.variant : fits ? VCR_POSEGRAPH_FORM_LDS : VCR_POSEGRAPH_FORM_GLOBAL;
  p->lds = pg_lds_bytes(a.K, p->form == VCR_POSEGRAPH_FORM_LDS);
  const size_t G = (size_t)a.G, E = (size_t)a.E;
  p->nbd = (size_t)a.K * (a.K + 1) / 2 * 36;
  p->H = 0;
  p->L = p->H + pg_up(G * p->nbd * 8);
  p->ed = p->L + (p->form == VCR_POSEGRAPH_FORM_GLOBAL ? pg_up(G * p->nbd * 8) : 0);
  p->st = p->ed + pg_up(G * E * PG_EW * 8);
  p->inc = p->st + pg_up(G * E * 4);
  p->bytes = p->inc + pg_up(G * E * 2 * 4) + 256;
  return VCR_OK;
}

int pg_take(const vcr_posegraph_args* user, vcr_posegraph_args* mine) {
  return vcr_take_args(user, mine, offsetof(vcr_posegraph_args, trials));
}

}  // namespace

extern "C" size_t vcr_posegraph_optimize_workspace_bytes(const vcr_posegraph_args* ua, int cu_count) {
  vcr_posegraph_args a;
  PgPlan p;
  if (pg_take(ua, &a) || cu_count < 0) return 0;
  return pg_plan(a, &p) ? 0 : p.bytes;
}

extern "C" int vcr_posegraph_optimize_form(const vcr_posegraph_args* ua, int cu_count, int* form, int* lds_bytes) {
  vcr_posegraph_args a;
  PgPlan p;
  if (pg_take(ua, &a) || cu_count < 0) return VCR_EINVAL;
  const int e = pg_plan(a, &p);
  if (e) return e;
  if (form) *form = p.form;
  if (lds_bytes) *lds_bytes = p.lds;
  return VCR_OK;
}

extern "C" int vcr_posegraph_check_edges(const int* src, const int* dst, int G, int K, int E) {
  if (G < 1 || K < 1 || E < 0 || (E > 0 && (!src || !dst))) return VCR_EINVAL;
  for (size_t i = 0; i < (size_t)G * E; ++i) {
    if (src[i] < 0) continue;                               // a blank
    if (src[i] >= K || dst[i] < 0 || dst[i] >= K || src[i] == dst[i]) return VCR_EINVAL;
  }
  return VCR_OK;
}

extern "C" int vcr_posegraph_optimize_f64(const vcr_posegraph_args* ua, void* workspace, size_t workspace_bytes, vcr_stream_t stream) {
  vcr_posegraph_args a;
  if (pg_take(ua, &a)) return VCR_EINVAL;
  PgPlan p;
  const int e = pg_plan(a, &p);
  if (e) return e;
  if (!workspace || (((uintptr_t)workspace) & 15)) return VCR_EINVAL;
  if (workspace_bytes < p.bytes) return VCR_EWORKSPACE;
  vcr_stream_scope scope(stream);
  unsigned char* w = reinterpret_cast<unsigned char*>(workspace);
  PgParams k{};
  k.K = a.K; k.E = a.E; k.anchor = a.anchor; k.prune = a.prune ? 1 : 0; k.max_it = a.max_iteration; k.max_lm = a.max_iteration_lm;
  k.mcd2 = a.max_correspondence_distance * a.max_correspondence_distance;
  k.thr = a.edge_prune_threshold; k.mri = a.min_relative_increment; k.mrri = a.min_relative_residual_increment;
  k.mrt = a.min_right_term; k.mres = a.min_residual; k.lsf = a.lower_scale_factor;
  k.R = a.R; k.t = a.t; k.src = a.src; k.dst = a.dst; k.Re = a.R_edge; k.te = a.t_edge; k.info = a.information; k.unc = a.uncertain;
  k.Hg = reinterpret_cast<double*>(w + p.H); k.Lg = reinterpret_cast<double*>(w + p.L); k.ed = reinterpret_cast<double*>(w + p.ed);
  k.st = reinterpret_cast<int*>(w + p.st); k.inc = reinterpret_cast<int*>(w + p.inc); k.nbd = p.nbd;
  k.R_out = a.R_out; k.t_out = a.t_out; k.weight = a.weight; k.kept = a.kept; k.residual = a.residual; k.iterations = a.iterations;
  k.converged = a.converged; k.trials = a.trials; k.H = a.H; k.b = a.b; k.residual0 = a.residual0; k.l0 = a.l0; k.delta0 = a.delta0;
  k.lambda0 = a.lambda0;
  hipStream_t s = (hipStream_t)stream;
  if (p.form == VCR_POSEGRAPH_FORM_LDS)
    return vcr_launch<posegraph_kernel<VCR_POSEGRAPH_FORM_LDS>>(dim3((unsigned)a.G), dim3(PG_BLOCK), (size_t)p.lds, s, k);
  return vcr_launch<posegraph_kernel<VCR_POSEGRAPH_FORM_GLOBAL>>(dim3((unsigned)a.G), dim3(PG_BLOCK), (size_t)p.lds, s, k);
}

// A pose from correspondences without trials (include/vcr_hip_fgr.h): Fast Global Registration as Open3D
// runs it.  Five launches (two without the tuple test), no host synchronisation:
//   fgr_pairs_kernel      (its body: corr_pairs.h, the RANSAC's) one workgroup per cloud: the pair list, gathered once.
//   fgr_tuple_kernel      one LANE per trial: the RANSAC's draws, the three edge tests; the trial's rank among its workgroup's
//                         passes (wg_scan.h's ballot rank), -1 for a failure, and the workgroup's count.
//   fgr_offsets_kernel    one workgroup per cloud: the counts become their exclusive scan (wg_scan.h), tuples = min(K, total).
//   fgr_scatter_kernel    one lane per trial: a pass whose position -- its workgroup's offset plus its rank -- is below K writes
//                         its three picks there: the first K passes in trial order, no atomic decides anything.
//   fgr_solve_kernel      one workgroup per cloud: the normalisation and ALL iterations (as fps.hip runs all its rounds).  The
//                         normalised pairs live in fp64 in the workspace, six planes of L (48 B per entry); entry c belongs to
//                         lane c % 256 throughout, so a lane only ever reads back what it wrote itself.  One pass per iteration:
//                         the moved point is written and its 27 values for the NEXT iteration are taken in the same sweep.
//                         The sums are folded in wg_scan.h's order; thread 0 solves (refine_solve6.h) and hands the update to
//                         the others through LDS.
// Every result is a function of the cloud pair alone; all writes are plain vector stores.
#include "seg_scan.h"
#include "corr_pairs.h"
#include "refine_solve6.h"
#include "../../include/vcr_hip_fgr.h"

namespace {

struct FgWork {                                            // the workspace, per cloud b
  float* rows;                                             // [B][Ns][8]
  int* M;                                                  // [B]
  int* ntup;                                               // [B]
  int* rank;                                               // [B][T]
  int* cnt;                                                // [B][nblk]: a workgroup's passes, then their exclusive scan
  int* list;                                               // [B][3 Keff]
  double* pq;                                              // [B][6][Lmax]: px, py, pz, qx, qy, qz
};

__global__ __launch_bounds__(RS_BLOCK) void fgr_pairs_kernel(RsPairs p) { rs_pairs_body(p); }

struct FgTuple { FgWork w; int Ns, T, nblk; unsigned seed; float s2; };

__global__ __launch_bounds__(RS_BLOCK) void fgr_tuple_kernel(FgTuple p) {
  __shared__ int wtot[WG_WAVES];
  const int b = (int)(blockIdx.x / (unsigned)p.nblk), blk = (int)(blockIdx.x % (unsigned)p.nblk);
  const int t = threadIdx.x, trial = blk * RS_BLOCK + t;
  const int M = p.w.M[b];
  const long limit = 100L * M < (long)p.T ? 100L * M : (long)p.T;
  bool ok = trial < limit;                                 // (limit > 0 implies M >= 1: the rows exist)
  if (ok) {
    const float* rows = p.w.rows + (size_t)b * p.Ns * 8;
    f32x4 s[3], q[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const unsigned at = rs_pick(p.seed, trial, j, M);    // < M
      s[j] = ld4(rows + (size_t)at * 8);
      q[j] = ld4(rows + (size_t)at * 8 + 4);
    }
#pragma unroll
    for (int e = 0; e < 3; ++e) {
      const int u = e == 2 ? 1 : 0, v = e == 0 ? 1 : 2;    // (0,1), (0,2), (1,2)
      const float ls2 = rs_len2(s[u], s[v]), lt2 = rs_len2(q[u], q[v]);
      ok = ok && p.s2 * ls2 < lt2 && p.s2 * lt2 < ls2;     // strict: a NaN and a zero edge fail
    }
  }
  int total;
  const int r = wg_rank(ok, t, wtot, &total);
  if (trial < p.T) p.w.rank[(size_t)b * p.T + trial] = ok ? r : -1;
  if (t == 0) p.w.cnt[(size_t)b * p.nblk + blk] = total;
}

struct FgOffsets { FgWork w; int nblk, K; int* tuples; };

__global__ __launch_bounds__(RS_BLOCK) void fgr_offsets_kernel(FgOffsets p) {
  __shared__ int wtot[WG_WAVES];
  const int b = blockIdx.x;
  const int total = wg_offsets(p.w.cnt + (size_t)b * p.nblk, p.nblk, wtot);
  if (threadIdx.x == 0) {
    const int n = total < p.K ? total : p.K;
    p.w.ntup[b] = n;
    if (p.tuples) p.tuples[b] = n;
  }
}

struct FgScatter { FgWork w; int Ns, T, nblk, K, Keff; unsigned seed; int* tuple_list; };

__global__ __launch_bounds__(RS_BLOCK) void fgr_scatter_kernel(FgScatter p) {
  const int b = (int)(blockIdx.x / (unsigned)p.nblk), blk = (int)(blockIdx.x % (unsigned)p.nblk);
  const int trial = blk * RS_BLOCK + (int)threadIdx.x;
  if (trial >= p.T) return;
  const int r = p.w.rank[(size_t)b * p.T + trial];
  if (r < 0) return;
  const int pos = p.w.cnt[(size_t)b * p.nblk + blk] + r;
  if (pos >= p.K) return;                                  // pos < min(K, passes) <= Keff = min(K, T)
  const int M = p.w.M[b];
  const float* rows = p.w.rows + (size_t)b * p.Ns * 8;
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const int i = __float_as_int(rows[(size_t)rs_pick(p.seed, trial, j, M) * 8 + 3]);
    p.w.list[(size_t)b * 3 * p.Keff + 3 * (size_t)pos + j] = i;
    if (p.tuple_list) p.tuple_list[(size_t)b * 3 * p.K + 3 * (size_t)pos + j] = i;
  }
}

constexpr int FG_NZ = 21;                                  // the 27 values without their six structural zeros, at:
__constant__ const int FG_AT[FG_NZ] = {0, 1, 2, 4, 5, 6, 7, 8, 10, 11, 12, 13, 15, 18, 20, 21, 22, 23, 24, 25, 26};

// the header's values of one entry, added onto acc in FG_AT's order
__device__ __forceinline__ void fg_add(double (&acc)[FG_NZ], double px, double py, double pz, double qx, double qy, double qz, double mu) {
  const double rx = px - qx, ry = py - qy, rz = pz - qz;
  const double d2 = fma(rz, rz, fma(ry, ry, rx * rx));
  const double w = mu / (d2 + mu);
  const double s = w * w;
  acc[0] += s * (qz * qz + qy * qy);
  acc[1] += s * -(qy * qx);
  acc[2] += s * -(qz * qx);
  acc[3] += s * -qz;
  acc[4] += s * qy;
  acc[5] += s * (qz * qz + qx * qx);
  acc[6] += s * -(qz * qy);
  acc[7] += s * qz;
  acc[8] += s * -qx;
  acc[9] += s * (qy * qy + qx * qx);
  acc[10] += s * -qy;
  acc[11] += s * qx;
  acc[12] += s;
  acc[13] += s;
  acc[14] += s;
  acc[15] += s * (qz * ry + -(qy * rz));
  acc[16] += s * (-(qz * rx) + qx * rz);
  acc[17] += s * (qy * rx + -(qx * ry));
  acc[18] += s * -rx;
  acc[19] += s * -ry;
  acc[20] += s * -rz;
}

// m(v) of the header: row r of Ri against v
__device__ __forceinline__ double fg_row(const double* Ri, int r, double v0, double v1, double v2) {
  return fma(Ri[3 * r + 2], v2, fma(Ri[3 * r + 1], v1, Ri[3 * r] * v0));
}

// the header's `sum order` behind the lanes' own sums: the wave butterfly, then the four waves ascending; every lane returns
// the sum.  wsum [WG_WAVES] is free again after the caller's next barrier.
__device__ __forceinline__ double fg_wg_sum(double v, int t, double* wsum) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
  __syncthreads();                                         // the previous sum's totals have been read
  if ((t & 63) == 0) wsum[t >> 6] = v;
  __syncthreads();
  return ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
}

__device__ __forceinline__ double fg_wg_max(double v, int t, double* wsum) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
  __syncthreads();
  if ((t & 63) == 0) wsum[t >> 6] = v;
  __syncthreads();
  return fmax(fmax(wsum[0], wsum[1]), fmax(wsum[2], wsum[3]));
}

struct FgSolve {
  FgWork w;
  const float* src; const float* tgt; const int* corr;
  int Ns, Nt, Keff, Lmax, tuple, iterations, decrease_mu;
  double division_factor, mu_floor;
  float* R_out; float* t_out;
  int* used; int* status; double* norm; double* pose64; double* sums; double* mu;
};

__global__ __launch_bounds__(RS_BLOCK) void fgr_solve_kernel(FgSolve p) {
  __shared__ double wsum[WG_WAVES];
  __shared__ double wacc[WG_WAVES][FG_NZ];
  __shared__ double S[27];
  __shared__ double upd[12];                               // Ri, ti of the iteration
  __shared__ int apply;                                    // 0: an identity update
  const int t = threadIdx.x, b = blockIdx.x, Ns = p.Ns, Nt = p.Nt;
  const float* sx = p.src + (size_t)b * 3 * Ns;
  const float* tx = p.tgt + (size_t)b * 3 * Nt;
  const int L = p.tuple ? 3 * p.w.ntup[b] : p.w.M[b];      // <= Lmax
  // ---- the normalisation
  double mean[6];
#pragma unroll
  for (int e = 0; e < 6; ++e) {
    const float* x = e < 3 ? sx + (size_t)e * Ns : tx + (size_t)(e - 3) * Nt;
    const int n = e < 3 ? Ns : Nt;
    double a = 0.;
    for (int i = t; i < n; i += RS_BLOCK) a += (double)x[i];
    mean[e] = fg_wg_sum(a, t, wsum) / (double)n;
  }
  double big = 0.;
  for (int i = t; i < Ns; i += RS_BLOCK) {
    const double dx = (double)sx[i] - mean[0], dy = (double)sx[Ns + i] - mean[1], dz = (double)sx[2 * (size_t)Ns + i] - mean[2];
    big = fmax(big, fma(dz, dz, fma(dy, dy, dx * dx)));
  }
  for (int i = t; i < Nt; i += RS_BLOCK) {
    const double dx = (double)tx[i] - mean[3], dy = (double)tx[Nt + i] - mean[4], dz = (double)tx[2 * (size_t)Nt + i] - mean[5];
    big = fmax(big, fma(dz, dz, fma(dy, dy, dx * dx)));
  }
  bool finite = true;
#pragma unroll
  for (int e = 0; e < 6; ++e) finite = finite && __builtin_isfinite(mean[e]);
  const double scale = finite ? sqrt(fg_wg_max(big, t, wsum)) : __builtin_nan("");   // (finite means: finite points, no NaN in the maximum)
  int status = L < VCR_FGR_MIN_ENTRIES ? 1 : (finite && __builtin_isfinite(scale) && scale != 0.) ? 0 : 2;
  // ---- the loop (status is workgroup-uniform: the barriers below are met by all or by none)
  double R[9] = {1., 0., 0., 0., 1., 0., 0., 0., 1.}, tr[3] = {0., 0., 0.}, mu = 1.;    // (thread 0's are the state)
  double* pl = p.w.pq + (size_t)b * 6 * p.Lmax;
  const size_t Lm = (size_t)p.Lmax;
  if (t < 27) S[t] = 0.;
  if (status == 0) {
    double acc[FG_NZ];
#pragma unroll
    for (int k = 0; k < FG_NZ; ++k) acc[k] = 0.;
    const int* list = p.w.list + (size_t)b * 3 * p.Keff;
    const float* rows = p.w.rows + (size_t)b * Ns * 8;
    const int* corr = p.corr + (size_t)b * Ns;
    for (int c = t; c < L; c += RS_BLOCK) {
      const int i = p.tuple ? list[c] : __float_as_int(rows[(size_t)c * 8 + 3]);     // a pair's source index: 0 <= corr[i] < Nt
      const int j = corr[i];
      const double qx = ((double)sx[i] - mean[0]) / scale, qy = ((double)sx[Ns + i] - mean[1]) / scale,
                   qz = ((double)sx[2 * (size_t)Ns + i] - mean[2]) / scale;
      const double px = ((double)tx[j] - mean[3]) / scale, py = ((double)tx[Nt + j] - mean[4]) / scale,
                   pz = ((double)tx[2 * (size_t)Nt + j] - mean[5]) / scale;
      pl[c] = px; pl[Lm + c] = py; pl[2 * Lm + c] = pz;
      pl[3 * Lm + c] = qx; pl[4 * Lm + c] = qy; pl[5 * Lm + c] = qz;
      if (p.iterations > 0) fg_add(acc, px, py, pz, qx, qy, qz, mu);
    }
    for (int it = 0; it < p.iterations; ++it) {
#pragma unroll
      for (int k = 0; k < FG_NZ; ++k) {
        double v = acc[k];
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
        if ((t & 63) == 0) wacc[t >> 6][k] = v;
        acc[k] = 0.;
      }
      __syncthreads();
      if (t < FG_NZ) S[FG_AT[t]] = ((wacc[0][t] + wacc[1][t]) + wacc[2][t]) + wacc[3][t];
      __syncthreads();
      if (t == 0) {
        double x[6], Ri[9], ti[3];
        bool ok = pl_solve(S, S + 21, x);
#pragma unroll
        for (int e = 0; e < 6; ++e) ok = ok && __builtin_isfinite(x[e]);
        if (ok) {
          pl_euler(x, Ri, ti);
          double Rn[9], tn[3];
#pragma unroll
          for (int r = 0; r < 3; ++r) {
#pragma unroll
            for (int c = 0; c < 3; ++c) Rn[3 * r + c] = fg_row(Ri, r, R[c], R[3 + c], R[6 + c]);
            tn[r] = fg_row(Ri, r, tr[0], tr[1], tr[2]) + ti[r];
          }
#pragma unroll
          for (int e = 0; e < 9; ++e) { R[e] = Rn[e]; upd[e] = Ri[e]; }
#pragma unroll
          for (int e = 0; e < 3; ++e) { tr[e] = tn[e]; upd[9 + e] = ti[e]; }
        } else {
          status |= 16;
        }
        apply = ok ? 1 : 0;
      }
      if (p.decrease_mu && it % 4 == 0 && mu > p.mu_floor) mu = mu / p.division_factor;   // (every lane: the next weights)
      __syncthreads();
      const bool last = it + 1 == p.iterations;
      if (apply) {
        double Ri[9], ti[3];
#pragma unroll
        for (int e = 0; e < 9; ++e) Ri[e] = upd[e];
#pragma unroll
        for (int e = 0; e < 3; ++e) ti[e] = upd[9 + e];
        for (int c = t; c < L; c += RS_BLOCK) {
          const double qx = pl[3 * Lm + c], qy = pl[4 * Lm + c], qz = pl[5 * Lm + c];
          const double nx = fg_row(Ri, 0, qx, qy, qz) + ti[0], ny = fg_row(Ri, 1, qx, qy, qz) + ti[1],
                       nz = fg_row(Ri, 2, qx, qy, qz) + ti[2];
          pl[3 * Lm + c] = nx; pl[4 * Lm + c] = ny; pl[5 * Lm + c] = nz;
          if (!last) fg_add(acc, pl[c], pl[Lm + c], pl[2 * Lm + c], nx, ny, nz, mu);
        }
      } else if (!last) {
        for (int c = t; c < L; c += RS_BLOCK)
          fg_add(acc, pl[c], pl[Lm + c], pl[2 * Lm + c], pl[3 * Lm + c], pl[4 * Lm + c], pl[5 * Lm + c], mu);
      }
      __syncthreads();                                     // upd, apply and S have been read
    }
  }
  __syncthreads();
  if (t < 27 && p.sums) p.sums[(size_t)b * 27 + t] = S[t];
  if (t != 0) return;
  if (p.norm) {
#pragma unroll
    for (int e = 0; e < 6; ++e) p.norm[(size_t)b * 7 + e] = mean[e];
    p.norm[(size_t)b * 7 + 6] = scale;
  }
  // ---- closing
  double P[12];
  const double nan = __builtin_nan("");
#pragma unroll
  for (int e = 0; e < 9; ++e) P[e] = status == 2 ? nan : R[e];
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    const double back = (scale * tr[r] + mean[3 + r]) - fg_row(R, r, mean[0], mean[1], mean[2]);
    P[9 + r] = status == 2 ? nan : status == 1 ? 0. : back;
  }
#pragma unroll
  for (int e = 0; e < 9; ++e) p.R_out[(size_t)b * 9 + e] = (float)P[e];
#pragma unroll
  for (int e = 0; e < 3; ++e) p.t_out[(size_t)b * 3 + e] = (float)P[9 + e];
  if (p.pose64)
#pragma unroll
    for (int e = 0; e < 12; ++e) p.pose64[(size_t)b * 12 + e] = P[e];
  if (p.used) p.used[b] = L;
  if (p.status) p.status[b] = status;
  if (p.mu) p.mu[b] = mu;
}

struct FgPlan { size_t rows, M, ntup, rank, cnt, list, pq, bytes; int nblk, Keff, Lmax; };

int fg_plan(const vcr_fgr_args& a, FgPlan* p) {
  *p = FgPlan{};
  if (!a.src || !a.tgt || !a.corr || !a.R_out || !a.t_out || a.B < 1 || a.Ns < 1 || a.Nt < 1 || a.tuple_trials < 1 || a.max_tuples < 1)
    return VCR_EINVAL;
  if (!(a.tuple_scale >= 0.f && a.tuple_scale <= 1.f)) return VCR_EINVAL;
  if (a.iterations < 0 || a.iterations > VCR_FGR_MAX_ITERATIONS) return VCR_EINVAL;
  if (!(a.division_factor > 1.) || a.division_factor == __builtin_huge_val()) return VCR_EINVAL;     // <= 1, NaN, +inf
  if (!(a.mu_floor > 0.) || a.mu_floor == __builtin_huge_val()) return VCR_EINVAL;
  const int Nmax = a.Ns > a.Nt ? a.Ns : a.Nt;
  if (a.tuple_trials > VCR_RANSAC_MAX_TRIALS || a.Ns > RS_MAX_N || a.Nt > RS_MAX_N || (long)a.B * Nmax >= (1L << 31) ||
      (long)a.B * a.tuple_trials >= (1L << 29))
    return VCR_EUNSUPPORTED;
  const bool tuple = a.tuple_scale != 0.f;
  const size_t B = (size_t)a.B;
  p->nblk = (a.tuple_trials + RS_BLOCK - 1) / RS_BLOCK;
  p->Keff = a.max_tuples < a.tuple_trials ? a.max_tuples : a.tuple_trials;
  p->Lmax = tuple ? 3 * p->Keff : a.Ns;                    // <= 3 * 2^20
  p->rows = 0;
  p->M = ws_up(B * a.Ns * 32);
  p->ntup = p->M + ws_up(B * 4);
  p->rank = p->ntup + ws_up(B * 4);
  p->cnt = p->rank + (tuple ? ws_up(B * a.tuple_trials * 4) : 0);
  p->list = p->cnt + (tuple ? ws_up(B * p->nblk * 4) : 0);
  p->pq = p->list + (tuple ? ws_up(B * 3 * p->Keff * 4) : 0);
  p->bytes = p->pq + ws_up(B * 6 * p->Lmax * sizeof(double));
  return VCR_OK;
}

int fg_take(const vcr_fgr_args* user, vcr_fgr_args* mine) { return vcr_take_args(user, mine, offsetof(vcr_fgr_args, pairs)); }

}  // namespace

extern "C" size_t vcr_fgr_workspace_bytes(const vcr_fgr_args* ua, int cu_count) {
  vcr_fgr_args a;
  FgPlan p;
  if (fg_take(ua, &a) || cu_count < 0) return 0;
  return fg_plan(a, &p) ? 0 : p.bytes;                     // (the form does not depend on the device)
}

extern "C" int vcr_fgr_f32(const vcr_fgr_args* ua, void* workspace, size_t workspace_bytes, vcr_stream_t stream) {
  vcr_fgr_args a;
  if (fg_take(ua, &a)) return VCR_EINVAL;
  FgPlan p;
  int e = fg_plan(a, &p);
  if (e) return e;
  if (!workspace || (((uintptr_t)workspace) & 15)) return VCR_EINVAL;
  if (workspace_bytes < p.bytes) return VCR_EWORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  unsigned char* w = reinterpret_cast<unsigned char*>(workspace);
  const FgWork wk{reinterpret_cast<float*>(w + p.rows), reinterpret_cast<int*>(w + p.M), reinterpret_cast<int*>(w + p.ntup),
                  reinterpret_cast<int*>(w + p.rank), reinterpret_cast<int*>(w + p.cnt), reinterpret_cast<int*>(w + p.list),
                  reinterpret_cast<double*>(w + p.pq)};
  const int B = a.B, T = a.tuple_trials, tuple = a.tuple_scale != 0.f ? 1 : 0;
  // the pairs kernel leaves tuples = 0 behind it: what a call without the tuple test reports
  const RsPairs pr{a.src, a.tgt, a.corr, a.Ns, a.Nt, wk.rows, wk.M, tuple || !a.tuples ? wk.ntup : a.tuples, a.pairs};
  hipLaunchKernelGGL(fgr_pairs_kernel, dim3((unsigned)B), dim3(RS_BLOCK), 0, s, pr);
  if ((e = VCR_LAUNCH_RC())) return e;
  if (tuple) {
    const unsigned grid = (unsigned)((long)B * p.nblk);    // B T < 2^29: below 2^31
    const FgTuple tp{wk, a.Ns, T, p.nblk, a.seed, a.tuple_scale * a.tuple_scale};
    hipLaunchKernelGGL(fgr_tuple_kernel, dim3(grid), dim3(RS_BLOCK), 0, s, tp);
    if ((e = VCR_LAUNCH_RC())) return e;
    const FgOffsets of{wk, p.nblk, a.max_tuples, a.tuples};
    hipLaunchKernelGGL(fgr_offsets_kernel, dim3((unsigned)B), dim3(RS_BLOCK), 0, s, of);
    if ((e = VCR_LAUNCH_RC())) return e;
    const FgScatter sc{wk, a.Ns, T, p.nblk, a.max_tuples, p.Keff, a.seed, a.tuple_list};
    hipLaunchKernelGGL(fgr_scatter_kernel, dim3(grid), dim3(RS_BLOCK), 0, s, sc);
    if ((e = VCR_LAUNCH_RC())) return e;
  }
  const FgSolve sv{wk, a.src, a.tgt, a.corr, a.Ns, a.Nt, p.Keff, p.Lmax, tuple, a.iterations, a.decrease_mu, a.division_factor,
                   a.mu_floor, a.R_out, a.t_out, a.used, a.status, a.norm, a.pose64, a.sums, a.mu};
  hipLaunchKernelGGL(fgr_solve_kernel, dim3((unsigned)B), dim3(RS_BLOCK), 0, s, sv);
  return VCR_LAUNCH_RC();
}

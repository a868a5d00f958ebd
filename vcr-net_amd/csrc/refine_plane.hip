// Refining a registration on the full clouds, point to plane (include/vcr_hip_plane.h): vcr_refine_f32's
// loop (refine.hip) with another fit.  The launches are the same -- refine_init_kernel up front (refine_state.h), then per round
// nn_scan_kernel<Q> (nn_scan.h) and two kernels of this file -- and so are the gate live[b], the fp64 pose, the evaluation and
// the stop test:
//   plane_merge_kernel    refine_merge_kernel's lane per source point: folds the S candidates, writes nn_idx / nn_d2, recomputes
//                         the moved point p (the scan's expression), gathers the neighbour q and ITS NORMAL, and reduces its 256
//                         points to twenty-nine fp64 values -- sum of d2, count, A = sum J J^T (21), g = sum J r (6) over the
//                         inliers, J = (p x nrm, nrm), r = p.nrm - q.nrm -- one value at a time through the butterfly, so that
//                         they are never live together.
//   plane_cloud_kernel    one workgroup per cloud: the partials in ascending order; then one lane: the round's evaluation, the
//                         convergence test, A x = -g by Cholesky, R_i = Rz(x2) Ry(x1) Rx(x0), t_i = (x3, x4, x5), the composed
//                         pose.  A singular system stops the cloud like too few inliers do.
#include "refine_state.h"
#include "../../include/vcr_hip_plane.h"

namespace {

constexpr int PL_VALUES = 29;                              // sum_d2, count, A's upper triangle by rows [21], g[6]
constexpr int PL_CHUNK = 64;                               // partials the per-cloud kernel stages in LDS at a time (15 KB)
constexpr int PL_MIN_INLIERS = 6;                          // six unknowns
constexpr double PL_PIVOT = 1e-12;                         // a Cholesky pivot at or below this times its diagonal entry: singular

struct PlMerge {
  const float* part_d2; const int* part_idx;
  const float* src; const float* tgt; const float* nrm; const float* R; const float* t;   // the fp32 pose the scan ran under
  int B, Ns, Nt, S, nblk;                                  // nblk = ceil(Ns / 256)
  float max_d2;
  int* nn_idx; float* nn_d2;
  double* part;                                            // [B][nblk][PL_VALUES]
  const int* live;
};

__global__ __launch_bounds__(NN_BLOCK) void plane_merge_kernel(PlMerge p) {
  __shared__ double red[NN_BLOCK / 64][PL_VALUES];
  const int t = threadIdx.x;
  const int b = (int)(blockIdx.x / (unsigned)p.nblk), blk = (int)(blockIdx.x % (unsigned)p.nblk);
  if (!p.live[b]) return;                                  // (workgroup-uniform)
  const int n = blk * NN_BLOCK + t;
  const int Ns = p.Ns, Nt = p.Nt;
  float best = __builtin_huge_valf();
  int bi = -1;
  if (n < Ns) {
    nn_fold(p.part_d2, p.part_idx, p.B, Ns, p.S, b, n, &best, &bi);
    const size_t o = (size_t)b * Ns + n;
    if (p.nn_idx) p.nn_idx[o] = bi;
    if (p.nn_d2) p.nn_d2[o] = best;
  }
  const bool in = n < Ns && bi >= 0 && best <= p.max_d2;   // nn_merge_kernel's inlier
  // every lane that is no inlier contributes exact zeros
  float pc[3] = {0.f, 0.f, 0.f}, qc[3] = {0.f, 0.f, 0.f}, nc[3] = {0.f, 0.f, 0.f};
  if (in) {                                                // bi is in [0, Nt): a target index the scan wrote
    const float* sx = p.src + (size_t)b * 3 * Ns;
    const float* tx = p.tgt + (size_t)b * 3 * Nt;
    const float* nx = p.nrm + (size_t)b * 3 * Nt;
    const float* r = p.R + (size_t)b * 9;
    const float* tr = p.t + (size_t)b * 3;
    const float x = sx[n], y = sx[Ns + n], z = sx[2 * (size_t)Ns + n];
    for (int c = 0; c < 3; ++c) {                          // the scan's expression, bit for bit
      pc[c] = fmaf(r[3 * c + 2], z, fmaf(r[3 * c + 1], y, r[3 * c] * x)) + tr[c];
      qc[c] = tx[(size_t)c * Nt + bi];
      nc[c] = nx[(size_t)c * Nt + bi];
    }
  }
  auto put = [&](int e, double v) {                        // one value across the wave, nn_merge_kernel's butterfly
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    if ((t & 63) == 0) red[t >> 6][e] = v;
  };
  const double p0 = (double)pc[0], p1 = (double)pc[1], p2 = (double)pc[2];
  const double m0 = (double)nc[0], m1 = (double)nc[1], m2 = (double)nc[2];
  double J[6];                                             // products of two fp32 values: exact
  J[0] = p1 * m2 - p2 * m1; J[1] = p2 * m0 - p0 * m2; J[2] = p0 * m1 - p1 * m0;
  J[3] = m0; J[4] = m1; J[5] = m2;
  const double res = ((p0 * m0 + p1 * m1) + p2 * m2) - (((double)qc[0] * m0 + (double)qc[1] * m1) + (double)qc[2] * m2);
  put(0, in ? (double)best : 0.);
  put(1, in ? 1. : 0.);
  int e = 2;
#pragma unroll
  for (int r = 0; r < 6; ++r)
#pragma unroll
    for (int c = r; c < 6; ++c) put(e++, J[r] * J[c]);
#pragma unroll
  for (int r = 0; r < 6; ++r) put(e++, J[r] * res);
  __syncthreads();
  if (t < PL_VALUES) {
    double s = red[0][t];
    for (int w = 1; w < NN_BLOCK / 64; ++w) s += red[w][t];
    p.part[((size_t)b * p.nblk + blk) * PL_VALUES + t] = s;
  }
}

struct PlCloud {
  const double* part; int Ns, nblk;
  int round, max_iterations; float rel_fitness, rel_rmse;
  RfState st;
  float* R_out; float* t_out; float* fitness; float* rmse; float* R_ba; float* t_ba;
  int* inliers; double* sum_d2; int* iterations; int* converged;
};

// A x = -g for the symmetric A (upper triangle by rows in a21) by Cholesky, fully unrolled: registers only.  false: singular.
__device__ bool pl_solve(const double* a21, const double* g, double* x) {
  double A[6][6], L[6][6];
  int e = 0;
#pragma unroll
  for (int r = 0; r < 6; ++r)
#pragma unroll
    for (int c = r; c < 6; ++c) { A[r][c] = a21[e]; A[c][r] = a21[e]; ++e; }
  bool ok = true;
#pragma unroll
  for (int j = 0; j < 6; ++j) {
    double s = A[j][j];
#pragma unroll
    for (int k = 0; k < j; ++k) s -= L[j][k] * L[j][k];
    ok = ok && __builtin_isfinite(s) && s > PL_PIVOT * A[j][j];
    const double d = sqrt(s);
    L[j][j] = d;
#pragma unroll
    for (int i = j + 1; i < 6; ++i) {
      double v = A[i][j];
#pragma unroll
      for (int k = 0; k < j; ++k) v -= L[i][k] * L[j][k];
      L[i][j] = v / d;
    }
  }
  double y[6];
#pragma unroll
  for (int i = 0; i < 6; ++i) {                            // L y = -g
    double v = -g[i];
#pragma unroll
    for (int k = 0; k < i; ++k) v -= L[i][k] * y[k];
    y[i] = v / L[i][i];
  }
#pragma unroll
  for (int i = 5; i >= 0; --i) {                           // L^T x = y
    double v = y[i];
#pragma unroll
    for (int k = i + 1; k < 6; ++k) v -= L[k][i] * x[k];
    x[i] = v / L[i][i];
  }
  return ok;
}

__global__ __launch_bounds__(NN_BLOCK) void plane_cloud_kernel(PlCloud p) {
  __shared__ double stage[PL_CHUNK * PL_VALUES];
  __shared__ double tot[PL_VALUES];
  const int t = threadIdx.x, b = blockIdx.x;
  if (!p.st.live[b]) return;                               // (workgroup-uniform; written only by this workgroup's thread 0, behind the barriers)
  const double* part = p.part + (size_t)b * p.nblk * PL_VALUES;
  double acc = 0.;
  for (int c0 = 0; c0 < p.nblk; c0 += PL_CHUNK) {          // (workgroup-uniform)
    const int m = p.nblk - c0 < PL_CHUNK ? p.nblk - c0 : PL_CHUNK;
    __syncthreads();
    for (int i = t; i < m * PL_VALUES; i += NN_BLOCK) stage[i] = part[(size_t)c0 * PL_VALUES + i];
    __syncthreads();
    if (t < PL_VALUES)
      for (int i = 0; i < m; ++i) acc += stage[i * PL_VALUES + t];      // ascending, one lane per value: the order is Ns's alone
  }
  if (t < PL_VALUES) tot[t] = acc;
  __syncthreads();
  if (t != 0) return;                                      // one lane finishes
  double v[PL_VALUES];
#pragma unroll
  for (int e = 0; e < PL_VALUES; ++e) v[e] = tot[e];
  // the round's evaluation: nn_final_kernel's expressions
  const double sum = v[0];
  const int cnt = (int)v[1];
  const float fitness = (float)cnt / (float)p.Ns;
  const float rmse = cnt > 0 ? (float)sqrt(sum / (double)cnt) : 0.f;
  bool conv = false;
  if (p.round > 0)
    conv = fabsf(fitness - p.st.prev[2 * b]) < p.rel_fitness && fabsf(rmse - p.st.prev[2 * b + 1]) < p.rel_rmse;
  bool step = !conv && p.round < p.max_iterations && cnt >= PL_MIN_INLIERS;
  bool finite = true;
#pragma unroll
  for (int e = 2; e < PL_VALUES; ++e) finite = finite && __builtin_isfinite(v[e]);
  double x[6] = {0., 0., 0., 0., 0., 0.};
  if (step && finite) step = pl_solve(v + 2, v + 23, x);   // (a singular system stops the cloud; non-finite sums step to a NaN pose)
  const int iters = p.st.iters[b] + (step ? 1 : 0);
  p.fitness[b] = fitness; p.rmse[b] = rmse;
  if (p.inliers) p.inliers[b] = cnt;
  if (p.sum_d2) p.sum_d2[b] = sum;
  if (p.iterations) p.iterations[b] = iters;
  if (p.converged) p.converged[b] = conv ? 1 : 0;
  p.st.prev[2 * b] = fitness; p.st.prev[2 * b + 1] = rmse;
  p.st.iters[b] = iters;
  p.st.live[b] = step ? 1 : 0;
  if (!step) return;
  double Ri[9], ti[3];
  {
    double s0, c0, s1, c1, s2, c2;
    sincos(x[0], &s0, &c0); sincos(x[1], &s1, &c1); sincos(x[2], &s2, &c2);
    Ri[0] = c2 * c1; Ri[1] = (c2 * s1) * s0 - s2 * c0; Ri[2] = (c2 * s1) * c0 + s2 * s0;
    Ri[3] = s2 * c1; Ri[4] = (s2 * s1) * s0 + c2 * c0; Ri[5] = (s2 * s1) * c0 - c2 * s0;
    Ri[6] = -s1;     Ri[7] = c1 * s0;                  Ri[8] = c1 * c0;
    ti[0] = x[3]; ti[1] = x[4]; ti[2] = x[5];
  }
  if (!finite) {
    for (int e = 0; e < 9; ++e) Ri[e] = __builtin_nan("");
    for (int r = 0; r < 3; ++r) ti[r] = __builtin_nan("");
  }
  double* pose = p.st.pose + (size_t)b * 12;
  double Rk[9], tk[3], Rn[9], tn[3];
  for (int i = 0; i < 9; ++i) Rk[i] = pose[i];
  for (int i = 0; i < 3; ++i) tk[i] = pose[9 + i];
  for (int i = 0; i < 3; ++i) {                            // refine_cloud_kernel's composition
    for (int j = 0; j < 3; ++j) Rn[3 * i + j] = (Ri[3 * i] * Rk[j] + Ri[3 * i + 1] * Rk[3 + j]) + Ri[3 * i + 2] * Rk[6 + j];
    tn[i] = ((Ri[3 * i] * tk[0] + Ri[3 * i + 1] * tk[1]) + Ri[3 * i + 2] * tk[2]) + ti[i];
  }
  float rf[9], tf[3];
  for (int i = 0; i < 9; ++i) { pose[i] = Rn[i]; rf[i] = (float)Rn[i]; }
  for (int i = 0; i < 3; ++i) { pose[9 + i] = tn[i]; tf[i] = (float)tn[i]; }
  rf_store_pose(rf, tf, b, p.R_out, p.t_out, p.R_ba, p.t_ba);
}

}  // namespace

// vcr_refine_args' fields lead vcr_refine_plane_args, in its order and at its offsets: the shared plan reads them as one
static_assert(offsetof(vcr_refine_plane_args, variant) == offsetof(vcr_refine_args, variant) &&
              offsetof(vcr_refine_plane_args, tgt_normals) == sizeof(vcr_refine_args), "vcr_refine_plane_args = vcr_refine_args + tgt_normals");

static int pl_take(const vcr_refine_plane_args* user, vcr_refine_plane_args* mine, vcr_refine_args* lead) {
  if (vcr_take_args(user, mine, sizeof(vcr_refine_plane_args))) return VCR_EINVAL;
  memcpy((void*)lead, (const void*)mine, sizeof(*lead));
  lead->struct_bytes = (uint32_t)sizeof(*lead);
  return VCR_OK;
}

static int pl_plan(const vcr_refine_plane_args& a, const vcr_refine_args& lead, int cu, RfPlan* p) {
  if (!a.tgt_normals) { *p = RfPlan{}; return VCR_EINVAL; }
  return rf_plan(lead, cu, PL_VALUES, p);
}

extern "C" int vcr_refine_plane_form(const vcr_refine_plane_args* ua, int cu_count, int* queries_per_lane, int* target_splits) {
  vcr_refine_plane_args a;
  vcr_refine_args lead;
  RfPlan p;
  if (pl_take(ua, &a, &lead) || cu_count < 0) return VCR_EINVAL;
  const int e = pl_plan(a, lead, cu_count ? cu_count : vcr_cu_count(), &p);
  if (e) return e;
  if (queries_per_lane) *queries_per_lane = p.nn.Q;
  if (target_splits) *target_splits = p.nn.S;
  return VCR_OK;
}

extern "C" size_t vcr_refine_plane_workspace_bytes(const vcr_refine_plane_args* ua, int cu_count) {
  vcr_refine_plane_args a;
  vcr_refine_args lead;
  RfPlan p;
  if (pl_take(ua, &a, &lead) || cu_count < 0) return 0;
  return pl_plan(a, lead, cu_count ? cu_count : vcr_cu_count(), &p) ? 0 : p.bytes;
}

extern "C" int vcr_refine_plane_f32(const vcr_refine_plane_args* ua, void* workspace, size_t workspace_bytes, vcr_stream_t stream) {
  vcr_refine_plane_args a;
  vcr_refine_args lead;
  if (pl_take(ua, &a, &lead)) return VCR_EINVAL;
  // the argument checks need no device: only a call that passes them asks for the CU count
  RfPlan p;
  int e = pl_plan(a, lead, 1, &p);
  if (e) return e;
  if (!workspace || (((uintptr_t)workspace) & 15)) return VCR_EINVAL;
  vcr_stream_scope scope_(stream);
  e = pl_plan(a, lead, vcr_cu_count(), &p);
  if (e) return e;
  if (workspace_bytes < p.bytes) return VCR_EWORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  unsigned char* w = reinterpret_cast<unsigned char*>(workspace);
  const NnPlan& nn = p.nn;
  double* part = reinterpret_cast<double*>(w + p.part_off);
  const RfState st{reinterpret_cast<double*>(w + p.pose_off), reinterpret_cast<float*>(w + p.prev_off),
                   reinterpret_cast<int*>(w + p.live_off), reinterpret_cast<int*>(w + p.iters_off)};
  const RfInit in{a.R, a.t, a.B, st, a.R_out, a.t_out, a.R_ba, a.t_ba};
  hipLaunchKernelGGL(refine_init_kernel, dim3((unsigned)((a.B + NN_BLOCK - 1) / NN_BLOCK)), dim3(NN_BLOCK), 0, s, in);
  if ((e = VCR_LAUNCH_RC())) return e;
  const PlMerge mg{reinterpret_cast<const float*>(w), reinterpret_cast<const int*>(w + nn.part_bytes), a.src, a.tgt, a.tgt_normals,
                   a.R_out, a.t_out, a.B, a.Ns, a.Nt, nn.S, nn.nblk, a.max_dist * a.max_dist, a.nn_idx, a.nn_d2, part, st.live};
  for (int round = 0; round <= a.max_iterations; ++round) {
    if ((e = nn_scan_launch(nn, workspace, st.live, s))) return e;
    hipLaunchKernelGGL(plane_merge_kernel, dim3(nn.merge_grid), dim3(NN_BLOCK), 0, s, mg);
    if ((e = VCR_LAUNCH_RC())) return e;
    const PlCloud cl{part, a.Ns, nn.nblk, round, a.max_iterations, a.rel_fitness, a.rel_rmse, st,
                     a.R_out, a.t_out, a.fitness, a.rmse, a.R_ba, a.t_ba, a.inliers, a.sum_d2, a.iterations, a.converged};
    hipLaunchKernelGGL(plane_cloud_kernel, dim3((unsigned)a.B), dim3(NN_BLOCK), 0, s, cl);
    if ((e = VCR_LAUNCH_RC())) return e;
  }
  return VCR_OK;
}

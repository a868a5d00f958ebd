// Refining a registration on the full clouds (include/vcr_hip_refine.h): a trimmed point-to-point ICP whose
// every round is nnscore's scan (nn_scan.h: one text, gated per cloud here) followed by two kernels of this file.
//
// One launch up front and three per round, max_iterations + 1 rounds, all enqueued at once (no host synchronisation):
//   refine_init_kernel    (refine_state.h, shared with refine_plane.hip) one lane per cloud: the fp64 pose, its fp32 rounding in
//                         R_out / t_out (what the scan reads), live = 1.
//   nn_scan_kernel<Q>     as vcr_nn_score_f32 runs it, under (R_out, t_out).
//   refine_merge_kernel   one lane per source point: folds the S candidates as nn_merge_kernel does (nn_fold), writes nn_idx /
//                         nn_d2, recomputes the moved point (the scan's expression), gathers the neighbour and reduces its 256
//                         points to seventeen fp64 values -- sum of d2, count, S_p, S_q, S_pq over the inliers -- in
//                         nn_merge_kernel's order: wave butterfly 32 ... 1, the four waves ascending.
//   refine_cloud_kernel   one workgroup per cloud: the partials in ascending order; the round's evaluation (nn_final_kernel's
//                         expressions); the convergence test; then H, the quad Jacobi and tail of svd3.h, the composed pose.
// live[b] is the gate: a workgroup of any of the three whose cloud has stopped returns before it loads anything else, and the
// cloud's outputs stay as its last evaluation wrote them -- a cloud's result does not depend on its batch.  The reductions'
// geometry depends on Ns alone, so every form of the scan returns the same bits.  No atomics.
#include "refine_state.h"
#include "svd3.h"

namespace {

constexpr int RF_VALUES = 17;                              // sum_d2, count, S_p[3], S_q[3], S_pq[9]
constexpr int RF_CHUNK = 128;                              // partials the per-cloud kernel stages in LDS at a time (17 KB)

struct RfMerge {
  const float* part_d2; const int* part_idx;
  const float* src; const float* tgt; const float* R; const float* t;   // the fp32 pose the scan ran under
  int B, Ns, Nt, S, nblk;                                  // nblk = ceil(Ns / 256)
  float max_d2;
  int* nn_idx; float* nn_d2;
  double* part;                                            // [B][nblk][RF_VALUES]
  const int* live;
};

__global__ __launch_bounds__(NN_BLOCK) void refine_merge_kernel(RfMerge p) {
  __shared__ double red[NN_BLOCK / 64][RF_VALUES];
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
  // an inlier's d2 is finite, so its moved point and its neighbour are; every other lane contributes exact zeros
  float pc[3] = {0.f, 0.f, 0.f}, qc[3] = {0.f, 0.f, 0.f};
  if (in) {                                                // bi is in [0, Nt): a target index the scan wrote
    const float* sx = p.src + (size_t)b * 3 * Ns;
    const float* tx = p.tgt + (size_t)b * 3 * Nt;
    const float* r = p.R + (size_t)b * 9;
    const float* tr = p.t + (size_t)b * 3;
    const float x = sx[n], y = sx[Ns + n], z = sx[2 * (size_t)Ns + n];
    for (int c = 0; c < 3; ++c) {                          // the scan's expression, bit for bit
      pc[c] = fmaf(r[3 * c + 2], z, fmaf(r[3 * c + 1], y, r[3 * c] * x)) + tr[c];
      qc[c] = tx[(size_t)c * Nt + bi];
    }
  }
  auto put = [&](int e, double v) {                        // one value across the wave, nn_merge_kernel's butterfly
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    if ((t & 63) == 0) red[t >> 6][e] = v;
  };
  put(0, in ? (double)best : 0.);
  put(1, in ? 1. : 0.);
#pragma unroll
  for (int c = 0; c < 3; ++c) { put(2 + c, (double)pc[c]); put(5 + c, (double)qc[c]); }
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c) put(8 + 3 * r + c, (double)pc[r] * (double)qc[c]);   // exact: 24 x 24 bits
  __syncthreads();
  if (t < RF_VALUES) {
    double s = red[0][t];
    for (int w = 1; w < NN_BLOCK / 64; ++w) s += red[w][t];
    p.part[((size_t)b * p.nblk + blk) * RF_VALUES + t] = s;
  }
}

struct RfCloud {
  const double* part; int Ns, nblk;
  int round, max_iterations; float rel_fitness, rel_rmse;
  RfState st;
  float* R_out; float* t_out; float* fitness; float* rmse; float* R_ba; float* t_ba;
  int* inliers; double* sum_d2; int* iterations; int* converged;
};

__global__ __launch_bounds__(NN_BLOCK) void refine_cloud_kernel(RfCloud p) {
  __shared__ double stage[RF_CHUNK * RF_VALUES];
  __shared__ double tot[RF_VALUES];
  const int t = threadIdx.x, b = blockIdx.x;
  if (!p.st.live[b]) return;                               // (workgroup-uniform; written only by this workgroup's thread 0, behind the barriers)
  const double* part = p.part + (size_t)b * p.nblk * RF_VALUES;
  double acc = 0.;
  for (int c0 = 0; c0 < p.nblk; c0 += RF_CHUNK) {          // (workgroup-uniform)
    const int m = p.nblk - c0 < RF_CHUNK ? p.nblk - c0 : RF_CHUNK;
    __syncthreads();
    for (int i = t; i < m * RF_VALUES; i += NN_BLOCK) stage[i] = part[(size_t)c0 * RF_VALUES + i];
    __syncthreads();
    if (t < RF_VALUES)
      for (int i = 0; i < m; ++i) acc += stage[i * RF_VALUES + t];      // ascending, one lane per value: the order is Ns's alone
  }
  if (t < RF_VALUES) tot[t] = acc;
  __syncthreads();
  if (t >= 64) return;                                     // wave 0 finishes; its first quad runs the Jacobi sweeps together
  double v17[RF_VALUES];
#pragma unroll
  for (int e = 0; e < RF_VALUES; ++e) v17[e] = tot[e];
  // the round's evaluation: nn_final_kernel's expressions
  const double sum = v17[0];
  const int cnt = (int)v17[1];
  const float fitness = (float)cnt / (float)p.Ns;
  const float rmse = cnt > 0 ? (float)sqrt(sum / (double)cnt) : 0.f;
  // prev[] and iters[b] are read here by every lane of wave 0 and written below by its lane 0 alone: one wave, program order
  bool conv = false;
  if (p.round > 0)
    conv = fabsf(fitness - p.st.prev[2 * b]) < p.rel_fitness && fabsf(rmse - p.st.prev[2 * b + 1]) < p.rel_rmse;
  const bool step = !conv && p.round < p.max_iterations && cnt >= 3;
  const int iters = p.st.iters[b] + (step ? 1 : 0);
  if (t == 0) {
    p.fitness[b] = fitness; p.rmse[b] = rmse;
    if (p.inliers) p.inliers[b] = cnt;
    if (p.sum_d2) p.sum_d2[b] = sum;
    if (p.iterations) p.iterations[b] = iters;
    if (p.converged) p.converged[b] = conv ? 1 : 0;
    p.st.prev[2 * b] = fitness; p.st.prev[2 * b + 1] = rmse;
    p.st.iters[b] = iters;
    p.st.live[b] = step ? 1 : 0;
  }
  if (!step) return;                                       // (wave-uniform)
  const double inv_n = 1.0 / v17[1];
  double H[9];
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c) H[3 * r + c] = v17[8 + 3 * r + c] - (v17[2 + r] * v17[5 + c]) * inv_n;
  const int li = t & 3;
  double a[3], v[3];
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    a[j] = li == 0 ? H[j] : li == 1 ? H[3 + j] : li == 2 ? H[6 + j] : 0.0;
    v[j] = li == j ? 1.0 : 0.0;
  }
  jacobi_sweeps_quad(a, v);
  double A[3][3], V[3][3];
#pragma unroll
  for (int j = 0; j < 3; ++j) {                            // gather the rows (lane i of the quad = row i)
    A[0][j] = quad_get(a[j], 0); A[1][j] = quad_get(a[j], 1); A[2][j] = quad_get(a[j], 2);
    V[0][j] = quad_get(v[j], 0); V[1][j] = quad_get(v[j], 1); V[2][j] = quad_get(v[j], 2);
  }
  if (t != 0) return;
  double Ri[9], ti[3];
  svd3_finish(A, V, Ri);
  bool finite = true;                                      // as rigid_svd_kernel: stated here, not left to the sweeps
  for (int e = 2; e < RF_VALUES; ++e) finite = finite && __builtin_isfinite(v17[e]);
  for (int r = 0; r < 3; ++r)
    ti[r] = v17[5 + r] * inv_n - (Ri[3 * r] * (v17[2] * inv_n) + Ri[3 * r + 1] * (v17[3] * inv_n) + Ri[3 * r + 2] * (v17[4] * inv_n));
  if (!finite) {
    for (int e = 0; e < 9; ++e) Ri[e] = __builtin_nan("");
    for (int r = 0; r < 3; ++r) ti[r] = __builtin_nan("");
  }
  double* pose = p.st.pose + (size_t)b * 12;
  double Rk[9], tk[3], Rn[9], tn[3];
  for (int i = 0; i < 9; ++i) Rk[i] = pose[i];
  for (int i = 0; i < 3; ++i) tk[i] = pose[9 + i];
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) Rn[3 * i + j] = (Ri[3 * i] * Rk[j] + Ri[3 * i + 1] * Rk[3 + j]) + Ri[3 * i + 2] * Rk[6 + j];
    tn[i] = ((Ri[3 * i] * tk[0] + Ri[3 * i + 1] * tk[1]) + Ri[3 * i + 2] * tk[2]) + ti[i];
  }
  float rf[9], tf[3];
  for (int i = 0; i < 9; ++i) { pose[i] = Rn[i]; rf[i] = (float)Rn[i]; }
  for (int i = 0; i < 3; ++i) { pose[9 + i] = tn[i]; tf[i] = (float)tn[i]; }
  rf_store_pose(rf, tf, b, p.R_out, p.t_out, p.R_ba, p.t_ba);
}

}  // namespace

static int rf_take(const vcr_refine_args* user, vcr_refine_args* mine) {
  return vcr_take_args(user, mine, offsetof(vcr_refine_args, R_ba));
}

extern "C" int vcr_refine_form(const vcr_refine_args* ua, int cu_count, int* queries_per_lane, int* target_splits) {
  vcr_refine_args a;
  RfPlan p;
  if (rf_take(ua, &a) || cu_count < 0) return VCR_EINVAL;
  const int e = rf_plan(a, cu_count ? cu_count : vcr_cu_count(), RF_VALUES, &p);
  if (e) return e;
  if (queries_per_lane) *queries_per_lane = p.nn.Q;
  if (target_splits) *target_splits = p.nn.S;
  return VCR_OK;
}

extern "C" size_t vcr_refine_workspace_bytes(const vcr_refine_args* ua, int cu_count) {
  vcr_refine_args a;
  RfPlan p;
  if (rf_take(ua, &a) || cu_count < 0) return 0;
  return rf_plan(a, cu_count ? cu_count : vcr_cu_count(), RF_VALUES, &p) ? 0 : p.bytes;
}

extern "C" int vcr_refine_f32(const vcr_refine_args* ua, void* workspace, size_t workspace_bytes, vcr_stream_t stream) {
  vcr_refine_args a;
  if (rf_take(ua, &a)) return VCR_EINVAL;
  // the argument checks need no device: only a call that passes them asks for the CU count
  RfPlan p;
  int e = rf_plan(a, 1, RF_VALUES, &p);
  if (e) return e;
  if (!workspace || (((uintptr_t)workspace) & 15)) return VCR_EINVAL;
  vcr_stream_scope scope_(stream);
  e = rf_plan(a, vcr_cu_count(), RF_VALUES, &p);
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
  const RfMerge mg{reinterpret_cast<const float*>(w), reinterpret_cast<const int*>(w + nn.part_bytes), a.src, a.tgt, a.R_out, a.t_out,
                   a.B, a.Ns, a.Nt, nn.S, nn.nblk, a.max_dist * a.max_dist, a.nn_idx, a.nn_d2, part, st.live};
  for (int round = 0; round <= a.max_iterations; ++round) {
    if ((e = nn_scan_launch(nn, workspace, st.live, s))) return e;
    hipLaunchKernelGGL(refine_merge_kernel, dim3(nn.merge_grid), dim3(NN_BLOCK), 0, s, mg);
    if ((e = VCR_LAUNCH_RC())) return e;
    const RfCloud cl{part, a.Ns, nn.nblk, round, a.max_iterations, a.rel_fitness, a.rel_rmse, st,
                     a.R_out, a.t_out, a.fitness, a.rmse, a.R_ba, a.t_ba, a.inliers, a.sum_d2, a.iterations, a.converged};
    hipLaunchKernelGGL(refine_cloud_kernel, dim3((unsigned)a.B), dim3(NN_BLOCK), 0, s, cl);
    if ((e = VCR_LAUNCH_RC())) return e;
  }
  return VCR_OK;
}

// Refining a registration on the full clouds (include/vcr_hip_refine.h): a trimmed point-to-point ICP whose
// every round is nnscore's scan (nn_scan.h: one text, gated per cloud here) followed by two kernels of this file.
//
// One launch up front and three per round, max_iterations + 1 rounds, all enqueued at once (no host synchronisation):
//   refine_init_kernel    (refine_round.h, shared with refine_plane.hip) one lane per cloud: the fp64 pose, its fp32 rounding in
//                         R_out / t_out (what the scan reads), live = 1.
//   nn_scan_kernel<Q>     as vcr_nn_score_f32 runs it, under (R_out, t_out).
//   refine_merge_kernel   rf_merge_body (refine_round.h) with PointFit: per workgroup of 256 source points seventeen fp64
//                         values -- sum of d2, count, S_p, S_q, S_pq over the inliers.
//   refine_cloud_kernel   one workgroup per cloud: the partials in ascending order, the round's evaluation and the convergence
//                         test (refine_round.h); then what is this file's: H, the quad Jacobi and tail of svd3.h; and the
//                         composed pose (refine_round.h again).
// live[b] is the gate: a workgroup of any of the three whose cloud has stopped returns before it loads anything else, and the
// cloud's outputs stay as its last evaluation wrote them -- a cloud's result does not depend on its batch.  The reductions'
// geometry depends on Ns alone, so every form of the scan returns the same bits.  No atomics.
// The loop itself -- the plan, the workspace, the launches -- is refine_round.h's rf_run; this file holds the fit.
#include "refine_round.h"
#include "svd3.h"

namespace {

struct PointFit {
  static constexpr int VALUES = 17;                        // sum_d2, count, S_p[3], S_q[3], S_pq[9]
  static constexpr int CHUNK = 128;                        // (17 KB of LDS)
  static constexpr int MIN_INLIERS = 3;
  __device__ float gather(int, int, int, int) const { return 0.f; }   // the neighbour is all it reads
  __device__ float source(int, int, int, int) const { return 0.f; }
  template <class Put>
  __device__ void sums(const RfPoint& pt, Put& put) const {
    const float* pc = pt.pc; const float* qc = pt.qc;
#pragma unroll
    for (int c = 0; c < 3; ++c) { put(2 + c, (double)pc[c]); put(5 + c, (double)qc[c]); }
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int c = 0; c < 3; ++c) put(8 + 3 * r + c, (double)pc[r] * (double)qc[c]);   // exact: 24 x 24 bits
  }
  using Args = vcr_refine_args;
  static int take(const Args* user, vcr_refine_args* mine, PointFit*) {
    return vcr_take_args(user, mine, offsetof(vcr_refine_args, R_ba));
  }
};

__global__ __launch_bounds__(NN_BLOCK) void refine_merge_kernel(RfMerge<PointFit> p) { rf_merge_body(p); }

__global__ __launch_bounds__(NN_BLOCK) void refine_cloud_kernel(RfCloud p) {
  const int t = threadIdx.x, b = blockIdx.x;
  if (!p.st.live[b]) return;                               // (workgroup-uniform; written only by this workgroup's thread 0, behind the barriers)
  const double* tot = rf_total<PointFit::VALUES, PointFit::CHUNK>(p.part + (size_t)b * p.nblk * PointFit::VALUES, p.nblk);
  if (t >= 64) return;                                     // wave 0 finishes; its first quad runs the Jacobi sweeps together
  double v17[PointFit::VALUES];
#pragma unroll
  for (int e = 0; e < PointFit::VALUES; ++e) v17[e] = tot[e];
  const bool step = rf_evaluate(p, b, v17, PointFit::MIN_INLIERS, t == 0, [](bool may) { return may; });
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
  const bool finite = rf_sums_finite<PointFit::VALUES>(v17);
  for (int r = 0; r < 3; ++r)
    ti[r] = v17[5 + r] * inv_n - (Ri[3 * r] * (v17[2] * inv_n) + Ri[3 * r + 1] * (v17[3] * inv_n) + Ri[3 * r + 2] * (v17[4] * inv_n));
  rf_step_pose(p, b, Ri, ti, finite);
}

}  // namespace

extern "C" int vcr_refine_form(const vcr_refine_args* ua, int cu_count, int* queries_per_lane, int* target_splits) {
  return rf_form<PointFit>(ua, cu_count, queries_per_lane, target_splits);
}

extern "C" size_t vcr_refine_workspace_bytes(const vcr_refine_args* ua, int cu_count) { return rf_workspace_bytes<PointFit>(ua, cu_count); }

extern "C" int vcr_refine_f32(const vcr_refine_args* ua, void* workspace, size_t workspace_bytes, vcr_stream_t stream) {
  return rf_run<PointFit>(ua, nullptr, workspace, workspace_bytes, stream, refine_merge_kernel, refine_cloud_kernel);
}

// The grid siblings (include/vcr_hip_gridnn.h): the same loop behind another search
extern "C" int vcr_refine_grid_form(const vcr_refine_args* ua, const vcr_grid_nn_args* ug, int cu_count, int* cells_per_cloud, int* order,
                                    int* queries_per_workgroup) {
  return rf_grid_form<PointFit>(ua, ug, cu_count, cells_per_cloud, order, queries_per_workgroup);
}

extern "C" size_t vcr_refine_grid_workspace_bytes(const vcr_refine_args* ua, const vcr_grid_nn_args* ug, int cu_count) {
  return rf_grid_workspace_bytes<PointFit>(ua, ug, cu_count);
}

extern "C" int vcr_refine_grid_f32(const vcr_refine_args* ua, const vcr_grid_nn_args* ug, void* workspace, size_t workspace_bytes,
                                   vcr_stream_t stream) {
  if (!ug) return VCR_EINVAL;
  return rf_run<PointFit>(ua, ug, workspace, workspace_bytes, stream, refine_merge_kernel, refine_cloud_kernel);
}

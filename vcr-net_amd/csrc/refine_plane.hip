// Refining a registration on the full clouds, point to plane (include/vcr_hip_plane.h): vcr_refine_f32's
// loop with another fit.  The loop is written once, in refine_round.h -- refine_init_kernel up front, then per round
// nn_scan_kernel<Q> (nn_scan.h) and two kernels of this file; the gate live[b], the fp64 pose, the evaluation, the stop test
// and the host driver rf_run -- and this file holds what is the fit's:
//   plane_merge_kernel    rf_merge_body with PlaneFit: it gathers the neighbour q AND ITS NORMAL, and reduces the workgroup's
//                         256 points to twenty-nine fp64 values -- sum of d2, count, A = sum J J^T (21), g = sum J r (6) over the
//                         inliers, J = (p x nrm, nrm), r = p.nrm - q.nrm -- one value at a time through the butterfly, so that
//                         they are never live together.
//   plane_cloud_kernel    one workgroup per cloud: the partials in ascending order; then one lane: the round's evaluation, the
//                         convergence test, A x = -g by Cholesky, R_i = Rz(x2) Ry(x1) Rx(x0), t_i = (x3, x4, x5) (both in
//                         refine_solve6.h, shared with refine_gicp.hip), the composed pose.  A singular system stops the cloud
//                         like too few inliers do: the solve runs before the state is written.
#include "refine_round.h"
#include "refine_solve6.h"
#include "../../include/vcr_hip_plane.h"

// vcr_refine_args' fields lead vcr_refine_plane_args, in its order and at its offsets: the shared plan reads them as one
static_assert(offsetof(vcr_refine_plane_args, variant) == offsetof(vcr_refine_args, variant) &&
              offsetof(vcr_refine_plane_args, tgt_normals) == sizeof(vcr_refine_args), "vcr_refine_plane_args = vcr_refine_args + tgt_normals");

namespace {

struct PlaneFit {
  static constexpr int VALUES = 29;                        // sum_d2, count, A's upper triangle by rows [21], g[6]
  static constexpr int CHUNK = 64;                         // (15 KB of LDS)
  static constexpr int MIN_INLIERS = 6;                    // six unknowns
  const float* nrm;                                        // the target's normals, [B][3][Nt]
  __device__ float gather(int b, int Nt, int c, int bi) const {
    const float* nx = nrm + (size_t)b * 3 * Nt;
    return nx[(size_t)c * Nt + bi];
  }
  __device__ float source(int, int, int, int) const { return 0.f; }   // nothing of the source but the point
  template <class Put>
  __device__ void sums(const RfPoint& pt, Put& put) const {
    const float* pc = pt.pc; const float* qc = pt.qc; const float* nc = pt.gc;
    const double p0 = (double)pc[0], p1 = (double)pc[1], p2 = (double)pc[2];
    const double m0 = (double)nc[0], m1 = (double)nc[1], m2 = (double)nc[2];
    double J[6];                                           // products of two fp32 values: exact
    J[0] = p1 * m2 - p2 * m1; J[1] = p2 * m0 - p0 * m2; J[2] = p0 * m1 - p1 * m0;
    J[3] = m0; J[4] = m1; J[5] = m2;
    const double res = ((p0 * m0 + p1 * m1) + p2 * m2) - (((double)qc[0] * m0 + (double)qc[1] * m1) + (double)qc[2] * m2);
    int e = 2;
#pragma unroll
    for (int r = 0; r < 6; ++r)
#pragma unroll
      for (int c = r; c < 6; ++c) put(e++, J[r] * J[c]);
#pragma unroll
    for (int r = 0; r < 6; ++r) put(e++, J[r] * res);
  }
  using Args = vcr_refine_plane_args;
  static int take(const Args* user, vcr_refine_args* lead, PlaneFit* fit) {
    Args mine;
    if (vcr_take_args(user, &mine, sizeof(Args)) || !mine.tgt_normals) return VCR_EINVAL;
    memcpy((void*)lead, (const void*)&mine, sizeof(*lead));
    lead->struct_bytes = (uint32_t)sizeof(*lead);
    fit->nrm = mine.tgt_normals;
    return VCR_OK;
  }
};

__global__ __launch_bounds__(NN_BLOCK) void plane_merge_kernel(RfMerge<PlaneFit> p) { rf_merge_body(p); }

__global__ __launch_bounds__(NN_BLOCK) void plane_cloud_kernel(RfCloud p) {
  const int t = threadIdx.x, b = blockIdx.x;
  if (!p.st.live[b]) return;                               // (workgroup-uniform; written only by this workgroup's thread 0, behind the barriers)
  const double* tot = rf_total<PlaneFit::VALUES, PlaneFit::CHUNK>(p.part + (size_t)b * p.nblk * PlaneFit::VALUES, p.nblk);
  if (t != 0) return;                                      // one lane finishes
  double v[PlaneFit::VALUES];
#pragma unroll
  for (int e = 0; e < PlaneFit::VALUES; ++e) v[e] = tot[e];
  const bool finite = rf_sums_finite<PlaneFit::VALUES>(v);
  double x[6] = {0., 0., 0., 0., 0., 0.};
  // (a singular system stops the cloud; non-finite sums step to a NaN pose)
  const bool step = rf_evaluate(p, b, v, PlaneFit::MIN_INLIERS, true, [&](bool may) { return may && finite ? pl_solve(v + 2, v + 23, x) : may; });
  if (!step) return;
  double Ri[9], ti[3];
  pl_euler(x, Ri, ti);
  rf_step_pose(p, b, Ri, ti, finite);
}

}  // namespace

extern "C" int vcr_refine_plane_form(const vcr_refine_plane_args* ua, int cu_count, int* queries_per_lane, int* target_splits) {
  return rf_form<PlaneFit>(ua, cu_count, queries_per_lane, target_splits);
}

extern "C" size_t vcr_refine_plane_workspace_bytes(const vcr_refine_plane_args* ua, int cu_count) { return rf_workspace_bytes<PlaneFit>(ua, cu_count); }

extern "C" int vcr_refine_plane_f32(const vcr_refine_plane_args* ua, void* workspace, size_t workspace_bytes, vcr_stream_t stream) {
  return rf_run<PlaneFit>(ua, nullptr, workspace, workspace_bytes, stream, plane_merge_kernel, plane_cloud_kernel);
}

// The grid siblings (include/vcr_hip_gridnn.h): the same loop behind another search
extern "C" int vcr_refine_plane_grid_form(const vcr_refine_plane_args* ua, const vcr_grid_nn_args* ug, int cu_count, int* cells_per_cloud, int* order,
                                          int* queries_per_workgroup) {
  return rf_grid_form<PlaneFit>(ua, ug, cu_count, cells_per_cloud, order, queries_per_workgroup);
}

extern "C" size_t vcr_refine_plane_grid_workspace_bytes(const vcr_refine_plane_args* ua, const vcr_grid_nn_args* ug, int cu_count) {
  return rf_grid_workspace_bytes<PlaneFit>(ua, ug, cu_count);
}

extern "C" int vcr_refine_plane_grid_f32(const vcr_refine_plane_args* ua, const vcr_grid_nn_args* ug, void* workspace, size_t workspace_bytes,
                                         vcr_stream_t stream) {
  if (!ug) return VCR_EINVAL;
  return rf_run<PlaneFit>(ua, ug, workspace, workspace_bytes, stream, plane_merge_kernel, plane_cloud_kernel);
}

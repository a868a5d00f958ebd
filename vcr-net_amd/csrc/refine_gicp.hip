// Refining a registration on the full clouds, plane to plane (include/vcr_hip_gicp.h): vcr_refine_f32's
// loop with a third fit, Open3D's generalized ICP with covariances built from the normals of both clouds.  The loop is
// refine_round.h's, the solve and the Euler step refine_solve6.h's (shared with refine_plane.hip); this file holds the fit:
//   gicp_merge_kernel     rf_merge_body with GicpFit: it gathers the neighbour q and ITS normal m, reads the source point's OWN
//                         normal s, turns it by the fp32 pose the merge holds, inverts M = C_t + R C_s R^T (3 x 3, symmetric,
//                         by cofactors) and reduces the workgroup's 256 points to twenty-nine fp64 values -- sum of d2, count,
//                         A = sum J^T W J (21), g = sum J^T W d (6), J = [-skew(p) | I] -- one value at a time through the
//                         butterfly: W (6), p and d are the live state.
//   gicp_cloud_kernel     plane_cloud_kernel with MIN_INLIERS = 3.
// THE MASK: PlaneFit's terms are products of the lane's inputs, so a lane that is no inlier (zero inputs) adds exact zeros.
// Here zero inputs give M = 2 I, W = I / 2 and a_3..5 = e_c: not zero.  Such lanes -- stopped by max_dist, without a neighbour,
// or beyond Ns in the last workgroup -- get W = 0 explicitly.
#include "refine_round.h"
#include "refine_solve6.h"
#include "../../include/vcr_hip_gicp.h"

// vcr_refine_args' fields lead vcr_refine_gicp_args, in its order and at its offsets: the shared plan reads them as one
static_assert(offsetof(vcr_refine_gicp_args, variant) == offsetof(vcr_refine_args, variant) &&
              offsetof(vcr_refine_gicp_args, tgt_normals) == sizeof(vcr_refine_args) &&
              offsetof(vcr_refine_gicp_args, tgt_normals) == offsetof(vcr_refine_plane_args, tgt_normals),
              "vcr_refine_gicp_args = vcr_refine_args + tgt_normals, src_normals, epsilon");

namespace {

struct GicpFit {
  static constexpr int VALUES = 29;                        // sum_d2, count, A's upper triangle by rows [21], g[6]
  static constexpr int CHUNK = 64;                         // (15 KB of LDS)
  static constexpr int MIN_INLIERS = 3;                    // three residuals a pair
  const float* nrm_t;                                      // the target's normals, [B][3][Nt]
  const float* nrm_s;                                      // the source's, [B][3][Ns]
  float epsilon;
  __device__ float gather(int b, int Nt, int c, int bi) const { return nrm_t[(size_t)b * 3 * Nt + (size_t)c * Nt + bi]; }
  __device__ float source(int b, int Ns, int c, int n) const { return nrm_s[(size_t)b * 3 * Ns + (size_t)c * Ns + n]; }
  template <class Put>
  __device__ void sums(const RfPoint& pt, Put& put) const {
    double W[6];                                           // W00 W01 W02 W11 W12 W22
    {
      const double kap = 1.0 - (double)epsilon;
      const double m0 = (double)pt.gc[0], m1 = (double)pt.gc[1], m2 = (double)pt.gc[2];
      const double s0 = (double)pt.sc[0], s1 = (double)pt.sc[1], s2 = (double)pt.sc[2];
      double n[3] = {0., 0., 0.};
      if (pt.in) {                                         // (the pose is read by inliers only, as the moved point's was)
#pragma unroll
        for (int c = 0; c < 3; ++c) n[c] = ((double)pt.R[3 * c] * s0 + (double)pt.R[3 * c + 1] * s1) + (double)pt.R[3 * c + 2] * s2;
      }
      const double M00 = 2.0 - kap * (m0 * m0 + n[0] * n[0]), M01 = 0.0 - kap * (m0 * m1 + n[0] * n[1]);
      const double M02 = 0.0 - kap * (m0 * m2 + n[0] * n[2]), M11 = 2.0 - kap * (m1 * m1 + n[1] * n[1]);
      const double M12 = 0.0 - kap * (m1 * m2 + n[1] * n[2]), M22 = 2.0 - kap * (m2 * m2 + n[2] * n[2]);
      const double K00 = M11 * M22 - M12 * M12, K01 = M02 * M12 - M01 * M22, K02 = M01 * M12 - M02 * M11;
      const double K11 = M00 * M22 - M02 * M02, K12 = M01 * M02 - M00 * M12, K22 = M00 * M11 - M01 * M01;
      const double det = (M00 * K00 + M01 * K01) + M02 * K02;
      W[0] = pt.in ? K00 / det : 0.; W[1] = pt.in ? K01 / det : 0.; W[2] = pt.in ? K02 / det : 0.;
      W[3] = pt.in ? K11 / det : 0.; W[4] = pt.in ? K12 / det : 0.; W[5] = pt.in ? K22 / det : 0.;   // the mask
    }
    const double p0 = (double)pt.pc[0], p1 = (double)pt.pc[1], p2 = (double)pt.pc[2];
    const double d0 = p0 - (double)pt.qc[0], d1 = p1 - (double)pt.qc[1], d2 = p2 - (double)pt.qc[2];
    auto w = [&](int i, int j) -> double {                 // W_ij of the symmetric W
      const int a = i < j ? i : j, b = i < j ? j : i;       // a <= b
      return W[a == 0 ? b : a == 1 ? 2 + b : 5];
    };
    // a_r . v
    auto dot = [&](int r, double v0, double v1, double v2) -> double {
      return r == 0 ? p1 * v2 - p2 * v1 : r == 1 ? p2 * v0 - p0 * v2 : r == 2 ? p0 * v1 - p1 * v0 : r == 3 ? v0 : r == 4 ? v1 : v2;
    };
    int e = 2;
#pragma unroll
    for (int r = 0; r < 6; ++r)
#pragma unroll
      for (int c = r; c < 6; ++c) {
        double u[3];                                       // u_c = W a_c
#pragma unroll
        for (int i = 0; i < 3; ++i)
          u[i] = c == 0 ? p1 * w(i, 2) - p2 * w(i, 1) : c == 1 ? p2 * w(i, 0) - p0 * w(i, 2) : c == 2 ? p0 * w(i, 1) - p1 * w(i, 0) : w(i, c - 3);
        put(e++, dot(r, u[0], u[1], u[2]));
      }
    {
      const double e0 = (w(0, 0) * d0 + w(0, 1) * d1) + w(0, 2) * d2;
      const double e1 = (w(1, 0) * d0 + w(1, 1) * d1) + w(1, 2) * d2;
      const double e2 = (w(2, 0) * d0 + w(2, 1) * d1) + w(2, 2) * d2;
#pragma unroll
      for (int r = 0; r < 6; ++r) put(e++, dot(r, e0, e1, e2));
    }
  }
  using Args = vcr_refine_gicp_args;
  static int take(const Args* user, vcr_refine_args* lead, GicpFit* fit) {
    Args mine;
    if (vcr_take_args(user, &mine, sizeof(Args)) || !mine.tgt_normals || !mine.src_normals) return VCR_EINVAL;
    if (!(mine.epsilon > 0.f) || !(mine.epsilon <= 1.f)) return VCR_EINVAL;      // (a NaN fails both, an inf the second)
    memcpy((void*)lead, (const void*)&mine, sizeof(*lead));
    lead->struct_bytes = (uint32_t)sizeof(*lead);
    fit->nrm_t = mine.tgt_normals; fit->nrm_s = mine.src_normals; fit->epsilon = mine.epsilon;
    return VCR_OK;
  }
};

__global__ __launch_bounds__(NN_BLOCK) void gicp_merge_kernel(RfMerge<GicpFit> p) { rf_merge_body(p); }

__global__ __launch_bounds__(NN_BLOCK) void gicp_cloud_kernel(RfCloud p) {
  const int t = threadIdx.x, b = blockIdx.x;
  if (!p.st.live[b]) return;                               // (workgroup-uniform; written only by this workgroup's thread 0, behind the barriers)
  const double* tot = rf_total<GicpFit::VALUES, GicpFit::CHUNK>(p.part + (size_t)b * p.nblk * GicpFit::VALUES, p.nblk);
  if (t != 0) return;                                      // one lane finishes
  double v[GicpFit::VALUES];
#pragma unroll
  for (int e = 0; e < GicpFit::VALUES; ++e) v[e] = tot[e];
  const bool finite = rf_sums_finite<GicpFit::VALUES>(v);
  double x[6] = {0., 0., 0., 0., 0., 0.};
  // (a singular system stops the cloud; non-finite sums step to a NaN pose)
  const bool step = rf_evaluate(p, b, v, GicpFit::MIN_INLIERS, true, [&](bool may) { return may && finite ? pl_solve(v + 2, v + 23, x) : may; });
  if (!step) return;
  double Ri[9], ti[3];
  pl_euler(x, Ri, ti);
  rf_step_pose(p, b, Ri, ti, finite);
}

}  // namespace

extern "C" int vcr_refine_gicp_form(const vcr_refine_gicp_args* ua, int cu_count, int* queries_per_lane, int* target_splits) {
  return rf_form<GicpFit>(ua, cu_count, queries_per_lane, target_splits);
}

extern "C" size_t vcr_refine_gicp_workspace_bytes(const vcr_refine_gicp_args* ua, int cu_count) { return rf_workspace_bytes<GicpFit>(ua, cu_count); }

extern "C" int vcr_refine_gicp_f32(const vcr_refine_gicp_args* ua, void* workspace, size_t workspace_bytes, vcr_stream_t stream) {
  return rf_run<GicpFit>(ua, nullptr, workspace, workspace_bytes, stream, gicp_merge_kernel, gicp_cloud_kernel);
}

// The grid siblings (include/vcr_hip_gridnn.h): the same loop behind another search
extern "C" int vcr_refine_gicp_grid_form(const vcr_refine_gicp_args* ua, const vcr_grid_nn_args* ug, int cu_count, int* cells_per_cloud, int* order,
                                         int* queries_per_workgroup) {
  return rf_grid_form<GicpFit>(ua, ug, cu_count, cells_per_cloud, order, queries_per_workgroup);
}

extern "C" size_t vcr_refine_gicp_grid_workspace_bytes(const vcr_refine_gicp_args* ua, const vcr_grid_nn_args* ug, int cu_count) {
  return rf_grid_workspace_bytes<GicpFit>(ua, ug, cu_count);
}

extern "C" int vcr_refine_gicp_grid_f32(const vcr_refine_gicp_args* ua, const vcr_grid_nn_args* ug, void* workspace, size_t workspace_bytes,
                                        vcr_stream_t stream) {
  if (!ug) return VCR_EINVAL;
  return rf_run<GicpFit>(ua, ug, workspace, workspace_bytes, stream, gicp_merge_kernel, gicp_cloud_kernel);
}

// Refining a registration on the full clouds by colour and shape (include/colored/vcr_hip_colored.h):
// vcr_refine_f32's loop with a fourth fit, Open3D's colored ICP.  The loop is refine_round.h's, the solve and the Euler step
// refine_solve6.h's (shared with refine_plane.hip and refine_gicp.hip); this file holds the fit:
//   colored_merge_kernel  rf_merge_body with ColoredFit: it gathers the neighbour q and ITS normal as PlaneFit does, and fetches
//                         by RfPoint's indices what gather() and source() do not carry -- the neighbour's gradient (three
//                         strided loads) and intensity, and the source point's own intensity -- and reduces the workgroup's 256
//                         points to twenty-nine fp64 values: sum of d2, count, A = sum (J_G J_G^T + J_I J_I^T) (21),
//                         g = sum (J_G r_G + J_I r_I) (6), one value at a time through the butterfly: J_G, J_I, r_G, r_I are the
//                         live state.
//   colored_cloud_kernel  plane_cloud_kernel's text.
// A lane that is no inlier has zero inputs -- its extra loads are skipped and read as zero -- and every term is a product of
// them: it adds exact zeros, as PlaneFit's.  At lambda = 1 the weight of J_I is an exact zero and J_G is PlaneFit's J.
#include "refine_round.h"
#include "refine_solve6.h"
#include "../../include/colored/vcr_hip_colored.h"

// vcr_refine_args' fields lead vcr_refine_colored_args, in its order and at its offsets: the shared plan reads them as one
static_assert(offsetof(vcr_refine_colored_args, variant) == offsetof(vcr_refine_args, variant) &&
              offsetof(vcr_refine_colored_args, tgt_normals) == sizeof(vcr_refine_args) &&
              offsetof(vcr_refine_colored_args, tgt_normals) == offsetof(vcr_refine_plane_args, tgt_normals),
              "vcr_refine_colored_args = vcr_refine_args + tgt_normals, tgt_gradient, tgt_intensity, src_intensity, lambda_geometric");

namespace {

struct ColoredFit {
  static constexpr int VALUES = 29;                        // sum_d2, count, A's upper triangle by rows [21], g[6]
  static constexpr int CHUNK = 64;                         // (15 KB of LDS)
  static constexpr int MIN_INLIERS = 6;                    // six unknowns
  const float* nrm;                                        // the target's normals, [B][3][Nt]
  const float* grad;                                       // its colour gradients, [B][3][Nt]
  const float* it;                                         // its intensities, [B][Nt]
  const float* is;                                         // the source's, [B][Ns]
  int Ns, Nt;
  double wg, wi;                                           // sqrt(lambda), sqrt(1 - lambda)
  __device__ float gather(int b, int Nt_, int c, int bi) const { return nrm[(size_t)b * 3 * Nt_ + (size_t)c * Nt_ + bi]; }
  __device__ float source(int, int, int, int) const { return 0.f; }   // the source's intensity is one value: sums() fetches it
  template <class Put>
  __device__ void sums(const RfPoint& pt, Put& put) const {
    double d0 = 0., d1 = 0., d2 = 0., It = 0., Is = 0.;
    if (pt.in) {                                           // bi in [0, Nt), n in [0, Ns): the merge's own bounds
      const float* gx = grad + (size_t)pt.b * 3 * Nt + pt.bi;
      d0 = (double)gx[0]; d1 = (double)gx[Nt]; d2 = (double)gx[2 * (size_t)Nt];
      It = (double)it[(size_t)pt.b * Nt + pt.bi];
      Is = (double)is[(size_t)pt.b * Ns + pt.n];
    }
    const double p0 = (double)pt.pc[0], p1 = (double)pt.pc[1], p2 = (double)pt.pc[2];
    const double q0 = (double)pt.qc[0], q1 = (double)pt.qc[1], q2 = (double)pt.qc[2];
    const double m0 = (double)pt.gc[0], m1 = (double)pt.gc[1], m2 = (double)pt.gc[2];
    const double s = ((p0 * m0 + p1 * m1) + p2 * m2) - ((q0 * m0 + q1 * m1) + q2 * m2);
    const double dn = (d0 * m0 + d1 * m1) + d2 * m2;
    const double h0 = d0 - dn * m0, h1 = d1 - dn * m1, h2 = d2 - dn * m2;        // Md
    const double e0 = (p0 - s * m0) - q0, e1 = (p1 - s * m1) - q1, e2 = (p2 - s * m2) - q2;
    const double rG = wg * s;
    const double rI = wi * ((It + ((d0 * e0 + d1 * e1) + d2 * e2)) - Is);
    double G[6], H[6];
    G[0] = wg * (p1 * m2 - p2 * m1); G[1] = wg * (p2 * m0 - p0 * m2); G[2] = wg * (p0 * m1 - p1 * m0);
    G[3] = wg * m0; G[4] = wg * m1; G[5] = wg * m2;
    H[0] = wi * (p1 * h2 - p2 * h1); H[1] = wi * (p2 * h0 - p0 * h2); H[2] = wi * (p0 * h1 - p1 * h0);
    H[3] = wi * h0; H[4] = wi * h1; H[5] = wi * h2;
    int e = 2;
#pragma unroll
    for (int r = 0; r < 6; ++r)
#pragma unroll
      for (int c = r; c < 6; ++c) put(e++, G[r] * G[c] + H[r] * H[c]);
#pragma unroll
    for (int r = 0; r < 6; ++r) put(e++, G[r] * rG + H[r] * rI);
  }
  using Args = vcr_refine_colored_args;
  static int take(const Args* user, vcr_refine_args* lead, ColoredFit* fit) {
    Args mine;
    if (vcr_take_args(user, &mine, sizeof(Args))) return VCR_EINVAL;
    if (!mine.tgt_normals || !mine.tgt_gradient || !mine.tgt_intensity || !mine.src_intensity) return VCR_EINVAL;
    if (!(mine.lambda_geometric >= 0.f) || !(mine.lambda_geometric <= 1.f)) return VCR_EINVAL;     // (a NaN fails both)
    memcpy((void*)lead, (const void*)&mine, sizeof(*lead));
    lead->struct_bytes = (uint32_t)sizeof(*lead);
    fit->nrm = mine.tgt_normals; fit->grad = mine.tgt_gradient; fit->it = mine.tgt_intensity; fit->is = mine.src_intensity;
    fit->Ns = mine.Ns; fit->Nt = mine.Nt;
    const double lam = (double)mine.lambda_geometric;
    fit->wg = sqrt(lam); fit->wi = sqrt(1.0 - lam);
    return VCR_OK;
  }
};

__global__ __launch_bounds__(NN_BLOCK) void colored_merge_kernel(RfMerge<ColoredFit> p) { rf_merge_body(p); }

__global__ __launch_bounds__(NN_BLOCK) void colored_cloud_kernel(RfCloud p) {
  const int t = threadIdx.x, b = blockIdx.x;
  if (!p.st.live[b]) return;                               // (workgroup-uniform; written only by this workgroup's thread 0, behind the barriers)
  const double* tot = rf_total<ColoredFit::VALUES, ColoredFit::CHUNK>(p.part + (size_t)b * p.nblk * ColoredFit::VALUES, p.nblk);
  if (t != 0) return;                                      // one lane finishes
  double v[ColoredFit::VALUES];
#pragma unroll
  for (int e = 0; e < ColoredFit::VALUES; ++e) v[e] = tot[e];
  const bool finite = rf_sums_finite<ColoredFit::VALUES>(v);
  double x[6] = {0., 0., 0., 0., 0., 0.};
  // (a singular system stops the cloud; non-finite sums step to a NaN pose)
  const bool step = rf_evaluate(p, b, v, ColoredFit::MIN_INLIERS, true, [&](bool may) { return may && finite ? pl_solve(v + 2, v + 23, x) : may; });
  if (!step) return;
  double Ri[9], ti[3];
  pl_euler(x, Ri, ti);
  rf_step_pose(p, b, Ri, ti, finite);
}

}  // namespace

extern "C" int vcr_refine_colored_form(const vcr_refine_colored_args* ua, int cu_count, int* queries_per_lane, int* target_splits) {
  return rf_form<ColoredFit>(ua, cu_count, queries_per_lane, target_splits);
}

extern "C" size_t vcr_refine_colored_workspace_bytes(const vcr_refine_colored_args* ua, int cu_count) { return rf_workspace_bytes<ColoredFit>(ua, cu_count); }

extern "C" int vcr_refine_colored_f32(const vcr_refine_colored_args* ua, void* workspace, size_t workspace_bytes, vcr_stream_t stream) {
  return rf_run<ColoredFit>(ua, nullptr, workspace, workspace_bytes, stream, colored_merge_kernel, colored_cloud_kernel);
}

// The grid siblings (include/vcr_hip_gridnn.h's contract): the same loop behind another search
extern "C" int vcr_refine_colored_grid_form(const vcr_refine_colored_args* ua, const vcr_grid_nn_args* ug, int cu_count, int* cells_per_cloud, int* order,
                                            int* queries_per_workgroup) {
  return rf_grid_form<ColoredFit>(ua, ug, cu_count, cells_per_cloud, order, queries_per_workgroup);
}

extern "C" size_t vcr_refine_colored_grid_workspace_bytes(const vcr_refine_colored_args* ua, const vcr_grid_nn_args* ug, int cu_count) {
  return rf_grid_workspace_bytes<ColoredFit>(ua, ug, cu_count);
}

extern "C" int vcr_refine_colored_grid_f32(const vcr_refine_colored_args* ua, const vcr_grid_nn_args* ug, void* workspace, size_t workspace_bytes,
                                           vcr_stream_t stream) {
  if (!ug) return VCR_EINVAL;
  return rf_run<ColoredFit>(ua, ug, workspace, workspace_bytes, stream, colored_merge_kernel, colored_cloud_kernel);
}

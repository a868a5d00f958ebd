// The point-to-plane refinement with a robust weight per pair, and the information matrix of a registered pair
// (include/robust/vcr_hip_robust.h).  Both are fits of refine_round.h's loop and run through rf_run, by
// scan or by grid; this file holds what is theirs:
//   robust_merge_kernel<LOSS>   rf_merge_body with RobustPlaneFit<LOSS>: PlaneFit's twenty-nine fp64 values (refine_plane.hip)
//                               with Jw = w J in front of the products.  The loss is a template parameter, one instantiation
//                               each, chosen on the host: no lane evaluates a switch.
//   robust_cloud_kernel         plane_cloud_kernel's body on refine_solve6.h.  All weights zero: A = 0, singular, the cloud stops.
//   info_merge_kernel           rf_merge_body with InfoFit: sum of d2, count and nine sums of the neighbour's coordinates.
//   info_cloud_kernel           the partials in ascending order, then the evaluation; the call runs at max_iterations = 0, so
//                               rf_evaluate cannot step.
//   info_matrix_kernel          the same totals again, and lanes 0 ... 35 write the matrix from them.  A launch of its own
//                               behind rf_run: RfCloud carries the outputs every fit has and no pointer of a fit's own, and
//                               refine_round.h stays as it is (the four fits built on it keep their objects).
#include "refine_round.h"
#include "refine_solve6.h"
#include "../../include/robust/vcr_hip_robust.h"

// vcr_refine_plane_args' fields lead vcr_refine_robust_args, in its order and at its offsets, and vcr_refine_args' lead
// vcr_information_args: the shared plan reads them as one
static_assert(offsetof(vcr_refine_robust_args, variant) == offsetof(vcr_refine_plane_args, variant) &&
              offsetof(vcr_refine_robust_args, tgt_normals) == offsetof(vcr_refine_plane_args, tgt_normals) &&
              offsetof(vcr_refine_robust_args, loss) == sizeof(vcr_refine_plane_args) &&
              offsetof(vcr_refine_robust_args, k) == sizeof(vcr_refine_plane_args) + sizeof(int),
              "vcr_refine_robust_args = vcr_refine_plane_args + loss + k");
static_assert(offsetof(vcr_refine_plane_args, variant) == offsetof(vcr_refine_args, variant) &&
              offsetof(vcr_refine_plane_args, tgt_normals) == sizeof(vcr_refine_args), "vcr_refine_plane_args = vcr_refine_args + tgt_normals");
static_assert(offsetof(vcr_information_args, variant) == offsetof(vcr_refine_args, variant) &&
              offsetof(vcr_information_args, information) == sizeof(vcr_refine_args), "vcr_information_args = vcr_refine_args + information");

namespace {

// ------------------------------------------------------------------------------------------------------------ the robust fit

// The header's weights, in its expressions (r and k in fp64; k > 0 except for L2, which does not read it)
template <int LOSS>
__device__ __forceinline__ double robust_weight(double r, double k) {
  if constexpr (LOSS == VCR_LOSS_HUBER) {
    const double a = fabs(r);
    return a <= k ? 1. : k / a;
  } else if constexpr (LOSS == VCR_LOSS_CAUCHY) {
    const double u = r / k;
    return 1. / (1. + u * u);
  } else if constexpr (LOSS == VCR_LOSS_GM) {
    const double s = k + r * r;
    return k / (s * s);
  } else if constexpr (LOSS == VCR_LOSS_TUKEY) {
    const double a = fabs(r), u = r / k, v = 1. - u * u;
    return a <= k ? v * v : 0.;
  } else {
    return 1.;
  }
}

// what the five instantiations share: the layout of a partial, the normals, the host's copy of the arguments
struct RobustArgs {
  static constexpr int VALUES = 29;                        // sum_d2, count, A's upper triangle by rows [21], g[6]
  static constexpr int CHUNK = 64;                         // (15 KB of LDS)
  static constexpr int MIN_INLIERS = 6;                    // six unknowns
  const float* nrm;                                        // the target's normals, [B][3][Nt]
  double k;                                                // the loss' scale, widened
  using Args = vcr_refine_robust_args;
  // the checked copy: the loss it names is returned through *loss
  static int take(const Args* user, vcr_refine_args* lead, RobustArgs* fit, int* loss) {
    Args mine;
    if (vcr_take_args(user, &mine, sizeof(Args)) || !mine.tgt_normals) return VCR_EINVAL;
    if (mine.loss < VCR_LOSS_L2 || mine.loss > VCR_LOSS_TUKEY) return VCR_EINVAL;
    if (mine.loss != VCR_LOSS_L2 && !(mine.k > 0.f && mine.k < __builtin_huge_valf())) return VCR_EINVAL;   // (a NaN fails both)
    memcpy((void*)lead, (const void*)&mine, sizeof(*lead));
    lead->struct_bytes = (uint32_t)sizeof(*lead);
    fit->nrm = mine.tgt_normals;
    fit->k = mine.loss == VCR_LOSS_L2 ? 1. : (double)mine.k;
    if (loss) *loss = mine.loss;
    return VCR_OK;
  }
};

template <int LOSS>
struct RobustPlaneFit : RobustArgs {
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
    double J[6], Jw[6];                                    // products of two fp32 values: exact
    J[0] = p1 * m2 - p2 * m1; J[1] = p2 * m0 - p0 * m2; J[2] = p0 * m1 - p1 * m0;
    J[3] = m0; J[4] = m1; J[5] = m2;
    const double res = ((p0 * m0 + p1 * m1) + p2 * m2) - (((double)qc[0] * m0 + (double)qc[1] * m1) + (double)qc[2] * m2);
    const double w = robust_weight<LOSS>(res, k);           // (a lane that is no inlier: res = 0, w finite, J = 0)
#pragma unroll
    for (int r = 0; r < 6; ++r) Jw[r] = w * J[r];
    int e = 2;
#pragma unroll
    for (int r = 0; r < 6; ++r)
#pragma unroll
      for (int c = r; c < 6; ++c) put(e++, Jw[r] * J[c]);
#pragma unroll
    for (int r = 0; r < 6; ++r) put(e++, Jw[r] * res);
  }
  static int take(const Args* user, vcr_refine_args* lead, RobustPlaneFit* fit) { return RobustArgs::take(user, lead, fit, nullptr); }
};

template <int LOSS>
__global__ __launch_bounds__(NN_BLOCK) void robust_merge_kernel(RfMerge<RobustPlaneFit<LOSS>> p) { rf_merge_body(p); }

__global__ __launch_bounds__(NN_BLOCK) void robust_cloud_kernel(RfCloud p) {
  const int t = threadIdx.x, b = blockIdx.x;
  if (!p.st.live[b]) return;                               // (workgroup-uniform; written only by this workgroup's thread 0, behind the barriers)
  const double* tot = rf_total<RobustArgs::VALUES, RobustArgs::CHUNK>(p.part + (size_t)b * p.nblk * RobustArgs::VALUES, p.nblk);
  if (t != 0) return;                                      // one lane finishes
  double v[RobustArgs::VALUES];
#pragma unroll
  for (int e = 0; e < RobustArgs::VALUES; ++e) v[e] = tot[e];
  const bool finite = rf_sums_finite<RobustArgs::VALUES>(v);
  double x[6] = {0., 0., 0., 0., 0., 0.};
  // (a singular system -- every weight zero is one -- stops the cloud; non-finite sums step to a NaN pose)
  const bool step = rf_evaluate(p, b, v, RobustArgs::MIN_INLIERS, true, [&](bool may) { return may && finite ? pl_solve(v + 2, v + 23, x) : may; });
  if (!step) return;
  double Ri[9], ti[3];
  pl_euler(x, Ri, ti);
  rf_step_pose(p, b, Ri, ti, finite);
}

// the loss of a call that take() accepts, or -1
int robust_loss(const vcr_refine_robust_args* ua) {
  vcr_refine_args a;
  RobustArgs fit;
  int loss = -1;
  return RobustArgs::take(ua, &a, &fit, &loss) ? -1 : loss;
}

template <int LOSS>
int robust_run(const vcr_refine_robust_args* ua, const vcr_grid_nn_args* ug, void* workspace, size_t workspace_bytes, vcr_stream_t stream) {
  return rf_run<RobustPlaneFit<LOSS>>(ua, ug, workspace, workspace_bytes, stream, robust_merge_kernel<LOSS>, robust_cloud_kernel);
}

int robust_dispatch(const vcr_refine_robust_args* ua, const vcr_grid_nn_args* ug, void* workspace, size_t workspace_bytes, vcr_stream_t stream) {
  switch (robust_loss(ua)) {
    case VCR_LOSS_L2: return robust_run<VCR_LOSS_L2>(ua, ug, workspace, workspace_bytes, stream);
    case VCR_LOSS_HUBER: return robust_run<VCR_LOSS_HUBER>(ua, ug, workspace, workspace_bytes, stream);
    case VCR_LOSS_CAUCHY: return robust_run<VCR_LOSS_CAUCHY>(ua, ug, workspace, workspace_bytes, stream);
    case VCR_LOSS_GM: return robust_run<VCR_LOSS_GM>(ua, ug, workspace, workspace_bytes, stream);
    case VCR_LOSS_TUKEY: return robust_run<VCR_LOSS_TUKEY>(ua, ug, workspace, workspace_bytes, stream);
  }
  return VCR_EINVAL;
}

using RobustAny = RobustPlaneFit<VCR_LOSS_L2>;             // the plan and the workspace do not depend on the loss

// ----------------------------------------------------------------------------------------------------- the information matrix

struct InfoFit {
  static constexpr int VALUES = 11;                        // sum_d2, count, Sx Sy Sz, Sxx Syy Szz, Sxy Sxz Syz
  static constexpr int CHUNK = 64;                         // (6 KB of LDS)
  static constexpr int MIN_INLIERS = 0;                    // (never asked: the call does not step)
  double* information;                                     // [B][6][6]
  __device__ float gather(int, int, int, int) const { return 0.f; }   // nothing gathered: the neighbour is all
  __device__ float source(int, int, int, int) const { return 0.f; }
  template <class Put>
  __device__ void sums(const RfPoint& pt, Put& put) const {
    const double x = (double)pt.qc[0], y = (double)pt.qc[1], z = (double)pt.qc[2];   // (zeros where the lane is no inlier)
    put(2, x); put(3, y); put(4, z);
    put(5, x * x); put(6, y * y); put(7, z * z);           // products of two fp32 values: exact
    put(8, x * y); put(9, x * z); put(10, y * z);
  }
  using Args = vcr_information_args;
  static int take(const Args* user, vcr_refine_args* lead, InfoFit* fit) {
    Args mine;
    if (vcr_take_args(user, &mine, sizeof(Args)) || !mine.information || mine.max_iterations != 0) return VCR_EINVAL;
    memcpy((void*)lead, (const void*)&mine, sizeof(*lead));
    lead->struct_bytes = (uint32_t)sizeof(*lead);
    fit->information = mine.information;
    return VCR_OK;
  }
};

__global__ __launch_bounds__(NN_BLOCK) void info_merge_kernel(RfMerge<InfoFit> p) { rf_merge_body(p); }

__global__ __launch_bounds__(NN_BLOCK) void info_cloud_kernel(RfCloud p) {
  const int t = threadIdx.x, b = blockIdx.x;
  if (!p.st.live[b]) return;                               // (workgroup-uniform; round 0: every cloud is live)
  const double* tot = rf_total<InfoFit::VALUES, InfoFit::CHUNK>(p.part + (size_t)b * p.nblk * InfoFit::VALUES, p.nblk);
  if (t != 0) return;
  const double v[2] = {tot[0], tot[1]};
  rf_evaluate(p, b, v, InfoFit::MIN_INLIERS, true, [](bool) { return false; });   // a fit that never steps
}

struct InfoMatrix {
  const double* part; int nblk;
  double* information;
};

// One workgroup per cloud: info_cloud_kernel's totals again (the same partials in the same order: the same bits), then a
// lane per element of the matrix
__global__ __launch_bounds__(NN_BLOCK) void info_matrix_kernel(InfoMatrix p) {
  const int t = threadIdx.x, b = blockIdx.x;
  const double* tot = rf_total<InfoFit::VALUES, InfoFit::CHUNK>(p.part + (size_t)b * p.nblk * InfoFit::VALUES, p.nblk);
  if (t >= 36) return;
  const int r = t / 6, c = t % 6;
  auto of3 = [](int i, double a0, double a1, double a2) { return i == 0 ? a0 : i == 1 ? a1 : a2; };   // (selects: no indexed array)
  double m;
  if (r >= 3 && c >= 3) {
    m = r == c ? tot[1] : 0.;                              // n
  } else if (r < 3 && c < 3) {
    if (r == c) m = of3(r, tot[6] + tot[7], tot[5] + tot[7], tot[5] + tot[6]);
    else m = -of3(r + c - 1, tot[8], tot[9], tot[10]);     // (0,1) Sxy, (0,2) Sxz, (1,2) Syz
  } else {
    // the top right block is [S]x = (0 -Sz Sy; Sz 0 -Sx; -Sy Sx 0), the bottom left its transpose
    const int i = r < 3 ? r : c, j = r < 3 ? c - 3 : r - 3;   // (element (i, j) of the top right block)
    if (i == j) m = 0.;
    else {
      const double s = of3(3 - i - j, tot[2], tot[3], tot[4]);
      m = (j - i + 3) % 3 == 1 ? -s : s;
    }
  }
  p.information[(size_t)b * 36 + t] = m;                   // t in [0, 36), b in [0, B)
}

// rf_run's round, then the matrix from the partials it left in the workspace (the plan is rf_run's own: the same arguments)
int info_run(const vcr_information_args* ua, const vcr_grid_nn_args* ug, void* workspace, size_t workspace_bytes, vcr_stream_t stream) {
  int e = rf_run<InfoFit>(ua, ug, workspace, workspace_bytes, stream, info_merge_kernel, info_cloud_kernel);
  if (e) return e;
  vcr_refine_args a;
  InfoFit fit;
  RfPlan p;
  if (InfoFit::take(ua, &a, &fit)) return VCR_EINVAL;
  vcr_stream_scope scope_(stream);
  if ((e = rf_plan(a, ug, ug ? 1 : vcr_cu_count(), InfoFit::VALUES, &p))) return e;
  const InfoMatrix im{reinterpret_cast<const double*>(reinterpret_cast<unsigned char*>(workspace) + p.part_off), p.nn.nblk, fit.information};
  hipLaunchKernelGGL(info_matrix_kernel, dim3((unsigned)a.B), dim3(NN_BLOCK), 0, (hipStream_t)stream, im);
  return VCR_LAUNCH_RC();
}

}  // namespace

extern "C" int vcr_refine_robust_form(const vcr_refine_robust_args* ua, int cu_count, int* queries_per_lane, int* target_splits) {
  return rf_form<RobustAny>(ua, cu_count, queries_per_lane, target_splits);
}

extern "C" size_t vcr_refine_robust_workspace_bytes(const vcr_refine_robust_args* ua, int cu_count) { return rf_workspace_bytes<RobustAny>(ua, cu_count); }

extern "C" int vcr_refine_robust_f32(const vcr_refine_robust_args* ua, void* workspace, size_t workspace_bytes, vcr_stream_t stream) {
  return robust_dispatch(ua, nullptr, workspace, workspace_bytes, stream);
}

// The grid siblings (include/vcr_hip_gridnn.h): the same loop behind another search
extern "C" int vcr_refine_robust_grid_form(const vcr_refine_robust_args* ua, const vcr_grid_nn_args* ug, int cu_count, int* cells_per_cloud, int* order,
                                           int* queries_per_workgroup) {
  return rf_grid_form<RobustAny>(ua, ug, cu_count, cells_per_cloud, order, queries_per_workgroup);
}

extern "C" size_t vcr_refine_robust_grid_workspace_bytes(const vcr_refine_robust_args* ua, const vcr_grid_nn_args* ug, int cu_count) {
  return rf_grid_workspace_bytes<RobustAny>(ua, ug, cu_count);
}

extern "C" int vcr_refine_robust_grid_f32(const vcr_refine_robust_args* ua, const vcr_grid_nn_args* ug, void* workspace, size_t workspace_bytes,
                                          vcr_stream_t stream) {
  if (!ug) return VCR_EINVAL;
  return robust_dispatch(ua, ug, workspace, workspace_bytes, stream);
}

extern "C" int vcr_information_form(const vcr_information_args* ua, int cu_count, int* queries_per_lane, int* target_splits) {
  return rf_form<InfoFit>(ua, cu_count, queries_per_lane, target_splits);
}

extern "C" size_t vcr_information_workspace_bytes(const vcr_information_args* ua, int cu_count) { return rf_workspace_bytes<InfoFit>(ua, cu_count); }

extern "C" int vcr_information_f32(const vcr_information_args* ua, void* workspace, size_t workspace_bytes, vcr_stream_t stream) {
  return info_run(ua, nullptr, workspace, workspace_bytes, stream);
}

extern "C" int vcr_information_grid_form(const vcr_information_args* ua, const vcr_grid_nn_args* ug, int cu_count, int* cells_per_cloud, int* order,
                                         int* queries_per_workgroup) {
  return rf_grid_form<InfoFit>(ua, ug, cu_count, cells_per_cloud, order, queries_per_workgroup);
}

extern "C" size_t vcr_information_grid_workspace_bytes(const vcr_information_args* ua, const vcr_grid_nn_args* ug, int cu_count) {
  return rf_grid_workspace_bytes<InfoFit>(ua, ug, cu_count);
}

extern "C" int vcr_information_grid_f32(const vcr_information_args* ua, const vcr_grid_nn_args* ug, void* workspace, size_t workspace_bytes,
                                        vcr_stream_t stream) {
  if (!ug) return VCR_EINVAL;
  return info_run(ua, ug, workspace, workspace_bytes, stream);
}

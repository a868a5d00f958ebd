// What the two refinements on the full clouds share besides the scan (nn_scan.h): the per-cloud state in the workspace, the
// kernel that initialises it, the store of the fp32 pose and its inverse, and the plan -- the argument checks, the form of the
// search and the workspace layout.  refine.hip (vcr_refine_f32, point to point) and refine_plane.hip (vcr_refine_plane_f32,
// point to plane) differ in the sums a round accumulates and in the solve behind them.
#pragma once
#include "nn_scan.h"
#include "../../include/vcr_hip_refine.h"

namespace {

struct RfState {                                           // per cloud, in the workspace
  double* pose;                                            // [B][12]: R row-major, t
  float* prev;                                             // [B][2]: the last evaluation's fitness, rmse
  int* live; int* iters;                                   // [B] each
};

// (R_ba, t_ba) of the fp32 pose: pose_step_kernel's expression (forward.hip)
__device__ void rf_store_pose(const float* r, const float* t, int b, float* R_out, float* t_out, float* R_ba, float* t_ba) {
  for (int i = 0; i < 9; ++i) R_out[(size_t)b * 9 + i] = r[i];
  for (int i = 0; i < 3; ++i) t_out[(size_t)b * 3 + i] = t[i];
  for (int i = 0; i < 3; ++i) {
    if (R_ba) for (int j = 0; j < 3; ++j) R_ba[(size_t)b * 9 + i * 3 + j] = r[j * 3 + i];
    if (t_ba) t_ba[(size_t)b * 3 + i] = -fmaf(r[6 + i], t[2], fmaf(r[3 + i], t[1], r[i] * t[0]));
  }
}

struct RfInit {
  const float* R; const float* t; int B;
  RfState st;
  float* R_out; float* t_out; float* R_ba; float* t_ba;
};

__global__ __launch_bounds__(NN_BLOCK) void refine_init_kernel(RfInit p) {
  const int b = blockIdx.x * NN_BLOCK + threadIdx.x;
  if (b >= p.B) return;
  float r[9] = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f}, t[3] = {0.f, 0.f, 0.f};
  if (p.R) {
    for (int i = 0; i < 9; ++i) r[i] = p.R[(size_t)b * 9 + i];
    for (int i = 0; i < 3; ++i) t[i] = p.t[(size_t)b * 3 + i];
  }
  for (int i = 0; i < 9; ++i) p.st.pose[(size_t)b * 12 + i] = (double)r[i];
  for (int i = 0; i < 3; ++i) p.st.pose[(size_t)b * 12 + 9 + i] = (double)t[i];
  rf_store_pose(r, t, b, p.R_out, p.t_out, p.R_ba, p.t_ba);
  p.st.live[b] = 1; p.st.iters[b] = 0;                     // (prev is written by round 0 before round 1 reads it)
}

// nn_plan on the search this call runs (under R_out / t_out), the arguments of its own checked first, and the workspace:
// the scan's candidates | the partials | the per-cloud state
struct RfPlan {
  NnPlan nn;
  size_t part_off, pose_off, prev_off, live_off, iters_off, bytes;
};

}  // namespace

// values: fp64 partials per 256 source points
static int rf_plan(const vcr_refine_args& a, int cu, int values, RfPlan* p) {
  *p = RfPlan{};
  if (!a.R_out || !a.t_out || (a.R == nullptr) != (a.t == nullptr) || a.max_iterations < 0) return VCR_EINVAL;
  const float inf = __builtin_huge_valf();
  if (!(a.rel_fitness >= 0.f) || a.rel_fitness == inf || !(a.rel_rmse >= 0.f) || a.rel_rmse == inf) return VCR_EINVAL;
  vcr_nn_score_args s{};
  s.struct_bytes = (uint32_t)sizeof(s);
  s.src = a.src; s.tgt = a.tgt; s.B = a.B; s.Ns = a.Ns; s.Nt = a.Nt;
  s.R = a.R_out; s.t = a.t_out; s.max_dist = a.max_dist;
  s.nn_idx = a.nn_idx; s.nn_d2 = a.nn_d2; s.inliers = a.inliers; s.sum_d2 = a.sum_d2; s.fitness = a.fitness; s.rmse = a.rmse;
  s.variant = a.variant;
  const int e = nn_plan(s, cu, &p->nn);
  if (e) return e;
  if (a.max_iterations > VCR_REFINE_MAX_ITERATIONS) return VCR_EUNSUPPORTED;
  const size_t B = (size_t)a.B;
  p->part_off = 2 * p->nn.part_bytes;
  p->pose_off = p->part_off + nn_up(B * p->nn.nblk * values * sizeof(double));
  p->prev_off = p->pose_off + nn_up(B * 12 * sizeof(double));
  p->live_off = p->prev_off + nn_up(B * 2 * sizeof(float));
  p->iters_off = p->live_off + nn_up(B * sizeof(int));
  p->bytes = p->iters_off + nn_up(B * sizeof(int));
  return VCR_OK;
}

// The round of the refinements on the full clouds, written once: refine.hip (vcr_refine_f32, point to point),
// refine_plane.hip (vcr_refine_plane_f32, point to plane), refine_gicp.hip (vcr_refine_gicp_f32, plane to plane) and
// refine_colored.hip (vcr_refine_colored_f32, colour and shape) run the same loop and differ in the FIT -- the sums a round accumulates over its inliers and the solve behind them.  Here: the per-cloud state in the workspace and the kernel that
// initialises it, the plan (argument checks, form of the search, workspace layout), the body of the merge kernel, the parts of
// the per-cloud kernel that do not solve (the sum of the partials, the evaluation and the stop test, the composed pose), and
// the host driver behind the three entry points of each header.
//
// A fit is a struct that travels to the merge kernel as RfMerge's last member and supplies
//   VALUES, CHUNK, MIN_INLIERS   fp64 values per partial (sum_d2 and the count lead), partials the per-cloud kernel stages in
//                                LDS at a time, inliers a step needs
//   gather()                     what it reads at the neighbour's index besides the neighbour, a coordinate at a time
//   source()                     what it reads at the SOURCE point's own index n besides the point, likewise
//   sums()                       values 2 ... VALUES - 1 of one source point -- from an RfPoint: the moved point, the neighbour,
//                                what gather() and source() read, the fp32 pose the merge holds, whether the lane is an
//                                inlier, and the indices (cloud, source point, neighbour) by which a fit that reads more
//                                than two triples fetches the rest -- handed to `put` one at a time.  A lane that is no inlier must contribute exact zeros:
//                                its four triples are zero, which is enough for a fit whose every term is a product of them.
//   Args, take()                 (host) the public argument struct, and the copy of it the call works on
// The kernels themselves stay in the fits' .hip files under their own names, as wrappers of the bodies below.
#pragma once
#include "nn_scan.h"
#include "grid_nn.h"
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

// ---------------------------------------------------------------------------------------------------------------- the merge

struct RfPoint {                                           // one lane of the merge, as a fit's sums() sees it
  const float* pc; const float* qc; const float* gc; const float* sc;   // [3] each: moved point, neighbour, gather()'s, source()'s
  const float* R;                                          // [9], the cloud's fp32 pose the scan ran under (read by inliers only)
  bool in;
  int b, n, bi;                                            // the cloud, the source point, its neighbour (bi in [0, Nt) where `in`): a fit
};                                                         // that reads more than gather() and source() carry fetches it by these

template <class Fit>
struct RfMerge {
  const float* part_d2; const int* part_idx;
  const float* src; const float* tgt; const float* R; const float* t;   // the fp32 pose the scan ran under
  int B, Ns, Nt, S, nblk;                                  // nblk = ceil(Ns / 256)
  float max_d2;
  int* nn_idx; float* nn_d2;
  double* part;                                            // [B][nblk][Fit::VALUES]
  const int* live;
  Fit fit;
};

// One lane per source point: folds the S candidates as nn_merge_kernel does (nn_fold), writes nn_idx / nn_d2, recomputes the
// moved point (the scan's expression), gathers the neighbour and reduces the workgroup's 256 points to Fit::VALUES fp64 values
// in nn_merge_kernel's order: wave butterfly 32 ... 1, the four waves ascending.
template <class Fit>
__device__ __forceinline__ void rf_merge_body(const RfMerge<Fit>& p) {
  __shared__ double red[NN_BLOCK / 64][Fit::VALUES];
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
  float pc[3] = {0.f, 0.f, 0.f}, qc[3] = {0.f, 0.f, 0.f}, gc[3] = {0.f, 0.f, 0.f}, sc[3] = {0.f, 0.f, 0.f};
  const float* r = p.R + (size_t)b * 9;
  if (in) {                                                // bi is in [0, Nt): a target index the scan wrote; n is in [0, Ns)
    const float* sx = p.src + (size_t)b * 3 * Ns;
    const float* tx = p.tgt + (size_t)b * 3 * Nt;
    const float* tr = p.t + (size_t)b * 3;
    const float x = sx[n], y = sx[Ns + n], z = sx[2 * (size_t)Ns + n];
    for (int c = 0; c < 3; ++c) {                          // the scan's expression, bit for bit
      pc[c] = fmaf(r[3 * c + 2], z, fmaf(r[3 * c + 1], y, r[3 * c] * x)) + tr[c];
      qc[c] = tx[(size_t)c * Nt + bi];
      gc[c] = p.fit.gather(b, Nt, c, bi);
      sc[c] = p.fit.source(b, Ns, c, n);
    }
  }
  auto put = [&](int e, double v) {                        // one value across the wave, nn_merge_kernel's butterfly
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    if ((t & 63) == 0) red[t >> 6][e] = v;
  };
  put(0, in ? (double)best : 0.);
  put(1, in ? 1. : 0.);
  p.fit.sums(RfPoint{pc, qc, gc, sc, r, in, b, n, bi}, put);
  __syncthreads();
  if (t < Fit::VALUES) {
    double s = red[0][t];
    for (int w = 1; w < NN_BLOCK / 64; ++w) s += red[w][t];
    p.part[((size_t)b * p.nblk + blk) * Fit::VALUES + t] = s;
  }
}

// ---------------------------------------------------------------------------------------------------- the per-cloud kernel

struct RfCloud {
  const double* part; int Ns, nblk;
  int round, max_iterations; float rel_fitness, rel_rmse;
  RfState st;
  float* R_out; float* t_out; float* fitness; float* rmse; float* R_ba; float* t_ba;
  int* inliers; double* sum_d2; int* iterations; int* converged;
};

// A cloud's nblk partials (part: its first) summed in ascending order, staged through LDS CHUNK at a time: the totals, in
// LDS, behind a barrier (every thread of the workgroup calls this)
template <int VALUES, int CHUNK>
__device__ __forceinline__ const double* rf_total(const double* part, int nblk) {
  __shared__ double stage[CHUNK * VALUES];
  __shared__ double tot[VALUES];
  const int t = threadIdx.x;
  double acc = 0.;
  for (int c0 = 0; c0 < nblk; c0 += CHUNK) {               // (workgroup-uniform)
    const int m = nblk - c0 < CHUNK ? nblk - c0 : CHUNK;
    __syncthreads();
    for (int i = t; i < m * VALUES; i += NN_BLOCK) stage[i] = part[(size_t)c0 * VALUES + i];
    __syncthreads();
    if (t < VALUES)
      for (int i = 0; i < m; ++i) acc += stage[i * VALUES + t];         // ascending, one lane per value: the order is Ns's alone
  }
  if (t < VALUES) tot[t] = acc;
  __syncthreads();
  return tot;
}

// The round's evaluation (nn_final_kernel's expressions) from the totals v, the stop test, and the cloud's outputs and state.
// veto(may_step): the fit's solve may refuse the step before the state is written.  Every lane that finishes calls this, one of
// them as the writer: prev[] and iters[b] are read by all of them and written by that lane alone -- one wave, program order.
// Returns whether the cloud steps.
template <class Veto>
__device__ __forceinline__ bool rf_evaluate(const RfCloud& p, int b, const double* v, int min_inliers, bool writer, Veto veto) {
  const double sum = v[0];
  const int cnt = (int)v[1];
  const float fitness = (float)cnt / (float)p.Ns;
  const float rmse = cnt > 0 ? (float)sqrt(sum / (double)cnt) : 0.f;
  bool conv = false;
  if (p.round > 0)
    conv = fabsf(fitness - p.st.prev[2 * b]) < p.rel_fitness && fabsf(rmse - p.st.prev[2 * b + 1]) < p.rel_rmse;
  const bool step = veto(!conv && p.round < p.max_iterations && cnt >= min_inliers);
  const int iters = p.st.iters[b] + (step ? 1 : 0);
  if (writer) {
    p.fitness[b] = fitness; p.rmse[b] = rmse;
    if (p.inliers) p.inliers[b] = cnt;
    if (p.sum_d2) p.sum_d2[b] = sum;
    if (p.iterations) p.iterations[b] = iters;
    if (p.converged) p.converged[b] = conv ? 1 : 0;
    p.st.prev[2 * b] = fitness; p.st.prev[2 * b + 1] = rmse;
    p.st.iters[b] = iters;
    p.st.live[b] = step ? 1 : 0;
  }
  return step;
}

// as rigid_svd_kernel: stated, not left to the solve
template <int VALUES>
__device__ __forceinline__ bool rf_sums_finite(const double* v) {
  bool finite = true;
#pragma unroll
  for (int e = 2; e < VALUES; ++e) finite = finite && __builtin_isfinite(v[e]);
  return finite;
}

// The step (Ri, ti) -- NaN where the sums were not finite -- composed onto cloud b's fp64 pose; its fp32 rounding and inverse
// to the outputs (one lane)
__device__ __forceinline__ void rf_step_pose(const RfCloud& p, int b, double* Ri, double* ti, bool finite) {
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

// nn_plan on the search this call runs (under R_out / t_out), the arguments of its own checked first, and the workspace:
// the scan's candidates | the partials | the per-cloud state | with the grid search (section 4.20), the grids
struct RfPlan {
  NnPlan nn;
  size_t part_off, pose_off, prev_off, live_off, iters_off, grid_off, bytes;
  bool on_grid;
  GridNnPlan grid;
};

}  // namespace

// ------------------------------------------------------------------------------------------------------------------ the host

// values: fp64 partials per 256 source points
// ug: NULL = the scan.  Otherwise the grid search of include/vcr_hip_gridnn.h: the scan's variant must be 0, and the scan's plan
// is taken at one target split -- the merge folds the grid search's one candidate a point
static int rf_plan(const vcr_refine_args& a, const vcr_grid_nn_args* ug, int cu, int values, RfPlan* p) {
  *p = RfPlan{};
  if (ug && a.variant != 0) return VCR_EINVAL;
  if (!a.R_out || !a.t_out || (a.R == nullptr) != (a.t == nullptr) || a.max_iterations < 0) return VCR_EINVAL;
  const float inf = __builtin_huge_valf();
  if (!(a.rel_fitness >= 0.f) || a.rel_fitness == inf || !(a.rel_rmse >= 0.f) || a.rel_rmse == inf) return VCR_EINVAL;
  vcr_nn_score_args s{};
  s.struct_bytes = (uint32_t)sizeof(s);
  s.src = a.src; s.tgt = a.tgt; s.B = a.B; s.Ns = a.Ns; s.Nt = a.Nt;
  s.R = a.R_out; s.t = a.t_out; s.max_dist = a.max_dist;
  s.nn_idx = a.nn_idx; s.nn_d2 = a.nn_d2; s.inliers = a.inliers; s.sum_d2 = a.sum_d2; s.fitness = a.fitness; s.rmse = a.rmse;
  s.variant = ug ? VCR_NN_SCORE_VARIANT(1, 1) : a.variant;
  int e = nn_plan(s, cu, &p->nn);
  if (e) return e;
  if (a.max_iterations > VCR_REFINE_MAX_ITERATIONS) return VCR_EUNSUPPORTED;
  const size_t B = (size_t)a.B;
  p->part_off = 2 * p->nn.part_bytes;
  p->pose_off = p->part_off + ws_up(B * p->nn.nblk * values * sizeof(double));
  p->prev_off = p->pose_off + ws_up(B * 12 * sizeof(double));
  p->live_off = p->prev_off + ws_up(B * 2 * sizeof(float));
  p->iters_off = p->live_off + ws_up(B * sizeof(int));
  p->grid_off = p->bytes = p->iters_off + ws_up(B * sizeof(int));
  if (ug) {
    if ((e = gridnn_plan(ug, GRIDNN_REFINE, a.max_iterations + 1, a.B, a.Ns, a.Nt, &p->grid))) return e;
    p->on_grid = true;
    p->bytes += p->grid.bytes;
  }
  return VCR_OK;
}

// The three entry points of a fit.  Fit::take(user, &a, &fit) copies what the call works on out of the public struct -- the
// vcr_refine_args that lead it, and the fit's own pointers -- or refuses it.
template <class Fit>
static int rf_form(const typename Fit::Args* ua, int cu_count, int* queries_per_lane, int* target_splits) {
  vcr_refine_args a;
  Fit fit;
  RfPlan p;
  if (Fit::take(ua, &a, &fit) || cu_count < 0) return VCR_EINVAL;
  const int e = rf_plan(a, nullptr, cu_count ? cu_count : vcr_cu_count(), Fit::VALUES, &p);
  if (e) return e;
  if (queries_per_lane) *queries_per_lane = p.nn.Q;
  if (target_splits) *target_splits = p.nn.scan.S;
  return VCR_OK;
}

// The grid sibling's: no device is asked (neither plan depends on one)
template <class Fit>
static int rf_grid_form(const typename Fit::Args* ua, const vcr_grid_nn_args* ug, int cu_count, int* cells_per_cloud, int* order,
                        int* queries_per_workgroup) {
  vcr_refine_args a;
  Fit fit;
  RfPlan p;
  if (Fit::take(ua, &a, &fit) || !ug || cu_count < 0) return VCR_EINVAL;
  const int e = rf_plan(a, ug, 1, Fit::VALUES, &p);
  if (e) return e;
  if (cells_per_cloud) *cells_per_cloud = p.grid.cells;
  if (order) *order = p.grid.order;
  if (queries_per_workgroup) *queries_per_workgroup = VCR_GRID_QUERIES;
  return VCR_OK;
}

template <class Fit>
static size_t rf_grid_workspace_bytes(const typename Fit::Args* ua, const vcr_grid_nn_args* ug, int cu_count) {
  vcr_refine_args a;
  Fit fit;
  RfPlan p;
  if (Fit::take(ua, &a, &fit) || !ug || cu_count < 0) return 0;
  return rf_plan(a, ug, 1, Fit::VALUES, &p) ? 0 : p.bytes;
}

template <class Fit>
static size_t rf_workspace_bytes(const typename Fit::Args* ua, int cu_count) {
  vcr_refine_args a;
  Fit fit;
  RfPlan p;
  if (Fit::take(ua, &a, &fit) || cu_count < 0) return 0;
  return rf_plan(a, nullptr, cu_count ? cu_count : vcr_cu_count(), Fit::VALUES, &p) ? 0 : p.bytes;
}

// One launch up front and three per round, max_iterations + 1 rounds, all enqueued at once (no host synchronisation).
// search: the search that fills part_d2 / part_idx each round -- NULL = the scan (nn_scan_launch, in the form its plan says);
// otherwise the grid search under these arguments (gridnn_search), its grids built once in front of round 0
template <class Fit>
static int rf_run(const typename Fit::Args* ua, const vcr_grid_nn_args* search, void* workspace, size_t workspace_bytes,
                  vcr_stream_t stream, void (*merge_kernel)(RfMerge<Fit>), void (*cloud_kernel)(RfCloud)) {
  vcr_refine_args a;
  Fit fit;
  if (Fit::take(ua, &a, &fit)) return VCR_EINVAL;
  // the argument checks need no device: only a call that passes them asks for the CU count (the grid's plan needs none)
  RfPlan p;
  int e = rf_plan(a, search, 1, Fit::VALUES, &p);
  if (e) return e;
  if (!workspace || (((uintptr_t)workspace) & 15)) return VCR_EINVAL;
  vcr_stream_scope scope_(stream);
  if (!search) e = rf_plan(a, nullptr, vcr_cu_count(), Fit::VALUES, &p);
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
  if (p.on_grid && (e = gridnn_build(p.grid, a.src, a.tgt, w + p.grid_off, s))) return e;
  const RfMerge<Fit> mg{reinterpret_cast<const float*>(w), reinterpret_cast<const int*>(w + nn.part_bytes), a.src, a.tgt, a.R_out, a.t_out,
                        a.B, a.Ns, a.Nt, nn.scan.S, nn.nblk, a.max_dist * a.max_dist, a.nn_idx, a.nn_d2, part, st.live, fit};
  for (int round = 0; round <= a.max_iterations; ++round) {
    e = p.on_grid ? gridnn_search(p.grid, a.src, a.R_out, a.t_out, a.max_dist * a.max_dist, w + p.grid_off,
                                  reinterpret_cast<float*>(w), reinterpret_cast<int*>(w + nn.part_bytes), st.live, s)
                  : nn_scan_launch(nn, workspace, st.live, s);
    if (e) return e;
    hipLaunchKernelGGL(merge_kernel, dim3(nn.merge_grid), dim3(NN_BLOCK), 0, s, mg);
    if ((e = VCR_LAUNCH_RC())) return e;
    const RfCloud cl{part, a.Ns, nn.nblk, round, a.max_iterations, a.rel_fitness, a.rel_rmse, st,
                     a.R_out, a.t_out, a.fitness, a.rmse, a.R_ba, a.t_ba, a.inliers, a.sum_d2, a.iterations, a.converged};
    hipLaunchKernelGGL(cloud_kernel, dim3((unsigned)a.B), dim3(NN_BLOCK), 0, s, cl);
    if ((e = VCR_LAUNCH_RC())) return e;
  }
  return VCR_OK;
}

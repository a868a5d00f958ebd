// Scoring a registration on the full clouds (include/vcr_hip_score.h): every source point's nearest target
// point by brute force, then per cloud the inlier count, the inliers' fp64 sum of squared distances, fitness and RMSE.
//
// Unlike icp_nn_kernel (icp.hip) the distance is the DIFFERENCE form, every fmaf spelled out (build.py: -ffp-contract=off):
//   dx = p_x - q_x ...;  d2 = fmaf(dz, dz, fmaf(dy, dy, dx * dx));  best only on d2 < best, from (+inf, -1), targets ascending
// so a residual of 1e-3 keeps its seven digits (the expansion 2 s.d - |s|^2 - |d|^2 leaves it one), a tie goes to the lowest
// target index, and a NaN / +inf d2 never wins.  The comparison is the whole non-finite rule.
//
// Three launches (nn_plan fixes the first one's form; vcr_nn_score_args.variant forces it).  The scan and the plan live in
// nn_scan.h, which refine.hip (the ICP on the full clouds) includes too:
//   nn_scan_kernel<Q>   256 lanes x Q source points per lane (point = base + q * 256 + lane, moved by the pose once, in
//                       registers) against one of the S segments of the target: tiles of NN_TILE points staged from the
//                       channels-first planes into three LDS planes (coalesced dword loads), read back four points a plane
//                       with one address for all lanes (a broadcast ds_read_b128) and used by the lane's Q queries.  The
//                       (d2, index) of every (segment, source point) goes to the workspace.
//   nn_merge_kernel     one lane per source point: folds the S candidates in ascending segment order with the same strict <
//                       (segments ascend in target index: the lowest-index rule survives the split), writes nn_idx / nn_d2,
//                       and reduces its 256 points to one (fp64 sum, count) partial in a fixed order.
//   nn_final_kernel     one workgroup per cloud: the partials in ascending order, then inliers / sum_d2 / fitness / rmse.
// The geometry of the last two depends on Ns alone, so every form of the first returns the same bits.  No atomics.  The scan's
// frame (seg_scan.h) and the two reductions (wg_scan.h) are the ones every scan of the library uses.
#include "nn_scan.h"
#include "grid_nn.h"

namespace {

struct NnMerge {
  const float* part_d2; const int* part_idx;
  int B, Ns, S, nblk;                                      // nblk = ceil(Ns / 256)
  float max_d2;
  int* nn_idx; float* nn_d2; NnPartial* partial;           // partial [B][nblk]
};

__global__ __launch_bounds__(NN_BLOCK) void nn_merge_kernel(NnMerge p) {
  __shared__ double wsum[NN_BLOCK / 64];
  __shared__ int wcnt[NN_BLOCK / 64];
  const int t = threadIdx.x;
  const int b = (int)(blockIdx.x / (unsigned)p.nblk), blk = (int)(blockIdx.x % (unsigned)p.nblk);
  const int n = blk * NN_BLOCK + t;
  float best = __builtin_huge_valf();
  int bi = -1;
  if (n < p.Ns) {
    nn_fold(p.part_d2, p.part_idx, p.B, p.Ns, p.S, b, n, &best, &bi);
    const size_t o = (size_t)b * p.Ns + n;
    if (p.nn_idx) p.nn_idx[o] = bi;
    if (p.nn_d2) p.nn_d2[o] = best;
  }
  const bool in = n < p.Ns && bi >= 0 && best <= p.max_d2;
  double sum = 0.;
  int cnt = 0;
  wg_sum_count(in ? (double)best : 0., in ? 1 : 0, t, wsum, wcnt, &sum, &cnt);
  if (t == 0) p.partial[(size_t)b * p.nblk + blk] = NnPartial{sum, cnt, 0};
}

struct NnFinal {
  const NnPartial* partial; int Ns, nblk;
  int* inliers; double* sum_d2; float* fitness; float* rmse;
};

__global__ __launch_bounds__(NN_BLOCK) void nn_final_kernel(NnFinal p) {
  __shared__ double ls[NN_BLOCK];
  __shared__ int lc[NN_BLOCK];
  const int t = threadIdx.x, b = blockIdx.x;
  const NnPartial* part = p.partial + (size_t)b * p.nblk;
  double sum = 0.;
  int cnt = 0;
  wg_fold(p.nblk, [&](int i, double* s, int* c) { *s = part[i].sum; *c = part[i].count; }, t, ls, lc, &sum, &cnt);
  if (t == 0) {
    if (p.inliers) p.inliers[b] = cnt;
    if (p.sum_d2) p.sum_d2[b] = sum;
    p.fitness[b] = (float)cnt / (float)p.Ns;
    p.rmse[b] = cnt > 0 ? (float)sqrt(sum / (double)cnt) : 0.f;
  }
}

}  // namespace

static int nn_take(const vcr_nn_score_args* user, vcr_nn_score_args* mine) {
  return vcr_take_args(user, mine, offsetof(vcr_nn_score_args, variant));
}

extern "C" int vcr_nn_score_form(const vcr_nn_score_args* ua, int cu_count, int* queries_per_lane, int* target_splits) {
  vcr_nn_score_args a;
  NnPlan p;
  if (nn_take(ua, &a) || cu_count < 0) return VCR_EINVAL;
  const int e = nn_plan(a, cu_count ? cu_count : vcr_cu_count(), &p);
  if (e) return e;
  if (queries_per_lane) *queries_per_lane = p.Q;
  if (target_splits) *target_splits = p.scan.S;
  return VCR_OK;
}

extern "C" size_t vcr_nn_score_workspace_bytes(const vcr_nn_score_args* ua, int cu_count) {
  vcr_nn_score_args a;
  NnPlan p;
  if (nn_take(ua, &a) || cu_count < 0) return 0;
  return nn_plan(a, cu_count ? cu_count : vcr_cu_count(), &p) ? 0 : p.bytes;
}

// The merge and the final reduction behind a search that has filled the workspace's candidates
static int nn_finish(const NnPlan& p, void* workspace, hipStream_t s) {
  const vcr_nn_score_args& a = p.a;
  unsigned char* w = reinterpret_cast<unsigned char*>(workspace);
  float* part_d2 = reinterpret_cast<float*>(w);
  int* part_idx = reinterpret_cast<int*>(w + p.part_bytes);
  NnPartial* partial = reinterpret_cast<NnPartial*>(w + p.partial_off);
  const NnMerge mg{part_d2, part_idx, a.B, a.Ns, p.scan.S, p.nblk, a.max_dist * a.max_dist, a.nn_idx, a.nn_d2, partial};
  hipLaunchKernelGGL(nn_merge_kernel, dim3(p.merge_grid), dim3(NN_BLOCK), 0, s, mg);
  int e;
  if ((e = VCR_LAUNCH_RC())) return e;
  const NnFinal fin{partial, a.Ns, p.nblk, a.inliers, a.sum_d2, a.fitness, a.rmse};
  hipLaunchKernelGGL(nn_final_kernel, dim3((unsigned)a.B), dim3(NN_BLOCK), 0, s, fin);
  return VCR_LAUNCH_RC();
}

extern "C" int vcr_nn_score_f32(const vcr_nn_score_args* ua, void* workspace, size_t workspace_bytes, vcr_stream_t stream) {
  vcr_nn_score_args a;
  if (nn_take(ua, &a)) return VCR_EINVAL;
  // the argument checks need no device: only a call that passes them asks for the CU count
  NnPlan p;
  int e = nn_plan(a, 1, &p);
  if (e) return e;
  if (!workspace || (((uintptr_t)workspace) & 15)) return VCR_EINVAL;
  vcr_stream_scope scope_(stream);
  e = nn_plan(a, vcr_cu_count(), &p);
  if (e) return e;
  if (workspace_bytes < p.bytes) return VCR_EWORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  if ((e = nn_scan_launch(p, workspace, nullptr, s))) return e;
  return nn_finish(p, workspace, s);
}

// ------------------------------------------------------------------------- the grid sibling (include/vcr_hip_gridnn.h, 4.20)

// The scan's plan at one target split -- the merge then folds the grid search's one candidate a point -- and the grid's behind
// its workspace.  No device is asked: neither plan depends on one.
static int nn_grid_plan(const vcr_nn_score_args* ua, const vcr_grid_nn_args* ug, NnPlan* p, GridNnPlan* g) {
  vcr_nn_score_args a;
  if (nn_take(ua, &a) || !ug || a.variant != 0) return VCR_EINVAL;
  a.variant = VCR_NN_SCORE_VARIANT(1, 1);
  int e = nn_plan(a, 1, p);
  if (e) return e;
  return gridnn_plan(ug, GRIDNN_SCORE, 1, a.B, a.Ns, a.Nt, g);
}

extern "C" int vcr_nn_score_grid_form(const vcr_nn_score_args* ua, const vcr_grid_nn_args* ug, int cu_count, int* cells_per_cloud,
                                      int* order, int* queries_per_workgroup) {
  NnPlan p;
  GridNnPlan g;
  if (cu_count < 0) return VCR_EINVAL;
  const int e = nn_grid_plan(ua, ug, &p, &g);
  if (e) return e;
  if (cells_per_cloud) *cells_per_cloud = g.cells;
  if (order) *order = g.order;
  if (queries_per_workgroup) *queries_per_workgroup = VCR_GRID_QUERIES;
  return VCR_OK;
}

extern "C" size_t vcr_nn_score_grid_workspace_bytes(const vcr_nn_score_args* ua, const vcr_grid_nn_args* ug, int cu_count) {
  NnPlan p;
  GridNnPlan g;
  if (cu_count < 0 || nn_grid_plan(ua, ug, &p, &g)) return 0;
  return p.bytes + g.bytes;
}

extern "C" int vcr_nn_score_grid_f32(const vcr_nn_score_args* ua, const vcr_grid_nn_args* ug, void* workspace, size_t workspace_bytes,
                                     vcr_stream_t stream) {
  NnPlan p;
  GridNnPlan g;
  int e = nn_grid_plan(ua, ug, &p, &g);
  if (e) return e;
  if (!workspace || (((uintptr_t)workspace) & 15)) return VCR_EINVAL;
  if (workspace_bytes < p.bytes + g.bytes) return VCR_EWORKSPACE;
  vcr_stream_scope scope_(stream);
  hipStream_t s = (hipStream_t)stream;
  unsigned char* w = reinterpret_cast<unsigned char*>(workspace);
  const vcr_nn_score_args& a = p.a;
  if ((e = gridnn_build(g, a.src, a.tgt, w + p.bytes, s))) return e;
  if ((e = gridnn_search(g, a.src, a.R, a.t, a.max_dist * a.max_dist, w + p.bytes, reinterpret_cast<float*>(w),
                         reinterpret_cast<int*>(w + p.part_bytes), nullptr, s))) return e;
  return nn_finish(p, workspace, s);
}

// All points within a radius of every point of a cloud, searched on the cloud's uniform grid (include/vcr_hip_radius.h, DESIGN
// section 4.22): rows of varying length in CSR form, and the radius outlier filter on the same count.  The result is the
// header's definition -- every hit (d2 <= r2, j != i), ascending in (d2, j) -- and nothing of the grid shows in it: the cells only
// decide which candidates are looked at, and the walk stops only where section 4.19's fp32 bound proves that no point behind
// the ring can be a hit (bound > r2, strictly).
//
// vcr_grid_radius_f32: the five launches of grid_build.h (the edge is the radius unless forced), then
//   radius_count_kernel       one lane per query, the queries in cell order: the walk, n_i to count[b, i]
//   rows_offsets_kernel       csr_rows.h's tail, shared with query.hip: the 64-bit scan of the counts to row_start, total
// and with idx, for the clouds that fit (total[b] <= capacity)
//   radius_fill_kernel        the same walk: lane i appends its hits' keys to its private segment of the scratch row
//   rows_order_kernel         csr_rows.h's rank sort out of the scratch, a wave per row, or
//   radius_order_lane_kernel  the same ranks, a lane per row; it lost every measurement, so rd_order_form(), the one place that
//                             decides, never takes it
//   rows_pad_kernel           -1 / +inf behind total[b], and over the clouds that do not fit
// vcr_outlier_radius_grid_f32: the grid, radius_count_kernel writing c_i = n_i + 1 (0 for a point that is not finite), then
// outlier_tail.h's mark, offsets and write -- vcr_outlier_radius_f32's own tail.
// The walk is grid_walk.h's (the query's cell decoded, the d * d term); rd_walk says once, for the two kernels that walk, what a
// candidate is and where the walk stops.  No scratch memory, no waits between workgroups; every loop is bounded by N, a row's
// length or the cells per axis; every run of candidates is clamped to [0, N), every write to its row.
#include "grid_walk.h"
#include "csr_rows.h"
#include "outlier_tail.h"

namespace {

static_assert(GD_BLOCK == NN_BLOCK, "outlier_tail.h's kernels run on the grid's point launches");

// hit(key) for every j != i with d2 <= r2 (a NaN or an overflowed d2 is no hit: r2 is finite).  The walk stops after a ring when
// bound > r2, STRICTLY -- an unseen point at exactly r2 is a hit --, or when the grid is exhausted (no side is left: the bound is
// +inf).  A query without a cell walks nothing.
template <class Hit>
__device__ __forceinline__ void rd_walk(const GdSelf& p, int b, const GdQuery& q, float r2, Hit& hit) {
  if (!q.ok) return;
  const int N = p.N;
  const float4* __restrict__ sorted = p.sorted + (size_t)b * N;
  auto run = [&](int a0, int a1) {
    a0 = a0 > 0 ? a0 : 0;
    a1 = a1 < N ? a1 : N;
    for (int c = a0; c < a1; ++c) {
      const u64 key = gd_key(sorted[c], q.x);
      // (&, not &&: with a branch between the two tests the compiler loads the index apart from the position and no longer
      // unrolls radius_count_kernel's candidate loop -- 33 VGPRs instead of 50, one 16-byte load in flight instead of two)
      if ((int)(gd_key_j(key) != q.i) & (int)(gd_key_d2(key) <= r2)) hit(key);
    }
  };
  auto stop = [&](float bound) { return bound > r2; };
  gd_self_walk(p, b, q, run, stop);
}

// self: what a finite point adds for itself (0: n_i, the search's count; 1: c_i, the filter's).  out1 is optional
struct RdCount { GdSelf w; float r2; int self; int* out0; int* out1; };

__global__ __launch_bounds__(GD_BLOCK) void radius_count_kernel(RdCount p) {
  const int b = (int)(blockIdx.x / (unsigned)p.w.nblk), blk = (int)(blockIdx.x % (unsigned)p.w.nblk);
  const int s = blk * GD_BLOCK + (int)threadIdx.x;
  if (s >= p.w.N) return;                                  // (no barrier below)
  const GdQuery q = gd_self_query(p.w, b, s);
  int n = 0;
  auto hit = [&](u64) { ++n; };
  rd_walk(p.w, b, q, p.r2, hit);
  const int c = q.ok ? n + p.self : 0;
  const size_t o = (size_t)b * p.w.N + q.i;
  p.out0[o] = c;
  if (p.out1) p.out1[o] = c;
}

struct RdFill { GdSelf w; float r2; const long long* row_start; int capacity; u64* scratch; };

__global__ __launch_bounds__(GD_BLOCK) void radius_fill_kernel(RdFill p) {
  const int b = (int)(blockIdx.x / (unsigned)p.w.nblk), blk = (int)(blockIdx.x % (unsigned)p.w.nblk);
  const int s = blk * GD_BLOCK + (int)threadIdx.x, N = p.w.N;
  const long long* __restrict__ rs = p.row_start + (size_t)b * ((size_t)N + 1);
  if (s >= N || rs[N] > (long long)p.capacity) return;     // (no barrier below; a cloud that does not fit: the pad writes it)
  const GdQuery q = gd_self_query(p.w, b, s);
  const RowsSeg sg = rows_segment(rs, q.i, p.capacity);    // the lane's segment
  const long long room = sg.len;
  if (sg.at < 0 || room <= 0) return;
  u64* __restrict__ row = p.scratch + (size_t)b * p.capacity + (size_t)sg.at;
  int w = 0;
  auto hit = [&](u64 key) { if (w < room) row[w] = key; ++w; };
  rd_walk(p.w, b, q, p.r2, hit);
}

// One lane per row, the rows in index order (neighbouring lanes read neighbouring segments): every key against every key
__global__ __launch_bounds__(GD_BLOCK) void radius_order_lane_kernel(RowsOrder p, int nblk) {
  const int b = (int)(blockIdx.x / (unsigned)nblk), blk = (int)(blockIdx.x % (unsigned)nblk);
  const int i = blk * GD_BLOCK + (int)threadIdx.x, N = p.n;
  const long long* __restrict__ rs = p.row_start + (size_t)b * ((size_t)N + 1);
  if (i >= N || rs[N] > (long long)p.capacity) return;     // (no barrier below)
  const long long at = rs[i];
  long long len = rs[i + 1] - at;
  len = len < (long long)p.capacity - at ? len : (long long)p.capacity - at;
  if (at < 0 || len <= 0) return;
  const int n = (int)len;
  const size_t base = (size_t)b * p.capacity + (size_t)at;
  const u64* __restrict__ row = p.scratch + base;
  for (int e = 0; e < n; ++e) {                            // (bounded by the row's length)
    const u64 key = row[e];
    int rank = 0;
    for (int f = 0; f < n; ++f) rank += row[f] < key ? 1 : 0;
    if (rank < n) {
      p.idx[base + rank] = (int)(uint32_t)key;
      if (p.d2) p.d2[base + rank] = __uint_as_float((uint32_t)(key >> 32));
    }
  }
}

// How one call runs: radius_plan() validates the arguments and lays out the workspace; the entry points answer from it.
struct RdPlan {
  vcr_grid_radius_args a;
  GdLayout at;
  int by_index, form;                                      // form: 1 = a wave per row, 2 = a lane per row, 0 = nothing to order
  float cell, r2;
  size_t scratch_off, bytes;
};

struct RdFilterPlan {
  vcr_outlier_radius_args a;
  GdLayout at;
  int by_index;
  float cell, r2;
  unsigned point_grid;
  size_t cnt_off, blk_off, bytes;                          // workspace: the grid | cnt | blkcnt
};

}  // namespace

// The ONE place that decides the ordering's form.  Measured (profiles/radius_bench.txt): a wave per row
// beats a lane per row beyond the blocks' spread in all 14 cases timed, from mean rows of 10 entries (0.089 against 0.149 ms at
// 16 x 1 024, 0.45 against 0.51 ms at 1 x 131 072) to 330 (2.8 against 100 ms) -- the lane form reads its row n times from
// global memory, a lane a row, and a wave waits for its longest.  So the plan takes the wave form whatever the shape; the lane
// form stays behind `variant` for the benchmark that shows this.
static int rd_order_form(int N, int capacity) {
  (void)N; (void)capacity;
  return 1;
}

static int radius_plan(const vcr_grid_radius_args& a, RdPlan* p) {
  *p = RdPlan{a};
  if (!a.xyz || !a.count || !a.row_start || !a.total || a.B < 1) return VCR_EINVAL;
  if (!gd_radius_ok(a.radius, &p->r2)) return VCR_EINVAL;
  if (!gd_cell_ok(a.cell)) return VCR_EINVAL;
  if (a.capacity < 0 || (!a.idx && a.capacity != 0) || (a.d2 && !a.idx)) return VCR_EINVAL;
  const int order = a.variant & 15, form = (a.variant >> 4) & 15;
  if (a.variant < 0 || (a.variant >> 8) || order > 2 || form > 2) return VCR_EINVAL;
  if (a.N < 1 || a.N > VCR_RADIUS_MAX_N || (long)a.B * a.N >= (1L << 31)) return VCR_EUNSUPPORTED;
  if ((long)a.B * a.capacity >= (1L << 31)) return VCR_EUNSUPPORTED;
  p->at = gd_layout(a.B, a.N);
  p->by_index = order == 2;
  p->form = !a.idx ? 0 : form ? form : rd_order_form(a.N, a.capacity);
  p->cell = a.cell > 0.f ? a.cell : a.radius;
  p->scratch_off = p->at.bytes;
  p->bytes = p->scratch_off + ws_up((size_t)a.B * a.capacity * sizeof(u64));
  return VCR_OK;
}

static int radius_take(const vcr_grid_radius_args* user, vcr_grid_radius_args* mine) {
  return vcr_take_args(user, mine, offsetof(vcr_grid_radius_args, idx));
}

extern "C" int vcr_grid_radius_form(const vcr_grid_radius_args* ua, int cu_count, int* cells_per_cloud, int* queries_per_workgroup,
                                    int* order_form) {
  vcr_grid_radius_args a;
  RdPlan p;
  if (radius_take(ua, &a) || cu_count < 0) return VCR_EINVAL;
  const int e = radius_plan(a, &p);
  if (e) return e;
  if (cells_per_cloud) *cells_per_cloud = p.at.gstride - 2;
  if (queries_per_workgroup) *queries_per_workgroup = GD_BLOCK;
  if (order_form) *order_form = p.form;
  return VCR_OK;
}

extern "C" size_t vcr_grid_radius_workspace_bytes(const vcr_grid_radius_args* ua, int cu_count) {
  vcr_grid_radius_args a;
  RdPlan p;
  if (radius_take(ua, &a) || cu_count < 0) return 0;
  return radius_plan(a, &p) ? 0 : p.bytes;
}

extern "C" int vcr_grid_radius_f32(const vcr_grid_radius_args* ua, void* workspace, size_t workspace_bytes, vcr_stream_t stream) {
  vcr_grid_radius_args a;
  if (radius_take(ua, &a)) return VCR_EINVAL;
  RdPlan p;
  int e = radius_plan(a, &p);
  if (e) return e;
  if (!workspace || (((uintptr_t)workspace) & 15)) return VCR_EINVAL;
  if (workspace_bytes < p.bytes) return VCR_EWORKSPACE;
  vcr_stream_scope scope_(stream);
  hipStream_t s = (hipStream_t)stream;
  unsigned char* w = reinterpret_cast<unsigned char*>(workspace);
  if ((e = gd_build(a.xyz, a.B, a.N, p.cell, p.at, w, s))) return e;
  const dim3 block(GD_BLOCK), points((unsigned)((long)a.B * p.at.nblk));
  const GdSelf wk = gd_self(a.xyz, a.N, p.at, w, p.by_index);
  long long* row_start = reinterpret_cast<long long*>(a.row_start);
  hipLaunchKernelGGL(radius_count_kernel, points, block, 0, s, RdCount{wk, p.r2, 0, a.count, nullptr});
  if ((e = VCR_LAUNCH_RC())) return e;
  if ((e = rows_offsets(a.count, row_start, reinterpret_cast<long long*>(a.total), a.B, a.N, s))) return e;
  if (!a.idx || a.capacity == 0) return VCR_OK;
  u64* scratch = reinterpret_cast<u64*>(w + p.scratch_off);
  hipLaunchKernelGGL(radius_fill_kernel, points, block, 0, s, RdFill{wk, p.r2, row_start, a.capacity, scratch});
  if ((e = VCR_LAUNCH_RC())) return e;
  const RowsOrder od{row_start, scratch, a.N, a.capacity, a.idx, a.d2};
  if (p.form != 2) return rows_order_pad(od, a.B, s);
  hipLaunchKernelGGL(radius_order_lane_kernel, points, block, 0, s, od, p.at.nblk);
  if ((e = VCR_LAUNCH_RC())) return e;
  return rows_pad(od, a.B, s);
}

// ---- the radius outlier filter on the grid

static int radius_filter_plan(const vcr_outlier_radius_args* ua, const vcr_grid_nn_args* ug, RdFilterPlan* p) {
  *p = RdFilterPlan{};
  vcr_grid_nn_args g;
  if (vcr_take_args(ua, &p->a, offsetof(vcr_outlier_radius_args, index))) return VCR_EINVAL;
  if (vcr_take_args(ug, &g, sizeof(vcr_grid_nn_args))) return VCR_EINVAL;
  const vcr_outlier_radius_args& a = p->a;
  if (!a.xyz || !a.points || !a.count || a.B < 1 || a.nb_points < 0 || a.variant != 0) return VCR_EINVAL;
  if (!gd_radius_ok(a.radius, &p->r2)) return VCR_EINVAL;
  if (!gd_cell_ok(g.cell)) return VCR_EINVAL;
  if (g.order < 0 || g.order > 2) return VCR_EINVAL;
  if (a.N < 1 || a.N > VCR_RADIUS_MAX_N || (long)a.B * a.N >= (1L << 31)) return VCR_EUNSUPPORTED;
  p->at = gd_layout(a.B, a.N);
  p->by_index = g.order == 2;
  p->cell = g.cell > 0.f ? g.cell : a.radius;
  p->point_grid = (unsigned)((long)a.B * p->at.nblk);
  p->cnt_off = p->at.bytes;
  p->blk_off = p->cnt_off + ws_up((size_t)a.B * a.N * 4);
  p->bytes = p->blk_off + ws_up((size_t)a.B * p->at.nblk * 4);
  return VCR_OK;
}

extern "C" int vcr_outlier_radius_grid_form(const vcr_outlier_radius_args* ua, const vcr_grid_nn_args* ug, int cu_count,
                                            int* cells_per_cloud, int* order, int* queries_per_workgroup) {
  RdFilterPlan p;
  if (cu_count < 0) return VCR_EINVAL;
  const int e = radius_filter_plan(ua, ug, &p);
  if (e) return e;
  if (cells_per_cloud) *cells_per_cloud = p.at.gstride - 2;
  if (order) *order = p.by_index ? 2 : 1;
  if (queries_per_workgroup) *queries_per_workgroup = GD_BLOCK;
  return VCR_OK;
}

extern "C" size_t vcr_outlier_radius_grid_workspace_bytes(const vcr_outlier_radius_args* ua, const vcr_grid_nn_args* ug,
                                                          int cu_count) {
  RdFilterPlan p;
  if (cu_count < 0) return 0;
  return radius_filter_plan(ua, ug, &p) ? 0 : p.bytes;
}

extern "C" int vcr_outlier_radius_grid_f32(const vcr_outlier_radius_args* ua, const vcr_grid_nn_args* ug, void* workspace,
                                           size_t workspace_bytes, vcr_stream_t stream) {
  RdFilterPlan p;
  int e = radius_filter_plan(ua, ug, &p);
  if (e) return e;
  if (!workspace || (((uintptr_t)workspace) & 15)) return VCR_EINVAL;
  if (workspace_bytes < p.bytes) return VCR_EWORKSPACE;
  const vcr_outlier_radius_args& a = p.a;
  vcr_stream_scope scope_(stream);
  hipStream_t s = (hipStream_t)stream;
  unsigned char* w = reinterpret_cast<unsigned char*>(workspace);
  if ((e = gd_build(a.xyz, a.B, a.N, p.cell, p.at, w, s))) return e;
  int* cnt = reinterpret_cast<int*>(w + p.cnt_off);
  int* blk = reinterpret_cast<int*>(w + p.blk_off);
  const dim3 block(GD_BLOCK), points(p.point_grid);
  hipLaunchKernelGGL(radius_count_kernel, points, block, 0, s,
                     RdCount{gd_self(a.xyz, a.N, p.at, w, p.by_index), p.r2, 1, cnt, a.neighbours});
  if ((e = VCR_LAUNCH_RC())) return e;
  const OlTail tl{nullptr, nullptr, cnt, a.nb_points, nullptr, a.xyz, a.N, p.at.nblk, blk, a.points, a.count, a.index};
  hipLaunchKernelGGL(outlier_mark_kernel, points, block, 0, s, tl);
  if ((e = VCR_LAUNCH_RC())) return e;
  return ol_compact(tl, a.B, p.point_grid, s);
}

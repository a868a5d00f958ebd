// The exact k nearest neighbours of every point among its cloud's other points, searched on a uniform grid
// (include/vcr_hip_grid.h).  The result is the header's definition -- the k smallest (d2, j) with d2 in
// difference form -- and nothing of the grid shows in it: the cells only decide which candidates are looked at, and the walk
// stops only where an fp32 lower bound proves that no point behind it can enter the row.
//
// Six launches: the five of grid_build.h (bounds, clear, count, scan, scatter -- shared with gridnn.hip), then
//   grid_search_kernel   one lane per query, the queries in cell order (a wave's lanes walk the same cells and load the same
//                        candidates).  The row is a lane-private column of k 64-bit keys in LDS, (d2's bits) << 32 | j --
//                        d2 >= +0, so the keys order as (d2, j) -- kept ascending; a candidate is compared with the k-th key in
//                        a register first, and only one that passes is inserted (grid_walk.h's gd_insert; the query itself is
//                        excluded by its index).  The rings of cells and the ring bound are grid_walk.h's gd_walk, with the
//                        query's cell decoded from cellof and the d * d term; the walk stops when the k-th d2 is STRICTLY below
//                        the bound.
// No scratch, no waits between workgroups; every loop is bounded by N, k or the cells per axis, and every run of candidates is
// clamped to [0, N).
#include "grid_walk.h"

namespace {

struct GdSearch { GdSelf w; int k; int* idx; float* d2; };

__global__ __launch_bounds__(GD_BLOCK) void grid_search_kernel(GdSearch p) {
  extern __shared__ __attribute__((aligned(16))) u64 gd_rows[];          // [k][GD_BLOCK]: lane t's column starts at gd_rows + t
  const int t = threadIdx.x;
  const int b = (int)(blockIdx.x / (unsigned)p.w.nblk), blk = (int)(blockIdx.x % (unsigned)p.w.nblk);
  const int s = blk * GD_BLOCK + t, N = p.w.N, k = p.k;
  if (s >= N) return;                                      // (no barrier below: every lane works on its own column)
  const GdQuery q = gd_self_query(p.w, b, s);
  u64* lk = gd_rows + t;
  const u64 none = (u64)GD_INF << 32 | (uint32_t)q.i;      // a slot without a neighbour: the query's own index, d2 = +inf
  for (int a = 0; a < k; ++a) lk[a * GD_BLOCK] = none;
  u64 kth = none;
  if (q.ok) {                                              // a finite query
    const float4* __restrict__ sorted = p.w.sorted + (size_t)b * N;
    auto run = [&](int a0, int a1) {
      a0 = a0 > 0 ? a0 : 0;
      a1 = a1 < N ? a1 : N;
      for (int c = a0; c < a1; ++c) {
        const u64 key = gd_key(sorted[c], q.x);
        gd_insert(lk, k, key, kth, gd_key_j(key) != q.i);              // (the query itself is no candidate)
      }
    };
    // STRICTLY below: a tie behind the ring could still enter
    auto stop = [&](float bound) { return gd_key_d2(kth) < bound; };
    gd_self_walk(p.w, b, q, run, stop);
  }
  int* __restrict__ oi = p.idx + ((size_t)b * N + q.i) * k;
  for (int a = 0; a < k; ++a) oi[a] = gd_key_j(lk[a * GD_BLOCK]);
  if (p.d2) {
    float* __restrict__ od = p.d2 + ((size_t)b * N + q.i) * k;
    for (int a = 0; a < k; ++a) od[a] = gd_key_d2(lk[a * GD_BLOCK]);
  }
}

// How one call runs: grid_plan() validates the arguments and lays out the workspace; the entry points answer from it.
struct GdPlan {
  vcr_grid_knn_args a;
  GdLayout at;
  int by_index;
  size_t lds;
};

}  // namespace

static int grid_plan(const vcr_grid_knn_args& a, GdPlan* p) {
  *p = GdPlan{a};
  if (!a.xyz || !a.idx || a.B < 1) return VCR_EINVAL;
  if (!gd_cell_ok(a.cell)) return VCR_EINVAL;
  if (a.variant < 0 || a.variant > 2) return VCR_EINVAL;
  if (a.N < 1 || a.N > VCR_GRID_MAX_N || (long)a.B * a.N >= (1L << 31)) return VCR_EUNSUPPORTED;
  if (a.k < 1 || a.k > VCR_GRID_MAX_K) return VCR_EUNSUPPORTED;
  p->at = gd_layout(a.B, a.N);
  p->by_index = a.variant == 2;
  p->lds = (size_t)a.k * GD_BLOCK * sizeof(u64);
  return VCR_OK;
}

static int grid_take(const vcr_grid_knn_args* user, vcr_grid_knn_args* mine) {
  return vcr_take_args(user, mine, offsetof(vcr_grid_knn_args, d2));
}

extern "C" int vcr_grid_knn_form(const vcr_grid_knn_args* ua, int cu_count, int* cells_per_cloud, int* queries_per_workgroup) {
  vcr_grid_knn_args a;
  GdPlan p;
  if (grid_take(ua, &a) || cu_count < 0) return VCR_EINVAL;
  const int e = grid_plan(a, &p);
  if (e) return e;
  if (cells_per_cloud) *cells_per_cloud = p.at.gstride - 2;
  if (queries_per_workgroup) *queries_per_workgroup = GD_BLOCK;
  return VCR_OK;
}

extern "C" size_t vcr_grid_knn_workspace_bytes(const vcr_grid_knn_args* ua, int cu_count) {
  vcr_grid_knn_args a;
  GdPlan p;
  if (grid_take(ua, &a) || cu_count < 0) return 0;
  return grid_plan(a, &p) ? 0 : p.at.bytes;
}

extern "C" int vcr_grid_knn_f32(const vcr_grid_knn_args* ua, void* workspace, size_t workspace_bytes, vcr_stream_t stream) {
  vcr_grid_knn_args a;
  if (grid_take(ua, &a)) return VCR_EINVAL;
  GdPlan p;
  int e = grid_plan(a, &p);
  if (e) return e;
  if (!workspace || (((uintptr_t)workspace) & 15)) return VCR_EINVAL;
  if (workspace_bytes < p.at.bytes) return VCR_EWORKSPACE;
  vcr_stream_scope scope_(stream);
  hipStream_t s = (hipStream_t)stream;
  unsigned char* w = reinterpret_cast<unsigned char*>(workspace);
  if ((e = gd_build(a.xyz, a.B, a.N, a.cell, p.at, w, s))) return e;
  const GdSearch sr{gd_self(a.xyz, a.N, p.at, w, p.by_index), a.k, a.idx, a.d2};
  return vcr_launch<grid_search_kernel>(dim3((unsigned)((long)a.B * p.at.nblk)), dim3(GD_BLOCK), p.lds, s, sr);
}

// The exact k nearest neighbours of every point among its cloud's other points, searched on a uniform grid
// (include/vcr_hip_grid.h).  The result is the header's definition -- the k smallest (d2, j) with d2 in
// difference form -- and nothing of the grid shows in it: the cells only decide which candidates are looked at, and the walk
// stops only where an fp32 lower bound proves that no point behind it can enter the row.
//
// Six launches: the five of grid_build.h (bounds, clear, count, scan, scatter -- shared with gridnn.hip), then
//   grid_search_kernel   one lane per query, the queries in cell order (a wave's lanes walk the same cells and load the same
//                        candidates).  The row is a lane-private column of k 64-bit keys in LDS, (d2's bits) << 32 | j --
//                        d2 >= +0, so the keys order as (d2, j) -- kept ascending; a candidate is compared with the k-th key in
//                        a register first, and only one that passes is inserted.  Rings of cells: along x a ring's cells are
//                        contiguous in the sorted order, one run of candidates a (y, z) row.
// No scratch, no waits between workgroups; every loop is bounded by N, k or the cells per axis, and every run of candidates is
// clamped to [0, N).
#include "grid_build.h"

namespace {

struct GdSearch {
  const float* xyz; const GdGrid* grid; const int* cellof; const int* counter; const float4* sorted;
  int N, k, nblk, gstride, by_index;
  int* idx; float* d2;
};

// One run sorted[a0 ... a1) of candidates against the lane's query: a candidate whose key is below the row's k-th is inserted
// into the ascending column (lk[s * GD_BLOCK], s < k), and the k-th key is read back
__device__ __forceinline__ void gd_run(const float4* __restrict__ sorted, int a0, int a1, int N, float qx, float qy, float qz,
                                       int qi, u64* lk, int k, u64& kth) {
  a0 = a0 > 0 ? a0 : 0;
  a1 = a1 < N ? a1 : N;
  for (int s = a0; s < a1; ++s) {
    const float4 c = sorted[s];
    const int j = __float_as_int(c.w);
    const float dx = c.x - qx, dy = c.y - qy, dz = c.z - qz;
    const float d2 = fmaf(dz, dz, fmaf(dy, dy, dx * dx));
    const uint32_t bits = __float_as_uint(d2);
    const u64 key = (u64)bits << 32 | (uint32_t)j;
    if (j != qi && bits < GD_INF && key < kth) {
      int at = k - 1;
      for (; at > 0; --at) {                               // (bounded by k)
        const u64 prev = lk[(at - 1) * GD_BLOCK];
        if (prev < key) break;
        lk[at * GD_BLOCK] = prev;
      }
      lk[at * GD_BLOCK] = key;
      kth = lk[(k - 1) * GD_BLOCK];
    }
  }
}

__global__ __launch_bounds__(GD_BLOCK) void grid_search_kernel(GdSearch p) {
  extern __shared__ __attribute__((aligned(16))) u64 gd_rows[];          // [k][GD_BLOCK]: lane t's column starts at gd_rows + t
  const int t = threadIdx.x;
  const int b = (int)(blockIdx.x / (unsigned)p.nblk), blk = (int)(blockIdx.x % (unsigned)p.nblk);
  const int s = blk * GD_BLOCK + t, N = p.N, k = p.k;
  if (s >= N) return;                                      // (no barrier below: every lane works on its own column)
  const GdGrid g = p.grid[b];
  const float4* __restrict__ sorted = p.sorted + (size_t)b * N;
  const int* __restrict__ start = p.counter + (size_t)b * p.gstride;     // cell c: sorted[start[c] ... start[c + 1])
  float qx, qy, qz;
  int qi;
  if (p.by_index) {
    const float* __restrict__ x = p.xyz + (size_t)b * 3 * N;
    qi = s; qx = x[s]; qy = x[N + s]; qz = x[2 * (size_t)N + s];
  } else {
    const float4 q = sorted[s];
    qx = q.x; qy = q.y; qz = q.z; qi = __float_as_int(q.w);
    qi = (unsigned)qi < (unsigned)N ? qi : 0;              // (always in range: the scatter wrote every slot)
  }
  const int cell = p.cellof[(size_t)b * N + qi];
  u64* lk = gd_rows + t;
  const u64 none = (u64)GD_INF << 32 | (uint32_t)qi;       // a slot without a neighbour: the query's own index, d2 = +inf
  for (int a = 0; a < k; ++a) lk[a * GD_BLOCK] = none;
  u64 kth = none;

  if (cell >= 0 && cell < g.cells) {                       // a finite query
    const int nx = g.n[0], ny = g.n[1], nz = g.n[2];
    const int cx = cell % nx, cy = (cell / nx) % ny, cz = cell / (nx * ny);
    int rmax = cx > nx - 1 - cx ? cx : nx - 1 - cx;
    rmax = cy > rmax ? cy : rmax; rmax = ny - 1 - cy > rmax ? ny - 1 - cy : rmax;
    rmax = cz > rmax ? cz : rmax; rmax = nz - 1 - cz > rmax ? nz - 1 - cz : rmax;
    const int q[3] = {cx, cy, cz};
    const float xq[3] = {qx, qy, qz};
    for (int r = 0; r <= rmax; ++r) {                      // (bounded by the cells per axis)
      const int z0 = cz - r > 0 ? cz - r : 0, z1 = cz + r < nz - 1 ? cz + r : nz - 1;
      const int y0 = cy - r > 0 ? cy - r : 0, y1 = cy + r < ny - 1 ? cy + r : ny - 1;
      const int x0 = cx - r > 0 ? cx - r : 0, x1 = cx + r < nx - 1 ? cx + r : nx - 1;
      for (int z = z0; z <= z1; ++z)
        for (int y = y0; y <= y1; ++y) {
          const int row = (z * ny + y) * nx;
          const bool shell = z - cz == r || cz - z == r || y - cy == r || cy - y == r;
          if (shell) {                                     // the whole x range of the ring: one run
            gd_run(sorted, start[row + x0], start[row + x1 + 1], N, qx, qy, qz, qi, lk, k, kth);
          } else {                                         // its two end cells
            if (cx - r >= 0) gd_run(sorted, start[row + cx - r], start[row + cx - r + 1], N, qx, qy, qz, qi, lk, k, kth);
            if (cx + r <= nx - 1) gd_run(sorted, start[row + cx + r], start[row + cx + r + 1], N, qx, qy, qz, qi, lk, k, kth);
          }
        }
      // what no point behind ring r can undercut: per side that exists one subtraction, the smallest square
      float bound = __builtin_huge_valf();
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        if (q[c] + r + 1 <= g.n[c] - 1) { const float d = gd_face(q[c] + r + 1, g.h, g.lo[c]) - xq[c]; bound = fminf(bound, d * d); }
        if (q[c] - r >= 1) { const float d = xq[c] - gd_face(q[c] - r, g.h, g.lo[c]); bound = fminf(bound, d * d); }
      }
      if (__uint_as_float((uint32_t)(kth >> 32)) < bound) break;         // STRICTLY below: a tie behind the ring could still enter
    }
  }
  int* __restrict__ oi = p.idx + ((size_t)b * N + qi) * k;
  for (int a = 0; a < k; ++a) oi[a] = (int)(uint32_t)lk[a * GD_BLOCK];
  if (p.d2) {
    float* __restrict__ od = p.d2 + ((size_t)b * N + qi) * k;
    for (int a = 0; a < k; ++a) od[a] = __uint_as_float((uint32_t)(lk[a * GD_BLOCK] >> 32));
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
  if (!(a.cell >= 0.f) || a.cell == __builtin_huge_valf()) return VCR_EINVAL;           // negative, NaN, +inf
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
  const GdSearch sr{a.xyz, reinterpret_cast<const GdGrid*>(w), reinterpret_cast<const int*>(w + p.at.cellof_off),
                    reinterpret_cast<const int*>(w + p.at.counter_off), reinterpret_cast<const float4*>(w + p.at.sorted_off),
                    a.N, a.k, p.at.nblk, p.at.gstride, p.by_index, a.idx, a.d2};
  return vcr_launch<grid_search_kernel>(dim3((unsigned)((long)a.B * p.at.nblk)), dim3(GD_BLOCK), p.lds, s, sr);
}

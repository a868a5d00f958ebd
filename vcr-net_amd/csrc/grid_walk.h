// What every search on a uniform grid runs per query, written once for grid.hip, gridnn.hip, radius.hip and query.hip (DESIGN
// sections 4.19, 4.20, 4.22, 4.28): the ring walk around the query's cell with its fp32 ring bound, a candidate's key, the
// insertion into a lane-private column of k keys, and the self searches' query load.  Device code without LDS of its own, without
// barriers and without read-modify-write memory operations; every loop is bounded by the cells per axis, N or k.
//
// gd_walk has three parameters besides the grid and the query, and its callers differ in nothing else:
//   the cell (cx, cy, cz)   the caller computes it: decoded from cellof (grid.hip, radius.hip: the query is a point of the cloud)
//                           or clamped by gd_cell (gridnn.hip, query.hip: the query may lie outside the box)
//   the side's term         what no point behind a side at distance d along axis C can undercut: GdSquare's d * d, or the
//                           caller's own (query.hip joins d with the query's distances to the box)
//   run and stop            run(a0, a1) looks at sorted[a0 ... a1); stop(bound) says after every ring whether the walk ends.
//                           The early-outs in front of the walk (a query that is not finite, an outside bound beyond the cap,
//                           a cloud without a finite point) stay with the callers
#pragma once
#include "grid_build.h"

namespace {

// section 4.19's term of a side: the square of the one subtraction
struct GdSquare {
  template <int C>
  __device__ __forceinline__ float term(float d) const { return d * d; }
};

template <int C, class Side>
__device__ __forceinline__ float gd_axis_bound(const GdGrid& g, const float xq[3], const Side& side, int qc, int r, float bound) {
  if (qc + r + 1 <= g.n[C] - 1) bound = fminf(bound, side.template term<C>(gd_face(qc + r + 1, g.h, g.lo[C]) - xq[C]));
  if (qc - r >= 1) bound = fminf(bound, side.template term<C>(xq[C] - gd_face(qc - r, g.h, g.lo[C])));
  return bound;
}

// The rings of cells around (cx, cy, cz), a cell of g: along x a ring's cells are contiguous in the sorted order (cell c is
// sorted[start[c] ... start[c + 1])), so a (y, z) row of the shell is ONE run and a row inside it is its two end cells.  After
// ring r the bound is what no point behind the ring can undercut: per side that exists one subtraction from a face, the smallest
// of the sides' terms; +inf when no side is left (the grid is exhausted).  The bound holds for a clamped cell too: a side that
// exists has a distance >= 0, one that does not contributes nothing.
template <class Side, class Run, class Stop>
__device__ __forceinline__ void gd_walk(const GdGrid& g, const int* __restrict__ start, int cx, int cy, int cz, const float xq[3],
                                        const Side& side, Run& run, Stop& stop) {
  const int nx = g.n[0], ny = g.n[1], nz = g.n[2];
  int rmax = cx > nx - 1 - cx ? cx : nx - 1 - cx;
  rmax = cy > rmax ? cy : rmax; rmax = ny - 1 - cy > rmax ? ny - 1 - cy : rmax;
  rmax = cz > rmax ? cz : rmax; rmax = nz - 1 - cz > rmax ? nz - 1 - cz : rmax;
  for (int r = 0; r <= rmax; ++r) {                        // (bounded by the cells per axis)
    const int z0 = cz - r > 0 ? cz - r : 0, z1 = cz + r < nz - 1 ? cz + r : nz - 1;
    const int y0 = cy - r > 0 ? cy - r : 0, y1 = cy + r < ny - 1 ? cy + r : ny - 1;
    const int x0 = cx - r > 0 ? cx - r : 0, x1 = cx + r < nx - 1 ? cx + r : nx - 1;
    for (int z = z0; z <= z1; ++z)
      for (int y = y0; y <= y1; ++y) {
        const int row = (z * ny + y) * nx;
        const bool shell = z - cz == r || cz - z == r || y - cy == r || cy - y == r;
        if (shell) {                                       // the whole x range of the ring: one run
          run(start[row + x0], start[row + x1 + 1]);
        } else {                                           // its two end cells
          if (cx - r >= 0) run(start[row + cx - r], start[row + cx - r + 1]);
          if (cx + r <= nx - 1) run(start[row + cx + r], start[row + cx + r + 1]);
        }
      }
    float bound = __builtin_huge_valf();
    bound = gd_axis_bound<0>(g, xq, side, cx, r, bound);
    bound = gd_axis_bound<1>(g, xq, side, cy, r, bound);
    bound = gd_axis_bound<2>(g, xq, side, cz, r, bound);
    if (stop(bound)) break;
  }
}

// the key of candidate c against the query: (d2's bits) << 32 | j, d2 = fmaf(dz, dz, fmaf(dy, dy, dx * dx)) of x_j - q.  d2 >= +0
// or NaN, so the keys order as (d2, j) and a NaN's lies above +inf's
__device__ __forceinline__ u64 gd_key(const float4 c, const float xq[3]) {
  const float dx = c.x - xq[0], dy = c.y - xq[1], dz = c.z - xq[2];
  const float d2 = fmaf(dz, dz, fmaf(dy, dy, dx * dx));
  return (u64)__float_as_uint(d2) << 32 | (uint32_t)__float_as_int(c.w);
}
__device__ __forceinline__ float gd_key_d2(u64 key) { return __uint_as_float((uint32_t)(key >> 32)); }
__device__ __forceinline__ int gd_key_j(u64 key) { return (int)(uint32_t)key; }

// The row of the k nearest: a lane-private ascending column of k keys in LDS (lk[s * GD_BLOCK], s < k) with its k-th key in a
// register.  A candidate is compared with the k-th first, and only one that passes -- with a finite d2, and that the caller
// takes (the self search drops the query's own index) -- is inserted: one test, no branch between its parts.  (k by
// REFERENCE, the caller's variable: by value the compiler schedules query_knn_kernel differently -- 31 instructions fewer, and
// measured 0.4-1.5 % slower; by reference it is the kernel query.hip had with the loop written in place.  profiles/NOTES.md)
__device__ __forceinline__ void gd_insert(u64* lk, const int& k, u64 key, u64& kth, bool take = true) {
  if (take && (uint32_t)(key >> 32) < GD_INF && key < kth) {
    int at = k - 1;
    for (; at > 0; --at) {                                 // (bounded by k)
      const u64 prev = lk[(at - 1) * GD_BLOCK];
      if (prev < key) break;
      lk[at * GD_BLOCK] = prev;
    }
    lk[at * GD_BLOCK] = key;
    kth = lk[(k - 1) * GD_BLOCK];
  }
}

// A cloud searched against itself (grid.hip, radius.hip): the cloud, its grid, and the order its points are served in
struct GdSelf {
  const float* xyz; const GdGrid* grid; const int* cellof; const int* counter; const float4* sorted;
  int N, nblk, gstride, by_index;
};

// the layout at w as the walking kernels take it
static inline GdSelf gd_self(const float* xyz, int N, const GdLayout& at, const unsigned char* w, int by_index) {
  return GdSelf{xyz, reinterpret_cast<const GdGrid*>(w), reinterpret_cast<const int*>(w + at.cellof_off),
                reinterpret_cast<const int*>(w + at.counter_off), reinterpret_cast<const float4*>(w + at.sorted_off),
                N, at.nblk, at.gstride, by_index};
}

// The lane's query: lane s of cloud b takes the s-th point in cell order (or point s in index order)
struct GdQuery { float x[3]; int i, cell; bool ok; };      // ok: the point is finite, so it has a cell

__device__ __forceinline__ GdQuery gd_self_query(const GdSelf& p, int b, int s) {
  const int N = p.N;
  GdQuery q;
  if (p.by_index) {
    const float* __restrict__ x = p.xyz + (size_t)b * 3 * N;
    q.i = s; q.x[0] = x[s]; q.x[1] = x[N + s]; q.x[2] = x[2 * (size_t)N + s];
  } else {
    const float4 v = p.sorted[(size_t)b * N + s];
    q.x[0] = v.x; q.x[1] = v.y; q.x[2] = v.z; q.i = __float_as_int(v.w);
    q.i = (unsigned)q.i < (unsigned)N ? q.i : 0;           // (always in range: the scatter wrote every slot)
  }
  q.cell = p.cellof[(size_t)b * N + q.i];
  q.ok = q.cell >= 0 && q.cell < p.grid[b].cells;
  return q;
}

// The self searches' walk: the query's cell decoded, section 4.19's term
template <class Run, class Stop>
__device__ __forceinline__ void gd_self_walk(const GdSelf& p, int b, const GdQuery& q, Run& run, Stop& stop) {
  const GdGrid g = p.grid[b];
  const int nx = g.n[0], ny = g.n[1];
  gd_walk(g, p.counter + (size_t)b * p.gstride, q.cell % nx, (q.cell / nx) % ny, q.cell / (nx * ny), q.x, GdSquare{}, run, stop);
}

}  // namespace

// The host's checks of a forced cell edge and of a radius, the same for every entry point that takes one
static inline bool gd_cell_ok(float cell) { return cell >= 0.f && cell != __builtin_huge_valf(); }   // not negative, NaN, +inf

static inline bool gd_radius_ok(float radius, float* r2) {
  if (!(radius > 0.f) || radius == __builtin_huge_valf()) return false;                   // <= 0, NaN, +inf
  *r2 = radius * radius;                                   // fp32, one rounding
  return *r2 < __builtin_huge_valf();
}

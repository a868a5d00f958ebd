// The capped nearest neighbour of every moved source point among the TARGET's points, searched on the target's uniform grid
// (include/vcr_hip_gridnn.h): what vcr_nn_score_grid_f32 and the three vcr_refine*_grid_f32 run where
// their scan siblings run nn_scan_kernel.  The result is the header's definition -- the smallest (d2, j) with d2 in the score's
// difference form where that d2 is within the cap, (-1, +inf) where it is not -- and nothing of the grid shows in it.
//
// Once a call (gridnn_build): grid_build.h's five launches on the target; with order 1 the same five on the SOURCE in its own
// frame and grid_perm_kernel, which keeps the cell order's permutation alone -- a rigid motion keeps neighbours together, so
// the one permutation serves every round.
// Every search (gridnn_search):
//   grid_nn_kernel   one lane per source point (lane s of the launch takes point perm[s], or s in index order), moved by the
//                    pose in registers (the scan's expression).  The best key (d2's bits) << 32 | j lives in a register pair.
//                    Rings of cells around the query's cell -- the query clamped into the grid per axis --: grid_walk.h's
//                    gd_walk, section 4.19's enumeration and ring bound with the d * d term.  After ring r the bound is the
//                    larger of the ring bound and the OUTSIDE bound (the query's distance to the target's box, per axis one
//                    subtraction); the walk stops when the best d2 is strictly below it, when it is strictly above the cap
//                    (or +inf: nothing behind it is a candidate), or when the grid is exhausted.  A query whose outside bound
//                    exceeds the cap, or that is not finite, walks nothing.  A best beyond the cap is written as (-1, +inf).
// No scratch, no atomics in the search, no waits between workgroups; every loop is bounded by Nt or the cells per axis, and
// every run of candidates is clamped to [0, Nt).
#include "grid_walk.h"
#include "grid_nn.h"

namespace {

__global__ __launch_bounds__(GD_BLOCK) void grid_perm_kernel(const float4* sorted, int* perm, long total) {
  const long i = (long)blockIdx.x * GD_BLOCK + threadIdx.x;
  if (i < total) perm[i] = __float_as_int(sorted[i].w);
}

struct GnSearch {
  const float* src; const float* R; const float* t;
  const GdGrid* grid; const int* counter; const float4* sorted;          // the target's
  const int* perm;                                         // [B][Ns] the source's cell order, or NULL: index order
  int Ns, Nt, nblk, gstride;
  float cap2;
  float* part_d2; int* part_idx;                           // [B][Ns]
  const int* live;
};

// One run sorted[a0 ... a1) of target points against the lane's moved point: the smallest key wins
__device__ __forceinline__ void gn_run(const float4* __restrict__ sorted, int a0, int a1, int Nt, float px, float py, float pz,
                                       u64& best) {
  a0 = a0 > 0 ? a0 : 0;
  a1 = a1 < Nt ? a1 : Nt;
  for (int s = a0; s < a1; ++s) {
    const float4 c = sorted[s];
    const float dx = px - c.x, dy = py - c.y, dz = pz - c.z;             // the score's expression, p - q
    const float d2 = fmaf(dz, dz, fmaf(dy, dy, dx * dx));
    const uint32_t bits = __float_as_uint(d2);                           // (d2 >= +0 or NaN: a NaN's bits are above +inf's)
    const u64 key = (u64)bits << 32 | (uint32_t)__float_as_int(c.w);
    best = bits < GD_INF && key < best ? key : best;
  }
}

__global__ __launch_bounds__(GD_BLOCK) void grid_nn_kernel(GnSearch p) {
  const int t = threadIdx.x;
  const int b = (int)(blockIdx.x / (unsigned)p.nblk), blk = (int)(blockIdx.x % (unsigned)p.nblk);
  if (p.live && !p.live[b]) return;                        // (workgroup-uniform)
  const int s = blk * GD_BLOCK + t, Ns = p.Ns, Nt = p.Nt;
  if (s >= Ns) return;                                     // (no barrier below)
  int n = s;
  if (p.perm) {
    n = p.perm[(size_t)b * Ns + s];
    n = (unsigned)n < (unsigned)Ns ? n : s;                // (always in range: the scatter wrote every slot)
  }
  const float* __restrict__ sx = p.src + (size_t)b * 3 * Ns;
  const float x = sx[n], y = sx[Ns + n], z = sx[2 * (size_t)Ns + n];
  float px = x, py = y, pz = z;
  if (p.R) {                                               // nn_scan_kernel's expression, bit for bit
    const float* __restrict__ r = p.R + (size_t)b * 9;
    const float* __restrict__ tr = p.t + (size_t)b * 3;
    px = fmaf(r[2], z, fmaf(r[1], y, r[0] * x)) + tr[0];
    py = fmaf(r[5], z, fmaf(r[4], y, r[3] * x)) + tr[1];
    pz = fmaf(r[8], z, fmaf(r[7], y, r[6] * x)) + tr[2];
  }
  const float inf = __builtin_huge_valf();
  const float cap2 = p.cap2;
  u64 best = (u64)GD_INF << 32 | 0xFFFFFFFFu;             // (+inf, -1)

  if (gd_finite(px, py, pz)) {
    const GdGrid g = p.grid[b];
    const float xq[3] = {px, py, pz};
    // what no target point can undercut: the distance to the target's box, per axis one subtraction, the largest square
    float out = 0.f;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float o = xq[c] < g.lo[c] ? g.lo[c] - xq[c] : xq[c] > g.hi[c] ? xq[c] - g.hi[c] : 0.f;
      out = fmaxf(out, o * o);
    }
    if (out <= cap2 && out < inf) {
      const float4* __restrict__ sorted = p.sorted + (size_t)b * Nt;
      const int* __restrict__ start = p.counter + (size_t)b * p.gstride; // cell c: sorted[start[c] ... start[c + 1])
      const int cx = gd_cell(px, g.lo[0], g.h, g.inv, g.n[0]);           // clamped into the grid: below lo cell 0, above n - 1
      const int cy = gd_cell(py, g.lo[1], g.h, g.inv, g.n[1]);
      const int cz = gd_cell(pz, g.lo[2], g.h, g.inv, g.n[2]);
      auto run = [&](int a0, int a1) { gn_run(sorted, a0, a1, Nt, px, py, pz, best); };
      // What no point behind ring r can undercut is never less than the outside bound.  The walk stops STRICTLY below the bound:
      // a tie behind the ring with a lower index could still win.  STRICTLY above the cap: nothing unseen is an inlier.  +inf: no
      // side is left (the grid is exhausted), or nothing behind it is a candidate
      auto stop = [&](float bound) {
        bound = fmaxf(bound, out);
        return __uint_as_float((uint32_t)(best >> 32)) < bound || bound > cap2 || bound == inf;
      };
      gd_walk(g, start, cx, cy, cz, xq, GdSquare{}, run, stop);
    }
  }
  const float d2 = __uint_as_float((uint32_t)(best >> 32));
  const bool in = d2 <= cap2;                              // a candidate beyond the cap was seen, not found: (-1, +inf)
  const size_t o = (size_t)b * Ns + n;
  p.part_d2[o] = in ? d2 : inf;
  p.part_idx[o] = in ? (int)(uint32_t)best : -1;
}

}  // namespace

// order = 0, per family -- the one place that decides it.  Measured (profiles/gridnn_bench.txt part a):
// the source's permutation costs about what the target's grid costs (0.08 ms at 16 x 16 384, 0.26 ms at 1 x 131 072), and a
// search in cell order gains 0 (uniform, 1 x 131 072) to 0.044 ms (a sphere's surface, 16 x 16 384) on one in index order.  So
// the ONE search of an evaluation never pays it back where the grid is worth taking (index order wins at every uniform and
// surface shape, by 1.1 to 1.9 times), and a refinement pays it back after 2 (surface) to 7 (uniform) rounds at 16 x 16 384
// and after about 20 (surface) or never (uniform: 0.3 ms lost of 1.3) at 1 x 131 072: the plan builds it for a call that
// enqueues at least GRIDNN_ORDER_ROUNDS searches.
static int gridnn_order(int family, int searches) {
  return family == GRIDNN_REFINE && searches >= GRIDNN_ORDER_ROUNDS ? 1 : 2;
}

int gridnn_plan(const vcr_grid_nn_args* user, int family, int searches, int B, int Ns, int Nt, GridNnPlan* p) {
  *p = GridNnPlan{};
  vcr_grid_nn_args g;
  if (vcr_take_args(user, &g, sizeof(vcr_grid_nn_args))) return VCR_EINVAL;
  if (!gd_cell_ok(g.cell)) return VCR_EINVAL;
  if (g.order < 0 || g.order > 2) return VCR_EINVAL;
  p->B = B; p->Ns = Ns; p->Nt = Nt;
  p->cell = g.cell;
  p->order = g.order ? g.order : gridnn_order(family, searches);
  p->cells = VCR_GRID_CELLS(Nt);
  p->src_off = gd_layout(B, Nt).bytes;
  p->bytes = p->src_off + (p->order == 1 ? gd_layout(B, Ns).bytes : 0);
  return VCR_OK;
}

int gridnn_build(const GridNnPlan& p, const float* src, const float* tgt, void* area, hipStream_t s) {
  unsigned char* w = reinterpret_cast<unsigned char*>(area);
  int e = gd_build(tgt, p.B, p.Nt, p.cell, gd_layout(p.B, p.Nt), w, s);
  if (e || p.order != 1) return e;
  // the source in its own frame, on its automatic grid: only the order of its cells is kept, in the place of cellof
  const GdLayout ls = gd_layout(p.B, p.Ns);
  unsigned char* ws = w + p.src_off;
  if ((e = gd_build(src, p.B, p.Ns, 0.f, ls, ws, s))) return e;
  const long total = (long)p.B * p.Ns;
  hipLaunchKernelGGL(grid_perm_kernel, dim3((unsigned)((total + GD_BLOCK - 1) / GD_BLOCK)), dim3(GD_BLOCK), 0, s,
                     reinterpret_cast<const float4*>(ws + ls.sorted_off), reinterpret_cast<int*>(ws + ls.cellof_off), total);
  return VCR_LAUNCH_RC();
}

int gridnn_search(const GridNnPlan& p, const float* src, const float* R, const float* t, float cap2, const void* area,
                  float* part_d2, int* part_idx, const int* live, hipStream_t s) {
  const unsigned char* w = reinterpret_cast<const unsigned char*>(area);
  const GdLayout lt = gd_layout(p.B, p.Nt), ls = gd_layout(p.B, p.Ns);
  const int nblk = (p.Ns + GD_BLOCK - 1) / GD_BLOCK;
  const GnSearch sr{src, R, t, reinterpret_cast<const GdGrid*>(w), reinterpret_cast<const int*>(w + lt.counter_off),
                    reinterpret_cast<const float4*>(w + lt.sorted_off),
                    p.order == 1 ? reinterpret_cast<const int*>(w + p.src_off + ls.cellof_off) : nullptr,
                    p.Ns, p.Nt, nblk, lt.gstride, cap2, part_d2, part_idx, live};
  hipLaunchKernelGGL(grid_nn_kernel, dim3((unsigned)((long)p.B * nblk)), dim3(GD_BLOCK), 0, s, sr);
  return VCR_LAUNCH_RC();
}

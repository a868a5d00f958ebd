// The uniform grid of one cloud and the five launches that build it (DESIGN sections 4.19, 4.20), written once for grid.hip
// (vcr_grid_knn_f32: the cloud is searched against itself) and gridnn.hip (the capped nearest neighbour across two clouds: the
// TARGET's grid is searched, the SOURCE's is built for its cell order alone):
//   grid_bounds_kernel   one workgroup per cloud: min and max over the finite points (voxel_bounds_kernel's loop), then one
//                        thread chooses the edge and the cells per axis under the budget G(N)
//   grid_clear_kernel    the cloud's counters: a zero in front, one per cell, one for the points that are not finite
//   grid_count_kernel    one lane per point: its cell by comparison against the faces (a first guess from a multiply, then the
//                        fix-up), kept per point; one int32 atomicAdd on the cell's counter
//   grid_scan_kernel     one workgroup per cloud: the counters become their exclusive scan (wg_offsets): cell c starts at
//                        counter[1 + c]
//   grid_scatter_kernel  one lane per point: slot = atomicAdd(counter[1 + cell], 1); (x, y, z, index) goes to sorted[slot].
//                        Afterwards counter[1 + c] is cell c's END, so cell c is sorted[counter[c] ... counter[c + 1]) with the
//                        zero in front.  The order inside a cell follows the atomics and may differ between runs; every
//                        selection behind it is on (d2, j), so nothing returned depends on it
#pragma once
#include "seg_scan.h"
#include "../../include/vcr_hip_grid.h"

namespace {

typedef unsigned long long u64;

constexpr int GD_BLOCK = VCR_GRID_QUERIES;
static_assert(GD_BLOCK == WG_BLOCK, "wg_scan.h serves workgroups of this size");
constexpr uint32_t GD_INF = 0x7F800000u;
constexpr float GD_FLT_MAX = 3.402823466e+38f, GD_FLT_MIN = 1.175494351e-38f;

// one per cloud; hi is read by the search across two clouds alone (its outside bound)
struct GdGrid { float lo[3]; float h; float inv; int n[3]; int cells; float hi[3]; int pad[4]; };
static_assert(sizeof(GdGrid) == 64, "workspace layout");

__device__ __forceinline__ bool gd_finite(float x, float y, float z) {
  const float inf = __builtin_huge_valf();
  return fabsf(x) < inf && fabsf(y) < inf && fabsf(z) < inf;
}

__device__ __forceinline__ float gd_face(int j, float h, float lo) { return fmaf((float)j, h, lo); }

// The cell of x along one axis: the largest j in [0, n) with face[j] <= x (the faces are monotone in j); an x below lo = face[0]
// is in cell 0.  The multiply only guesses -- clamped as a float, so no guess overflows the conversion --; the comparisons decide.
__device__ __forceinline__ int gd_cell(float x, float lo, float h, float inv, int n) {
  const float g = (x - lo) * inv;
  int j = g >= 0.f ? (g < (float)n ? (int)g : n - 1) : 0;                 // (a NaN guess starts at 0)
  for (int it = 0; it < n && j > 0 && gd_face(j, h, lo) > x; ++it) --j;
  for (int it = 0; it < n && j < n - 1 && gd_face(j + 1, h, lo) <= x; ++it) ++j;
  return j;
}

__global__ __launch_bounds__(GD_BLOCK) void grid_bounds_kernel(const float* xyz, int N, float cell, GdGrid* grid) {
  __shared__ float wlo[3][WG_WAVES], whi[3][WG_WAVES];
  const int t = threadIdx.x, b = blockIdx.x;
  const float* __restrict__ x = xyz + (size_t)b * 3 * N;
  const float inf = __builtin_huge_valf();
  float lo[3] = {inf, inf, inf}, hi[3] = {-inf, -inf, -inf};
#pragma unroll 4
  for (int i = t; i < N; i += GD_BLOCK) {
    const float v[3] = {x[i], x[N + i], x[2 * (size_t)N + i]};
    const bool ok = gd_finite(v[0], v[1], v[2]);
#pragma unroll
    for (int c = 0; c < 3; ++c) { lo[c] = ok ? fminf(lo[c], v[c]) : lo[c]; hi[c] = ok ? fmaxf(hi[c], v[c]) : hi[c]; }
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) { lo[c] = fminf(lo[c], __shfl_xor(lo[c], o, 64)); hi[c] = fmaxf(hi[c], __shfl_xor(hi[c], o, 64)); }
    if ((t & 63) == 0) { wlo[c][t >> 6] = lo[c]; whi[c][t >> 6] = hi[c]; }
  }
  __syncthreads();
  if (t == 0) {
    GdGrid g{};
    float e[3];
    int flat = 0;
    double vol = 1.;
    for (int c = 0; c < 3; ++c) {
      float l = wlo[c][0], u = whi[c][0];
      for (int w = 1; w < WG_WAVES; ++w) { l = fminf(l, wlo[c][w]); u = fmaxf(u, whi[c][w]); }
      if (!(l <= u)) l = u = 0.f;                          // a cloud without a finite point: one cell, nobody in it
      g.lo[c] = l;
      g.hi[c] = u;
      e[c] = fminf(u - l, GD_FLT_MAX);                     // (an extent that overflows fp32 counts as the largest finite one)
      if (e[c] > 0.f) vol *= (double)e[c]; else ++flat;
    }
    float h = cell;
    if (!(h > 0.f)) {                                      // the automatic grid: one point a cell of the bounding box
      const double per = vol / (double)N;
      h = flat == 3 ? 1.f : (float)(flat == 0 ? cbrt(per) : flat == 1 ? sqrt(per) : per);
    }
    h = fminf(fmaxf(h, GD_FLT_MIN), GD_FLT_MAX);
    const long budget = VCR_GRID_CELLS((long)N);
    int n[3] = {1, 1, 1};
    for (int it = 0; it < 1024; ++it) {                    // (1.25^1024 spans fp32: at the largest h every n_c is 1 or 2)
      long cells = 1;
      for (int c = 0; c < 3; ++c) {
        const float q = e[c] / h;
        n[c] = q < 1048575.f ? (int)q + 1 : 1 << 20;          // (2^20 cells along an axis never fit)
        cells *= n[c];
      }
      if (cells <= budget) break;
      n[0] = n[1] = n[2] = 1;
      h = fminf(h * 1.25f, GD_FLT_MAX);
    }
    g.h = h;
    g.inv = 1.f / h;
    for (int c = 0; c < 3; ++c) g.n[c] = n[c];
    g.cells = n[0] * n[1] * n[2];                          // <= G(N)
    grid[b] = g;
  }
}

// counter [B][gstride]: gstride = G(N) + 2
__global__ __launch_bounds__(GD_BLOCK) void grid_clear_kernel(const GdGrid* grid, int* counter, int gstride, int per_cloud) {
  const int b = (int)(blockIdx.x / (unsigned)per_cloud), blk = (int)(blockIdx.x % (unsigned)per_cloud);
  const int used = grid[b].cells + 2;                      // <= gstride
  for (int i = blk * GD_BLOCK + (int)threadIdx.x; i < used && i < gstride; i += per_cloud * GD_BLOCK)
    counter[(size_t)b * gstride + i] = 0;
}

struct GdPoints { const float* xyz; const GdGrid* grid; int* cellof; int* counter; float4* sorted; int N, nblk, gstride; };

__global__ __launch_bounds__(GD_BLOCK) void grid_count_kernel(GdPoints p) {
  const int b = (int)(blockIdx.x / (unsigned)p.nblk), blk = (int)(blockIdx.x % (unsigned)p.nblk);
  const int i = blk * GD_BLOCK + (int)threadIdx.x, N = p.N;
  if (i >= N) return;
  const float* __restrict__ x = p.xyz + (size_t)b * 3 * N;
  const GdGrid g = p.grid[b];
  const float v[3] = {x[i], x[N + i], x[2 * (size_t)N + i]};
  int cell = g.cells;                                      // the points that are not finite: behind the last cell
  if (gd_finite(v[0], v[1], v[2])) {
    const int cx = gd_cell(v[0], g.lo[0], g.h, g.inv, g.n[0]);
    const int cy = gd_cell(v[1], g.lo[1], g.h, g.inv, g.n[1]);
    const int cz = gd_cell(v[2], g.lo[2], g.h, g.inv, g.n[2]);
    cell = (cz * g.n[1] + cy) * g.n[0] + cx;
  }
  p.cellof[(size_t)b * N + i] = cell;
  atomicAdd(p.counter + (size_t)b * p.gstride + 1 + cell, 1);
}

__global__ __launch_bounds__(GD_BLOCK) void grid_scan_kernel(const GdGrid* grid, int* counter, int gstride) {
  __shared__ int wtot[WG_WAVES];
  const int b = blockIdx.x;
  int used = grid[b].cells + 1;
  used = used < gstride - 1 ? used : gstride - 1;
  wg_offsets(counter + (size_t)b * gstride + 1, used, wtot);
}

__global__ __launch_bounds__(GD_BLOCK) void grid_scatter_kernel(GdPoints p) {
  const int b = (int)(blockIdx.x / (unsigned)p.nblk), blk = (int)(blockIdx.x % (unsigned)p.nblk);
  const int i = blk * GD_BLOCK + (int)threadIdx.x, N = p.N;
  if (i >= N) return;
  const float* __restrict__ x = p.xyz + (size_t)b * 3 * N;
  const int cell = p.cellof[(size_t)b * N + i];
  const int slot = atomicAdd(p.counter + (size_t)b * p.gstride + 1 + cell, 1);
  if ((unsigned)slot < (unsigned)N)                        // (always: the counts add up to N)
    p.sorted[(size_t)b * N + slot] = make_float4(x[i], x[N + i], x[2 * (size_t)N + i], __int_as_float(i));
}

// One cloud set's grid in the workspace: per cloud the grid | per point its cell | per cloud a zero, a counter per cell and one
// for the points that are not finite | per point its (x, y, z, index) in cell order
struct GdLayout { int nblk, gstride; size_t cellof_off, counter_off, sorted_off, bytes; };

}  // namespace

static inline GdLayout gd_layout(int B, int N) {
  GdLayout l{};
  l.nblk = (N + GD_BLOCK - 1) / GD_BLOCK;
  l.gstride = VCR_GRID_CELLS(N) + 2;
  const size_t BN = (size_t)B * N;
  l.cellof_off = ws_up((size_t)B * sizeof(GdGrid));
  l.counter_off = l.cellof_off + ws_up(BN * 4);
  l.sorted_off = l.counter_off + ws_up((size_t)B * l.gstride * 4);
  l.bytes = l.sorted_off + ws_up(BN * 16);
  return l;
}

// The five launches on xyz [B,3,N] into the layout at w
static inline int gd_build(const float* xyz, int B, int N, float cell, const GdLayout& l, unsigned char* w, hipStream_t s) {
  GdGrid* grid = reinterpret_cast<GdGrid*>(w);
  int* cellof = reinterpret_cast<int*>(w + l.cellof_off);
  int* counter = reinterpret_cast<int*>(w + l.counter_off);
  float4* sorted = reinterpret_cast<float4*>(w + l.sorted_off);
  const dim3 block(GD_BLOCK), clouds((unsigned)B), points((unsigned)((long)B * l.nblk));
  const int clear_x = (l.gstride + GD_BLOCK - 1) / GD_BLOCK < 64 ? (l.gstride + GD_BLOCK - 1) / GD_BLOCK : 64;
  int e;
  hipLaunchKernelGGL(grid_bounds_kernel, clouds, block, 0, s, xyz, N, cell, grid);
  if ((e = VCR_LAUNCH_RC())) return e;
  hipLaunchKernelGGL(grid_clear_kernel, dim3((unsigned)((long)B * clear_x)), block, 0, s, grid, counter, l.gstride, clear_x);
  if ((e = VCR_LAUNCH_RC())) return e;
  const GdPoints pt{xyz, grid, cellof, counter, sorted, N, l.nblk, l.gstride};
  hipLaunchKernelGGL(grid_count_kernel, points, block, 0, s, pt);
  if ((e = VCR_LAUNCH_RC())) return e;
  hipLaunchKernelGGL(grid_scan_kernel, clouds, block, 0, s, grid, counter, l.gstride);
  if ((e = VCR_LAUNCH_RC())) return e;
  hipLaunchKernelGGL(grid_scatter_kernel, points, block, 0, s, pt);
  return VCR_LAUNCH_RC();
}

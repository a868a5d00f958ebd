// The exact k nearest neighbours of every point among its cloud's other points, searched on a uniform grid
// (include/vcr_hip_grid.h).  The result is the header's definition -- the k smallest (d2, j) with d2 in
// difference form -- and nothing of the grid shows in it: the cells only decide which candidates are looked at, and the walk
// stops only where an fp32 lower bound proves that no point behind it can enter the row.
//
// Six launches:
//   grid_bounds_kernel   one workgroup per cloud: min and max over the finite points (voxel_bounds_kernel's loop), then one
//                        thread chooses the edge and the cells per axis under the budget G(N)
//   grid_clear_kernel    the cloud's counters: a zero in front, one per cell, one for the points that are not finite
//   grid_count_kernel    one lane per point: its cell by comparison against the faces (a first guess from a multiply, then the
//                        fix-up), kept per point; one int32 atomicAdd on the cell's counter
//   grid_scan_kernel     one workgroup per cloud: the counters become their exclusive scan (wg_offsets): cell c starts at
//                        counter[1 + c]
//   grid_scatter_kernel  one lane per point: slot = atomicAdd(counter[1 + cell], 1); (x, y, z, index) goes to sorted[slot].
//                        Afterwards counter[1 + c] is cell c's END, so cell c is sorted[counter[c] ... counter[c + 1]) with the
//                        zero in front.  The order inside a cell follows the atomics and may differ between runs; the
//                        selection is on (d2, j), so nothing returned depends on it
//   grid_search_kernel   one lane per query, the queries in cell order (a wave's lanes walk the same cells and load the same
//                        candidates).  The row is a lane-private column of k 64-bit keys in LDS, (d2's bits) << 32 | j --
//                        d2 >= +0, so the keys order as (d2, j) -- kept ascending; a candidate is compared with the k-th key in
//                        a register first, and only one that passes is inserted.  Rings of cells: along x a ring's cells are
//                        contiguous in the sorted order, one run of candidates a (y, z) row.
// No scratch, no waits between workgroups; every loop is bounded by N, k or the cells per axis, and every run of candidates is
// clamped to [0, N).
#include "seg_scan.h"
#include "../../include/vcr_hip_grid.h"

namespace {

typedef unsigned long long u64;

constexpr int GD_BLOCK = VCR_GRID_QUERIES;
static_assert(GD_BLOCK == WG_BLOCK, "wg_scan.h serves workgroups of this size");
constexpr uint32_t GD_INF = 0x7F800000u;
constexpr float GD_FLT_MAX = 3.402823466e+38f, GD_FLT_MIN = 1.175494351e-38f;

struct GdGrid { float lo[3]; float h; float inv; int n[3]; int cells; int pad[7]; };      // one per cloud
static_assert(sizeof(GdGrid) == 64, "workspace layout");

__device__ __forceinline__ bool gd_finite(float x, float y, float z) {
  const float inf = __builtin_huge_valf();
  return fabsf(x) < inf && fabsf(y) < inf && fabsf(z) < inf;
}

__device__ __forceinline__ float gd_face(int j, float h, float lo) { return fmaf((float)j, h, lo); }

// The cell of x along one axis: the largest j in [0, n) with face[j] <= x (x >= lo = face[0]; the faces are monotone in j).
// The multiply only guesses; the comparisons decide.
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
  int nblk, gstride, by_index;
  size_t cellof_off, counter_off, sorted_off, bytes, lds;
};

}  // namespace

static int grid_plan(const vcr_grid_knn_args& a, GdPlan* p) {
  *p = GdPlan{a};
  if (!a.xyz || !a.idx || a.B < 1) return VCR_EINVAL;
  if (!(a.cell >= 0.f) || a.cell == __builtin_huge_valf()) return VCR_EINVAL;           // negative, NaN, +inf
  if (a.variant < 0 || a.variant > 2) return VCR_EINVAL;
  if (a.N < 1 || a.N > VCR_GRID_MAX_N || (long)a.B * a.N >= (1L << 31)) return VCR_EUNSUPPORTED;
  if (a.k < 1 || a.k > VCR_GRID_MAX_K) return VCR_EUNSUPPORTED;
  p->nblk = (a.N + GD_BLOCK - 1) / GD_BLOCK;
  p->gstride = VCR_GRID_CELLS(a.N) + 2;
  p->by_index = a.variant == 2;
  const size_t BN = (size_t)a.B * a.N;
  p->cellof_off = ws_up((size_t)a.B * sizeof(GdGrid));
  p->counter_off = p->cellof_off + ws_up(BN * 4);
  p->sorted_off = p->counter_off + ws_up((size_t)a.B * p->gstride * 4);
  p->bytes = p->sorted_off + ws_up(BN * 16);
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
  if (cells_per_cloud) *cells_per_cloud = p.gstride - 2;
  if (queries_per_workgroup) *queries_per_workgroup = GD_BLOCK;
  return VCR_OK;
}

extern "C" size_t vcr_grid_knn_workspace_bytes(const vcr_grid_knn_args* ua, int cu_count) {
  vcr_grid_knn_args a;
  GdPlan p;
  if (grid_take(ua, &a) || cu_count < 0) return 0;
  return grid_plan(a, &p) ? 0 : p.bytes;
}

extern "C" int vcr_grid_knn_f32(const vcr_grid_knn_args* ua, void* workspace, size_t workspace_bytes, vcr_stream_t stream) {
  vcr_grid_knn_args a;
  if (grid_take(ua, &a)) return VCR_EINVAL;
  GdPlan p;
  int e = grid_plan(a, &p);
  if (e) return e;
  if (!workspace || (((uintptr_t)workspace) & 15)) return VCR_EINVAL;
  if (workspace_bytes < p.bytes) return VCR_EWORKSPACE;
  vcr_stream_scope scope_(stream);
  hipStream_t s = (hipStream_t)stream;
  unsigned char* w = reinterpret_cast<unsigned char*>(workspace);
  GdGrid* grid = reinterpret_cast<GdGrid*>(w);
  int* cellof = reinterpret_cast<int*>(w + p.cellof_off);
  int* counter = reinterpret_cast<int*>(w + p.counter_off);
  float4* sorted = reinterpret_cast<float4*>(w + p.sorted_off);
  const dim3 block(GD_BLOCK), clouds((unsigned)a.B), points((unsigned)((long)a.B * p.nblk));
  const int clear_x = (p.gstride + GD_BLOCK - 1) / GD_BLOCK < 64 ? (p.gstride + GD_BLOCK - 1) / GD_BLOCK : 64;

  hipLaunchKernelGGL(grid_bounds_kernel, clouds, block, 0, s, a.xyz, a.N, a.cell, grid);
  if ((e = VCR_LAUNCH_RC())) return e;
  hipLaunchKernelGGL(grid_clear_kernel, dim3((unsigned)((long)a.B * clear_x)), block, 0, s, grid, counter, p.gstride, clear_x);
  if ((e = VCR_LAUNCH_RC())) return e;
  const GdPoints pt{a.xyz, grid, cellof, counter, sorted, a.N, p.nblk, p.gstride};
  hipLaunchKernelGGL(grid_count_kernel, points, block, 0, s, pt);
  if ((e = VCR_LAUNCH_RC())) return e;
  hipLaunchKernelGGL(grid_scan_kernel, clouds, block, 0, s, grid, counter, p.gstride);
  if ((e = VCR_LAUNCH_RC())) return e;
  hipLaunchKernelGGL(grid_scatter_kernel, points, block, 0, s, pt);
  if ((e = VCR_LAUNCH_RC())) return e;
  const GdSearch sr{a.xyz, grid, cellof, counter, sorted, a.N, a.k, p.nblk, p.gstride, p.by_index, a.idx, a.d2};
  return vcr_launch<grid_search_kernel>(points, block, p.lds, s, sr);
}

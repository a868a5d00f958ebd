// All points within a radius of every point of a cloud, searched on the cloud's uniform grid (include/vcr_hip_radius.h, DESIGN
// section 4.22): rows of varying length in CSR form, and the radius outlier filter on the same count.  The result is the
// header's definition -- every hit (d2 <= r2, j != i), ascending in (d2, j) -- and nothing of the grid shows in it: the cells only
// decide which candidates are looked at, and the walk stops only where section 4.19's fp32 bound proves that no point behind
// the ring can be a hit (bound > r2, strictly).
//
// vcr_grid_radius_f32: the five launches of grid_build.h (the edge is the radius unless forced), then
//   radius_count_kernel       one lane per query, the queries in cell order: the walk, n_i to count[b, i]
//   radius_offsets_kernel     one workgroup per cloud: the 64-bit exclusive scan of the counts (wg_offsets64) to row_start, total
// and with idx, for the clouds that fit (total[b] <= capacity)
//   radius_fill_kernel        the same walk: lane i appends its hits' keys (d2 bits) << 32 | j to its private segment of the
//                             scratch row, at row_start[b, i], clamped to n_i entries; no atomics.  The order inside a segment
//                             follows the cells and the scatter's atomics and is not defined
//   radius_order_kernel       a rank sort out of the scratch: a row's keys are distinct, so rank(e) = #{keys < key_e} is a
//   radius_order_lane_kernel  permutation, and idx / d2 are written at row_start + rank: no atomics, no in-place hazard, any row
//                             length.  The first: a wave (a workgroup of 64 lanes) per row, the keys staged through LDS in
//                             chunks of RD_CHUNK, 64 elements ranked a pass.  The second: a lane per row; it lost every
//                             measurement, so rd_order_form(), the one place that decides, never takes it
//   radius_pad_kernel         -1 / +inf behind total[b], and over the clouds that do not fit
// vcr_outlier_radius_grid_f32: the grid, radius_count_kernel writing c_i = n_i + 1 (0 for a point that is not finite), then
// outlier_tail.h's mark, offsets and write -- vcr_outlier_radius_f32's own tail.
// The ring enumeration is written once, rd_walk, for the two kernels that walk.  No scratch memory, no waits between
// workgroups; every loop is bounded by N, a row's length or the cells per axis; every run of candidates is clamped to [0, N),
// every write to its row.
#include "grid_build.h"
#include "outlier_tail.h"
#include "../../include/vcr_hip_radius.h"

namespace {

constexpr int RD_CHUNK = VCR_RADIUS_CHUNK;                 // keys of a row in LDS at a time (the wave-per-row form)
constexpr int RD_WAVE = 64;
static_assert(RD_CHUNK % RD_WAVE == 0, "a wave stages a chunk in whole passes");
static_assert(GD_BLOCK == NN_BLOCK, "outlier_tail.h's kernels run on the grid's point launches");

// what the two walking kernels share: the cloud, its grid and the order the queries are served in
struct RdWalk {
  const float* xyz; const GdGrid* grid; const int* cellof; const int* counter; const float4* sorted;
  int N, nblk, gstride, by_index;
  float r2;
};

// One run sorted[a0 ... a1) of candidates against the lane's query: hit(key) for every j != qi with d2 <= r2 (a NaN or an
// overflowed d2 is no hit: r2 is finite)
template <class Hit>
__device__ __forceinline__ void rd_run(const float4* __restrict__ sorted, int a0, int a1, int N, float qx, float qy, float qz,
                                       int qi, float r2, Hit& hit) {
  a0 = a0 > 0 ? a0 : 0;
  a1 = a1 < N ? a1 : N;
  for (int s = a0; s < a1; ++s) {
    const float4 c = sorted[s];
    const int j = __float_as_int(c.w);
    const float dx = c.x - qx, dy = c.y - qy, dz = c.z - qz;
    const float d2 = fmaf(dz, dz, fmaf(dy, dy, dx * dx));
    if (j != qi && d2 <= r2) hit((u64)__float_as_uint(d2) << 32 | (uint32_t)j);
  }
}

// The lane's query: lane s of cloud b takes the s-th point in cell order (or point s in index order)
struct RdQuery { float x, y, z; int i, cell; bool ok; };   // ok: the point is finite, so it has a cell

__device__ __forceinline__ RdQuery rd_query(const RdWalk& p, int b, int s) {
  const int N = p.N;
  RdQuery q;
  if (p.by_index) {
    const float* __restrict__ x = p.xyz + (size_t)b * 3 * N;
    q.i = s; q.x = x[s]; q.y = x[N + s]; q.z = x[2 * (size_t)N + s];
  } else {
    const float4 v = p.sorted[(size_t)b * N + s];
    q.x = v.x; q.y = v.y; q.z = v.z; q.i = __float_as_int(v.w);
    q.i = (unsigned)q.i < (unsigned)N ? q.i : 0;           // (always in range: the scatter wrote every slot)
  }
  q.cell = p.cellof[(size_t)b * N + q.i];
  q.ok = q.cell >= 0 && q.cell < p.grid[b].cells;
  return q;
}

// The rings around the query's cell: section 4.19's enumeration (one run a (y, z) row of the shell, two end cells inside it)
// and its ring bound; the walk stops after ring r when bound > r2, STRICTLY, or when the grid is exhausted (no side is left:
// the bound is +inf).  A query without a cell walks nothing.
template <class Hit>
__device__ __forceinline__ void rd_walk(const RdWalk& p, int b, const RdQuery& qq, Hit& hit) {
  if (!qq.ok) return;
  const int N = p.N;
  const GdGrid g = p.grid[b];
  const float4* __restrict__ sorted = p.sorted + (size_t)b * N;
  const int* __restrict__ start = p.counter + (size_t)b * p.gstride;     // cell c: sorted[start[c] ... start[c + 1])
  const float qx = qq.x, qy = qq.y, qz = qq.z;
  const int qi = qq.i, cell = qq.cell;
  const float r2 = p.r2;
  const int nx = g.n[0], ny = g.n[1], nz = g.n[2];
  const int cx = cell % nx, cy = (cell / nx) % ny, cz = cell / (nx * ny);
  int rmax = cx > nx - 1 - cx ? cx : nx - 1 - cx;
  rmax = cy > rmax ? cy : rmax; rmax = ny - 1 - cy > rmax ? ny - 1 - cy : rmax;
  rmax = cz > rmax ? cz : rmax; rmax = nz - 1 - cz > rmax ? nz - 1 - cz : rmax;
  const int q[3] = {cx, cy, cz};
  const float xq[3] = {qx, qy, qz};
  for (int r = 0; r <= rmax; ++r) {                        // (bounded by the cells per axis)
    const int z0 = cz - r > 0 ? cz - r : 0, z1 = cz + r < nz - 1 ? cz + r : nz - 1;
    const int y0 = cy - r > 0 ? cy - r : 0, y1 = cy + r < ny - 1 ? cy + r : ny - 1;
    const int x0 = cx - r > 0 ? cx - r : 0, x1 = cx + r < nx - 1 ? cx + r : nx - 1;
    for (int z = z0; z <= z1; ++z)
      for (int y = y0; y <= y1; ++y) {
        const int row = (z * ny + y) * nx;
        const bool shell = z - cz == r || cz - z == r || y - cy == r || cy - y == r;
        if (shell) {                                       // the whole x range of the ring: one run
          rd_run(sorted, start[row + x0], start[row + x1 + 1], N, qx, qy, qz, qi, r2, hit);
        } else {                                           // its two end cells
          if (cx - r >= 0) rd_run(sorted, start[row + cx - r], start[row + cx - r + 1], N, qx, qy, qz, qi, r2, hit);
          if (cx + r <= nx - 1) rd_run(sorted, start[row + cx + r], start[row + cx + r + 1], N, qx, qy, qz, qi, r2, hit);
        }
      }
    // what no point behind ring r can undercut: per side that exists one subtraction, the smallest square
    float bound = __builtin_huge_valf();
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      if (q[c] + r + 1 <= g.n[c] - 1) { const float d = gd_face(q[c] + r + 1, g.h, g.lo[c]) - xq[c]; bound = fminf(bound, d * d); }
      if (q[c] - r >= 1) { const float d = xq[c] - gd_face(q[c] - r, g.h, g.lo[c]); bound = fminf(bound, d * d); }
    }
    if (bound > r2) break;                                 // STRICTLY above: an unseen point at exactly r2 is a hit
  }
}

// self: what a finite point adds for itself (0: n_i, the search's count; 1: c_i, the filter's).  out1 is optional
struct RdCount { RdWalk w; int self; int* out0; int* out1; };

__global__ __launch_bounds__(GD_BLOCK) void radius_count_kernel(RdCount p) {
  const int b = (int)(blockIdx.x / (unsigned)p.w.nblk), blk = (int)(blockIdx.x % (unsigned)p.w.nblk);
  const int s = blk * GD_BLOCK + (int)threadIdx.x;
  if (s >= p.w.N) return;                                  // (no barrier below)
  const RdQuery q = rd_query(p.w, b, s);
  int n = 0;
  auto hit = [&](u64) { ++n; };
  rd_walk(p.w, b, q, hit);
  const int c = q.ok ? n + p.self : 0;
  const size_t o = (size_t)b * p.w.N + q.i;
  p.out0[o] = c;
  if (p.out1) p.out1[o] = c;
}

__global__ __launch_bounds__(GD_BLOCK) void radius_offsets_kernel(const int* count, long long* row_start, long long* total, int N) {
  __shared__ long long wtot[WG_WAVES];
  const int b = blockIdx.x;
  long long* rs = row_start + (size_t)b * ((size_t)N + 1);
  const long long all = wg_offsets64(count + (size_t)b * N, rs, N, wtot);
  if (threadIdx.x == 0) { rs[N] = all; total[b] = all; }
}

// row_start [B][N + 1]; scratch [B][capacity]: a cloud's unordered keys, row i at row_start[b, i]
struct RdFill { RdWalk w; const long long* row_start; int capacity; u64* scratch; };

__global__ __launch_bounds__(GD_BLOCK) void radius_fill_kernel(RdFill p) {
  const int b = (int)(blockIdx.x / (unsigned)p.w.nblk), blk = (int)(blockIdx.x % (unsigned)p.w.nblk);
  const int s = blk * GD_BLOCK + (int)threadIdx.x, N = p.w.N;
  const long long* __restrict__ rs = p.row_start + (size_t)b * ((size_t)N + 1);
  if (s >= N || rs[N] > (long long)p.capacity) return;     // (no barrier below; a cloud that does not fit: the pad writes it)
  const RdQuery q = rd_query(p.w, b, s);
  const long long at = rs[q.i];
  const long long len = rs[q.i + 1] - at, left = (long long)p.capacity - at;
  const long long room = len < left ? len : left;          // the lane's segment, clamped to the row and to the cloud's slots
  if (at < 0 || room <= 0) return;
  u64* __restrict__ row = p.scratch + (size_t)b * p.capacity + (size_t)at;
  int w = 0;
  auto hit = [&](u64 key) { if (w < room) row[w] = key; ++w; };
  rd_walk(p.w, b, q, hit);
}

struct RdOrder { const long long* row_start; const u64* scratch; int N, capacity; int* idx; float* d2; };

// One workgroup of ONE wave per row: 64 elements are ranked a pass against the whole row, which passes through LDS in chunks
__global__ __launch_bounds__(RD_WAVE) void radius_order_kernel(RdOrder p) {
  __shared__ u64 keys[RD_CHUNK];
  const int lane = threadIdx.x, N = p.N;
  const int b = (int)(blockIdx.x / (unsigned)N), i = (int)(blockIdx.x % (unsigned)N);
  const long long* __restrict__ rs = p.row_start + (size_t)b * ((size_t)N + 1);
  if (rs[N] > (long long)p.capacity) return;               // (workgroup-uniform)
  const long long at = rs[i];
  long long len = rs[i + 1] - at;
  len = len < (long long)p.capacity - at ? len : (long long)p.capacity - at;
  if (at < 0 || len <= 0) return;                          // (workgroup-uniform)
  const int n = (int)len;                                  // <= N
  const size_t base = (size_t)b * p.capacity + (size_t)at;
  const u64* __restrict__ row = p.scratch + base;
  for (int e0 = 0; e0 < n; e0 += RD_WAVE) {                // (workgroup-uniform: bounded by the row's length)
    const int e = e0 + lane;
    const u64 key = e < n ? row[e] : ~0ull;
    int rank = 0;
    for (int c0 = 0; c0 < n; c0 += RD_CHUNK) {
      const int m = n - c0 < RD_CHUNK ? n - c0 : RD_CHUNK;
      __syncthreads();                                     // the previous chunk has been read
      for (int f = lane; f < m; f += RD_WAVE) keys[f] = row[c0 + f];
      __syncthreads();
      for (int f = 0; f < m; ++f) rank += keys[f] < key ? 1 : 0;         // one address for every lane: broadcast reads
    }
    if (e < n && rank < n) {                               // (rank < n always: the keys are distinct)
      p.idx[base + rank] = (int)(uint32_t)key;
      if (p.d2) p.d2[base + rank] = __uint_as_float((uint32_t)(key >> 32));
    }
  }
}

// One lane per row, the rows in index order (neighbouring lanes read neighbouring segments): every key against every key
__global__ __launch_bounds__(GD_BLOCK) void radius_order_lane_kernel(RdOrder p, int nblk) {
  const int b = (int)(blockIdx.x / (unsigned)nblk), blk = (int)(blockIdx.x % (unsigned)nblk);
  const int i = blk * GD_BLOCK + (int)threadIdx.x, N = p.N;
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

__global__ __launch_bounds__(GD_BLOCK) void radius_pad_kernel(const long long* row_start, int N, int capacity, int per_cloud,
                                                              int* idx, float* d2) {
  const int b = (int)(blockIdx.x / (unsigned)per_cloud), blk = (int)(blockIdx.x % (unsigned)per_cloud);
  const long long all = row_start[(size_t)b * ((size_t)N + 1) + N];
  const int from = all >= 0 && all <= (long long)capacity ? (int)all : 0;           // a cloud that does not fit: every slot
  const size_t base = (size_t)b * capacity;
  for (long long s = (long long)from + blk * GD_BLOCK + (int)threadIdx.x; s < capacity; s += (long long)per_cloud * GD_BLOCK) {
    idx[base + s] = -1;
    if (d2) d2[base + s] = __builtin_huge_valf();
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

static bool rd_radius_ok(float radius, float* r2) {
  if (!(radius > 0.f) || radius == __builtin_huge_valf()) return false;                   // <= 0, NaN, +inf
  *r2 = radius * radius;                                   // fp32, one rounding
  return *r2 < __builtin_huge_valf();
}

static int radius_plan(const vcr_grid_radius_args& a, RdPlan* p) {
  *p = RdPlan{a};
  if (!a.xyz || !a.count || !a.row_start || !a.total || a.B < 1) return VCR_EINVAL;
  if (!rd_radius_ok(a.radius, &p->r2)) return VCR_EINVAL;
  if (!(a.cell >= 0.f) || a.cell == __builtin_huge_valf()) return VCR_EINVAL;             // negative, NaN, +inf
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

static RdWalk rd_walk_args(const float* xyz, int N, const GdLayout& at, const unsigned char* w, int by_index, float r2) {
  return RdWalk{xyz, reinterpret_cast<const GdGrid*>(w), reinterpret_cast<const int*>(w + at.cellof_off),
                reinterpret_cast<const int*>(w + at.counter_off), reinterpret_cast<const float4*>(w + at.sorted_off),
                N, at.nblk, at.gstride, by_index, r2};
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
  const dim3 block(GD_BLOCK), clouds((unsigned)a.B), points((unsigned)((long)a.B * p.at.nblk));
  const RdWalk wk = rd_walk_args(a.xyz, a.N, p.at, w, p.by_index, p.r2);
  long long* row_start = reinterpret_cast<long long*>(a.row_start);
  hipLaunchKernelGGL(radius_count_kernel, points, block, 0, s, RdCount{wk, 0, a.count, nullptr});
  if ((e = VCR_LAUNCH_RC())) return e;
  hipLaunchKernelGGL(radius_offsets_kernel, clouds, block, 0, s, a.count, row_start, reinterpret_cast<long long*>(a.total), a.N);
  if ((e = VCR_LAUNCH_RC())) return e;
  if (!a.idx || a.capacity == 0) return VCR_OK;
  u64* scratch = reinterpret_cast<u64*>(w + p.scratch_off);
  hipLaunchKernelGGL(radius_fill_kernel, points, block, 0, s, RdFill{wk, row_start, a.capacity, scratch});
  if ((e = VCR_LAUNCH_RC())) return e;
  const RdOrder od{row_start, scratch, a.N, a.capacity, a.idx, a.d2};
  if (p.form == 2) hipLaunchKernelGGL(radius_order_lane_kernel, points, block, 0, s, od, p.at.nblk);
  else hipLaunchKernelGGL(radius_order_kernel, dim3((unsigned)((long)a.B * a.N)), dim3(RD_WAVE), 0, s, od);
  if ((e = VCR_LAUNCH_RC())) return e;
  const int pad_x = (a.capacity + GD_BLOCK - 1) / GD_BLOCK < 256 ? (a.capacity + GD_BLOCK - 1) / GD_BLOCK : 256;
  hipLaunchKernelGGL(radius_pad_kernel, dim3((unsigned)((long)a.B * pad_x)), block, 0, s, row_start, a.N, a.capacity, pad_x,
                     a.idx, a.d2);
  return VCR_LAUNCH_RC();
}

// ---- the radius outlier filter on the grid

static int radius_filter_plan(const vcr_outlier_radius_args* ua, const vcr_grid_nn_args* ug, RdFilterPlan* p) {
  *p = RdFilterPlan{};
  vcr_grid_nn_args g;
  if (vcr_take_args(ua, &p->a, offsetof(vcr_outlier_radius_args, index))) return VCR_EINVAL;
  if (vcr_take_args(ug, &g, sizeof(vcr_grid_nn_args))) return VCR_EINVAL;
  const vcr_outlier_radius_args& a = p->a;
  if (!a.xyz || !a.points || !a.count || a.B < 1 || a.nb_points < 0 || a.variant != 0) return VCR_EINVAL;
  if (!rd_radius_ok(a.radius, &p->r2)) return VCR_EINVAL;
  if (!(g.cell >= 0.f) || g.cell == __builtin_huge_valf()) return VCR_EINVAL;             // negative, NaN, +inf
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
                     RdCount{rd_walk_args(a.xyz, a.N, p.at, w, p.by_index, p.r2), 1, cnt, a.neighbours});
  if ((e = VCR_LAUNCH_RC())) return e;
  const OlTail tl{nullptr, nullptr, cnt, a.nb_points, nullptr, a.xyz, a.N, p.at.nblk, blk, a.points, a.count, a.index};
  hipLaunchKernelGGL(outlier_mark_kernel, points, block, 0, s, tl);
  if ((e = VCR_LAUNCH_RC())) return e;
  return ol_compact(tl, a.B, p.point_grid, s);
}

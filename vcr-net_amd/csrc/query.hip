// Neighbours of ANY query positions in a cloud, searched on the cloud's uniform grid (include/query/vcr_hip_query.h, DESIGN
// section 4.28): the k nearest points of every query, and all points within a radius of it as rows of varying length in CSR
// form.  The result is the header's definition -- (d2, j) order, d2 in difference form, no self exclusion -- and nothing of the
// grid shows in it: the cells only decide which candidates are looked at, and a walk stops only where an fp32 bound proves that
// no point behind the ring can enter the row.
//
// Once a call: grid_build.h's five launches on the POINTS; with order 1 the queries are counting-sorted by their clamped cell in
// THAT grid -- grid_build.h's clear, count, scan and scatter over the queries, with the points' grid supplied -- so that a wave's
// lanes walk the same cells.
// vcr_query_knn_f32:
//   query_knn_kernel      one lane per query; the row is a lane-private ascending column of k 64-bit keys in LDS,
//                         (d2's bits) << 32 | j, as in grid.hip; a slot without a neighbour holds (+inf, -1)
// vcr_query_radius_f32: radius.hip's sequence over the M rows
//   query_count_kernel    one lane per query: the walk, n_i to count[b, i]
//   rows_offsets_kernel   csr_rows.h's tail, shared with radius.hip: the 64-bit scan of the counts to row_start, total
//   query_fill_kernel     the same walk: lane i appends its hits' keys to its private segment of the scratch row; no atomics
//   rows_order_kernel     a wave per row: csr_rows.h's rank sort out of the scratch through LDS in chunks of VCR_QUERY_CHUNK
//   rows_pad_kernel       -1 / +inf behind total[b], and over the clouds that do not fit
// The walk is grid_walk.h's, with the query's cell clamped and each side's term joined with the query's distances to the box
// (QySide); qy_walk puts the three kernels' common early-outs in front of it.  No scratch memory, no waits between workgroups;
// every loop is bounded by N, M, k, a row's length or the cells per axis; every run of candidates is clamped to [0, N), every
// write to its row.
#include "grid_walk.h"
#include "csr_rows.h"

namespace {

static_assert(VCR_QUERY_MAX_N == VCR_GRID_MAX_N && VCR_QUERY_MAX_K == VCR_GRID_MAX_K, "the points' grid is grid_build.h's");

// what the walking kernels share: the points' grid and the queries, in index order (qsorted == NULL) or in cell order
struct QyWalk {
  const float* queries; const GdGrid* grid; const int* counter; const float4* sorted; const float4* qsorted;
  int N, M, nblk, gstride;
};

struct QyQuery { float x[3]; int i; bool ok; };            // ok: the query is finite

// lane s of cloud b takes the s-th query in cell order, or query s
__device__ __forceinline__ QyQuery qy_query(const QyWalk& p, int b, int s) {
  const int M = p.M;
  QyQuery q;
  if (p.qsorted) {
    const float4 v = p.qsorted[(size_t)b * M + s];
    q.x[0] = v.x; q.x[1] = v.y; q.x[2] = v.z; q.i = __float_as_int(v.w);
    q.i = (unsigned)q.i < (unsigned)M ? q.i : 0;           // (always in range: the scatter wrote every slot)
  } else {
    const float* __restrict__ x = p.queries + (size_t)b * 3 * M;
    q.i = s; q.x[0] = x[s]; q.x[1] = x[M + s]; q.x[2] = x[2 * (size_t)M + s];
  }
  q.ok = gd_finite(q.x[0], q.x[1], q.x[2]);
  return q;
}

// Per axis the query's distance to the points' box, one subtraction (0 inside): no point of the cloud is nearer along that axis.
// The largest square is vcr_hip_gridnn.h's outside bound
__device__ __forceinline__ float qy_outside(const GdGrid& g, const float xq[3], float o[3]) {
  float out = 0.f;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    o[c] = xq[c] < g.lo[c] ? g.lo[c] - xq[c] : xq[c] > g.hi[c] ? xq[c] - g.hi[c] : 0.f;
    out = fmaxf(out, o[c] * o[c]);
  }
  return out;
}

// What no point behind the side at distance d along axis C can undercut: its difference along C is at least max(d, o_C) and
// along the other axes at least o_a, and d2's expression is monotone in each of them (every rounding is).  Inside the box
// (o = 0) this is d * d, section 4.19's term, bit for bit
struct QySide {
  const float* o;
  template <int C>
  __device__ __forceinline__ float term(float d) const {
    const float mx = C == 0 ? fmaxf(d, o[0]) : o[0], my = C == 1 ? fmaxf(d, o[1]) : o[1], mz = C == 2 ? fmaxf(d, o[2]) : o[2];
    return fmaf(mz, mz, fmaf(my, my, mx * mx));
  }
};

// The rings around the query's CLAMPED cell (below lo cell 0, above the last face n - 1), each side's term joined with the
// query's distances o to the box.  Nothing is walked in a cloud without a finite point (start[cells], the end of its last cell,
// is the number of its finite points).
template <class Run, class Stop>
__device__ __forceinline__ void qy_walk(const GdGrid& g, const int* __restrict__ start, const float xq[3], const float o[3],
                                        Run& run, Stop& stop) {
  if (g.cells < 1 || start[g.cells] <= 0) return;
  const int cx = gd_cell(xq[0], g.lo[0], g.h, g.inv, g.n[0]);
  const int cy = gd_cell(xq[1], g.lo[1], g.h, g.inv, g.n[1]);
  const int cz = gd_cell(xq[2], g.lo[2], g.h, g.inv, g.n[2]);
  gd_walk(g, start, cx, cy, cz, xq, QySide{o}, run, stop);
}

// ---- the k nearest

struct QyKnn { QyWalk w; int k; int* idx; float* d2; };

__global__ __launch_bounds__(GD_BLOCK) void query_knn_kernel(QyKnn p) {
  extern __shared__ __attribute__((aligned(16))) u64 qy_rows[];          // [k][GD_BLOCK]: lane t's column starts at qy_rows + t
  const int t = threadIdx.x;
  const int b = (int)(blockIdx.x / (unsigned)p.w.nblk), blk = (int)(blockIdx.x % (unsigned)p.w.nblk);
  const int s = blk * GD_BLOCK + t, N = p.w.N, M = p.w.M, k = p.k;
  if (s >= M) return;                                      // (no barrier below: every lane works on its own column)
  const QyQuery q = qy_query(p.w, b, s);
  u64* lk = qy_rows + t;
  const u64 none = (u64)GD_INF << 32 | 0xFFFFFFFFu;        // a slot without a neighbour: (+inf, -1)
  for (int a = 0; a < k; ++a) lk[a * GD_BLOCK] = none;
  u64 kth = none;
  if (q.ok) {
    const GdGrid g = p.w.grid[b];
    const float4* __restrict__ sorted = p.w.sorted + (size_t)b * N;
    auto run = [&](int a0, int a1) {
      a0 = a0 > 0 ? a0 : 0;
      a1 = a1 < N ? a1 : N;
      for (int c = a0; c < a1; ++c) gd_insert(lk, k, gd_key(sorted[c], q.x), kth);       // (kth <= none)
    };
    // STRICTLY below: a tie behind the ring could still enter
    auto stop = [&](float bound) { return gd_key_d2(kth) < bound; };
    float o[3];
    // (an outside bound of +inf: every d2 overflows, nothing is a candidate)
    if (qy_outside(g, q.x, o) < __builtin_huge_valf()) qy_walk(g, p.w.counter + (size_t)b * p.w.gstride, q.x, o, run, stop);
  }
  int* __restrict__ oi = p.idx + ((size_t)b * M + q.i) * k;
  for (int a = 0; a < k; ++a) oi[a] = gd_key_j(lk[a * GD_BLOCK]);
  if (p.d2) {
    float* __restrict__ od = p.d2 + ((size_t)b * M + q.i) * k;
    for (int a = 0; a < k; ++a) od[a] = gd_key_d2(lk[a * GD_BLOCK]);
  }
}

// ---- all within a radius

// The radius walk of one query: hit(key) for every candidate with d2 <= r2 (a NaN or an overflowed d2 is no hit: r2 is finite).
// A query that is not finite, or whose outside bound exceeds r2, walks nothing
template <class Hit>
__device__ __forceinline__ void qy_radius_walk(const QyWalk& p, int b, const QyQuery& q, float r2, Hit& hit) {
  if (!q.ok) return;
  const GdGrid g = p.grid[b];
  float o[3];
  const float out = qy_outside(g, q.x, o);
  if (!(out <= r2)) return;                                // (no point is nearer than out)
  const int N = p.N;
  const float4* __restrict__ sorted = p.sorted + (size_t)b * N;
  auto run = [&](int a0, int a1) {
    a0 = a0 > 0 ? a0 : 0;
    a1 = a1 < N ? a1 : N;
    for (int c = a0; c < a1; ++c) {
      const u64 key = gd_key(sorted[c], q.x);
      if (gd_key_d2(key) <= r2) hit(key);
    }
  };
  // STRICTLY above: an unseen point at exactly r2 is a hit (the bound is never below out: every side's term holds every o_c)
  auto stop = [&](float bound) { return bound > r2; };
  qy_walk(g, p.counter + (size_t)b * p.gstride, q.x, o, run, stop);
}

struct QyCount { QyWalk w; float r2; int* count; };

__global__ __launch_bounds__(GD_BLOCK) void query_count_kernel(QyCount p) {
  const int b = (int)(blockIdx.x / (unsigned)p.w.nblk), blk = (int)(blockIdx.x % (unsigned)p.w.nblk);
  const int s = blk * GD_BLOCK + (int)threadIdx.x;
  if (s >= p.w.M) return;                                  // (no barrier below)
  const QyQuery q = qy_query(p.w, b, s);
  int n = 0;
  auto hit = [&](u64) { ++n; };
  qy_radius_walk(p.w, b, q, p.r2, hit);
  p.count[(size_t)b * p.w.M + q.i] = n;
}

// row_start [B][M + 1]; scratch [B][capacity]: a cloud's unordered keys, row i at row_start[b, i]
struct QyFill { QyWalk w; float r2; const long long* row_start; int capacity; u64* scratch; };

__global__ __launch_bounds__(GD_BLOCK) void query_fill_kernel(QyFill p) {
  const int b = (int)(blockIdx.x / (unsigned)p.w.nblk), blk = (int)(blockIdx.x % (unsigned)p.w.nblk);
  const int s = blk * GD_BLOCK + (int)threadIdx.x, M = p.w.M;
  const long long* __restrict__ rs = p.row_start + (size_t)b * ((size_t)M + 1);
  if (s >= M || rs[M] > (long long)p.capacity) return;     // (no barrier below; a cloud that does not fit: the pad writes it)
  const QyQuery q = qy_query(p.w, b, s);
  const RowsSeg sg = rows_segment(rs, q.i, p.capacity);    // the lane's segment
  const long long room = sg.len;
  if (sg.at < 0 || room <= 0) return;
  u64* __restrict__ row = p.scratch + (size_t)b * p.capacity + (size_t)sg.at;
  long long w = 0;
  auto hit = [&](u64 key) { if (w < room) row[w] = key; ++w; };
  qy_radius_walk(p.w, b, q, p.r2, hit);
}

// How one call runs: the points' grid | the queries' cells, counters and cell order | (radius) the unordered keys
struct QyLayout {
  GdLayout at;                                             // the points' grid
  int nblk_q, order;                                       // workgroups a cloud's queries take; 1 = cell order, 2 = index order
  size_t qcell_off, qcounter_off, qsorted_off, scratch_off, bytes;
};

}  // namespace

// The ONE place that decides the order the queries are served in.  Measured (profiles/query_bench.txt part c, DESIGN section
// 4.28; 80 cases, index order's time over cell order's): the sort costs what a second grid costs -- 0.2 ms at 131 072 points, of
// which 0.17 ms is the one-workgroup scan over the 262 208 counters -- and that is all cell order ever loses: x0.64-x0.98 on
// queries near the points where the rows are short (k = 1 on nearly every shape; k = 20 and rows of 12 on a uniform cloud of
// 131 072 points: 0.32 against 0.50 ms at the worst), x0.65-x0.92 on radius rows of queries beyond the box, most of which walk
// nothing.  Index order loses without such a limit where a wave's queries lie apart: x1.2-x3.0 on every kNN search from beyond
// the box (51 against 151 ms at 1 x 131 072 on a surface), x1.1-x1.5 on radius rows of 100.  The host cannot see where the
// queries lie, so the plan takes the order whose loss is bounded, whatever the shape; index order stays behind `variant`.
static int qy_order_form(int N, int M, int k_or_0) {
  (void)N; (void)M; (void)k_or_0;
  return 1;
}

static int qy_layout(int B, int N, int M, int capacity, int variant, int k_or_0, QyLayout* l) {
  if (variant < 0 || variant > 2) return VCR_EINVAL;
  if (N < 1 || N > VCR_QUERY_MAX_N || (long)B * N >= (1L << 31)) return VCR_EUNSUPPORTED;
  if (M < 1 || M > VCR_QUERY_MAX_N || (long)B * M >= (1L << 31)) return VCR_EUNSUPPORTED;
  if ((long)B * capacity >= (1L << 31)) return VCR_EUNSUPPORTED;
  l->at = gd_layout(B, N);
  l->nblk_q = (M + GD_BLOCK - 1) / GD_BLOCK;
  l->order = variant ? variant : qy_order_form(N, M, k_or_0);
  const size_t BM = (size_t)B * M;
  l->qcell_off = l->at.bytes;
  l->qcounter_off = l->qcell_off + ws_up(BM * 4);
  l->qsorted_off = l->qcounter_off + ws_up((size_t)B * l->at.gstride * 4);
  l->scratch_off = l->qsorted_off + ws_up(BM * 16);
  l->bytes = l->scratch_off + ws_up((size_t)B * capacity * sizeof(u64));
  return VCR_OK;
}

// The points' grid, and with order 1 the queries in the order of their clamped cells in it: grid_build.h's clear, count, scan
// and scatter over the queries with the points' grid supplied (gd_cell clamps; a query that is not finite goes behind the last
// cell).  -> what the walking kernels share
static int qy_build(const float* xyz, const float* queries, int B, int N, int M, float cell, const QyLayout& l, unsigned char* w,
                    hipStream_t s, QyWalk* wk) {
  int e = gd_build(xyz, B, N, cell, l.at, w, s);
  if (e) return e;
  const GdGrid* grid = reinterpret_cast<const GdGrid*>(w);
  float4* qsorted = reinterpret_cast<float4*>(w + l.qsorted_off);
  *wk = QyWalk{queries, grid, reinterpret_cast<const int*>(w + l.at.counter_off), reinterpret_cast<const float4*>(w + l.at.sorted_off),
               l.order == 1 ? qsorted : nullptr, N, M, l.nblk_q, l.at.gstride};
  if (l.order != 1) return VCR_OK;
  int* qcounter = reinterpret_cast<int*>(w + l.qcounter_off);
  const dim3 block(GD_BLOCK), clouds((unsigned)B), points((unsigned)((long)B * l.nblk_q));
  const int clear_x = (l.at.gstride + GD_BLOCK - 1) / GD_BLOCK < 64 ? (l.at.gstride + GD_BLOCK - 1) / GD_BLOCK : 64;
  hipLaunchKernelGGL(grid_clear_kernel, dim3((unsigned)((long)B * clear_x)), block, 0, s, grid, qcounter, l.at.gstride, clear_x);
  if ((e = VCR_LAUNCH_RC())) return e;
  const GdPoints pt{queries, grid, reinterpret_cast<int*>(w + l.qcell_off), qcounter, qsorted, M, l.nblk_q, l.at.gstride};
  hipLaunchKernelGGL(grid_count_kernel, points, block, 0, s, pt);
  if ((e = VCR_LAUNCH_RC())) return e;
  hipLaunchKernelGGL(grid_scan_kernel, clouds, block, 0, s, grid, qcounter, l.at.gstride);
  if ((e = VCR_LAUNCH_RC())) return e;
  hipLaunchKernelGGL(grid_scatter_kernel, points, block, 0, s, pt);
  return VCR_LAUNCH_RC();
}

// ---- vcr_query_knn_*

static int qy_knn_plan(const vcr_query_knn_args* ua, vcr_query_knn_args* a, QyLayout* l) {
  if (vcr_take_args(ua, a, offsetof(vcr_query_knn_args, d2))) return VCR_EINVAL;
  if (!a->xyz || !a->queries || !a->idx || a->B < 1 || !gd_cell_ok(a->cell)) return VCR_EINVAL;
  const int e = qy_layout(a->B, a->N, a->M, 0, a->variant, a->k, l);
  if (e) return e;
  return a->k < 1 || a->k > VCR_QUERY_MAX_K ? VCR_EUNSUPPORTED : VCR_OK;
}

extern "C" int vcr_query_knn_form(const vcr_query_knn_args* ua, int cu_count, int* cells_per_cloud, int* query_order) {
  vcr_query_knn_args a;
  QyLayout l;
  if (cu_count < 0) return VCR_EINVAL;
  const int e = qy_knn_plan(ua, &a, &l);
  if (e) return e;
  if (cells_per_cloud) *cells_per_cloud = l.at.gstride - 2;
  if (query_order) *query_order = l.order;
  return VCR_OK;
}

extern "C" size_t vcr_query_knn_workspace_bytes(const vcr_query_knn_args* ua, int cu_count) {
  vcr_query_knn_args a;
  QyLayout l;
  if (cu_count < 0) return 0;
  return qy_knn_plan(ua, &a, &l) ? 0 : l.bytes;
}

extern "C" int vcr_query_knn_f32(const vcr_query_knn_args* ua, void* workspace, size_t workspace_bytes, vcr_stream_t stream) {
  vcr_query_knn_args a;
  QyLayout l;
  int e = qy_knn_plan(ua, &a, &l);
  if (e) return e;
  if (!workspace || (((uintptr_t)workspace) & 15)) return VCR_EINVAL;
  if (workspace_bytes < l.bytes) return VCR_EWORKSPACE;
  vcr_stream_scope scope_(stream);
  hipStream_t s = (hipStream_t)stream;
  QyWalk wk;
  if ((e = qy_build(a.xyz, a.queries, a.B, a.N, a.M, a.cell, l, reinterpret_cast<unsigned char*>(workspace), s, &wk))) return e;
  return vcr_launch<query_knn_kernel>(dim3((unsigned)((long)a.B * l.nblk_q)), dim3(GD_BLOCK), (size_t)a.k * GD_BLOCK * sizeof(u64),
                                      s, QyKnn{wk, a.k, a.idx, a.d2});
}

// ---- vcr_query_radius_*

static int qy_radius_plan(const vcr_query_radius_args* ua, vcr_query_radius_args* a, QyLayout* l, float* r2) {
  if (vcr_take_args(ua, a, offsetof(vcr_query_radius_args, idx))) return VCR_EINVAL;
  if (!a->xyz || !a->queries || !a->count || !a->row_start || !a->total || a->B < 1) return VCR_EINVAL;
  if (!gd_radius_ok(a->radius, r2) || !gd_cell_ok(a->cell)) return VCR_EINVAL;
  if (a->capacity < 0 || (!a->idx && a->capacity != 0) || (a->d2 && !a->idx)) return VCR_EINVAL;
  return qy_layout(a->B, a->N, a->M, a->capacity, a->variant, 0, l);
}

extern "C" int vcr_query_radius_form(const vcr_query_radius_args* ua, int cu_count, int* cells_per_cloud, int* query_order) {
  vcr_query_radius_args a;
  QyLayout l;
  float r2;
  if (cu_count < 0) return VCR_EINVAL;
  const int e = qy_radius_plan(ua, &a, &l, &r2);
  if (e) return e;
  if (cells_per_cloud) *cells_per_cloud = l.at.gstride - 2;
  if (query_order) *query_order = l.order;
  return VCR_OK;
}

extern "C" size_t vcr_query_radius_workspace_bytes(const vcr_query_radius_args* ua, int cu_count) {
  vcr_query_radius_args a;
  QyLayout l;
  float r2;
  if (cu_count < 0) return 0;
  return qy_radius_plan(ua, &a, &l, &r2) ? 0 : l.bytes;
}

extern "C" int vcr_query_radius_f32(const vcr_query_radius_args* ua, void* workspace, size_t workspace_bytes, vcr_stream_t stream) {
  vcr_query_radius_args a;
  QyLayout l;
  float r2;
  int e = qy_radius_plan(ua, &a, &l, &r2);
  if (e) return e;
  if (!workspace || (((uintptr_t)workspace) & 15)) return VCR_EINVAL;
  if (workspace_bytes < l.bytes) return VCR_EWORKSPACE;
  vcr_stream_scope scope_(stream);
  hipStream_t s = (hipStream_t)stream;
  unsigned char* w = reinterpret_cast<unsigned char*>(workspace);
  QyWalk wk;
  if ((e = qy_build(a.xyz, a.queries, a.B, a.N, a.M, a.cell > 0.f ? a.cell : a.radius, l, w, s, &wk))) return e;
  const dim3 block(GD_BLOCK), lanes((unsigned)((long)a.B * l.nblk_q));
  long long* row_start = reinterpret_cast<long long*>(a.row_start);
  hipLaunchKernelGGL(query_count_kernel, lanes, block, 0, s, QyCount{wk, r2, a.count});
  if ((e = VCR_LAUNCH_RC())) return e;
  if ((e = rows_offsets(a.count, row_start, reinterpret_cast<long long*>(a.total), a.B, a.M, s))) return e;
  if (!a.idx || a.capacity == 0) return VCR_OK;
  u64* scratch = reinterpret_cast<u64*>(w + l.scratch_off);
  hipLaunchKernelGGL(query_fill_kernel, lanes, block, 0, s, QyFill{wk, r2, row_start, a.capacity, scratch});
  if ((e = VCR_LAUNCH_RC())) return e;
  return rows_order_pad(RowsOrder{row_start, scratch, a.M, a.capacity, a.idx, a.d2}, a.B, s);
}

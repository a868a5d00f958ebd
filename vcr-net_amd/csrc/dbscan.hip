// DBSCAN over ragged rows (include/cluster/vcr_hip_dbscan.h): vcr_rows_dbscan_f32 -- the clusters are the
// connected components of the core points' graph, found by a lock-free union-find in global memory -- and
// vcr_cluster_largest_f32, which hands the largest cluster's members to the outlier filters' tail (outlier.hip).
//
//   dbscan_check_kernel     a thread per (row_start[i], row_start[i+1]) pair: one flag per 256 pairs, "one of them descends"
//   dbscan_served_kernel    one workgroup per cloud: those flags, row_start's two ends and total -> served[b], by ONE thread.
//                           Every later kernel reads it first; a cloud that is not served has no idx entry read
//   dbscan_core_kernel      <form> per row: L_i, the entries inside [0, N) that are not i, counted; node[i] = i for a core point,
//                           DB_PLAIN for any other finite one, DB_NONFINITE otherwise; the optional core output
//   dbscan_hook_kernel      <form> per core row: union(i, j) for every core entry j.  THE hot path, see below
//   dbscan_flatten_kernel   a lane a point: root[i] = find(i) (negative values copied), the roots counted per 256 points
//   dbscan_offsets_kernel   one workgroup per cloud: the exclusive scan of those counts (wg_scan.h), n_clusters[b]
//   dbscan_rank_kernel      a lane a point: a root's rank among the cloud's roots, ascending in index -- its cluster's label --
//                           and sizes zeroed
//   dbscan_label_kernel     <form> per row: rank[root[i]] for a core point; for any other finite one the minimum of
//                           rank[root[j]] over its row's core entries, -1 without one; -1 for a non-finite point; sizes counted by
//                           integer atomic adds (order-free), one per wave and slot in the lane form
//   largest_pick_kernel     one workgroup per cloud: the largest slot of sizes, the lowest label among equals
//   largest_member_kernel   a lane a point: 1 for a member of that cluster, the filters' tail compacts them
// <form>: a lane a row (DB_LANE), or a wave a row with the entries dealt to its 64 lanes (DB_WAVE); one template.
//
// The union-find.  node[] holds a forest over the core points of a cloud; every access to it in the hook kernel is a relaxed
// agent-scope atomic (the XCDs' L2s are not coherent: such a load is served past them), the hook itself an atomicCAS.
//   (1) node[x] <= x for every core x, always: a root holds itself, anything else a smaller index
//   (2) only a root is ever hooked: the CAS expects node[hi] == hi and installs lo < hi.  A node that has stopped being a root
//       never becomes one again, since no store ever writes x to node[x]
//   (3) a compression store writes to a NON-root x an ancestor of x (its grandparent as read): smaller than x, in x's tree
//   (4) a stale read of node[x] is an older ancestor of x: still in x's tree, so find() still ends at a node of the tree
//   (5) no lane waits for another.  find() descends strictly (1); a union retries only when its CAS found hi hooked by somebody
//       else, and at most N - 1 hooks succeed in a cloud: the kernel cannot hang
//   (6) when the kernel ends, every edge's two ends share a root, and by (1) a root is the lowest index of its tree: the
//       component's lowest core index, whichever lane's CAS won which hook
// So the forest's shape depends on arrival order and its roots do not; everything behind the hook reads roots alone.
#include "wg_scan.h"
#include "outlier_flags.h"
#include "../../include/cluster/vcr_hip_dbscan.h"

namespace {

typedef long long i64;

constexpr int DB_BLOCK = WG_BLOCK;
constexpr int DB_WAVES = DB_BLOCK / 64;
constexpr int DB_LANE = VCR_DBSCAN_LANE, DB_WAVE = VCR_DBSCAN_WAVE;
constexpr int DB_PLAIN = -1;                               // node / root of a finite point that is not core
constexpr int DB_NONFINITE = -2;                           // ... of a point with a non-finite coordinate
constexpr int DB_BIG = 0x7FFFFFFF;
constexpr int DB_AHEAD = 4;                                // entries of a row the hook loads before it works on them

struct DbRows { const int* idx; const i64* row_start; const i64* total; const int* served; int N, capacity; long rows; };   // rows = B N

struct DbCheck { const i64* row_start; const i64* total; int N, capacity, nblk; int* blkbad; int* served; };
struct DbCore { DbRows r; const float* xyz; int min_points; int* node; int* core; };
struct DbHook { DbRows r; int* node; };
struct DbFlatten { const int* served; int* node; int N, nblk; int* root; int* blkcnt; };
struct DbOffsets { const int* served; int* blkcnt; int nblk; int* n_clusters; };
struct DbRank { const int* served; const int* root; const int* blkcnt; int N, nblk; int* rank; int* sizes; };
struct DbLabel { DbRows r; const int* root; const int* rank; int* labels; int* sizes; };
struct LgPick { const int* sizes; int N; int* winner; };
struct LgMember { const int* labels; const int* winner; int N; long total; int* flags; };

__device__ __forceinline__ bool db_finite(float v) { return fabsf(v) < __builtin_huge_valf(); }

__device__ __forceinline__ int db_ld(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void db_st(int* p, int v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// The root of core x's tree as far as this lane can see, with path halving: x's parent becomes its grandparent on the way (3).
// Every step goes to a strictly smaller index (1), so the loop ends.
__device__ __forceinline__ int db_find(int* node, int x) {
  for (;;) {
    const int p = db_ld(node + x);
    if (p == x) return x;
    const int gp = db_ld(node + p);
    if (gp == p) return p;
    db_st(node + x, gp);
    x = gp;
  }
}

// One tree for x and y (both core).  Returns a node of it near the root, for the caller's next union.
__device__ __forceinline__ int db_union(int* node, int x, int y) {
  int a = db_find(node, x), b = db_find(node, y);
  while (a != b) {
    const int hi = a > b ? a : b, lo = a > b ? b : a;
    const int old = atomicCAS(node + hi, hi, lo);          // (2): hooks hi only while it is a root
    if (old == hi) return lo;
    a = db_find(node, old);                                // somebody else hooked hi under old < hi: go on from there (5)
    b = db_find(node, lo);
  }
  return a;
}

// Row g = (b, i) of a served cloud: its entries and their number; 0 entries where the cloud is not served.  A served cloud's
// row_start ascends from 0 to total <= capacity, so the row lies inside the cloud's capacity.
__device__ __forceinline__ bool db_row(const DbRows& r, long g, long& b, int& i, const int*& nb, int& n) {
  b = g / r.N;
  i = (int)(g - b * r.N);
  const bool ok = r.served[b] != 0;
  n = 0;
  nb = r.idx;
  if (ok) {
    const i64* rs = r.row_start + (size_t)b * ((size_t)r.N + 1) + i;
    const i64 s = rs[0];
    n = (int)(rs[1] - s);
    nb = r.idx + (size_t)b * r.capacity + s;
  }
  return ok;
}

// blockIdx, threadIdx -> the row this lane works on, its first entry and its step: a lane a row, or a wave a row
template <int FORM>
__device__ __forceinline__ long db_mine(int& first, int& step) {
  if (FORM == DB_WAVE) {
    first = threadIdx.x & 63; step = 64;
    return (long)blockIdx.x * DB_WAVES + (threadIdx.x >> 6);
  }
  first = 0; step = 1;
  return (long)blockIdx.x * DB_BLOCK + threadIdx.x;
}

template <int FORM>
__device__ __forceinline__ int db_sum(int v) {
  if (FORM == DB_WAVE) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
  }
  return v;
}

template <int FORM>
__device__ __forceinline__ int db_min(int v) {
  if (FORM == DB_WAVE) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) { const int u = __shfl_xor(v, o, 64); v = u < v ? u : v; }
  }
  return v;
}

__global__ __launch_bounds__(DB_BLOCK) void dbscan_check_kernel(DbCheck p) {
  const int b = (int)(blockIdx.x / (unsigned)p.nblk), blk = (int)(blockIdx.x % (unsigned)p.nblk);
  const int i = blk * DB_BLOCK + threadIdx.x, N = p.N;     // the pair (i, i + 1)
  const i64* rs = p.row_start + (size_t)b * ((size_t)N + 1);
  const bool bad = i < N && rs[i] > rs[i + 1];
  const int any = __syncthreads_or(bad);
  if (threadIdx.x == 0) p.blkbad[(size_t)b * p.nblk + blk] = any;
}

__global__ __launch_bounds__(DB_BLOCK) void dbscan_served_kernel(DbCheck p) {
  const int b = blockIdx.x, N = p.N;
  const i64* rs = p.row_start + (size_t)b * ((size_t)N + 1);
  const i64 tot = p.total[b];
  bool bad = tot < 0 || tot > (i64)p.capacity || rs[0] != 0 || rs[N] != tot;
  for (int k = threadIdx.x; k < p.nblk; k += DB_BLOCK) bad |= p.blkbad[(size_t)b * p.nblk + k] != 0;
  const int any = __syncthreads_or(bad);
  if (threadIdx.x == 0) p.served[b] = any ? 0 : 1;
}

template <int FORM>
__global__ __launch_bounds__(DB_BLOCK) void dbscan_core_kernel(DbCore p) {
  int first, step;
  const long g = db_mine<FORM>(first, step);
  if (g >= p.r.rows) return;                               // (a whole wave in the wave form: no barrier below)
  long b;
  int i, n;
  const int* nb;
  const bool ok = db_row(p.r, g, b, i, nb, n);
  const int N = p.r.N;
  int cnt = 0;
  for (long e = first; e < n; e += step) {          // (long: a row may be as long as an int holds)
    const int j = nb[e];
    cnt += (unsigned)j < (unsigned)N && j != i;
  }
  cnt = db_sum<FORM>(cnt);
  if (first != 0) return;
  bool finite = true;
  if (p.xyz) {
    const float* x = p.xyz + (size_t)b * 3 * N + i;
    finite = db_finite(x[0]) && db_finite(x[N]) && db_finite(x[2 * (size_t)N]);
  }
  const bool core = ok && finite && (long)cnt + 1 >= (long)p.min_points;
  p.node[g] = core ? i : finite ? DB_PLAIN : DB_NONFINITE;
  if (p.core) p.core[g] = core ? 1 : 0;
}

template <int FORM>
__global__ __launch_bounds__(DB_BLOCK) void dbscan_hook_kernel(DbHook p) {
  int first, step;
  const long g = db_mine<FORM>(first, step);
  if (g >= p.r.rows) return;
  long b;
  int i, n;
  const int* nb;
  if (!db_row(p.r, g, b, i, nb, n)) return;
  const int N = p.r.N;
  int* node = p.node + (size_t)b * N;
  if (db_ld(node + i) < 0) return;                         // not core: no edge starts here
  int at = db_find(node, i);                               // a node of i's tree, as near its root as this lane has seen
  // DB_AHEAD entries at a time: their indices, then their nodes, are loads that do not wait for each other -- the lane form
  // has few waves a SIMD and nothing else to hide a load behind
  for (long e = first; e < n; e += DB_AHEAD * step) {
    int j[DB_AHEAD], pj[DB_AHEAD];
#pragma unroll
    for (int u = 0; u < DB_AHEAD; ++u) j[u] = e + u * step < n ? nb[e + u * step] : -1;
#pragma unroll
    for (int u = 0; u < DB_AHEAD; ++u) pj[u] = (unsigned)j[u] < (unsigned)N && j[u] != i ? db_ld(node + j[u]) : DB_PLAIN;
#pragma unroll
    for (int u = 0; u < DB_AHEAD; ++u) {
      // not core, or j hangs under `at` as this lane read it: by (4) that is an ancestor of j, and j is in i's tree already
      if (pj[u] < 0 || pj[u] == at) continue;
      at = db_union(node, at, j[u]);
    }
  }
}

__global__ __launch_bounds__(DB_BLOCK) void dbscan_flatten_kernel(DbFlatten p) {
  __shared__ int wcnt[DB_WAVES];
  const int t = threadIdx.x;
  const int b = (int)(blockIdx.x / (unsigned)p.nblk), blk = (int)(blockIdx.x % (unsigned)p.nblk);
  const int i = blk * DB_BLOCK + t, N = p.N;
  const bool live = i < N && p.served[b] != 0;             // (served: workgroup-uniform)
  int r = DB_PLAIN;
  if (live) {
    int* node = p.node + (size_t)b * N;
    r = db_ld(node + i);
    if (r >= 0) r = db_find(node, i);                      // no hook runs any more: the root is the final one
    p.root[(size_t)b * N + i] = r;
  }
  int roots;
  wg_rank(live && r == i, t, wcnt, &roots);
  if (t == 0) p.blkcnt[(size_t)b * p.nblk + blk] = roots;
}

__global__ __launch_bounds__(DB_BLOCK) void dbscan_offsets_kernel(DbOffsets p) {
  __shared__ int wtot[DB_WAVES];
  const int b = blockIdx.x;
  if (!p.served[b]) {                                      // (workgroup-uniform)
    if (threadIdx.x == 0) p.n_clusters[b] = -1;
    return;
  }
  const int roots = wg_offsets(p.blkcnt + (size_t)b * p.nblk, p.nblk, wtot);
  if (threadIdx.x == 0) p.n_clusters[b] = roots;
}

__global__ __launch_bounds__(DB_BLOCK) void dbscan_rank_kernel(DbRank p) {
  __shared__ int wcnt[DB_WAVES];
  const int t = threadIdx.x;
  const int b = (int)(blockIdx.x / (unsigned)p.nblk), blk = (int)(blockIdx.x % (unsigned)p.nblk);
  const int i = blk * DB_BLOCK + t, N = p.N;
  const size_t at = (size_t)b * N + (i < N ? i : 0);
  if (p.sizes && i < N) p.sizes[at] = 0;
  if (!p.served[b]) return;                                // (workgroup-uniform: in front of the barrier)
  const bool is_root = i < N && p.root[at] == i;
  int roots;
  const int below = wg_rank(is_root, t, wcnt, &roots);
  if (is_root) p.rank[at] = p.blkcnt[(size_t)b * p.nblk + blk] + below;
}

// One more member for the slot `cell` of sizes (none where cell < 0).  Integer counts are order-free.  In the lane form the lanes
// of a wave that count into the same slot add ONCE, their number: a cloud that is one cluster would otherwise send every point's
// add to one address.  Called by all 64 lanes of the wave.
template <int FORM>
__device__ __forceinline__ void db_count(int* sizes, int cell, int first) {
  if (FORM == DB_WAVE) {
    if (first == 0 && cell >= 0) atomicAdd(sizes + cell, 1);
    return;
  }
  const int lane = threadIdx.x & 63;
  unsigned long long todo = __ballot(cell >= 0);           // (wave-uniform, and so is the loop)
  while (todo) {
    const int leader = __ffsll((long long)todo) - 1;
    const int c = __shfl(cell, leader, 64);
    const unsigned long long same = __ballot(cell == c);
    if (lane == leader) atomicAdd(sizes + c, __popcll(same));
    todo &= ~same;
  }
}

template <int FORM>
__global__ __launch_bounds__(DB_BLOCK) void dbscan_label_kernel(DbLabel p) {
  int first, step;
  const long g = db_mine<FORM>(first, step);
  const bool live = g < p.r.rows;                          // (a whole wave in the wave form; the lane form's last wave may be mixed)
  long b = 0;
  int i = 0, n = 0;
  const int* nb = nullptr;
  int label = VCR_DBSCAN_NOT_SERVED;
  if (live && db_row(p.r, g, b, i, nb, n)) {
    const int N = p.r.N;
    const int* root = p.root + (size_t)b * N;
    const int* rank = p.rank + (size_t)b * N;
    const int mine = root[i];
    if (mine >= 0) {
      label = rank[mine];
    } else if (mine == DB_NONFINITE) {
      label = VCR_DBSCAN_NOISE;
    } else {
      int best = DB_BIG;
      for (long e = first; e < n; e += step) {          // (long: a row may be as long as an int holds)
        const int j = nb[e];
        if ((unsigned)j >= (unsigned)N || j == i) continue;
        const int rj = root[j];
        if (rj < 0) continue;
        const int lj = rank[rj];
        best = lj < best ? lj : best;
      }
      best = db_min<FORM>(best);
      label = best == DB_BIG ? VCR_DBSCAN_NOISE : best;
    }
  }
  if (p.sizes) db_count<FORM>(p.sizes, label >= 0 ? (int)(b * p.r.N + label) : -1, first);      // (B N < 2^31)
  if (live && first == 0) p.labels[g] = label;
}

__global__ __launch_bounds__(DB_BLOCK) void largest_pick_kernel(LgPick p) {
  __shared__ int wbest[DB_WAVES], wat[DB_WAVES];
  const int b = blockIdx.x, t = threadIdx.x;
  const int* sizes = p.sizes + (size_t)b * p.N;
  int best = 0, at = -1;                                   // a size of 0 or less names no cluster
  for (int c = t; c < p.N; c += DB_BLOCK) {                // ascending labels: the strict > keeps the lowest among equals
    const int s = sizes[c];
    if (s > best) { best = s; at = c; }
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    const int s = __shfl_xor(best, o, 64), a = __shfl_xor(at, o, 64);
    if (s > best || (s == best && s > 0 && a < at)) { best = s; at = a; }
  }
  if ((t & 63) == 0) { wbest[t >> 6] = best; wat[t >> 6] = at; }
  __syncthreads();
  if (t == 0) {
    for (int w = 1; w < DB_WAVES; ++w)
      if (wbest[w] > best || (wbest[w] == best && best > 0 && wat[w] < at)) { best = wbest[w]; at = wat[w]; }
    p.winner[b] = at;
  }
}

__global__ __launch_bounds__(DB_BLOCK) void largest_member_kernel(LgMember p) {
  const long g = (long)blockIdx.x * DB_BLOCK + threadIdx.x;
  if (g >= p.total) return;
  const int w = p.winner[g / p.N];
  p.flags[g] = w >= 0 && p.labels[g] == w ? 1 : 0;
}

// What the entry points and the form query ask of the numbers
int db_numbers(int B, int N, int capacity, int min_points, int variant) {
  if (B < 1 || capacity < 0 || min_points < 1) return VCR_EINVAL;
  if (variant != 0 && variant != DB_LANE && variant != DB_WAVE) return VCR_EINVAL;
  if (N < 1 || N > VCR_DBSCAN_MAX_N || (long)B * N >= (1L << 31) || (long)B * capacity >= (1L << 31)) return VCR_EUNSUPPORTED;
  return VCR_OK;
}

int db_check(const vcr_rows_dbscan_args& a) {
  if (!a.row_start || !a.total || !a.labels || !a.n_clusters || (!a.idx && a.capacity != 0)) return VCR_EINVAL;
  return db_numbers(a.B, a.N, a.capacity, a.min_points, a.variant);
}

// THE one place that decides a pass's form: the row length the host can see
int db_form(int N, int capacity, int variant, int threshold) {
  if (variant) return variant;
  return (long)capacity / N >= threshold ? DB_WAVE : DB_LANE;
}

inline size_t db_up(size_t v) { return (v + 255) & ~(size_t)255; }

// workspace: served [B] | node [B N] | root [B N] | rank [B N] | blkcnt [B nblk]
struct DbPlan { int nblk; size_t node_off, root_off, rank_off, blk_off, bytes; };

DbPlan db_plan(int B, int N) {
  DbPlan p;
  p.nblk = (N + DB_BLOCK - 1) / DB_BLOCK;
  const size_t BN = (size_t)B * N * 4;
  p.node_off = db_up((size_t)B * 4);
  p.root_off = p.node_off + db_up(BN);
  p.rank_off = p.root_off + db_up(BN);
  p.blk_off = p.rank_off + db_up(BN);
  p.bytes = p.blk_off + db_up((size_t)B * p.nblk * 4);
  return p;
}

int db_take(const vcr_rows_dbscan_args* user, vcr_rows_dbscan_args* mine) {
  return vcr_take_args(user, mine, offsetof(vcr_rows_dbscan_args, core));
}

unsigned db_blocks(long items, int per_block) { return (unsigned)((items + per_block - 1) / per_block); }

// a row pass's grid: a lane a row or a wave a row
unsigned db_grid(long rows, int form) { return db_blocks(rows, form == DB_WAVE ? DB_WAVES : DB_BLOCK); }

int lg_take(const vcr_cluster_largest_args* user, vcr_cluster_largest_args* mine) {
  return vcr_take_args(user, mine, offsetof(vcr_cluster_largest_args, index));
}

int lg_check(const vcr_cluster_largest_args& a) {
  if (!a.xyz || !a.labels || !a.sizes || !a.points || !a.count || a.B < 1) return VCR_EINVAL;
  if (a.N < 1 || a.N > VCR_DBSCAN_MAX_N || (long)a.B * a.N >= (1L << 31)) return VCR_EUNSUPPORTED;
  return VCR_OK;
}

// workspace: winner [B] | flags [B N] | blkcnt [B nblk]
struct LgPlan { int nblk; size_t flag_off, blk_off, bytes; };

LgPlan lg_plan(int B, int N) {
  LgPlan p;
  p.nblk = (N + DB_BLOCK - 1) / DB_BLOCK;
  p.flag_off = db_up((size_t)B * 4);
  p.blk_off = p.flag_off + db_up((size_t)B * N * 4);
  p.bytes = p.blk_off + db_up((size_t)B * p.nblk * 4);
  return p;
}

}  // namespace

extern "C" int vcr_rows_dbscan_form(const vcr_rows_dbscan_args* ua, int cu_count, int* hook_form, int* label_form) {
  vcr_rows_dbscan_args a;
  if (db_take(ua, &a) || cu_count < 0) return VCR_EINVAL;
  const int e = db_numbers(a.B, a.N, a.capacity, a.min_points, a.variant);
  if (e) return e;
  if (hook_form) *hook_form = db_form(a.N, a.capacity, a.variant, VCR_DBSCAN_WAVE_HOOK);
  if (label_form) *label_form = db_form(a.N, a.capacity, a.variant, VCR_DBSCAN_WAVE_LABEL);
  return VCR_OK;
}

extern "C" size_t vcr_rows_dbscan_workspace_bytes(const vcr_rows_dbscan_args* ua, int cu_count) {
  vcr_rows_dbscan_args a;
  if (db_take(ua, &a) || cu_count < 0 || db_check(a)) return 0;
  return db_plan(a.B, a.N).bytes;
}

extern "C" int vcr_rows_dbscan_f32(const vcr_rows_dbscan_args* ua, void* workspace, size_t workspace_bytes, vcr_stream_t stream) {
  vcr_rows_dbscan_args a;
  if (db_take(ua, &a)) return VCR_EINVAL;
  int e = db_check(a);
  if (e) return e;
  const DbPlan pl = db_plan(a.B, a.N);
  if (!workspace || (((uintptr_t)workspace) & 255) || workspace_bytes < pl.bytes) return VCR_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  unsigned char* w = reinterpret_cast<unsigned char*>(workspace);
  int* served = reinterpret_cast<int*>(w);
  int* node = reinterpret_cast<int*>(w + pl.node_off);
  int* root = reinterpret_cast<int*>(w + pl.root_off);
  int* rank = reinterpret_cast<int*>(w + pl.rank_off);
  int* blk = reinterpret_cast<int*>(w + pl.blk_off);
  const long rows = (long)a.B * a.N;
  const int hook = db_form(a.N, a.capacity, a.variant, VCR_DBSCAN_WAVE_HOOK);
  const int label = db_form(a.N, a.capacity, a.variant, VCR_DBSCAN_WAVE_LABEL);
  const dim3 block(DB_BLOCK), clouds((unsigned)a.B), points((unsigned)((long)a.B * pl.nblk));
  const DbRows r{a.idx, (const i64*)a.row_start, (const i64*)a.total, served, a.N, a.capacity, rows};

  const DbCheck kk{r.row_start, r.total, a.N, a.capacity, pl.nblk, blk, served};     // (blk: read back before the flatten counts into it)
  hipLaunchKernelGGL(dbscan_check_kernel, points, block, 0, s, kk);
  if ((e = VCR_LAUNCH_RC())) return e;
  hipLaunchKernelGGL(dbscan_served_kernel, clouds, block, 0, s, kk);
  if ((e = VCR_LAUNCH_RC())) return e;
  const DbCore kc{r, a.xyz, a.min_points, node, a.core};
  const DbHook kh{r, node};
  if (hook == DB_WAVE) {
    hipLaunchKernelGGL(dbscan_core_kernel<DB_WAVE>, dim3(db_grid(rows, DB_WAVE)), block, 0, s, kc);
    if ((e = VCR_LAUNCH_RC())) return e;
    hipLaunchKernelGGL(dbscan_hook_kernel<DB_WAVE>, dim3(db_grid(rows, DB_WAVE)), block, 0, s, kh);
  } else {
    hipLaunchKernelGGL(dbscan_core_kernel<DB_LANE>, dim3(db_grid(rows, DB_LANE)), block, 0, s, kc);
    if ((e = VCR_LAUNCH_RC())) return e;
    hipLaunchKernelGGL(dbscan_hook_kernel<DB_LANE>, dim3(db_grid(rows, DB_LANE)), block, 0, s, kh);
  }
  if ((e = VCR_LAUNCH_RC())) return e;
  hipLaunchKernelGGL(dbscan_flatten_kernel, points, block, 0, s, DbFlatten{served, node, a.N, pl.nblk, root, blk});
  if ((e = VCR_LAUNCH_RC())) return e;
  hipLaunchKernelGGL(dbscan_offsets_kernel, clouds, block, 0, s, DbOffsets{served, blk, pl.nblk, a.n_clusters});
  if ((e = VCR_LAUNCH_RC())) return e;
  hipLaunchKernelGGL(dbscan_rank_kernel, points, block, 0, s, DbRank{served, root, blk, a.N, pl.nblk, rank, a.sizes});
  if ((e = VCR_LAUNCH_RC())) return e;
  const DbLabel kl{r, root, rank, a.labels, a.sizes};
  if (label == DB_WAVE)
    hipLaunchKernelGGL(dbscan_label_kernel<DB_WAVE>, dim3(db_grid(rows, DB_WAVE)), block, 0, s, kl);
  else
    hipLaunchKernelGGL(dbscan_label_kernel<DB_LANE>, dim3(db_grid(rows, DB_LANE)), block, 0, s, kl);
  return VCR_LAUNCH_RC();
}

extern "C" size_t vcr_cluster_largest_workspace_bytes(const vcr_cluster_largest_args* ua, int cu_count) {
  vcr_cluster_largest_args a;
  if (lg_take(ua, &a) || cu_count < 0 || lg_check(a)) return 0;
  return lg_plan(a.B, a.N).bytes;
}

extern "C" int vcr_cluster_largest_f32(const vcr_cluster_largest_args* ua, void* workspace, size_t workspace_bytes,
                                       vcr_stream_t stream) {
  vcr_cluster_largest_args a;
  if (lg_take(ua, &a)) return VCR_EINVAL;
  int e = lg_check(a);
  if (e) return e;
  const LgPlan pl = lg_plan(a.B, a.N);
  if (!workspace || (((uintptr_t)workspace) & 255) || workspace_bytes < pl.bytes) return VCR_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  unsigned char* w = reinterpret_cast<unsigned char*>(workspace);
  int* winner = reinterpret_cast<int*>(w);
  int* flags = reinterpret_cast<int*>(w + pl.flag_off);
  int* blk = reinterpret_cast<int*>(w + pl.blk_off);
  const long total = (long)a.B * a.N;
  hipLaunchKernelGGL(largest_pick_kernel, dim3((unsigned)a.B), dim3(DB_BLOCK), 0, s, LgPick{a.sizes, a.N, winner});
  if ((e = VCR_LAUNCH_RC())) return e;
  hipLaunchKernelGGL(largest_member_kernel, dim3(db_blocks(total, DB_BLOCK)), dim3(DB_BLOCK), 0, s,
                     LgMember{a.labels, winner, a.N, total, flags});
  if ((e = VCR_LAUNCH_RC())) return e;
  return outlier_compact_flags(flags, a.xyz, a.B, a.N, blk, a.points, a.count, a.index, s);
}

// The voxel grid of voxel.hip by a stable radix sort, with member lists (include/vcr_hip_voxel_sort.h): the
// same definition and the same bits, in passes linear in N.
//
// A point's key is its three cells packed to the cloud's own width W = w_x + w_y + w_z (each axis as many bits as its largest
// cell needs, at most 21); a point without a voxel (a non-finite one, every point of a cloud whose grid is too fine) holds the
// single bit above W and sorts behind every voxel.  The sort (radix_sort.h) is stable and its input is in index order, so every
// voxel's members end up contiguous and in ascending index order; the order of the voxels among each other means nothing and
// is never returned.
//
// 10 + 3 rs_passes(d) launches:
//   vs_bounds_kernel   per tile of T points: the fp32 minimum and maximum over its finite points (exact in any order)
//   vs_fold_kernel     one workgroup per cloud folds the tiles': the origin in fp64, "too fine", per axis the cell of the
//                      maximum -- the largest cell, the cell being monotone in the coordinate -- and from it the widths, W and
//                      the passes the cloud needs, ceil((W + 1) / d); none for a cloud too fine or without a finite point
//   vs_keys_kernel     one lane per point: voxel_keys_kernel's cells (one fp64 subtraction, one fp64 division), packed
//   the sort           (key, index) into the cloud's own order
//   vs_heads_kernel    one lane per sorted slot: a head's key differs from its predecessor's; a head's index is its voxel's
//                      representative (the lowest, by stability) and learns its slot.  A point without a voxel: point_voxel -1
//   vs_count_kernel    one lane per point: the representatives per 256 points         } voxel.hip's merge / offsets / rank:
//   vs_offsets_kernel  one workgroup per cloud: their exclusive scan, count[b]        } the voxel numbers are the ranks of the
//   vs_rank_kernel     one lane per point: a representative's rank numbers its voxel  } representatives in index order
//   vs_means_kernel    one lane per voxel walks its own contiguous segment: one fp64 accumulator per coordinate that STARTS AS
//                      the first member, the additions in segment order -- the definition itself.  Four members a round are
//                      loaded ahead of the dependent adds; what lies beyond 65 members is staged by the lane's whole wave, 64
//                      members a round through LDS, two rounds of loads ahead of the owner's adds.  Writes points,
//                      voxel_points, point_voxel of every member, and the members per 256 voxels
//   vs_mstart_kernel   one workgroup per cloud: the exclusive scan of those, the number of finite points
//   vs_members_kernel  one lane per sorted slot moves its index into voxel order; the same lane, as a voxel, writes voxel_start
// No atomics but the sort's LDS counts, no scratch, no wait between workgroups.
#include "radix_sort.h"
#include "seg_scan.h"
#include "../../include/vcr_hip_voxel_sort.h"

namespace {

typedef unsigned long long u64;

constexpr int VS_BLOCK = WG_BLOCK;
constexpr int VS_MAX_N = 131072;                           // vcr_voxel_f32's limit
constexpr int VS_SOLO = 64;                                // members a lane adds on its own before its wave stages the rest
constexpr double VS_MAX_CELLS = (double)VCR_VOXEL_MAX_CELLS;

struct VsState {                                           // one per cloud
  double origin[3];
  int shift_y, shift_z, W;                                 // key = cx | cy << shift_y | cz << shift_z; W = the key's width
  int too_fine, voxels, nfinite;
  int pad[4];
};
static_assert(sizeof(VsState) == 64, "workspace layout");

struct VsBounds { float lo[3], hi[3]; };                   // of one tile
static_assert(sizeof(VsBounds) == 24, "workspace layout");

// A sorted index or slot as read from the workspace, held inside the cloud: the sort permutes 0 ... N-1, so this changes nothing
// -- it keeps a read or a write inside the buffers whatever the workspace holds.
__device__ __forceinline__ unsigned vs_inside(unsigned i, int N) { return i < (unsigned)N ? i : 0u; }

__device__ __forceinline__ bool vs_finite(float x, float y, float z) {
  const float inf = __builtin_huge_valf();
  return fabsf(x) < inf && fabsf(y) < inf && fabsf(z) < inf;
}

// The workgroup's minimum / maximum of three coordinates; thread 0 returns them.  wlo / whi [3][WG_WAVES].
__device__ __forceinline__ void vs_reduce_bounds(float lo[3], float hi[3], int t, float (*wlo)[WG_WAVES], float (*whi)[WG_WAVES]) {
#pragma unroll
  for (int c = 0; c < 3; ++c) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) { lo[c] = fminf(lo[c], __shfl_xor(lo[c], o, 64)); hi[c] = fmaxf(hi[c], __shfl_xor(hi[c], o, 64)); }
    if ((t & 63) == 0) { wlo[c][t >> 6] = lo[c]; whi[c][t >> 6] = hi[c]; }
  }
  __syncthreads();
  if (t == 0)
    for (int c = 0; c < 3; ++c)
      for (int w = 0; w < WG_WAVES; ++w) { lo[c] = fminf(lo[c], wlo[c][w]); hi[c] = fmaxf(hi[c], whi[c][w]); }
}

template <int E>
__global__ __launch_bounds__(VS_BLOCK) void vs_bounds_kernel(const float* xyz, int N, int nt, VsBounds* part) {
  __shared__ float wlo[3][WG_WAVES], whi[3][WG_WAVES];
  const int t = threadIdx.x;
  const int b = (int)(blockIdx.x / (unsigned)nt), k = (int)(blockIdx.x % (unsigned)nt);
  const float* __restrict__ x = xyz + (size_t)b * 3 * N;
  const float inf = __builtin_huge_valf();
  float lo[3] = {inf, inf, inf}, hi[3] = {-inf, -inf, -inf};
#pragma unroll
  for (int r = 0; r < E; ++r) {                            // (selects, no branch: the loads of every round are in flight together)
    const int i = k * (VS_BLOCK * E) + r * VS_BLOCK + t;
    const int j = i < N ? i : 0;
    const float v[3] = {x[j], x[N + j], x[2 * (size_t)N + j]};
    const bool ok = i < N && vs_finite(v[0], v[1], v[2]);
#pragma unroll
    for (int c = 0; c < 3; ++c) { lo[c] = ok ? fminf(lo[c], v[c]) : lo[c]; hi[c] = ok ? fmaxf(hi[c], v[c]) : hi[c]; }
  }
  vs_reduce_bounds(lo, hi, t, wlo, whi);
  if (t == 0) part[(size_t)b * nt + k] = VsBounds{{lo[0], lo[1], lo[2]}, {hi[0], hi[1], hi[2]}};
}

__device__ __forceinline__ int vs_width(double cell) {     // the bits of the largest cell, 0 ... 21
  const u64 c = (u64)cell;
  return c ? 64 - __clzll((long long)c) : 0;
}

__global__ __launch_bounds__(VS_BLOCK) void vs_fold_kernel(const VsBounds* part, int nt, float h, int bits, VsState* state, int* npass) {
  __shared__ float wlo[3][WG_WAVES], whi[3][WG_WAVES];
  const int t = threadIdx.x, b = blockIdx.x;
  const float inf = __builtin_huge_valf();
  float lo[3] = {inf, inf, inf}, hi[3] = {-inf, -inf, -inf};
  for (int k = t; k < nt; k += VS_BLOCK) {
    const VsBounds p = part[(size_t)b * nt + k];
#pragma unroll
    for (int c = 0; c < 3; ++c) { lo[c] = fminf(lo[c], p.lo[c]); hi[c] = fmaxf(hi[c], p.hi[c]); }
  }
  vs_reduce_bounds(lo, hi, t, wlo, whi);
  if (t == 0) {
    VsState g{{0., 0., 0.}, 0, 0, 0, 0, 0, 0, {0, 0, 0, 0}};
    int width[3] = {0, 0, 0};
    const bool any = lo[0] <= hi[0];                       // (a cloud without a finite point keeps (+inf, -inf))
    if (any)
      for (int c = 0; c < 3; ++c) {
        g.origin[c] = (double)lo[c] - 0.5 * (double)h;
        const double top = floor(((double)hi[c] - g.origin[c]) / (double)h);      // the largest cell: the cell is monotone
        if (!(top < VS_MAX_CELLS)) g.too_fine = 1;
        else width[c] = vs_width(top);
      }
    int passes = 0;
    if (any && !g.too_fine) {
      g.shift_y = width[0];
      g.shift_z = width[0] + width[1];
      g.W = width[0] + width[1] + width[2];                // <= 63
      passes = (g.W + 1 + bits - 1) / bits;                // the keys and the bit above them
    }
    state[b] = g;                                          // (W = 0 otherwise: every point holds bit 0, no pass is needed)
    npass[b] = passes;
  }
}

struct VsKeys { const float* xyz; const VsState* state; u64* keys; unsigned* idx; int N, nb; float h; };

__global__ __launch_bounds__(VS_BLOCK) void vs_keys_kernel(VsKeys p) {
  const int b = (int)(blockIdx.x / (unsigned)p.nb), blk = (int)(blockIdx.x % (unsigned)p.nb);
  const int i = blk * VS_BLOCK + (int)threadIdx.x, N = p.N;
  if (i >= N) return;
  const float* __restrict__ x = p.xyz + (size_t)b * 3 * N;
  const VsState g = p.state[b];
  const float v[3] = {x[i], x[N + i], x[2 * (size_t)N + i]};
  u64 key = 1ull << g.W;
  if (!g.too_fine && vs_finite(v[0], v[1], v[2])) {
    const double h = (double)p.h;
    const u64 cx = (u64)floor(((double)v[0] - g.origin[0]) / h);       // below 2^w_x: the fold saw the largest
    const u64 cy = (u64)floor(((double)v[1] - g.origin[1]) / h);
    const u64 cz = (u64)floor(((double)v[2] - g.origin[2]) / h);
    key = cz << g.shift_z | cy << g.shift_y | cx;
  }
  p.keys[(size_t)b * N + i] = key;
  p.idx[(size_t)b * N + i] = (unsigned)i;
}

struct VsSorted { const u64* keys[2]; const unsigned* idx[2]; const VsState* state; const int* npass; int N, nb; };

struct VsHeads { VsSorted s; int* headslot; int* point_voxel; };

__global__ __launch_bounds__(VS_BLOCK) void vs_heads_kernel(VsHeads p) {
  const int b = (int)(blockIdx.x / (unsigned)p.s.nb), blk = (int)(blockIdx.x % (unsigned)p.s.nb);
  const int s = blk * VS_BLOCK + (int)threadIdx.x, N = p.s.N;
  if (s >= N) return;
  const size_t row = (size_t)b * N;
  const int in = p.s.npass[b] & 1, W = p.s.state[b].W;
  const u64* __restrict__ key = p.s.keys[in] + row;
  const u64 k = key[s], prev = s ? key[s - 1] : ~0ull;
  const unsigned i = p.s.idx[in][row + s];
  if (i >= (unsigned)N) return;                            // (cannot happen: the sort permutes 0 ... N-1)
  const bool voxel = (k >> W) == 0;
  p.headslot[row + i] = voxel && (s == 0 || k != prev) ? s + 1 : 0;
  if (!voxel) p.point_voxel[row + i] = -1;
}

__global__ __launch_bounds__(VS_BLOCK) void vs_count_kernel(const int* headslot, int N, int nb, int* blkcnt) {
  __shared__ int wcnt[WG_WAVES];
  const int t = threadIdx.x;
  const int b = (int)(blockIdx.x / (unsigned)nb), blk = (int)(blockIdx.x % (unsigned)nb);
  const int i = blk * VS_BLOCK + t;
  int reps;
  wg_rank(i < N && headslot[(size_t)b * N + (i < N ? i : 0)] != 0, t, wcnt, &reps);
  if (t == 0) blkcnt[(size_t)b * nb + blk] = reps;
}

__global__ __launch_bounds__(VS_BLOCK) void vs_offsets_kernel(int* blkcnt, int nb, VsState* state, int* count) {
  __shared__ int wtot[WG_WAVES];
  const int b = blockIdx.x;
  const int voxels = wg_offsets(blkcnt + (size_t)b * nb, nb, wtot);
  if (threadIdx.x == 0) {
    state[b].voxels = voxels;                              // (0 when the grid is too fine: no point has a voxel)
    count[b] = state[b].too_fine ? -1 : voxels;
  }
}

__global__ __launch_bounds__(VS_BLOCK) void vs_rank_kernel(const int* headslot, const int* blkoff, int N, int nb, int* rep_slot) {
  __shared__ int wcnt[WG_WAVES];
  const int t = threadIdx.x;
  const int b = (int)(blockIdx.x / (unsigned)nb), blk = (int)(blockIdx.x % (unsigned)nb);
  const int i = blk * VS_BLOCK + t;
  const size_t row = (size_t)b * N;
  const int hs = i < N ? headslot[row + i] : 0;
  int reps;
  const int rank = wg_rank(hs != 0, t, wcnt, &reps);
  if (hs != 0) {
    const int v = blkoff[(size_t)b * nb + blk] + rank;     // < the cloud's voxels <= N
    if (v < N) rep_slot[row + v] = hs - 1;
  }
}

struct VsMeans {
  const float* xyz; VsSorted s; const int* rep_slot;
  float* points; int* point_voxel; int* voxel_points; int* below; int* blksum;      // below: the members of the lower voxels of the 256
};

// Orders the LDS traffic of ONE wave: what its lanes wrote in front of it is what any of its lanes reads behind it (a wave's LDS
// instructions execute in order; this keeps the compiler from moving them across).  No other wave is waited for.
__device__ __forceinline__ void vs_wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ u64 vs_shfl64(u64 v, int src) {
  const unsigned lo = (unsigned)__shfl((int)(unsigned)v, src, 64), hi = (unsigned)__shfl((int)(unsigned)(v >> 32), src, 64);
  return (u64)hi << 32 | lo;
}

__global__ __launch_bounds__(VS_BLOCK) void vs_means_kernel(VsMeans p) {
  __shared__ __attribute__((aligned(16))) double stage[WG_WAVES][3][64];
  __shared__ int wtot[WG_WAVES];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int b = (int)(blockIdx.x / (unsigned)p.s.nb), blk = (int)(blockIdx.x % (unsigned)p.s.nb);
  const int v = blk * VS_BLOCK + t, N = p.s.N;
  const size_t row = (size_t)b * N;
  const int in = p.s.npass[b] & 1, M = p.s.state[b].voxels;
  const float* __restrict__ x = p.xyz + row * 3;
  const u64* __restrict__ key = p.s.keys[in] + row;
  const unsigned* __restrict__ idx = p.s.idx[in] + row;
  int* __restrict__ pv = p.point_voxel + row;

  const bool own = v < M;                                  // the lane as a voxel (M <= N)
  int n = 0, next = N;                                     // next: the slot the wave goes on from
  u64 kq = 0;
  double sx = 0., sy = 0., sz = 0.;
  bool more = false;
  if (own) {
    const int s0 = (int)vs_inside((unsigned)p.rep_slot[row + v], N);
    kq = key[s0];
    const unsigned i0 = vs_inside(idx[s0], N);
    sx = (double)x[i0]; sy = (double)x[N + i0]; sz = (double)x[2 * (size_t)N + i0];       // the sum STARTS AS the first member
    pv[i0] = v;
    n = 1;
    int s = s0 + 1;
    bool go = true;
    for (int round = 0; round < VS_SOLO / 4 && go; ++round, s += 4) {
      u64 k[4];
      unsigned i[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {                        // four keys and four indices in flight, then twelve coordinates
        const bool inside = s + u < N;
        k[u] = inside ? key[s + u] : ~kq;
        i[u] = inside ? vs_inside(idx[s + u], N) : i0;
      }
      bool hit[4];
      float X[4], Y[4], Z[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        go = go && k[u] == kq;                             // (sorted: a voxel's slots are contiguous)
        hit[u] = go;
        const unsigned j = go ? i[u] : i0;
        X[u] = x[j]; Y[u] = x[N + j]; Z[u] = x[2 * (size_t)N + j];
      }
#pragma unroll
      for (int u = 0; u < 4; ++u)
        if (hit[u]) {
          sx += (double)X[u]; sy += (double)Y[u]; sz += (double)Z[u];
          pv[i[u]] = v;
          ++n;
        }
    }
    more = go;                                             // 65 members and the next slot not looked at yet
    next = s;
  }

  // What lies beyond: the wave stages 64 slots a round for one owner at a time.  Three rounds are in flight: round c's
  // coordinates are in registers when its turn comes, round c+1's indices are, round c+2's keys and indices are asked for.
  u64 todo = __ballot(more);
  while (todo) {                                           // (wave-uniform)
    const int L = __ffsll((long long)todo) - 1;
    todo &= todo - 1;
    const int s0 = __shfl(next, L, 64), vv = __shfl(v, L, 64);
    const u64 q = vs_shfl64(kq, L);
    // round c = 0: all of it; round 1: keys and indices
    int at = s0 + lane;
    bool hit0 = at < N && key[at < N ? at : 0] == q;
    unsigned i0 = hit0 ? vs_inside(idx[at], N) : 0u;
    double X = 0., Y = 0., Z = 0.;
    if (hit0) { X = (double)x[i0]; Y = (double)x[N + i0]; Z = (double)x[2 * (size_t)N + i0]; }
    at += 64;
    u64 k1 = at < N ? key[at] : ~q;
    unsigned i1 = at < N ? vs_inside(idx[at], N) : 0u;
    for (;;) {
      const int cnt = __popcll(__ballot(hit0));            // (sorted: the hits are the lowest lanes)
      double* st = &stage[w][0][0];
      vs_wave_lds_sync();                                  // (the owner has read the previous round)
      st[lane] = X; st[64 + lane] = Y; st[128 + lane] = Z;
      vs_wave_lds_sync();
      if (hit0) pv[i0] = vv;
      // round c+1's coordinates, round c+2's keys and indices: asked for in front of the owner's adds
      const bool hit1 = cnt == 64 && k1 == q;
      double X1 = 0., Y1 = 0., Z1 = 0.;
      if (hit1) { X1 = (double)x[i1]; Y1 = (double)x[N + i1]; Z1 = (double)x[2 * (size_t)N + i1]; }
      at += 64;
      const u64 k2 = at < N ? key[at] : ~q;
      const unsigned i2 = at < N ? vs_inside(idx[at], N) : 0u;
      if (lane == L) {
        if (cnt == 64) {
#pragma unroll
          for (int j0 = 0; j0 < 64; j0 += 8) {             // eight members of each coordinate read ahead of their adds
            double a[8], c[8], d[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) { a[j] = st[j0 + j]; c[j] = st[64 + j0 + j]; d[j] = st[128 + j0 + j]; }
#pragma unroll
            for (int j = 0; j < 8; ++j) { sx += a[j]; sy += c[j]; sz += d[j]; }
          }
        } else {
          for (int j = 0; j < cnt; ++j) { sx += st[j]; sy += st[64 + j]; sz += st[128 + j]; }
        }
        n += cnt;
      }
      if (cnt < 64) break;
      hit0 = hit1; i0 = i1; X = X1; Y = Y1; Z = Z1;
      k1 = k2; i1 = i2;
    }
  }

  int total;
  const int lower = wg_excl_scan(n, t, wtot, &total);
  if (t == 0) p.blksum[(size_t)b * p.s.nb + blk] = total;
  if (v < N) {
    const float nan = __uint_as_float(0x7FC00000u);
    float ox = nan, oy = nan, oz = nan;
    if (own) {
      const double dn = (double)n;
      ox = (float)(sx / dn); oy = (float)(sy / dn); oz = (float)(sz / dn);       // (n = 1: the point's own bits, -0.0 included)
    }
    float* o = p.points + row * 3;
    o[v] = ox; o[N + v] = oy; o[2 * (size_t)N + v] = oz;
    p.voxel_points[row + v] = n;
    p.below[row + v] = lower;
  }
}

__global__ __launch_bounds__(VS_BLOCK) void vs_mstart_kernel(int* blksum, int nb, VsState* state) {
  __shared__ int wtot[WG_WAVES];
  const int b = blockIdx.x;
  const int finite = wg_offsets(blksum + (size_t)b * nb, nb, wtot);
  if (threadIdx.x == 0) state[b].nfinite = finite;
}

struct VsMembers { VsSorted s; const int* rep_slot; const int* point_voxel; const int* below; const int* blkoff; int* members; int* voxel_start; };

__global__ __launch_bounds__(VS_BLOCK) void vs_members_kernel(VsMembers p) {
  const int b = (int)(blockIdx.x / (unsigned)p.s.nb), blk = (int)(blockIdx.x % (unsigned)p.s.nb);
  const int s = blk * VS_BLOCK + (int)threadIdx.x, N = p.s.N;
  if (s >= N) return;
  const size_t row = (size_t)b * N;
  const VsState g = p.s.state[b];
  const int* __restrict__ blkoff = p.blkoff + (size_t)b * p.s.nb;
  if (p.voxel_start)                                       // the lane as a voxel
    p.voxel_start[row + s] = s < g.voxels ? blkoff[blk] + p.below[row + s] : g.nfinite;
  if (!p.members) return;
  if (s >= g.nfinite) p.members[row + s] = -1;             // (the finite points fill the slots in front)
  const int in = p.s.npass[b] & 1;
  if ((p.s.keys[in][row + s] >> g.W) != 0) return;         // the lane as a sorted slot: a point without a voxel moves nowhere
  const unsigned i = vs_inside(p.s.idx[in][row + s], N);
  const int v = p.point_voxel[row + i];
  if ((unsigned)v >= (unsigned)g.voxels) return;           // (cannot happen)
  const int to = blkoff[v / VS_BLOCK] + p.below[row + v] + (s - p.rep_slot[row + v]);
  if ((unsigned)to < (unsigned)N) p.members[row + to] = (int)i;
}

// How one call runs: vs_plan() validates both structs, picks the digit width and the elements per lane and lays out the
// workspace; the entry points answer from it.  The plan's width is 11, the widest: a call is bound by the NUMBER of its launches
// (about 4 us each, a pass that a cloud does not need included), and 11 bits launch six passes where 8 launch eight.  Measured
// (profiles/voxel_sort_bench.txt): 11 bits beat 8 by 10 % on 131 072 points of one point a voxel and on
// 16 x 1 024, tie on 131 072 points at 8 a voxel, lose 6 % on 16 x 16 384; 4 bits lose everywhere.
struct VsPlan {
  vcr_voxel_args a;
  vcr_voxel_sort_args sa;
  int bits, per_lane, nt, nb;
  size_t npass_off, part_off, keys_off, keys_bytes, idx_off, idx_bytes, hist_off, tot_off, plane_off, plane_bytes, blk_off, blk_bytes, bytes;
};

constexpr int VS_PLAN_BITS = 11;

int vs_per_lane(int bits) { return bits == 11 ? 8 : 4; }

}  // namespace

static int vs_plan(const vcr_voxel_args& a, const vcr_voxel_sort_args& sa, VsPlan* p) {
  *p = VsPlan{a, sa};
  if (!a.xyz || !a.points || !a.count || a.B < 1) return VCR_EINVAL;
  if (!(a.voxel_size > 0.f) || a.voxel_size == __builtin_huge_valf()) return VCR_EINVAL;     // <= 0, NaN, +inf
  if (a.variant != 0) return VCR_EINVAL;                   // the scan's forms do not apply
  if (sa.variant != 0 && sa.variant != 4 && sa.variant != 8 && sa.variant != 11) return VCR_EINVAL;
  if (a.N < 1 || a.N > VS_MAX_N || (long)a.B * a.N >= (1L << 31)) return VCR_EUNSUPPORTED;
  p->bits = sa.variant ? sa.variant : VS_PLAN_BITS;
  p->per_lane = vs_per_lane(p->bits);
  const int T = VS_BLOCK * p->per_lane;
  p->nt = (a.N + T - 1) / T;
  p->nb = (a.N + VS_BLOCK - 1) / VS_BLOCK;
  const size_t B = (size_t)a.B, BN = B * a.N, R = (size_t)1 << p->bits;
  p->npass_off = ws_up(B * sizeof(VsState));
  p->part_off = p->npass_off + ws_up(B * 4);
  p->keys_off = p->part_off + ws_up(B * p->nt * sizeof(VsBounds));
  p->keys_bytes = ws_up(BN * 8);
  p->idx_off = p->keys_off + 2 * p->keys_bytes;
  p->idx_bytes = ws_up(BN * 4);
  p->hist_off = p->idx_off + 2 * p->idx_bytes;
  p->tot_off = p->hist_off + ws_up(B * R * p->nt * 4);
  p->plane_off = p->tot_off + ws_up(B * R * 4);
  p->plane_bytes = ws_up(BN * 4);
  p->blk_off = p->plane_off + 5 * p->plane_bytes;
  p->blk_bytes = ws_up(B * p->nb * 4);
  p->bytes = p->blk_off + 2 * p->blk_bytes;
  return VCR_OK;
}

static int vs_take(const vcr_voxel_args* ua, const vcr_voxel_sort_args* us, vcr_voxel_args* a, vcr_voxel_sort_args* sa) {
  if (vcr_take_args(ua, a, offsetof(vcr_voxel_args, point_voxel))) return VCR_EINVAL;
  return vcr_take_args(us, sa, offsetof(vcr_voxel_sort_args, members));
}

extern "C" int vcr_voxel_sort_form(const vcr_voxel_args* ua, const vcr_voxel_sort_args* us, int cu_count, int* digit_bits, int* passes,
                                   int* elements_per_lane) {
  vcr_voxel_args a;
  vcr_voxel_sort_args sa;
  VsPlan p;
  if (vs_take(ua, us, &a, &sa) || cu_count < 0) return VCR_EINVAL;
  const int e = vs_plan(a, sa, &p);
  if (e) return e;
  if (digit_bits) *digit_bits = p.bits;
  if (passes) *passes = rs_passes(p.bits);
  if (elements_per_lane) *elements_per_lane = p.per_lane;
  return VCR_OK;
}

extern "C" size_t vcr_voxel_sort_workspace_bytes(const vcr_voxel_args* ua, const vcr_voxel_sort_args* us, int cu_count) {
  vcr_voxel_args a;
  vcr_voxel_sort_args sa;
  VsPlan p;
  if (vs_take(ua, us, &a, &sa) || cu_count < 0) return 0;
  return vs_plan(a, sa, &p) ? 0 : p.bytes;
}

template <int BITS, int E>
static int vs_front(const VsPlan& p, const RsSort& rs, VsBounds* part, VsState* state, int* npass, hipStream_t s) {
  const vcr_voxel_args& a = p.a;
  int e;
  hipLaunchKernelGGL((vs_bounds_kernel<E>), dim3((unsigned)((long)a.B * p.nt)), dim3(VS_BLOCK), 0, s, a.xyz, a.N, p.nt, part);
  if ((e = VCR_LAUNCH_RC())) return e;
  hipLaunchKernelGGL(vs_fold_kernel, dim3((unsigned)a.B), dim3(VS_BLOCK), 0, s, (const VsBounds*)part, p.nt, a.voxel_size, BITS, state, npass);
  if ((e = VCR_LAUNCH_RC())) return e;
  const VsKeys ky{a.xyz, state, rs.keys[0], rs.vals[0], a.N, p.nb, a.voxel_size};
  hipLaunchKernelGGL(vs_keys_kernel, dim3((unsigned)((long)a.B * p.nb)), dim3(VS_BLOCK), 0, s, ky);
  if ((e = VCR_LAUNCH_RC())) return e;
  return rs_sort_launch<BITS, E>(rs, a.B, s);
}

extern "C" int vcr_voxel_sort_f32(const vcr_voxel_args* ua, const vcr_voxel_sort_args* us, void* workspace, size_t workspace_bytes,
                                  vcr_stream_t stream) {
  vcr_voxel_args a;
  vcr_voxel_sort_args sa;
  if (vs_take(ua, us, &a, &sa)) return VCR_EINVAL;
  VsPlan p;
  int e = vs_plan(a, sa, &p);
  if (e) return e;
  if (!workspace || (((uintptr_t)workspace) & 15)) return VCR_EINVAL;
  if (workspace_bytes < p.bytes) return VCR_EWORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  unsigned char* w = reinterpret_cast<unsigned char*>(workspace);
  VsState* state = reinterpret_cast<VsState*>(w);
  int* npass = reinterpret_cast<int*>(w + p.npass_off);
  VsBounds* part = reinterpret_cast<VsBounds*>(w + p.part_off);
  RsSort rs{};
  for (int k = 0; k < 2; ++k) {
    rs.keys[k] = reinterpret_cast<u64*>(w + p.keys_off + k * p.keys_bytes);
    rs.vals[k] = reinterpret_cast<unsigned*>(w + p.idx_off + k * p.idx_bytes);
  }
  rs.hist = reinterpret_cast<int*>(w + p.hist_off);
  rs.tot = reinterpret_cast<int*>(w + p.tot_off);
  rs.npass = npass;
  rs.N = a.N;
  rs.nt = p.nt;
  auto plane = [&](int k) { return reinterpret_cast<int*>(w + p.plane_off + k * p.plane_bytes); };
  int* headslot = plane(0);
  int* rep_slot = plane(1);
  int* below = plane(2);
  int* point_voxel = a.point_voxel ? a.point_voxel : plane(3);        // an output nobody asked for lands in the workspace
  int* voxel_points = a.voxel_points ? a.voxel_points : plane(4);
  int* blkcnt = reinterpret_cast<int*>(w + p.blk_off);
  int* blksum = reinterpret_cast<int*>(w + p.blk_off + p.blk_bytes);
  const dim3 block(VS_BLOCK), clouds((unsigned)a.B), points((unsigned)((long)a.B * p.nb));

  e = p.bits == 4 ? vs_front<4, 4>(p, rs, part, state, npass, s)
    : p.bits == 8 ? vs_front<8, 4>(p, rs, part, state, npass, s)
                  : vs_front<11, 8>(p, rs, part, state, npass, s);
  if (e) return e;
  const VsSorted so{{rs.keys[0], rs.keys[1]}, {rs.vals[0], rs.vals[1]}, state, npass, a.N, p.nb};
  const VsHeads hd{so, headslot, point_voxel};
  hipLaunchKernelGGL(vs_heads_kernel, points, block, 0, s, hd);
  if ((e = VCR_LAUNCH_RC())) return e;
  hipLaunchKernelGGL(vs_count_kernel, points, block, 0, s, (const int*)headslot, a.N, p.nb, blkcnt);
  if ((e = VCR_LAUNCH_RC())) return e;
  hipLaunchKernelGGL(vs_offsets_kernel, clouds, block, 0, s, blkcnt, p.nb, state, a.count);
  if ((e = VCR_LAUNCH_RC())) return e;
  hipLaunchKernelGGL(vs_rank_kernel, points, block, 0, s, (const int*)headslot, (const int*)blkcnt, a.N, p.nb, rep_slot);
  if ((e = VCR_LAUNCH_RC())) return e;
  const VsMeans mn{a.xyz, so, rep_slot, a.points, point_voxel, voxel_points, below, blksum};
  hipLaunchKernelGGL(vs_means_kernel, points, block, 0, s, mn);
  if ((e = VCR_LAUNCH_RC())) return e;
  hipLaunchKernelGGL(vs_mstart_kernel, clouds, block, 0, s, blksum, p.nb, state);
  if ((e = VCR_LAUNCH_RC())) return e;
  const VsMembers mb{so, rep_slot, point_voxel, below, blksum, sa.members, sa.voxel_start};
  hipLaunchKernelGGL(vs_members_kernel, points, block, 0, s, mb);
  return VCR_LAUNCH_RC();
}

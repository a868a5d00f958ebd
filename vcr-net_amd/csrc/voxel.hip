// Down-sampling a cloud on a voxel grid (include/vcr_hip_voxel.h): the points of one grid cell are replaced
// by their mean, the voxels numbered in order of first appearance, every sum in ascending point order in fp64.
//
// A point's voxel is a 64-bit key (its three cells, 21 bits each); "the same voxel" is one integer equality, so the search is
// nn_scan_kernel's brute-force scan (nn_scan.h) with a cheaper pair operation, and every fold of it is an exact integer
// operation: any split of the scan returns the same bits.  A point without a voxel (a non-finite one, every point of a cloud
// whose grid is too fine) stores VX_NO_KEY and asks for VX_NO_QUERY, which is never stored: it matches nobody, itself included.
//
// Seven launches (voxel_plan cuts the scan as nn_plan does, seg_scan.h; vcr_voxel_args.variant forces it):
//   voxel_bounds_kernel   one workgroup per cloud: min and max over the finite points, the grid's origin in fp64, "too fine"
//   voxel_keys_kernel     one lane per point: its key
//   voxel_scan_kernel     256 lanes x one point per lane against one of the S segments of the cloud's own key plane: tiles of
//                         NN_TILE keys staged into LDS, read back two keys a ds_read_b128 with one address for all lanes; per
//                         pair one 64-bit equality, the number of matches and -- in the tiles that do not lie behind the
//                         workgroup's own points -- the lowest matching index
//   voxel_merge_kernel    one lane per point: the first match of the lowest segment that has one, the matches added; a point
//                         whose first match is itself is its voxel's representative: one count of them per 256 points
//   voxel_offsets_kernel  one workgroup per cloud: the exclusive scan of those counts, count[b]
//   voxel_rank_kernel     one lane per point: a representative's rank among its 256 gives its voxel its number
//   voxel_means_kernel    one lane per OUTPUT voxel walks the key plane and the three coordinate planes from its
//                         representative's tile to the cloud's end, unsplit: ascending order, one accumulator -- the definition
//                         itself.  Matches are rare: sixteen keys a round, the fp64 adds behind ONE branch; a voxel of one
//                         point copies it.  The same lane, as a point, looks up point_voxel.
// No atomics, no scratch, no loop whose trip count depends on anything but N, S and a tile index.
#include "nn_scan.h"
#include "../../include/vcr_hip_voxel.h"

namespace {

typedef unsigned long long u64;
typedef u64 u64x2 __attribute__((ext_vector_type(2)));

constexpr u64 VX_NO_KEY = ~0ull;                           // stored for a point without a voxel, and behind a tile's end
constexpr u64 VX_NO_QUERY = ~0ull - 1;                     // what a lane without a voxel looks for: never stored
constexpr double VX_MAX_CELLS = (double)VCR_VOXEL_MAX_CELLS;

struct VxGrid { double origin[3]; int too_fine; int voxels; };   // one per cloud
static_assert(sizeof(VxGrid) == 32, "workspace layout");

__device__ __forceinline__ bool vx_finite(float x, float y, float z) {
  const float inf = __builtin_huge_valf();
  return fabsf(x) < inf && fabsf(y) < inf && fabsf(z) < inf;
}

__global__ __launch_bounds__(NN_BLOCK) void voxel_bounds_kernel(const float* xyz, int N, float h, VxGrid* grid) {
  __shared__ float wlo[3][NN_BLOCK / 64], whi[3][NN_BLOCK / 64];
  const int t = threadIdx.x, b = blockIdx.x;
  const float* __restrict__ x = xyz + (size_t)b * 3 * N;
  const float inf = __builtin_huge_valf();
  float lo[3] = {inf, inf, inf}, hi[3] = {-inf, -inf, -inf};
#pragma unroll 4
  for (int i = t; i < N; i += NN_BLOCK) {                  // (selects, no branch: the loads of four rounds are in flight together)
    const float v[3] = {x[i], x[N + i], x[2 * (size_t)N + i]};
    const bool ok = vx_finite(v[0], v[1], v[2]);
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
    VxGrid g{{0., 0., 0.}, 0, 0};
    for (int c = 0; c < 3; ++c) {
      float l = wlo[c][0], u = whi[c][0];
      for (int w = 1; w < NN_BLOCK / 64; ++w) { l = fminf(l, wlo[c][w]); u = fmaxf(u, whi[c][w]); }
      if (l <= u) {                                        // (a cloud without a finite point keeps (+inf, -inf): no key is made)
        g.origin[c] = (double)l - 0.5 * (double)h;
        // the cell is monotone in the coordinate: the maximum's cell decides
        if (!(floor(((double)u - g.origin[c]) / (double)h) < VX_MAX_CELLS)) g.too_fine = 1;
      }
    }
    grid[b] = g;
  }
}

struct VxKeys { const float* xyz; const VxGrid* grid; u64* keys; int N, nblk; float h; };

__global__ __launch_bounds__(NN_BLOCK) void voxel_keys_kernel(VxKeys p) {
  const int b = (int)(blockIdx.x / (unsigned)p.nblk), blk = (int)(blockIdx.x % (unsigned)p.nblk);
  const int i = blk * NN_BLOCK + (int)threadIdx.x, N = p.N;
  if (i >= N) return;
  const float* __restrict__ x = p.xyz + (size_t)b * 3 * N;
  const VxGrid g = p.grid[b];
  const float v[3] = {x[i], x[N + i], x[2 * (size_t)N + i]};
  u64 key = VX_NO_KEY;
  if (!g.too_fine && vx_finite(v[0], v[1], v[2])) {
    const double h = (double)p.h;
    const u64 cx = (u64)floor(((double)v[0] - g.origin[0]) / h);       // in [0, 2^21): the bounds kernel saw the largest
    const u64 cy = (u64)floor(((double)v[1] - g.origin[1]) / h);
    const u64 cz = (u64)floor(((double)v[2] - g.origin[2]) / h);
    key = cz << 42 | cy << 21 | cx;
  }
  p.keys[(size_t)b * N + i] = key;
}

// A tile of keys [t0, t0 + cnt) of one cloud's plane into LDS, padded to `padded` (a multiple of the keys a loop round reads,
// <= NN_TILE) with keys nobody looks for
__device__ __forceinline__ void vx_stage_keys(u64* lk, const u64* __restrict__ key, int t0, int cnt, int padded, int t) {
  for (int i = t; i < padded; i += NN_BLOCK) lk[i] = i < cnt ? key[t0 + i] : VX_NO_KEY;
}

// One staged tile against the lane's key: the matches counted and, with FIRST, the lowest matching index kept (j ascends)
template <bool FIRST>
__device__ __forceinline__ void vx_scan_tile(const u64* lk, int cnt4, int t0, u64 kq, unsigned& first, int& members) {
  for (int j = 0; j < cnt4; j += 4) {
    const u64x2 k01 = *reinterpret_cast<const u64x2*>(lk + j), k23 = *reinterpret_cast<const u64x2*>(lk + j + 2);
    const u64 k[4] = {k01[0], k01[1], k23[0], k23[1]};                // one address for every lane: broadcast reads
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const bool eq = k[u] == kq;
      if (FIRST) {
        const unsigned at = eq ? (unsigned)(t0 + j + u) : ~0u;
        first = at < first ? at : first;
      }
      members += eq ? 1 : 0;
    }
  }
}

struct VxScan {
  const u64* keys;
  int B, N, S, seg_len, nblk;                              // nblk = ceil(N / 256)
  int* part_first; int* part_members;                      // [S][B][N]
};

__global__ __launch_bounds__(NN_BLOCK) void voxel_scan_kernel(VxScan p) {
  __shared__ __attribute__((aligned(16))) u64 lk[NN_TILE];
  const int t = threadIdx.x;
  int s, blk, b;
  seg_workgroup(blockIdx.x, p.S, p.nblk, &s, &blk, &b);
  const int N = p.N;
  const u64* __restrict__ key = p.keys + (size_t)b * N;
  const int i = blk * NN_BLOCK + t;
  u64 kq = i < N ? key[i] : VX_NO_QUERY;
  kq = kq == VX_NO_KEY ? VX_NO_QUERY : kq;
  unsigned first = ~0u;                                    // (reads as -1: no match) the lowest matching index: j ascends
  int members = 0;

  int lo, hi;
  seg_range(s, p.seg_len, N, &lo, &hi);
  for (int t0 = lo; t0 < hi; t0 += NN_TILE) {                          // (workgroup-uniform: the barriers are met by all)
    const int cnt = hi - t0 < NN_TILE ? hi - t0 : NN_TILE;
    const int cnt4 = (cnt + 3) & ~3;                                   // <= NN_TILE
    __syncthreads();                                                   // the previous tile has been read
    vx_stage_keys(lk, key, t0, cnt, cnt4, t);
    __syncthreads();
    // a tile that starts behind the workgroup's last point cannot hold anybody's lowest match (a point matches itself)
    if (t0 >= (blk + 1) * NN_BLOCK) vx_scan_tile<false>(lk, cnt4, t0, kq, first, members);
    else vx_scan_tile<true>(lk, cnt4, t0, kq, first, members);
  }
  if (i < N) {
    const size_t at = ((size_t)s * p.B + b) * (size_t)N + i;
    p.part_first[at] = (int)first;
    p.part_members[at] = members;
  }
}

struct VxMerge {
  const int* part_first; const int* part_members;
  int B, N, S, nblk;
  int* first; int* members; int* blkcnt;                   // [B][N], [B][N], [B][nblk]
};

__global__ __launch_bounds__(NN_BLOCK) void voxel_merge_kernel(VxMerge p) {
  __shared__ int wcnt[NN_BLOCK / 64];
  const int t = threadIdx.x;
  const int b = (int)(blockIdx.x / (unsigned)p.nblk), blk = (int)(blockIdx.x % (unsigned)p.nblk);
  const int i = blk * NN_BLOCK + t;
  int f = -1, m = 0;
  if (i < p.N) {
    for (int s = 0; s < p.S; ++s) {                        // ascending segments = ascending index: the lowest that has a match
      const size_t at = ((size_t)s * p.B + b) * (size_t)p.N + i;
      const int pf = p.part_first[at];
      f = f < 0 ? pf : f;
      m += p.part_members[at];
    }
    const size_t o = (size_t)b * p.N + i;
    p.first[o] = f;
    p.members[o] = m;
  }
  int reps;
  wg_rank(i < p.N && f == i, t, wcnt, &reps);
  if (t == 0) p.blkcnt[(size_t)b * p.nblk + blk] = reps;
}

__global__ __launch_bounds__(NN_BLOCK) void voxel_offsets_kernel(int* blkcnt, int nblk, VxGrid* grid, int* count) {
  __shared__ int wtot[NN_BLOCK / 64];
  const int b = blockIdx.x;
  const int voxels = wg_offsets(blkcnt + (size_t)b * nblk, nblk, wtot);
  if (threadIdx.x == 0) {
    const int fine = grid[b].too_fine;
    grid[b].voxels = voxels;                               // (0 when the grid is too fine: no point has a key)
    count[b] = fine ? -1 : voxels;
  }
}

struct VxRank {
  const int* first; const int* members; const int* blkoff;
  int N, nblk;
  int* vox; int* rep_of; int* voxel_points;                // [B][N] each; voxel_points optional
};

__global__ __launch_bounds__(NN_BLOCK) void voxel_rank_kernel(VxRank p) {
  __shared__ int wcnt[NN_BLOCK / 64];
  const int t = threadIdx.x;
  const int b = (int)(blockIdx.x / (unsigned)p.nblk), blk = (int)(blockIdx.x % (unsigned)p.nblk);
  const int i = blk * NN_BLOCK + t;
  const size_t row = (size_t)b * p.N;
  const bool rep = i < p.N && p.first[row + (i < p.N ? i : 0)] == i;
  int reps;
  const int rank = wg_rank(rep, t, wcnt, &reps);
  if (rep) {
    const int v = p.blkoff[(size_t)b * p.nblk + blk] + rank;          // < the cloud's voxels <= N
    p.vox[row + i] = v;
    p.rep_of[row + v] = i;
    if (p.voxel_points) p.voxel_points[row + v] = p.members[row + i];
  }
}

struct VxMeans {
  const float* xyz; const u64* keys; const VxGrid* grid;
  const int* first; const int* members; const int* vox; const int* rep_of;
  int N, nblk;
  float* points; int* point_voxel; int* voxel_points;
};

__global__ __launch_bounds__(NN_BLOCK) void voxel_means_kernel(VxMeans p) {
  __shared__ __attribute__((aligned(16))) u64 lk[NN_TILE];
  __shared__ __attribute__((aligned(16))) float lx[NN_TILE], ly[NN_TILE], lz[NN_TILE];
  __shared__ int wmin[NN_BLOCK / 64];
  const int t = threadIdx.x;
  const int b = (int)(blockIdx.x / (unsigned)p.nblk), blk = (int)(blockIdx.x % (unsigned)p.nblk);
  const int v = blk * NN_BLOCK + t, N = p.N;
  const size_t row = (size_t)b * N;
  const float* __restrict__ x = p.xyz + row * 3;
  const u64* __restrict__ key = p.keys + row;
  const int M = p.grid[b].voxels;

  if (v < N && p.point_voxel) {                            // the lane as a point
    const int f = p.first[row + v];
    p.point_voxel[row + v] = f >= 0 ? p.vox[row + f] : -1;
  }
  const bool own = v < M;                                  // the lane as a voxel (M <= N)
  int rep = 0, n = 0;
  double sx = 0., sy = 0., sz = 0.;
  float px = 0.f, py = 0.f, pz = 0.f;
  u64 kq = VX_NO_QUERY;
  if (own) {
    rep = p.rep_of[row + v];
    n = p.members[row + rep];
    px = x[rep]; py = x[N + rep]; pz = x[2 * (size_t)N + rep];
    sx = (double)px; sy = (double)py; sz = (double)pz;    // the sum STARTS AS the first member
    if (n > 1) kq = key[rep];
  }
  // the tiles from the lowest representative that has a second member (the lanes' ascend with v) to the cloud's end
  int start = own && n > 1 ? rep : N;
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) { const int other = __shfl_xor(start, o, 64); start = other < start ? other : start; }
  if ((t & 63) == 0) wmin[t >> 6] = start;
  __syncthreads();
  for (int w = 0; w < NN_BLOCK / 64; ++w) start = wmin[w] < start ? wmin[w] : start;
  for (int t0 = start < N ? start / NN_TILE * NN_TILE : N; t0 < N; t0 += NN_TILE) {      // (workgroup-uniform, as the barriers need)
    const int cnt = N - t0 < NN_TILE ? N - t0 : NN_TILE;
    const int cnt16 = (cnt + 15) & ~15;                                // <= NN_TILE
    __syncthreads();
    vx_stage_keys(lk, key, t0, cnt, cnt16, t);
    for (int i = t; i < cnt16; i += NN_BLOCK) {
      const int g = t0 + (i < cnt ? i : 0);
      lx[i] = x[g]; ly[i] = x[N + g]; lz[i] = x[2 * (size_t)N + g];
    }
    __syncthreads();
    for (int j = 0; j < cnt16; j += 16) {                              // sixteen keys a round: eight reads in flight, ONE branch
      u64x2 k[8];
#pragma unroll
      for (int q = 0; q < 8; ++q) k[q] = *reinterpret_cast<const u64x2*>(lk + j + 2 * q);
      bool hit[4];
#pragma unroll
      for (int g = 0; g < 4; ++g) hit[g] = k[2 * g][0] == kq || k[2 * g][1] == kq || k[2 * g + 1][0] == kq || k[2 * g + 1][1] == kq;
      if (hit[0] || hit[1] || hit[2] || hit[3]) {
#pragma unroll
        for (int g = 0; g < 4; ++g)
          if (hit[g]) {
            const f32x4 X = ld4(lx + j + 4 * g), Y = ld4(ly + j + 4 * g), Z = ld4(lz + j + 4 * g);
#pragma unroll
            for (int u = 0; u < 4; ++u)
              if (k[2 * g + (u >> 1)][u & 1] == kq && t0 + j + 4 * g + u != rep) {       // (a match is never below the representative)
                sx += (double)X[u]; sy += (double)Y[u]; sz += (double)Z[u];
              }
          }
      }
    }
  }
  if (v < N) {
    const float nan = __uint_as_float(0x7FC00000u);
    float ox = nan, oy = nan, oz = nan;
    if (own) {
      const double dn = (double)n;
      ox = n > 1 ? (float)(sx / dn) : px; oy = n > 1 ? (float)(sy / dn) : py; oz = n > 1 ? (float)(sz / dn) : pz;
    } else if (p.voxel_points) {
      p.voxel_points[row + v] = 0;
    }
    float* o = p.points + row * 3;
    o[v] = ox; o[N + v] = oy; o[2 * (size_t)N + v] = oz;
  }
}

// How one call runs: voxel_plan() validates the arguments, cuts the scan as nn_plan cuts B clouds of N points against
// themselves, one point per lane (seg_split under NN_LIMITS), and lays out the workspace; the entry points answer from it.
struct VxPlan {
  vcr_voxel_args a;
  SegSplit scan;                                           // (one point per lane: its nblk is the per-point launches' too)
  unsigned point_grid;
  size_t keys_off, part_off, part_bytes, plane_off, plane_bytes, blk_off, bytes;
};

}  // namespace

static int voxel_plan(const vcr_voxel_args& a, int cu, VxPlan* p) {
  *p = VxPlan{a};
  if (!a.xyz || !a.points || !a.count || a.B < 1) return VCR_EINVAL;
  if (!(a.voxel_size > 0.f) || a.voxel_size == __builtin_huge_valf()) return VCR_EINVAL;     // <= 0, NaN, +inf
  int fq, fs;
  if (seg_variant(a.variant, SEG_Q_1, NN_LIMITS, &fq, &fs)) return VCR_EINVAL;
  if (a.N < 1 || a.N > NN_MAX_N || (long)a.B * a.N >= (1L << 31)) return VCR_EUNSUPPORTED;
  const int e = seg_split(a.B, a.N, a.N, 1, fs, cu, NN_LIMITS, &p->scan);
  if (e) return e;
  p->point_grid = (unsigned)((long)a.B * p->scan.nblk);
  const size_t BN = (size_t)a.B * a.N;
  p->keys_off = ws_up((size_t)a.B * sizeof(VxGrid));
  p->part_off = p->keys_off + ws_up(BN * 8);
  p->part_bytes = ws_up((size_t)p->scan.S * BN * 4);
  p->plane_off = p->part_off + 2 * p->part_bytes;
  p->plane_bytes = ws_up(BN * 4);
  p->blk_off = p->plane_off + 4 * p->plane_bytes;
  p->bytes = p->blk_off + ws_up((size_t)a.B * p->scan.nblk * 4);
  return VCR_OK;
}

static int voxel_take(const vcr_voxel_args* user, vcr_voxel_args* mine) {
  return vcr_take_args(user, mine, offsetof(vcr_voxel_args, point_voxel));
}

extern "C" int vcr_voxel_form(const vcr_voxel_args* ua, int cu_count, int* points_per_lane, int* splits) {
  vcr_voxel_args a;
  VxPlan p;
  if (voxel_take(ua, &a) || cu_count < 0) return VCR_EINVAL;
  const int e = voxel_plan(a, cu_count ? cu_count : vcr_cu_count(), &p);
  if (e) return e;
  if (points_per_lane) *points_per_lane = 1;
  if (splits) *splits = p.scan.S;
  return VCR_OK;
}

extern "C" size_t vcr_voxel_workspace_bytes(const vcr_voxel_args* ua, int cu_count) {
  vcr_voxel_args a;
  VxPlan p;
  if (voxel_take(ua, &a) || cu_count < 0) return 0;
  return voxel_plan(a, cu_count ? cu_count : vcr_cu_count(), &p) ? 0 : p.bytes;
}

extern "C" int vcr_voxel_f32(const vcr_voxel_args* ua, void* workspace, size_t workspace_bytes, vcr_stream_t stream) {
  vcr_voxel_args a;
  if (voxel_take(ua, &a)) return VCR_EINVAL;
  // the argument checks need no device: only a call that passes them asks for the CU count
  VxPlan p;
  int e = voxel_plan(a, 1, &p);
  if (e) return e;
  if (!workspace || (((uintptr_t)workspace) & 15)) return VCR_EINVAL;
  vcr_stream_scope scope_(stream);
  e = voxel_plan(a, vcr_cu_count(), &p);
  if (e) return e;
  if (workspace_bytes < p.bytes) return VCR_EWORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  unsigned char* w = reinterpret_cast<unsigned char*>(workspace);
  VxGrid* grid = reinterpret_cast<VxGrid*>(w);
  u64* keys = reinterpret_cast<u64*>(w + p.keys_off);
  int* part_first = reinterpret_cast<int*>(w + p.part_off);
  int* part_members = reinterpret_cast<int*>(w + p.part_off + p.part_bytes);
  int* first = reinterpret_cast<int*>(w + p.plane_off);
  int* members = reinterpret_cast<int*>(w + p.plane_off + p.plane_bytes);
  int* vox = reinterpret_cast<int*>(w + p.plane_off + 2 * p.plane_bytes);
  int* rep_of = reinterpret_cast<int*>(w + p.plane_off + 3 * p.plane_bytes);
  int* blk = reinterpret_cast<int*>(w + p.blk_off);
  const dim3 block(NN_BLOCK), clouds((unsigned)a.B), points(p.point_grid);

  hipLaunchKernelGGL(voxel_bounds_kernel, clouds, block, 0, s, a.xyz, a.N, a.voxel_size, grid);
  if ((e = VCR_LAUNCH_RC())) return e;
  const VxKeys ky{a.xyz, grid, keys, a.N, p.scan.nblk, a.voxel_size};
  hipLaunchKernelGGL(voxel_keys_kernel, points, block, 0, s, ky);
  if ((e = VCR_LAUNCH_RC())) return e;
  const VxScan sc{keys, a.B, a.N, p.scan.S, p.scan.seg_len, p.scan.nblk, part_first, part_members};
  hipLaunchKernelGGL(voxel_scan_kernel, dim3(p.scan.grid), block, 0, s, sc);
  if ((e = VCR_LAUNCH_RC())) return e;
  const VxMerge mg{part_first, part_members, a.B, a.N, p.scan.S, p.scan.nblk, first, members, blk};
  hipLaunchKernelGGL(voxel_merge_kernel, points, block, 0, s, mg);
  if ((e = VCR_LAUNCH_RC())) return e;
  hipLaunchKernelGGL(voxel_offsets_kernel, clouds, block, 0, s, blk, p.scan.nblk, grid, a.count);
  if ((e = VCR_LAUNCH_RC())) return e;
  const VxRank rk{first, members, blk, a.N, p.scan.nblk, vox, rep_of, a.voxel_points};
  hipLaunchKernelGGL(voxel_rank_kernel, points, block, 0, s, rk);
  if ((e = VCR_LAUNCH_RC())) return e;
  const VxMeans mn{a.xyz, keys, grid, first, members, vox, rep_of, a.N, p.scan.nblk, a.points, a.point_voxel, a.voxel_points};
  hipLaunchKernelGGL(voxel_means_kernel, points, block, 0, s, mn);
  return VCR_LAUNCH_RC();
}

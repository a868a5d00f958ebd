// The tail the outlier filters share (DESIGN sections 4.12, 4.22), written once for outlier.hip (the statistical filter and the
// radius filter by scan) and radius.hip (the radius filter on the grid): a keep flag per point, then the kept points compacted in
// ascending index order.
//   outlier_mark_kernel     one lane per point: keep, one count of them per 256 points (ballot + popcount)
//   outlier_offsets_kernel  one workgroup per cloud: the exclusive scan of those counts, count[b]
//   outlier_write_kernel    one lane per point writes ONE slot of points / index: a kept point its own (the block's offset + its
//                           rank among the block's kept), a dropped one the padding of slot count + (its rank among the dropped)
#pragma once
#include "nn_scan.h"
#include "../../include/vcr_hip_outlier.h"

namespace {

struct OlStat { double mu, var, sigma, thr; int n; int pad; };        // one per cloud
static_assert(sizeof(OlStat) == 40, "workspace layout");

__device__ __forceinline__ bool ol_finite(float v) { return fabsf(v) < __builtin_huge_valf(); }

// The tail both filters share.  keep comes from ONE of two sources: the statistical filter's (mean, st) or the radius
// filter's (cnt, nb_points); the kept points' coordinates from rows [B,N,4] or planes [B,3,N].
struct OlTail {
  const float* mean; const OlStat* st;                     // statistical
  const int* cnt; int nb_points;                           // radius
  const float* rows; const float* planes;
  int N, nblk;
  int* blkcnt;                                             // [B][nblk]: counts, then (in place) their exclusive scan
  float* points; int* count; int* index;
};

__device__ __forceinline__ bool ol_keep(const OlTail& p, int b, size_t o) {
  if (p.cnt) return p.cnt[o] > p.nb_points;
  const float m = p.mean[o];
  return ol_finite(m) && (double)m <= p.st[b].thr;         // (a NaN threshold keeps nothing)
}

__global__ __launch_bounds__(NN_BLOCK) void outlier_mark_kernel(OlTail p) {
  __shared__ int wcnt[NN_BLOCK / 64];
  const int t = threadIdx.x;
  const int b = (int)(blockIdx.x / (unsigned)p.nblk), blk = (int)(blockIdx.x % (unsigned)p.nblk);
  const int i = blk * NN_BLOCK + t;
  const bool keep = i < p.N && ol_keep(p, b, (size_t)b * p.N + (i < p.N ? i : 0));
  int kept;
  wg_rank(keep, t, wcnt, &kept);
  if (t == 0) p.blkcnt[(size_t)b * p.nblk + blk] = kept;
}

__global__ __launch_bounds__(NN_BLOCK) void outlier_offsets_kernel(int* blkcnt, int nblk, int* count) {
  __shared__ int wtot[NN_BLOCK / 64];
  const int b = blockIdx.x;
  const int kept = wg_offsets(blkcnt + (size_t)b * nblk, nblk, wtot);
  if (threadIdx.x == 0) count[b] = kept;
}

__global__ __launch_bounds__(NN_BLOCK) void outlier_write_kernel(OlTail p) {
  __shared__ int wcnt[NN_BLOCK / 64];
  const int t = threadIdx.x;
  const int b = (int)(blockIdx.x / (unsigned)p.nblk), blk = (int)(blockIdx.x % (unsigned)p.nblk);
  const int i = blk * NN_BLOCK + t, N = p.N;
  const size_t row = (size_t)b * N;
  const bool keep = i < N && ol_keep(p, b, row + (i < N ? i : 0));
  int kept;
  const int rank = wg_rank(keep, t, wcnt, &kept);
  if (i >= N) return;
  const int before = p.blkcnt[(size_t)b * p.nblk + blk] + rank;       // kept points below i: <= i
  // a kept point's slot is its rank among the kept, < count; a dropped one's count + its rank among the dropped, i - before:
  // count <= slot < N, and the two ranges are met exactly once each
  const int slot = keep ? before : p.count[b] + (i - before);
  const float nan = __uint_as_float(0x7FC00000u);
  float x = nan, y = nan, z = nan;
  if (keep) {
    if (p.rows) {
      const f32x4 me = ld4(p.rows + (row + i) * 4);
      x = me[0]; y = me[1]; z = me[2];
    } else {
      const float* pl = p.planes + row * 3;
      x = pl[i]; y = pl[N + i]; z = pl[2 * (size_t)N + i];
    }
  }
  float* o = p.points + row * 3;
  o[slot] = x; o[N + slot] = y; o[2 * (size_t)N + slot] = z;
  if (p.index) p.index[row + slot] = keep ? i : -1;
}

// The tail's two last launches
int ol_compact(const OlTail& tl, int B, unsigned point_grid, hipStream_t s) {
  hipLaunchKernelGGL(outlier_offsets_kernel, dim3((unsigned)B), dim3(NN_BLOCK), 0, s, tl.blkcnt, tl.nblk, tl.count);
  const int e = VCR_LAUNCH_RC();
  if (e) return e;
  hipLaunchKernelGGL(outlier_write_kernel, dim3(point_grid), dim3(NN_BLOCK), 0, s, tl);
  return VCR_LAUNCH_RC();
}

}  // namespace

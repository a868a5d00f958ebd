// What the global registrations share around their own work (ransac.hip, fgr.hip, consistency.hip; include/vcr_hip_match.h,
// include/vcr_hip_fgr.h and include/consistency/vcr_hip_consistency.h state it once each): the pair list of a correspondence
// array, the hash of the draws, the squared edge length and the distance of a pair under an fp32 pose.  One text, so the draws
// of a seed, the order of the pairs and a pose's count are the same in all of them.
#pragma once
#include "wg_scan.h"

namespace {

typedef unsigned long long u64;

constexpr int RS_BLOCK = 256;
static_assert(RS_BLOCK == WG_BLOCK, "wg_scan.h serves workgroups of this size");
constexpr int RS_MAX_N = 131072;

// rows [B][Ns][8], M [B], zeroed [B]: a counter of the caller's that starts at 0; pairs: optional [B]
struct RsPairs { const float* src; const float* tgt; const int* corr; int Ns, Nt; float* rows; int* M; int* zeroed; int* pairs; };

// One workgroup per cloud: the source points with a partner, ascending, gathered ONCE into contiguous 32-B rows
// (sx, sy, sz, source index | tx, ty, tz, 0) by a ballot prefix over chunks of 256; M behind them.  The body of
// ransac_pairs_kernel and fgr_pairs_kernel: each file launches it under a name of its own, so that the build's resource remarks
// tell the two objects' copies apart.
__device__ __forceinline__ void rs_pairs_body(const RsPairs& p) {
  __shared__ int wtot[RS_BLOCK / 64];
  const int t = threadIdx.x, b = blockIdx.x, Ns = p.Ns, Nt = p.Nt;
  const float* sx = p.src + (size_t)b * 3 * Ns;
  const float* tx = p.tgt + (size_t)b * 3 * Nt;
  const int* corr = p.corr + (size_t)b * Ns;
  float* rows = p.rows + (size_t)b * Ns * 8;
  int base = 0;
  for (int c0 = 0; c0 < Ns; c0 += RS_BLOCK) {              // (workgroup-uniform: the barriers are met by all)
    const int i = c0 + t;
    const int j = i < Ns ? corr[i] : -1;
    const bool has = (unsigned)j < (unsigned)Nt;
    __syncthreads();                                       // the previous chunk's totals have been read
    int found;
    const int at = base + wg_rank(has, t, wtot, &found);
    if (has) {                                             // at < Ns: at most one row per source point
      const f32x4 s4 = {sx[i], sx[Ns + i], sx[2 * (size_t)Ns + i], __int_as_float(i)};
      const f32x4 t4 = {tx[j], tx[Nt + j], tx[2 * (size_t)Nt + j], 0.f};
      st4(rows + (size_t)at * 8, s4);
      st4(rows + (size_t)at * 8 + 4, t4);
    }
    base += found;
  }
  if (t == 0) {
    p.M[b] = base;
    p.zeroed[b] = 0;
    if (p.pairs) p.pairs[b] = base;
  }
}

__device__ __forceinline__ uint32_t rs_mix32(uint32_t x) {
  x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16;
  return x;
}

// the position in the pair list of pick j of trial t: < M
__device__ __forceinline__ unsigned rs_pick(unsigned seed, int trial, int j, int M) {
  return (unsigned)(((u64)rs_mix32(seed ^ rs_mix32(3u * (unsigned)trial + (unsigned)j)) * (u64)(unsigned)M) >> 32);
}

__device__ __forceinline__ float rs_len2(const f32x4& u, const f32x4& v) {
  const float dx = u[0] - v[0], dy = u[1] - v[1], dz = u[2] - v[2];
  return fmaf(dz, dz, fmaf(dy, dy, dx * dx));
}

// (ransac.hip's and consistency.hip's distance check and count) vcr_hip_score.h's `moved source` and `distance` under the fp32 pose (R row-major, then t)
__device__ __forceinline__ float rs_d2(const float (&P)[12], float x, float y, float z, float qx, float qy, float qz) {
  const float px = fmaf(P[2], z, fmaf(P[1], y, P[0] * x)) + P[9];
  const float py = fmaf(P[5], z, fmaf(P[4], y, P[3] * x)) + P[10];
  const float pz = fmaf(P[8], z, fmaf(P[7], y, P[6] * x)) + P[11];
  const float dx = px - qx, dy = py - qy, dz = pz - qz;
  return fmaf(dz, dz, fmaf(dy, dy, dx * dx));
}

}  // namespace

// What a workgroup of 256 lanes (four waves) does with one value per lane, written once: the ballot rank,
// the exclusive scan of a cloud's per-block counts, the (fp64 sum, count) reduction and the fold of a cloud's partials.  Every
// function is called by ALL lanes of the workgroup (each holds a barrier) and works in the caller's __shared__ arrays.
//
// The contract: lanes, waves and partials are taken in ASCENDING order, and no addition is ever reordered -- the fp64 sums are
// the wave butterfly 32 ... 1, then waves 0 .. 3, then the partials ascending, each by one thread -- so a result depends on the
// cloud's size alone, never on how the scan in front of it was cut.  The integer ones are exact in any order and keep theirs.
#pragma once
#include "common.h"

namespace {

constexpr int WG_BLOCK = 256;                              // NN_BLOCK, FN_BLOCK and RS_BLOCK are this
constexpr int WG_WAVES = WG_BLOCK / 64;

// The number of lanes of the workgroup whose flag is set, and this lane's rank among them (lanes ascending).  wcnt [WG_WAVES]
// is free again after the caller's next barrier.
__device__ __forceinline__ int wg_rank(bool flag, int t, int* wcnt, int* total) {
  const unsigned long long bal = __ballot(flag);
  const int lane = t & 63, w = t >> 6;
  if (lane == 0) wcnt[w] = __popcll(bal);
  __syncthreads();
  int below = 0, all = 0;
  for (int k = 0; k < WG_WAVES; ++k) { below += k < w ? wcnt[k] : 0; all += wcnt[k]; }
  *total = all;
  return below + __popcll(bal & ((1ull << lane) - 1ull));
}

// cnt [nblk] becomes its own exclusive scan, in place (a lane reads and writes its own two entries: two counts a lane, a wave
// scan, four wave totals); every lane returns the total.  wtot [WG_WAVES].
__device__ __forceinline__ int wg_offsets(int* cnt, int nblk, int* wtot) {
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  int carry = 0;
  for (int c0 = 0; c0 < nblk; c0 += 2 * WG_BLOCK) {        // (workgroup-uniform; one round up to 131 072 points)
    const int i0 = c0 + 2 * t, i1 = i0 + 1;
    const int a0 = i0 < nblk ? cnt[i0] : 0, a1 = i1 < nblk ? cnt[i1] : 0;
    int incl = a0 + a1;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int v = __shfl_up(incl, o, 64);
      incl += lane >= o ? v : 0;
    }
    __syncthreads();                                       // the previous round's totals have been read
    if (lane == 63) wtot[w] = incl;
    __syncthreads();
    int below = 0, all = 0;
    for (int k = 0; k < WG_WAVES; ++k) { below += k < w ? wtot[k] : 0; all += wtot[k]; }
    const int excl = carry + below + incl - (a0 + a1);
    if (i0 < nblk) cnt[i0] = excl;
    if (i1 < nblk) cnt[i1] = excl + a0;
    carry += all;
  }
  return carry;
}

// wg_offsets' sibling for sums that may pass 2^31: out [n] (int64) becomes the exclusive scan of cnt [n] (int32, >= 0), not in
// place (the same two counts a lane, wave scan and four wave totals, in 64-bit); every lane returns the total.  wtot [WG_WAVES].
__device__ __forceinline__ long long wg_offsets64(const int* cnt, long long* out, int n, long long* wtot) {
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  long long carry = 0;
  for (int c0 = 0; c0 < n; c0 += 2 * WG_BLOCK) {           // (workgroup-uniform: 256 rounds at 131 072 counts)
    const int i0 = c0 + 2 * t, i1 = i0 + 1;
    const long long a0 = i0 < n ? cnt[i0] : 0, a1 = i1 < n ? cnt[i1] : 0;
    long long incl = a0 + a1;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const long long v = __shfl_up(incl, o, 64);
      incl += lane >= o ? v : 0;
    }
    __syncthreads();                                       // the previous round's totals have been read
    if (lane == 63) wtot[w] = incl;
    __syncthreads();
    long long below = 0, all = 0;
    for (int k = 0; k < WG_WAVES; ++k) { below += k < w ? wtot[k] : 0; all += wtot[k]; }
    const long long excl = carry + below + incl - (a0 + a1);
    if (i0 < n) out[i0] = excl;
    if (i1 < n) out[i1] = excl + a0;
    carry += all;
  }
  return carry;
}

// The workgroup's 256 (v, c): the wave butterfly 32 ... 1, then the four waves ascending.  Thread 0 alone returns the sums;
// wsum / wcnt [WG_WAVES] are free again after the caller's next barrier.
__device__ __forceinline__ void wg_sum_count(double v, int c, int t, double* wsum, int* wcnt, double* sum, int* cnt) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) { v += __shfl_xor(v, o, 64); c += __shfl_xor(c, o, 64); }
  if ((t & 63) == 0) { wsum[t >> 6] = v; wcnt[t >> 6] = c; }
  __syncthreads();
  if (t == 0) {
    double s = wsum[0];
    int n = wcnt[0];
    for (int w = 1; w < WG_WAVES; ++w) { s += wsum[w]; n += wcnt[w]; }
    *sum = s; *cnt = n;
  }
}

// One cloud's nblk partials -- load(i, &sum, &count) reads the i-th -- added in ascending order by thread 0, which alone
// returns the sums: the order is the cloud's size's alone.  ls / lc [WG_BLOCK] stage them.
template <class Load>
__device__ __forceinline__ void wg_fold(int nblk, Load load, int t, double* ls, int* lc, double* sum, int* cnt) {
  double s = 0.;
  int n = 0;
  for (int c0 = 0; c0 < nblk; c0 += WG_BLOCK) {            // (workgroup-uniform)
    const int m = nblk - c0 < WG_BLOCK ? nblk - c0 : WG_BLOCK;
    __syncthreads();
    if (t < m) load(c0 + t, &ls[t], &lc[t]);
    __syncthreads();
    if (t == 0)
      for (int i = 0; i < m; ++i) { s += ls[i]; n += lc[i]; }
  }
  *sum = s; *cnt = n;
}

}  // namespace

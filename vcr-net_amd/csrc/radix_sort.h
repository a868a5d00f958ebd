// A stable least-significant-digit radix sort of (64-bit key, 32-bit value) pairs, one independent sort per cloud of a batch,
// written once: voxel_sort.hip is its first user.  The input of pass 0 is buffer 0; pass p reads buffer
// p & 1 and writes the other.  A cloud's number of passes is DATA (npass[b], on the device): the host launches the passes the
// full 64 bits need, and a cloud's workgroups leave a pass it does not need at once -- so a cloud's sorted order ends up in
// buffer npass[b] & 1, which every reader works out from npass[b] itself.
//
// One pass is three launches over workgroups of 256 lanes x E elements (a tile of T = 256 E consecutive elements):
//   rs_hist_kernel     per tile the number of elements of every digit (LDS integer atomics: a count has no order)
//   rs_scan_kernel     per digit the exclusive scan of its counts over the cloud's tiles, in place, and the digit's total
//   rs_scatter_kernel  every element goes to  [elements of a lower digit] + [of its digit in earlier tiles] + [of its digit
//                      earlier in its tile].  The last is a RANK, not a ticket: wave w of the tile takes the 64 E consecutive
//                      elements [64 E w, 64 E (w + 1)) in E rounds of 64, and an element's rank is  the digit's count in the
//                      lower waves (LDS, after a barrier)  +  in the earlier rounds of its wave (a per-wave LDS counter that
//                      only this wave reads and then advances)  +  in the lower lanes of its round (ballots: one per digit
//                      bit gives the mask of the lanes that hold the same digit).  Equal digits therefore keep their order
//                      inside the wave, inside the tile and across tiles: the pass is stable.
// No atomic hands out a slot, no workgroup waits for another, no loop's trip count depends on anything but E, the digit width
// and the number of tiles.
#pragma once
#include "wg_scan.h"

namespace {

typedef unsigned long long rs_u64;

struct RsSort {
  rs_u64* keys[2]; unsigned* vals[2];                      // [B][N] each
  int* hist;                                               // [B][nt][R]: counts, then per digit their exclusive scan over the tiles
  int* tot;                                                // [B][R]
  const int* npass;                                        // [B]
  int N, nt;
};

__host__ __device__ constexpr int rs_passes(int bits) { return (64 + bits - 1) / bits; }       // what 64 bits need

// The exclusive scan of one int per lane over the workgroup (lanes ascending) and the total.  wtot [WG_WAVES] is free again
// after the caller's next barrier.  Called by all lanes.
__device__ __forceinline__ int wg_excl_scan(int v, int t, int* wtot, int* total) {
  const int lane = t & 63, w = t >> 6;
  int incl = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int u = __shfl_up(incl, o, 64);
    incl += lane >= o ? u : 0;
  }
  if (lane == 63) wtot[w] = incl;
  __syncthreads();
  int below = 0, all = 0;
  for (int k = 0; k < WG_WAVES; ++k) { below += k < w ? wtot[k] : 0; all += wtot[k]; }
  *total = all;
  return below + incl - v;
}

template <int BITS>
__device__ __forceinline__ int rs_digit(rs_u64 key, int shift) { return (int)((key >> shift) & (rs_u64)((1 << BITS) - 1)); }

template <int BITS, int E>
__global__ __launch_bounds__(WG_BLOCK) void rs_hist_kernel(RsSort p, int pass) {
  constexpr int R = 1 << BITS, T = WG_BLOCK * E;
  __shared__ int h[R];
  const int t = threadIdx.x;
  const int b = (int)(blockIdx.x / (unsigned)p.nt), k = (int)(blockIdx.x % (unsigned)p.nt);
  if (pass >= p.npass[b]) return;                          // (workgroup-uniform)
  const rs_u64* __restrict__ key = p.keys[pass & 1] + (size_t)b * p.N;
  for (int g = t; g < R; g += WG_BLOCK) h[g] = 0;
  __syncthreads();
#pragma unroll
  for (int r = 0; r < E; ++r) {
    const int i = k * T + r * WG_BLOCK + t;
    if (i < p.N) atomicAdd(&h[rs_digit<BITS>(key[i], pass * BITS)], 1);
  }
  __syncthreads();
  for (int g = t; g < R; g += WG_BLOCK) p.hist[((size_t)b * p.nt + k) * R + g] = h[g];
}

template <int BITS>
__global__ __launch_bounds__(WG_BLOCK) void rs_scan_kernel(RsSort p, int pass) {
  constexpr int R = 1 << BITS, G = (R + WG_BLOCK - 1) / WG_BLOCK;
  const int b = (int)(blockIdx.x / (unsigned)G), g = (int)(blockIdx.x % (unsigned)G) * WG_BLOCK + (int)threadIdx.x;
  if (pass >= p.npass[b] || g >= R) return;
  int* h = p.hist + (size_t)b * p.nt * R + g;               // the digit's column: lane g beside lane g + 1, every access coalesced
  int run = 0;
  for (int k0 = 0; k0 < p.nt; k0 += 16) {                  // sixteen counts in flight, then their sixteen prefixes
    int c[16];
#pragma unroll
    for (int u = 0; u < 16; ++u) c[u] = k0 + u < p.nt ? h[(size_t)(k0 + u) * R] : 0;
#pragma unroll
    for (int u = 0; u < 16; ++u) {
      if (k0 + u < p.nt) h[(size_t)(k0 + u) * R] = run;
      run += c[u];
    }
  }
  p.tot[(size_t)b * R + g] = run;
}

template <int BITS, int E>
__global__ __launch_bounds__(WG_BLOCK) void rs_scatter_kernel(RsSort p, int pass) {
  constexpr int R = 1 << BITS, T = WG_BLOCK * E, J = R >= WG_BLOCK ? R / WG_BLOCK : 1;
  __shared__ int cnt[WG_WAVES][R];
  __shared__ int wtot[WG_WAVES];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int b = (int)(blockIdx.x / (unsigned)p.nt), k = (int)(blockIdx.x % (unsigned)p.nt);
  if (pass >= p.npass[b]) return;                          // (workgroup-uniform: the barriers below are met by all or none)
  const int N = p.N, shift = pass * BITS;
  const size_t row = (size_t)b * N;
  const rs_u64* __restrict__ kin = p.keys[pass & 1] + row;
  const unsigned* __restrict__ vin = p.vals[pass & 1] + row;
  rs_u64* __restrict__ kout = p.keys[(pass & 1) ^ 1] + row;
  unsigned* __restrict__ vout = p.vals[(pass & 1) ^ 1] + row;

  for (int g = t; g < WG_WAVES * R; g += WG_BLOCK) (&cnt[0][0])[g] = 0;
  rs_u64 key[E];
  unsigned val[E];
  const int first = k * T + w * 64 * E + lane;
#pragma unroll
  for (int r = 0; r < E; ++r) {                            // (all the loads in flight together)
    const int i = first + r * 64;
    key[r] = i < N ? kin[i] : 0ull;
    val[r] = i < N ? vin[i] : 0u;
  }
  __syncthreads();
  volatile int* mine = cnt[w];                             // this wave's counters: read by all its lanes, then advanced by one
  const rs_u64 below_me = (1ull << lane) - 1ull;
  int dig[E], off[E];
#pragma unroll
  for (int r = 0; r < E; ++r) {
    const bool valid = first + r * 64 < N;
    const int d = rs_digit<BITS>(key[r], shift);
    rs_u64 peers = __ballot(valid);                        // the lanes of this round that hold the same digit
#pragma unroll
    for (int bit = 0; bit < BITS; ++bit) {
      const bool one = (d >> bit) & 1;
      const rs_u64 bal = __ballot(one);
      peers &= one ? bal : ~bal;
    }
    const int before = __popcll(peers & below_me);
    int old = 0;
    if (valid) old = mine[d];                              // the digit's count in the earlier rounds of this wave
    if (valid && before == 0) mine[d] = old + __popcll(peers);
    dig[r] = d;
    off[r] = old + before;
  }
  __syncthreads();
  // cnt[w][g] becomes where wave w's first element of digit g goes: the digits below g, g's in the earlier tiles, g's in the
  // lower waves.  Thread t takes the J consecutive digits from t J.
  int sum = 0;
  const size_t trow = (size_t)b * R;
#pragma unroll
  for (int j = 0; j < J; ++j) sum += t * J + j < R ? p.tot[trow + t * J + j] : 0;
  int all;
  int base = wg_excl_scan(sum, t, wtot, &all);
#pragma unroll
  for (int j = 0; j < J; ++j) {
    const int g = t * J + j;
    if (g < R) {
      int o = base + p.hist[((size_t)b * p.nt + k) * R + g];
#pragma unroll
      for (int u = 0; u < WG_WAVES; ++u) { const int c = cnt[u][g]; cnt[u][g] = o; o += c; }
      base += p.tot[trow + g];
    }
  }
  __syncthreads();
#pragma unroll
  for (int r = 0; r < E; ++r) {
    const int to = cnt[w][dig[r]] + off[r];
    if (first + r * 64 < N && (unsigned)to < (unsigned)N) { kout[to] = key[r]; vout[to] = val[r]; }
  }
}

// The launches of one sort: rs_passes(BITS) passes of three.  grid: B * nt workgroups (hist, scatter), B * ceil(R / 256) (scan).
template <int BITS, int E>
int rs_sort_launch(const RsSort& p, int B, hipStream_t s) {
  constexpr int R = 1 << BITS, G = (R + WG_BLOCK - 1) / WG_BLOCK;
  const dim3 block(WG_BLOCK), tiles((unsigned)((long)B * p.nt)), digits((unsigned)((long)B * G));
  for (int pass = 0; pass < rs_passes(BITS); ++pass) {
    int e;
    hipLaunchKernelGGL((rs_hist_kernel<BITS, E>), tiles, block, 0, s, p, pass);
    if ((e = VCR_LAUNCH_RC())) return e;
    hipLaunchKernelGGL((rs_scan_kernel<BITS>), digits, block, 0, s, p, pass);
    if ((e = VCR_LAUNCH_RC())) return e;
    hipLaunchKernelGGL((rs_scatter_kernel<BITS, E>), tiles, block, 0, s, p, pass);
    if ((e = VCR_LAUNCH_RC())) return e;
  }
  return VCR_OK;
}

}  // namespace

// The tail of a search that returns rows of varying length in CSR form, written once for radius.hip (a cloud's points against
// itself) and query.hip (any query positions): n rows a cloud, their lengths in count [B][n].
//   rows_offsets_kernel  one workgroup per cloud: the 64-bit exclusive scan of the counts (wg_offsets64) to row_start [B][n + 1]
//                        and total [B]
//   (the caller's fill)  lane i appends its hits' keys (d2 bits) << 32 | j to its private segment of the scratch [B][capacity],
//                        rows_segment(): at row_start[b, i], clamped to the row and to the cloud's slots; no atomics.  The order
//                        inside a segment follows the walk and is not defined
//   rows_order_kernel    a rank sort out of the scratch, a wave (a workgroup of 64 lanes) per row: a row's keys are distinct, so
//                        rank(e) = #{keys < key_e} is a permutation, and idx / d2 are written at row_start + rank: no atomics, no
//                        in-place hazard, any row length.  The row passes through LDS in chunks of ROWS_CHUNK keys, 64 elements
//                        are ranked a pass
//   rows_pad_kernel      -1 / +inf behind total[b], and over the clouds that do not fit (total[b] > capacity), which the fill and
//                        the ordering leave alone
// Every loop is bounded by n, a row's length or the capacity; every write is clamped to its row.
#pragma once
#include "grid_build.h"
#include "../../include/vcr_hip_radius.h"
#include "../../include/query/vcr_hip_query.h"

namespace {

constexpr int ROWS_CHUNK = VCR_RADIUS_CHUNK;               // keys of a row in LDS at a time
constexpr int ROWS_WAVE = 64;
static_assert(VCR_RADIUS_CHUNK == VCR_QUERY_CHUNK, "one ordering kernel serves both searches");
static_assert(ROWS_CHUNK % ROWS_WAVE == 0, "a wave stages a chunk in whole passes");

__global__ __launch_bounds__(GD_BLOCK) void rows_offsets_kernel(const int* count, long long* row_start, long long* total, int n) {
  __shared__ long long wtot[WG_WAVES];
  const int b = blockIdx.x;
  long long* rs = row_start + (size_t)b * ((size_t)n + 1);
  const long long all = wg_offsets64(count + (size_t)b * n, rs, n, wtot);
  if (threadIdx.x == 0) { rs[n] = all; total[b] = all; }
}

// The fill's segment of row i among its cloud's `capacity` slots, rs the cloud's n + 1 offsets: where it starts and how many
// entries it holds, the row's length clamped to the slots that are left.  Nothing is written unless at >= 0 and len > 0.  (The
// ordering kernels, here and radius.hip's lane form, keep the arithmetic in their own statements: through this helper the
// wave form's inner loop counts in a VGPR and the kernel is 17 % slower on long rows)
struct RowsSeg { long long at, len; };

__device__ __forceinline__ RowsSeg rows_segment(const long long* __restrict__ rs, int i, int capacity) {
  const long long at = rs[i];
  const long long len = rs[i + 1] - at, left = (long long)capacity - at;
  return RowsSeg{at, len < left ? len : left};
}

// row_start [B][n + 1]; scratch [B][capacity]: a cloud's unordered keys, row i at row_start[b, i]
struct RowsOrder { const long long* row_start; const u64* scratch; int n, capacity; int* idx; float* d2; };

// One workgroup of ONE wave per row: 64 elements are ranked a pass against the whole row, which passes through LDS in chunks
__global__ __launch_bounds__(ROWS_WAVE) void rows_order_kernel(RowsOrder p) {
  __shared__ u64 keys[ROWS_CHUNK];
  const int lane = threadIdx.x;
  const int b = (int)(blockIdx.x / (unsigned)p.n), i = (int)(blockIdx.x % (unsigned)p.n);
  const long long* __restrict__ rs = p.row_start + (size_t)b * ((size_t)p.n + 1);
  if (rs[p.n] > (long long)p.capacity) return;             // (workgroup-uniform)
  const long long at = rs[i];
  long long len = rs[i + 1] - at;
  len = len < (long long)p.capacity - at ? len : (long long)p.capacity - at;
  if (at < 0 || len <= 0) return;                          // (workgroup-uniform)
  const int n = (int)len;                                  // <= the capacity
  const size_t base = (size_t)b * p.capacity + (size_t)at;
  const u64* __restrict__ row = p.scratch + base;
  for (int e0 = 0; e0 < n; e0 += ROWS_WAVE) {              // (workgroup-uniform: bounded by the row's length)
    const int e = e0 + lane;
    const u64 key = e < n ? row[e] : ~0ull;
    int rank = 0;
    for (int c0 = 0; c0 < n; c0 += ROWS_CHUNK) {
      const int m = n - c0 < ROWS_CHUNK ? n - c0 : ROWS_CHUNK;
      __syncthreads();                                     // the previous chunk has been read
      for (int f = lane; f < m; f += ROWS_WAVE) keys[f] = row[c0 + f];
      __syncthreads();
      for (int f = 0; f < m; ++f) rank += keys[f] < key ? 1 : 0;         // one address for every lane: broadcast reads
    }
    if (e < n && rank < n) {                               // (rank < n always: the keys are distinct)
      p.idx[base + rank] = (int)(uint32_t)key;
      if (p.d2) p.d2[base + rank] = __uint_as_float((uint32_t)(key >> 32));
    }
  }
}

__global__ __launch_bounds__(GD_BLOCK) void rows_pad_kernel(const long long* row_start, int n, int capacity, int per_cloud,
                                                            int* idx, float* d2) {
  const int b = (int)(blockIdx.x / (unsigned)per_cloud), blk = (int)(blockIdx.x % (unsigned)per_cloud);
  const long long all = row_start[(size_t)b * ((size_t)n + 1) + n];
  const int from = all >= 0 && all <= (long long)capacity ? (int)all : 0;           // a cloud that does not fit: every slot
  const size_t base = (size_t)b * capacity;
  for (long long s = (long long)from + blk * GD_BLOCK + (int)threadIdx.x; s < capacity; s += (long long)per_cloud * GD_BLOCK) {
    idx[base + s] = -1;
    if (d2) d2[base + s] = __builtin_huge_valf();
  }
}

}  // namespace

static inline int rows_offsets(const int* count, long long* row_start, long long* total, int B, int n, hipStream_t s) {
  hipLaunchKernelGGL(rows_offsets_kernel, dim3((unsigned)B), dim3(GD_BLOCK), 0, s, count, row_start, total, n);
  return VCR_LAUNCH_RC();
}

static inline int rows_pad(const RowsOrder& od, int B, hipStream_t s) {
  const int pad_x = (od.capacity + GD_BLOCK - 1) / GD_BLOCK < 256 ? (od.capacity + GD_BLOCK - 1) / GD_BLOCK : 256;
  hipLaunchKernelGGL(rows_pad_kernel, dim3((unsigned)((long)B * pad_x)), dim3(GD_BLOCK), 0, s, od.row_start, od.n, od.capacity,
                     pad_x, od.idx, od.d2);
  return VCR_LAUNCH_RC();
}

// the wave-per-row ordering, then the pad
static inline int rows_order_pad(const RowsOrder& od, int B, hipStream_t s) {
  hipLaunchKernelGGL(rows_order_kernel, dim3((unsigned)((long)B * od.n)), dim3(ROWS_WAVE), 0, s, od);
  const int e = VCR_LAUNCH_RC();
  return e ? e : rows_pad(od, B, s);
}

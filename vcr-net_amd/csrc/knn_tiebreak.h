// The kNN searches' tie replay: an exact replica of Tensor.topk's tie-breaking (included by knn.hip; one translation unit).
// The searches write idx = top-(k+1) of D_i. by value with rank 0 dropped (util/util.py:159), as a SET.  Two kinds of exact tie make
// that set depend on more than the values:
//   * at the (k+1)-th value: Tensor.topk on the CPU is libstdc++'s std::nth_element (or std::partial_sort when (k+1)*64 <= N) with a
//     value-only comparator, so WHICH of the tied candidates it keeps is an artefact of introselect's pivoting / the heap's shape.
//     The searches' value lists carry one entry more than needed, which makes such a tie visible (about 1 row in 10^4 in fp32);
//     those rows are re-done here, by ports of the libstdc++ algorithms, so that the neighbour SETS equal the reference's on every
//     row (validated against torch.topk on tie-heavy inputs).  Without tie_scratch a boundary tie keeps the candidates scanned first.
//   * a shared BEST value (copies of a point, or a neighbour so close that its distance rounds to the point's own -- fp32
//     self-distances are not exactly 0): util.py:159 drops whichever entry topk returns first, and that is position 0 after ATen's
//     sort of the selected entries (std::sort of the first k after nth_element, or partial_sort's heap sort), not the lowest index.
//     Such rows are replayed as well; the replay ends with a port of that sort.  (Found in round 6 by the vcrnetIter reuse soak: two
//     launch forms of the Cartesian search logged such a pair in different orders and kept different copies.)
// A replay runs in a launch of its own (knn_tiebreak_kernel / knn_tiebreak2_kernel) or inside the search that found the row
// (replay_block_ties); either way tiebreak_row does one row with one workgroup.
#pragma once
#include "common.h"
#include "vcr_internal.h"

namespace {

// In-kernel tie replay (vcr_knn_args.tie_inline, set by the host when a row's replay image fits the workgroup's LDS): the
// rows of a workgroup whose (k+1)-th and (k+2)-th values tie are listed in LDS and replayed by that workgroup itself
// once its four waves have written their results -- the separate, latency-bound replay launch (36 us at BASELINE
// configs[1] for a handful of rows) disappears; only the few workgroups that own a tied row run ~20 us longer.
constexpr int BLK_TIES = 64;                             // a 64-query workgroup cannot list more
constexpr int TB_LDS_PAD = 8;                            // see tiebreak_row (8: N = 10 091 still fits 160 KB)
__host__ __device__ constexpr size_t tiebreak_lds(int N) { return TB_LDS_PAD + (size_t)N * 16 + 256 + (16 + 2 * 256 + 2) * 4; }
// the list sits behind whichever is larger, the waves' logs or the replay's LDS image of a row
__host__ __device__ constexpr size_t inline_tie_offset(size_t log_bytes, int N) {
  return ((log_bytes > tiebreak_lds(N) ? log_bytes : tiebreak_lds(N)) + 15) & ~(size_t)15;
}
constexpr size_t INLINE_TIE_MAX_LDS = 40 * 1024;         // four workgroups per CU must still fit
__device__ void tiebreak_row(const vcr_knn_args& a, int row, unsigned char* smem, unsigned char* gwork);
// gwork (tie_inline == 2): the row image lives in THIS workgroup's 16 N-byte slot of vcr_knn_args.tie_work instead of LDS --
// rows too long for an LDS image beside three or four resident workgroups (N > ~2400) are then replayed by the workgroup
// that found them too, under the other workgroups' scans, instead of by a separate launch (0.16 ms at 64 x 4096, k = 40).
__device__ __forceinline__ void replay_block_ties(const vcr_knn_args& a, int* blk_ties, unsigned char* smem, unsigned char* gwork = nullptr) {
  __syncthreads();                                       // every wave is done with its log: the LDS is free
  const int n = min(blk_ties[0], BLK_TIES);
  int rows[4];                                           // (the list itself lies behind the replay's LDS image)
  for (int t0 = 0; t0 < n; t0 += 4) {
#pragma unroll
    for (int u = 0; u < 4; ++u) rows[u] = t0 + u < n ? blk_ties[1 + t0 + u] : -1;
#pragma unroll
    for (int u = 0; u < 4; ++u)
      if (rows[u] >= 0) tiebreak_row(a, rows[u], smem, gwork);
  }
}

// ---------------------------------------------------------------- exact replica of Tensor.topk's tie-breaking
// Sequential port of libstdc++'s std::nth_element (__introselect: median-of-three to first, unguarded partition,
// depth limit 2 log2 n with __heap_select fallback, final insertion sort) and of std::partial_sort's __heap_select,
// on (value, index) pairs ordered by VALUE ONLY, exactly as ATen's CPU topk runs them (TopKImpl: queue[j] = (x[j], j);
// partial_sort when k*64 <= n, else nth_element(k-1) + sort of the first k-1).  Only the SET of the first K entries
// matters here.  One thread per tied row; rows are rare.
struct PairArr {
  float* v; int* id;
  __device__ __forceinline__ bool gt(int a, int b) const { return v[a] > v[b]; }
  __device__ __forceinline__ void swap(int a, int b) {
    const float tv = v[a]; v[a] = v[b]; v[b] = tv;
    const int ti = id[a]; id[a] = id[b]; id[b] = ti;
  }
};

__device__ void tb_push_heap(PairArr& q, int first, int hole, int top, float val, int vid) {
  int parent = (hole - 1) / 2;
  while (hole > top && q.v[first + parent] > val) {
    q.v[first + hole] = q.v[first + parent]; q.id[first + hole] = q.id[first + parent];
    hole = parent;
    parent = (hole - 1) / 2;
  }
  q.v[first + hole] = val; q.id[first + hole] = vid;
}

__device__ void tb_adjust_heap(PairArr& q, int first, int hole, int len, float val, int vid) {
  const int top = hole;
  int child = hole;
  while (child < (len - 1) / 2) {
    child = 2 * (child + 1);
    if (q.v[first + child] > q.v[first + child - 1]) --child;
    q.v[first + hole] = q.v[first + child]; q.id[first + hole] = q.id[first + child];
    hole = child;
  }
  if ((len & 1) == 0 && child == (len - 2) / 2) {
    child = 2 * (child + 1);
    q.v[first + hole] = q.v[first + child - 1]; q.id[first + hole] = q.id[first + child - 1];
    hole = child - 1;
  }
  tb_push_heap(q, first, hole, top, val, vid);
}

__device__ void tb_heap_select(PairArr& q, int first, int middle, int last) {
  const int len = middle - first;
  if (len >= 2) {                                        // std::__make_heap
    for (int parent = (len - 2) / 2;; --parent) {
      tb_adjust_heap(q, first, parent, len, q.v[first + parent], q.id[first + parent]);
      if (parent == 0) break;
    }
  }
  for (int i = middle; i < last; ++i) {
    if (q.v[i] > q.v[first]) {                           // std::__pop_heap(first, middle, i)
      const float val = q.v[i]; const int vid = q.id[i];
      q.v[i] = q.v[first]; q.id[i] = q.id[first];
      tb_adjust_heap(q, first, 0, len, val, vid);
    }
  }
}

__device__ void tb_nth_element(PairArr& q, int first, int last, int nth, int depth) {
  while (last - first > 3) {
    if (depth == 0) {
      tb_heap_select(q, first, nth + 1, last);
      q.swap(first, nth);
      return;
    }
    --depth;
    // __unguarded_partition_pivot: median of (first+1, mid, last-1) to first, then partition [first+1, last)
    const int mid = first + (last - first) / 2, a = first + 1, b = mid, c = last - 1;
    if (q.gt(a, b)) {
      if (q.gt(b, c)) q.swap(first, b);
      else if (q.gt(a, c)) q.swap(first, c);
      else q.swap(first, a);
    } else if (q.gt(a, c)) q.swap(first, a);
    else if (q.gt(b, c)) q.swap(first, c);
    else q.swap(first, b);
    int lo = first + 1, hi = last;
    for (;;) {
      while (q.gt(lo, first)) ++lo;
      --hi;
      while (q.gt(first, hi)) --hi;
      if (!(lo < hi)) break;
      q.swap(lo, hi);
      ++lo;
    }
    if (lo <= nth) first = lo; else last = lo;
  }
  for (int i = first + 1; i < last; ++i) {               // std::__insertion_sort(first, last)
    const float val = q.v[i]; const int vid = q.id[i];
    if (val > q.v[first]) {
      for (int j = i; j > first; --j) { q.v[j] = q.v[j - 1]; q.id[j] = q.id[j - 1]; }
      q.v[first] = val; q.id[first] = vid;
    } else {
      int j = i;
      while (val > q.v[j - 1]) { q.v[j] = q.v[j - 1]; q.id[j] = q.id[j - 1]; --j; }
      q.v[j] = val; q.id[j] = vid;
    }
  }
}

// std::__sort_heap(first, first + len): what std::partial_sort runs on its heap, and std::sort when its depth limit runs out
__device__ void tb_sort_heap(PairArr& q, int first, int len) {
  while (len > 1) {
    --len;                                               // std::__pop_heap(first, last, last)
    const float val = q.v[first + len]; const int vid = q.id[first + len];
    q.v[first + len] = q.v[first]; q.id[first + len] = q.id[first];
    tb_adjust_heap(q, first, 0, len, val, vid);
  }
}

__device__ void tb_unguarded_linear_insert(PairArr& q, int last) {
  const float val = q.v[last]; const int vid = q.id[last];
  int next = last - 1;
  while (val > q.v[next]) { q.v[last] = q.v[next]; q.id[last] = q.id[next]; last = next; --next; }
  q.v[last] = val; q.id[last] = vid;
}
__device__ void tb_insertion_sort(PairArr& q, int first, int last) {
  for (int i = first + 1; i < last; ++i) {
    if (q.v[i] > q.v[first]) {
      const float val = q.v[i]; const int vid = q.id[i];
      for (int j = i; j > first; --j) { q.v[j] = q.v[j - 1]; q.id[j] = q.id[j - 1]; }
      q.v[first] = val; q.id[first] = vid;
    } else {
      tb_unguarded_linear_insert(q, i);
    }
  }
}
// Sequential port of libstdc++'s std::sort on [first, last) (__introsort_loop: median-of-three to first + unguarded partition
// while a range is longer than 16, depth limit 2 log2 n with the heap sort fallback; then __final_insertion_sort) with the
// value-only comparator: the ORDER it leaves equal values in is what decides Tensor.topk's rank 0 among tied best values.
// Ranges here are the <= 62 kept entries of a row.  The recursion on the right-hand parts: only a part of more than 16 entries
// has work left, the parts are disjoint (the order they are finished in does not matter) -- at most three are ever pending,
// kept packed (first | last << 8 | depth << 16) in the caller's LDS scratch (stk[0..2]).
__device__ void tb_sort(PairArr& q, int first, int last, int* stk) {
  if (last - first < 2) return;
  int depth0 = 0;
  for (int m = last - first; m > 1; m >>= 1) ++depth0;
  depth0 *= 2;
  int sp = 1;
  stk[0] = first | (last << 8) | (depth0 << 16);
  while (sp > 0) {
    --sp;
    const int e = stk[sp];
    int f = e & 255, l = (e >> 8) & 255, depth = e >> 16;
    while (l - f > 16) {
      if (depth == 0) {                                  // std::__partial_sort(f, l, l): heap sort of the range
        tb_heap_select(q, f, l, l);
        tb_sort_heap(q, f, l - f);
        break;
      }
      --depth;
      const int mid = f + (l - f) / 2, a = f + 1, b = mid, c = l - 1;
      if (q.gt(a, b)) {
        if (q.gt(b, c)) q.swap(f, b);
        else if (q.gt(a, c)) q.swap(f, c);
        else q.swap(f, a);
      } else if (q.gt(a, c)) q.swap(f, a);
      else if (q.gt(b, c)) q.swap(f, c);
      else q.swap(f, b);
      int lo = f + 1, hi = l;
      for (;;) {
        while (q.gt(lo, f)) ++lo;
        --hi;
        while (q.gt(f, hi)) --hi;
        if (!(lo < hi)) break;
        q.swap(lo, hi);
        ++lo;
      }
      if (l - lo > 16 && sp < 3) {                       // __introsort_loop(cut, last, depth_limit): later
        stk[sp++] = lo | (l << 8) | (depth << 16);
      }
      l = lo;
    }
  }
  if (last - first > 16) {                               // std::__final_insertion_sort
    tb_insertion_sort(q, first, first + 16);
    for (int i = first + 16; i < last; ++i) tb_unguarded_linear_insert(q, i);
  } else {
    tb_insertion_sort(q, first, last);
  }
}

// std::partial_sort's __heap_select(first = 0, middle = K, last = n) with the K-entry heap held ACROSS THE LANES of one
// wave (lane j = heap[j]; K <= 64): every heap access is a v_readlane / v_writelane with a scalar index instead of a
// dependent LDS round trip, and the scan over the n - K remaining values tests 64 of them per step.  Same compares,
// same moves as libstdc++ (__make_heap, then __pop_heap for every v[i] > heap[0]); the values evicted to positions
// >= K are not written back: nothing reads them again.  Returns with (hv, hid) = the kept set in lanes 0..K-1.
struct LaneHeap {
  float hv; int hid; int lane;
  __device__ __forceinline__ float val(int i) const {
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(hv), __builtin_amdgcn_readfirstlane(i)));
  }
  __device__ __forceinline__ int idx(int i) const {
    return __builtin_amdgcn_readlane(hid, __builtin_amdgcn_readfirstlane(i));
  }
  __device__ __forceinline__ void set(int i, float v, int id) {
    const int si = __builtin_amdgcn_readfirstlane(i);   // (v, id) are wave-uniform: a lane-select is a writelane
    hv = lane == si ? v : hv;
    hid = lane == si ? id : hid;
  }
  __device__ void push(int hole, int top, float v, int id) {          // std::__push_heap
    int parent = (hole - 1) / 2;
    while (hole > top && val(parent) > v) {
      set(hole, val(parent), idx(parent));
      hole = parent;
      parent = (hole - 1) / 2;
    }
    set(hole, v, id);
  }
  __device__ void adjust(int hole, int len, float v, int id) {        // std::__adjust_heap
    const int top = hole;
    int child = hole;
    while (child < (len - 1) / 2) {
      child = 2 * (child + 1);
      if (val(child) > val(child - 1)) --child;
      set(hole, val(child), idx(child));
      hole = child;
    }
    if ((len & 1) == 0 && child == (len - 2) / 2) {
      child = 2 * (child + 1);
      set(hole, val(child - 1), idx(child - 1));
      hole = child - 1;
    }
    push(hole, top, v, id);
  }
};

__device__ void tb_heap_select_wave(const float* v, int n, int K, LaneHeap& h, int lane) {
  h.hv = lane < K ? v[lane] : VCR_NEG_INF;
  h.hid = lane;
  h.lane = lane;
  if (K >= 2) {
    for (int parent = (K - 2) / 2;; --parent) {
      h.adjust(parent, K, h.val(parent), h.idx(parent));
      if (parent == 0) break;
    }
  }
  float top = h.val(0);
  for (int base = K; base < n; base += 64) {
    const int x = base + lane;
    const float c = x < n ? v[x] : VCR_NEG_INF;
    unsigned long long mask = __builtin_amdgcn_ballot_w64(c > top);
    while (mask) {
      const int i = __builtin_ctzll(mask);
      const float cv = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(c), __builtin_amdgcn_readfirstlane(i)));
      h.adjust(0, K, cv, base + i);                      // __pop_heap: the candidate replaces the root
      top = h.val(0);
      mask = __builtin_amdgcn_ballot_w64(c > top) & ~((2ull << i) - 1ull);
    }
  }
}

// One __unguarded_partition_pivot pass of introselect on [first, last), run by the whole block with the SAME result
// as the sequential loop.  With pivot p = v[first] after the median-of-three, the left scan stops at the elements
// <= p and the right scan at the elements >= p, in order: if A lists the positions > first with v <= p (ascending)
// and Bd the positions > first with v >= p (descending), the loop swaps A[i] <-> Bd[i] while A[i] < Bd[i] (m swaps)
// and returns cut = min(A[m], Bd[m-1]) (A[0] when m = 0).  A / Bd are built by an ordered block compaction.
__device__ int tb_partition_parallel(PairArr& q, int first, int last, int* A, int* Bd, int* red) {
  const int t = threadIdx.x, nt = blockDim.x;
  if (t == 0) {
    const int mid = first + (last - first) / 2, a = first + 1, b = mid, c = last - 1;
    if (q.gt(a, b)) {
      if (q.gt(b, c)) q.swap(first, b);
      else if (q.gt(a, c)) q.swap(first, c);
      else q.swap(first, a);
    } else if (q.gt(a, c)) q.swap(first, a);
    else if (q.gt(b, c)) q.swap(first, c);
    else q.swap(first, b);
  }
  __syncthreads();
  const float pv = q.v[first];
  const int n = last - (first + 1);
  const int per = (n + nt - 1) / nt;
  const int x0 = first + 1 + t * per, x1 = min(last, x0 + per);
  int ca = 0, cb = 0;
  for (int x = x0; x < x1; ++x) { ca += q.v[x] <= pv ? 1 : 0; cb += q.v[x] >= pv ? 1 : 0; }
  // exclusive prefix of ca over ascending threads, exclusive SUFFIX of cb (threads to the right come first in Bd):
  // wave-level shuffles + four wave totals through LDS
  const int lane = t & 63, wv = t >> 6, nwv = nt >> 6;
  int ia = ca, ib = cb;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int ua = __shfl_up(ia, o, 64), ub = __shfl_down(ib, o, 64);
    if (lane >= o) ia += ua;
    if (lane + o < 64) ib += ub;
  }
  if (lane == 63) red[wv] = ia;                          // wave totals
  if (lane == 0) red[8 + wv] = ib;
  __syncthreads();
  int offa = ia - ca, offb = ib - cb, sa = 0, sb = 0;
  for (int i = 0; i < nwv; ++i) {
    if (i < wv) offa += red[i];
    if (i > wv) offb += red[8 + i];
    sa += red[i]; sb += red[8 + i];
  }
  __syncthreads();
  red[16 + t] = offa; red[16 + nt + t] = offb;
  if (t == 0) { red[2 * nt + 16] = sa; red[2 * nt + 17] = sb; }
  __syncthreads();
  const int na = red[2 * nt + 16], nb = red[2 * nt + 17];
  {
    int oa = red[16 + t];
    for (int x = x0; x < x1; ++x) if (q.v[x] <= pv) A[oa++] = x;
    int ob = red[16 + nt + t];                           // descending order: this chunk's elements from the right
    for (int x = x1 - 1; x >= x0; --x) if (q.v[x] >= pv) Bd[ob++] = x;
  }
  __syncthreads();
  const int lim = min(na, nb);
  int mloc = 0;
  for (int i = t; i < lim; i += nt) mloc += A[i] < Bd[i] ? 1 : 0;   // monotone in i: the count is the first failure
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) mloc += __shfl_xor(mloc, o, 64);
  if (lane == 0) red[wv] = mloc;
  __syncthreads();
  int m = 0;
  for (int i = 0; i < nwv; ++i) m += red[i];
  int cut;
  if (m == 0) cut = A[0];
  else cut = min(m < na ? A[m] : 0x7fffffff, Bd[m - 1]);
  __syncthreads();                                       // everyone has read A / Bd / red before the swaps reuse LDS
  for (int i = t; i < m; i += nt) q.swap(A[i], Bd[i]);
  __syncthreads();
  return cut;
}

constexpr size_t TB_LDS_MAX = 160 * 1024;
constexpr int TB_BLOCKS = 64;

// One block per tied row: all threads recompute the row's N distances with the SAME arithmetic as the main kernels
// (C == 64: the k-ascending fma chain the MFMA produces, then the -sq_j/2 step, then 2 acc - sq_i; C == 4: the VALU
// expression of knn3_kernel), thread 0 replays the selection and rewrites the row's k indices.
__device__ void tiebreak_row(const vcr_knn_args& a, int row, unsigned char* smem, unsigned char* gwork) {
  float *val, *qrow;
  int *id, *A, *Bd, *red;
  if (!gwork) {
    // (8 bytes of padding in front: the arrays the sequential ports walk downwards must not start at LDS offset 0.  This code
    // reaches LDS through flat instructions wherever val / id may also be global (see below); the compiler turns the `v[j - 1]`
    // of a descending loop into (base - 4) + an immediate offset of 4, and a flat address below the LDS aperture faults
    // whatever the offset -- MEMORY_APERTURE_VIOLATION in the replay launch, located with rocgdb when the rank-0 sort was
    // added.  The ports never index more than one entry below their position.)
    val = reinterpret_cast<float*>(smem) + TB_LDS_PAD / 4;
    id = reinterpret_cast<int*>(val + a.N);
    qrow = reinterpret_cast<float*>(id + a.N);           // [64]
    A = reinterpret_cast<int*>(qrow + 64);               // [N] left stoppers, [N] right stoppers, block scratch
    Bd = A + a.N;
    red = Bd + a.N;                                      // [16 + 2*256 + 2]
  } else {
    // rows too long for an LDS image (N > ~10 100): the four row-sized arrays live in the caller's tie_work, one 16 N-byte
    // slice per block (the host checked that it is there); __syncthreads() orders a block's global accesses as well
    val = reinterpret_cast<float*>(gwork);
    id = reinterpret_cast<int*>(val + a.N);
    A = id + a.N;
    Bd = A + a.N;
    qrow = reinterpret_cast<float*>(smem);
    red = reinterpret_cast<int*>(qrow + 64);
  }
  {
    const int b = row / a.N, qi = row - b * a.N;
    const float* xb = a.x + (size_t)b * a.N * a.ldx;
    __syncthreads();
    if (a.C == 64 && threadIdx.x < 64) qrow[threadIdx.x] = xb[(size_t)qi * a.ldx + threadIdx.x];
    __syncthreads();
    for (int j = threadIdx.x; j < a.N; j += blockDim.x) {
      float d;
      if (a.C == 64) {
        const float* c = xb + (size_t)j * a.ldx;
        f32x4 cr[16];
#pragma unroll
        for (int m = 0; m < 16; ++m) cr[m] = ld4(c + 4 * m);    // the whole row in flight, then the chain
        float acc = 0.f;
#pragma unroll
        for (int kk = 0; kk < 64; ++kk) acc = fmaf(cr[kk >> 2][kk & 3], qrow[kk], acc);
        acc = fmaf(-0.5f * a.sq[(size_t)b * a.N + j], 1.f, acc);
        d = 2.f * acc - a.sq[(size_t)b * a.N + qi];
      } else {
        const f32x4 qv = ld4(xb + (size_t)qi * a.ldx), cv = ld4(xb + (size_t)j * a.ldx);
        const float dot = fmaf(qv[2], cv[2], fmaf(qv[1], cv[1], qv[0] * cv[0]));
        d = (2.f * dot - cv[3]) - qv[3];
      }
      val[j] = d == d ? d : VCR_NEG_INF;                 // NaN (a non-finite point): below everything, as the main kernels filter it;
      id[j] = j;                                         // the ports' stoppers and the block partition need a total order
    }
    __syncthreads();
    PairArr q{val, id};
    const int K = a.k + 1;                               // topk(k + 1)
    const bool use_heap = (long)K * 64 <= a.N;
    if (!use_heap) {
      // std::nth_element(K-1): the partition passes over long ranges run on the whole block (see below); the tail
      // (range <= 24, depth exhaustion, final insertion sort) is finished by thread 0 with the sequential port.
      int first = 0, last = a.N, depth = 0;
      for (int m = a.N; m > 1; m >>= 1) ++depth;
      depth *= 2;
      while (last - first > 24 && depth > 0) {
        --depth;
        const int cut = tb_partition_parallel(q, first, last, A, Bd, red);
        if (cut <= K - 1) first = cut; else last = cut;
      }
      if (threadIdx.x == 0) tb_nth_element(q, first, last, K - 1, depth);
    } else if (threadIdx.x < 64) {
      // std::partial_sort branch ((k+1)*64 <= N): heap across the lanes of wave 0
      LaneHeap h;
      const int lane = threadIdx.x;
      tb_heap_select_wave(val, a.N, K, h, lane);
      if (lane < K) { val[lane] = h.hv; id[lane] = h.hid; }           // the kept set, like the sequential port leaves it
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      // rank 0 = the largest of the K kept.  Shared by two or more of them (duplicate points ...): the one Tensor.topk
      // returns FIRST, i.e. position 0 after what ATen does next with the selected entries -- std::sort of the first K - 1
      // (the nth_element branch; the K-th is not above any of them) or partial_sort's __sort_heap of the K-entry heap
      int best = 0, nbest = 1;
      for (int i = 1; i < K; ++i) {
        if (val[i] > val[best]) { best = i; nbest = 1; }
        else if (val[i] == val[best]) ++nbest;
      }
      if (nbest > 1) {
        if (use_heap) tb_sort_heap(q, 0, K); else tb_sort(q, 0, K - 1, red);
        best = 0;
      }
      int32_t* o = a.idx + (size_t)row * a.k;
      int w = 0;
      for (int i = 0; i < K; ++i)
        if (i != best) o[w++] = id[i];
    }
  }
}

__device__ __forceinline__ void tiebreak_body(const vcr_knn_args& a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  // (rows too long for an LDS image: this block's slice of tie_work, see tiebreak_row)
  unsigned char* gwork = tiebreak_lds(a.N) <= TB_LDS_MAX ? nullptr
                                                         : reinterpret_cast<unsigned char*>(a.tie_work) + (size_t)blockIdx.x * 16 * a.N;
  const int count = min(a.tie_scratch[0], a.tie_cap);
  for (int t = blockIdx.x; t < count; t += gridDim.x) tiebreak_row(a, a.tie_scratch[1 + t], smem, gwork);
}

__global__ __launch_bounds__(256) void knn_tiebreak_kernel(vcr_knn_args a) { tiebreak_body(a); }
// the replays of two kNN launches in one launch (blockIdx.y picks the launch): one latency instead of two
__global__ __launch_bounds__(256) void knn_tiebreak2_kernel(vcr_knn_args a, vcr_knn_args b) {
  if (blockIdx.y == 0) tiebreak_body(a); else tiebreak_body(b);
}

}  // namespace

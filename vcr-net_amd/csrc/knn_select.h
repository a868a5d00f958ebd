// The kNN searches' selection (included by knn.hip; one translation unit): the lane geometries of the three bodies, the per-query
// value list + LDS log (Selector), the sample floor (SampleNet) and the final stage that writes a row (finish).
// Selection, round 2 (measured on the round-1 kernels: 40 % of their time went into the sorted-insert network that moved
// (value, index) pairs through 22-42 register slots, ~100 issue slots per insertion):
//   * registers hold the sorted top-KS VALUES only: an insertion is one v_med3_f32 per slot, no compares, no index traffic.  The
//     list of a query is spread over the lanes that share the query (2 for the 32-query MFMA layout, 4 in the 16-query and the
//     Cartesian VALU bodies); lane segment s takes min(d, last value of segment s-1) -- what falls off the segment above, known
//     before the insertion -- so the segments need one cross-lane move per insertion and no chain;
//   * every candidate that passed the filter stays in the query's LDS log as (value, index).  The log is compacted in place
//     against the current KS-th best value whenever it runs out of room (entries strictly above it, at most KS-1, plus as many
//     equal ones as the list itself holds), and once more at the end against the (k+2)-th best value: what is left ARE the k+1
//     neighbours.
#pragma once
#include "knn_tiebreak.h"                                // BLK_TIES: finish() lists a workgroup's tied rows for replay_block_ties

namespace {

// Row whose (k+1)-th and (k+2)-th best values are equal: hand it to knn_tiebreak_kernel (ties[0] = count).
__device__ __forceinline__ void report_tie(int32_t* ties, int cap, int row) {
  if (!ties) return;
  const int pos = atomicAdd(&ties[0], 1);
  if (pos < cap) ties[1 + pos] = row;
}

// ---- lane geometry of a query's lanes.  Every cross-lane move is issued with all lanes active and only its RESULT
// is selected per lane (DPP / permlane reads of switched-off lanes return 0).
struct GeomMfma {                    // 32 query columns, lanes l and l+32 share one: segment = lane >> 5
  static constexpr int COLS = 32, LPQ = 2;
  static constexpr bool SPLIT_COMPACT = false;
  __device__ static __forceinline__ int ord(int) { return 0; }
  __device__ static __forceinline__ int prefix(int x, int, int& total) { total = x; return 0; }
  __device__ static __forceinline__ int col(int lane) { return lane & 31; }
  __device__ static __forceinline__ int seg(int lane) { return lane >> 5; }
  // x of segment `which` (0 / 1), in every lane of the column (v_permlane32_swap: result 0 = the lower half's values
  // in both halves, result 1 = the upper half's)
  __device__ static __forceinline__ int from_seg(int x, int which) {
    const auto r = __builtin_amdgcn_permlane32_swap(x, x, false, false);
    return which ? r[1] : r[0];
  }
  __device__ static __forceinline__ int from_prev(int x, int, int) { return from_seg(x, 0); }   // only segment 1 has a predecessor
  __device__ static __forceinline__ int prev_addr(int) { return 0; }
  __device__ static __forceinline__ int col_sum(int x, int sg) { return x + from_seg(x, sg ^ 1); }
};
struct GeomCol16 {                   // v_mfma_f32_16x16x4_f32 layout: 16 query columns, lanes c, c+16, c+32, c+48 share one.
  // The value list of a query runs through its four lanes in the row order 0 -> 1 -> 3 -> 2 (seg 0..3), chosen so that
  // every segment's predecessor is ONE row swap away: v_permlane16_swap exchanges rows (0,1) and (2,3),
  // v_permlane32_swap rows (0,2) and (1,3).  With both operands = x, swap16 returns {even row of the pair, odd row of
  // the pair} in every lane of the pair, swap32 {row of the lower half, row of the upper half} in both halves.
  static constexpr int COLS = 16, LPQ = 4;
  __device__ static __forceinline__ int col(int lane) { return lane & 15; }
  __device__ static __forceinline__ int seg(int lane) { const int q = lane >> 4; return q ^ (q >> 1); }   // 0,1,3,2
  __device__ static __forceinline__ int from_seg(int x, int which) {      // `which` is wave-uniform
    const int q = which ^ (which >> 1);                                   // the row that holds segment `which`
    const auto a = __builtin_amdgcn_permlane16_swap(x, x, false, false);
    const int v = (q & 1) ? a[1] : a[0];
    const auto b = __builtin_amdgcn_permlane32_swap(v, v, false, false);
    return (q >> 1) ? b[1] : b[0];
  }
  // segment sg - 1's value (sg == 0: unused): row 1 <- row 0; row 3 <- row 1; row 2 <- row 3.  ONE ds_bpermute_b32 on the
  // otherwise idle LDS crossbar instead of both row swaps, their operand copies and the selects (9 VALU instructions of
  // the 17 an insertion cost -- the drains are bound by VALU issue, four waves per SIMD cover the longer latency).
  // (The same exchange for the per-tile / per-compaction-round prefixes was measured and is slower: those chains are
  // short and wait for the crossbar.)
  __device__ static __forceinline__ int prev_addr(int lane) {
    const int q = lane >> 4, pq = q == 1 ? 0 : q == 3 ? 1 : q == 2 ? 3 : 0;
    return 4 * (16 * pq + (lane & 15));
  }
  __device__ static __forceinline__ int from_prev(int x, int, int pa) { return __builtin_amdgcn_ds_bpermute(pa, x); }
  __device__ static __forceinline__ int col_sum(int x, int sg) {
    const int q = sg ^ (sg >> 1);
    const auto a = __builtin_amdgcn_permlane16_swap(x, x, false, false);
    x += (q & 1) ? a[0] : a[1];
    const auto b = __builtin_amdgcn_permlane32_swap(x, x, false, false);
    return x + ((q >> 1) ? b[0] : b[1]);
  }
  // exclusive prefix of x over the four lanes of a column in ROW order (row = lane >> 4), and the total
  static constexpr bool SPLIT_COMPACT = true;            // log rows PEND .. PEND + 3 exist (one trash row per lane row)
  __device__ static __forceinline__ int ord(int lane) { return lane >> 4; }
  __device__ static __forceinline__ int prefix(int x, int row, int& total) {
    const auto a = __builtin_amdgcn_permlane16_swap(x, x, false, false);      // {even row, odd row} of the pair
    const int pair_total = a[0] + a[1];
    const auto b = __builtin_amdgcn_permlane32_swap(pair_total, pair_total, false, false);   // {rows 0+1, rows 2+3}
    total = b[0] + b[1];
    return ((row & 1) ? a[0] : 0) + ((row >> 1) ? b[0] : 0);
  }
};
struct GeomQuad {                    // 16 queries, one DPP quad each: segment = lane & 3
  static constexpr int COLS = 16, LPQ = 4;
  static constexpr bool SPLIT_COMPACT = false;
  __device__ static __forceinline__ int ord(int) { return 0; }
  __device__ static __forceinline__ int prefix(int x, int, int& total) { total = x; return 0; }
  __device__ static __forceinline__ int col(int lane) { return lane >> 2; }
  __device__ static __forceinline__ int seg(int lane) { return lane & 3; }
  __device__ static __forceinline__ int from_seg(int x, int which) {
    const int a = __builtin_amdgcn_mov_dpp(x, 0x00, 0xF, 0xF, true), b = __builtin_amdgcn_mov_dpp(x, 0x55, 0xF, 0xF, true);
    const int c = __builtin_amdgcn_mov_dpp(x, 0xAA, 0xF, 0xF, true), d = __builtin_amdgcn_mov_dpp(x, 0xFF, 0xF, 0xF, true);
    return which == 0 ? a : which == 1 ? b : which == 2 ? c : d;
  }
  __device__ static __forceinline__ int from_prev(int x, int, int) { return __builtin_amdgcn_mov_dpp(x, 0x90, 0xF, 0xF, true); }
  __device__ static __forceinline__ int prev_addr(int) { return 0; }
  __device__ static __forceinline__ int col_sum(int x, int) {
    x += __builtin_amdgcn_mov_dpp(x, 0xB1, 0xF, 0xF, true);    // quad_perm [1,0,3,2]
    x += __builtin_amdgcn_mov_dpp(x, 0x4E, 0xF, 0xF, true);    // quad_perm [2,3,0,1]
    return x;
  }
};
template <class G> __device__ __forceinline__ float gf_from_seg(float x, int which) {
  return __int_as_float(G::from_seg(__float_as_int(x), which));
}

// ---- log capacity per query (rows of the LDS log): room for the KS-1 entries a compaction can leave, the <= 16 a step adds,
// and slack so that compactions stay rare.
// 32-query kernels: measured for the MFMA kernel at k = 20 (MI355X, 32 clouds): 96 / 128 entries make the kernel alone 7 %
// faster at N = 1024 (fewer compactions) but cost the second workgroup per CU at N = 2048 (+20 %) and the co-residency of the
// one-launch kNN pair (+20 %): 64 stays.
constexpr int KNN_PEND_MFMA = 64;
// 16-query kernels (k <= 20): 72 -- the most that keeps four workgroups per CU (4 x (76 rows x 16 queries x 8 B x 4 waves
// + the tie list) = 157 KB of the 160): a compaction then frees 35 slots instead of 27.  Measured against 64: the pair
// launch 151.4 -> 147.7 us at BASELINE configs[1], 147.5 -> 136.7 at N = 768 (configs[2]), 439 -> 432 at N = 2048.
constexpr int KNN_PEND_COL16 = 72;                       // (the sweeps: profiles/experiments/probe_build.py --set NAME=VALUE)
constexpr int KNN_PEND_K40 = 96;                         // k = 21 .. 40 (lists of 42)
template <class G, int KS> constexpr int pend_of() {
  return KS > 22 ? KNN_PEND_K40 : std::is_same<G, GeomMfma>::value ? KNN_PEND_MFMA : std::is_same<G, GeomCol16>::value ? KNN_PEND_COL16 : 64;
}

// ---- per-query selection state of one wave: sorted top-KS values in registers (T per lane), (value, index) log in LDS
// v_med3_f32 a, b, (+-inf in an SGPR): see Selector::insert
__device__ __forceinline__ float med3_inf(float a, float b, float inf) {
  float r;
  asm("v_med3_f32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "s"(inf));
  return r;
}
template <class G, int KS>
struct Selector {
  static constexpr int PEND = pend_of<G, KS>();
  static constexpr int T = (KS + G::LPQ - 1) / G::LPQ;   // values per lane; the list holds LPQ*T >= KS values
  static constexpr int TL = (KS - 1) / T, TS = (KS - 1) % T;   // segment / slot of rank KS-1: the filter threshold
  float v[T];
  float* lv; int* li;                                    // log [PEND + 1][COLS]; row PEND swallows the writes of lanes
                                                         // that have nothing to log (branch-free appends)
  int cnt, done;                                         // entries logged / already inserted (same in a query's lanes)
  float thr;                                             // max(thr0, rank KS-1 value): nothing <= thr can be a neighbour
  float thr0;                                            // filter floor taken from a sample of the candidates (see SampleNet; -inf: none)
  int col, sg, pa;

  __device__ __forceinline__ void init(float* lv_, int* li_, int lane, float floor0 = VCR_NEG_INF) {
    lv = lv_; li = li_; cnt = 0; done = 0; thr = thr0 = floor0; col = G::col(lane); sg = G::seg(lane); pa = G::prev_addr(lane);
#pragma unroll
    for (int t = 0; t < T; ++t) v[t] = VCR_NEG_INF;
  }
  // one value into the query's list, all segments at once (inserting -inf or anything <= the last value is a no-op)
  __device__ __forceinline__ void insert(float d) {
    const float pb = __int_as_float(G::from_prev(__float_as_int(v[T - 1]), sg, pa));
    // (v_med3_f32 with an infinite third operand: min / max in ONE instruction.  Spelled as inline assembly: hipcc folds
    // the builtin with an infinite constant back into v_min / v_max plus a NaN-quieting v_max x, x per operand -- four
    // instructions for the clamp, three for the head of the list)
    d = med3_inf(d, sg ? pb : __builtin_huge_valf(), VCR_NEG_INF);       // min(d, predecessor's last); segment 0 has none
#pragma unroll
    for (int t = T - 1; t >= 1; --t) v[t] = __builtin_amdgcn_fmed3f(v[t - 1], d, v[t]);
    v[0] = med3_inf(v[0], d, __builtin_huge_valf());
  }
  __device__ __forceinline__ void refresh_thr() {
    const float mine = v[TS];
    thr = fmaxf(thr0, gf_from_seg<G>(mine, TL));
  }
  // The floor came from a sample: it is only valid if at least KS candidates lie above it.  False -> the list is not
  // full although a floor was used: the caller scans again without one.
  __device__ __forceinline__ bool floor_held() const {
    const float last = gf_from_seg<G>(v[TS], TL);
    return !(thr0 > VCR_NEG_INF) || last > VCR_NEG_INF;
  }
  // value at global rank r (wave-uniform r) in every lane of the column
  __device__ __forceinline__ float rank_value(int r) const {
    const int rs = r / T, rt = r % T;
    int bits = 0;                                        // (an OR of masked words: a select chain over v[] would be
#pragma unroll                                           // turned into a dynamically indexed scratch array)
    for (int t = 0; t < T; ++t) bits |= (rt == t ? -1 : 0) & __float_as_int(v[t]);
    return gf_from_seg<G>(__int_as_float(bits), rs);
  }
  // insert the values logged since the last drain.  Four log reads are in flight per round trip: the loop is bound by
  // LDS latency, not by the 1-med3-per-slot network.
  __device__ __forceinline__ void drain() {
    int i = done;
    while (__any(i < cnt)) {
      float d[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) d[u] = lv[min(i + u, PEND - 1) * G::COLS + col];
#pragma unroll
      for (int u = 0; u < 4; ++u) insert(i + u < cnt ? d[u] : VCR_NEG_INF);      // idle lanes insert -inf: a no-op
      i += 4;
    }
    done = cnt;
    refresh_thr();
  }
  // keep the log entries above x, plus at most `emax` equal to x (the earliest logged); cnt = done = kept
  __device__ __forceinline__ void compact(float x, int emax) {
    if constexpr (G::SPLIT_COMPACT) {
      // the four lanes of a column take one entry each per round (the loop below has every lane walk all four: four
      // times the LDS instructions): keep flags and write positions come from prefixes over the lanes in row order, so
      // the kept entries stay in logging order and the "at most emax equal to x, the earliest" rule is unchanged
      int w = 0, ne = 0;
      const int od = G::ord((int)__lane_id());            // (recomputed here: a register less across the scan)
      for (int i = 0; __any(i < cnt); i += 4) {
        const int ii = i + od;
        const bool valid = ii < cnt;
        const int ic = min(ii, PEND - 1);
        const float d = lv[ic * G::COLS + col];
        const int j = li[ic * G::COLS + col];
        const bool gt = valid && d > x, eq = valid && d == x;
        // ONE prefix for both counts (packed: entries above x in the low half, entries equal to x in the high half); of
        // the equal ones the first `cap` still wanted are kept, so their kept-prefix is min(prefix, cap)
        int tot;
        const int pre = G::prefix((gt ? 1 : 0) | (eq ? 0x10000 : 0), od, tot);
        const int cap = max(emax - ne, 0), epre = pre >> 16, etot = tot >> 16;
        const bool keep = gt || (eq && epre < cap);
        const int kpre = (pre & 0xffff) + min(epre, cap);
        const int wr = keep ? w + kpre : PEND + od;      // w + kpre <= i + od: in place; reads of the round precede its writes
        lv[wr * G::COLS + col] = d;
        li[wr * G::COLS + col] = j;
        w += (tot & 0xffff) + min(etot, cap);
        ne += min(etot, cap);
      }
      cnt = done = w;
      return;
    }
    int w = 0, ne = 0;
    for (int i = 0; __any(i < cnt); i += 4) {
      float d[4];
      int j[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {                      // all four entries are in registers before any is rewritten
        const int ii = min(i + u, PEND - 1);
        d[u] = lv[ii * G::COLS + col];
        j[u] = li[ii * G::COLS + col];
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const bool eq = d[u] == x && ne < emax;
        const bool keep = i + u < cnt && (d[u] > x || eq);
        const int wr = keep ? w : PEND;                  // w <= i + u: in place (the lanes of a column write the same words)
        lv[wr * G::COLS + col] = d[u];
        li[wr * G::COLS + col] = j[u];
        w += keep ? 1 : 0;
        ne += (keep && eq) ? 1 : 0;
      }
    }
    cnt = done = w;
  }
  __device__ __forceinline__ int count_above(float x) const {
    int c = 0;
#pragma unroll
    for (int t = 0; t < T; ++t) c += v[t] > x ? 1 : 0;
    return G::col_sum(c, sg);
  }
  // make room for the next step (<= 16 new entries per query)
  __device__ __forceinline__ void make_room() {
    if (__any(cnt > PEND - 16)) {
      drain();
      compact(thr, KS - count_above(thr));
    }
  }
};

// Filter floor from a SAMPLE of the candidates.  A streaming top-k logs k (1 + ln(n / k)) candidates per query because
// its threshold starts at -inf; most of those are entries the first few hundred candidates push through a list that
// later ones empty again.  A values-only pre-pass (R v_med3 per candidate) over a lane's share of the first 256
// candidates keeps its R best; the smallest of the lanes' R-th values is a floor with at least LPQ * R - 1 sample
// values strictly above it, and R is chosen so that this is >= KS: the floor is below the final KS-th best value by
// construction, for ANY ordering of the cloud.  The scan proper then starts with a useful threshold: at N = 1024,
// k = 20 it logs ~55 candidates per query instead of ~125, and the log rarely needs compacting.  (Exact ties AT the
// floor value could still leave fewer than KS values strictly above it; that is checked at the end -- floor_held() --
// and such a wave scans again without a floor.)
constexpr int SAMPLE = 256;
template <int R>
struct SampleNet {
  float s[R];
  __device__ __forceinline__ void init() {
#pragma unroll
    for (int t = 0; t < R; ++t) s[t] = VCR_NEG_INF;
  }
  __device__ __forceinline__ void insert(float d) {
#pragma unroll
    for (int t = R - 1; t >= 1; --t) s[t] = __builtin_amdgcn_fmed3f(s[t - 1], d, s[t]);
    s[0] = med3_inf(s[0], d, __builtin_huge_valf());
  }
};
template <class G> __device__ __forceinline__ float col_min(float x, int sg) {   // min over the lanes of a query
  float m = x;
#pragma unroll
  for (int w = 0; w < G::LPQ; ++w) m = fminf(m, gf_from_seg<G>(x, w));
  (void)sg;
  return m;
}

// Final stage shared by the three bodies: the log holds every candidate above the (k+2)-th best value; fold the lists /
// logs of the S waves of a query group into wave part 0, reduce the log to the k+1 best, drop rank 0, write the set.
// perm (ordered search): q and the logged indices are RANKS of the cloud's Morton order; the kept entries are translated to
// point indices before the rank-0 rule and the output, which goes to the row of the point at rank q
template <class G, int KS, int S>
__device__ __forceinline__ void finish(Selector<G, KS>& sel, const vcr_knn_args& a, int b, int q, int wave, int part,
                                       unsigned char* smem, int* blk_ties = nullptr, const int32_t* perm = nullptr) {
  constexpr int T = Selector<G, KS>::T;
  constexpr int PEND = Selector<G, KS>::PEND;
  constexpr int AREA = 2 * (PEND + 1) * G::COLS;         // floats per wave
  sel.drain();
  if (S > 1) {
    // every wave first shrinks its log to its own top-KS and parks its sorted values behind it (KS <= 22: 22 + 24 <= 64)
    sel.compact(sel.thr, KS - sel.count_above(sel.thr));
#pragma unroll
    for (int t = 0; t < T; ++t) sel.lv[(PEND - G::LPQ * T + sel.sg * T + t) * G::COLS + sel.col] = sel.v[t];
    if (sel.sg == 0) sel.li[(PEND - 1) * G::COLS + sel.col] = sel.cnt;
    __syncthreads();
    if (part == 0) {
      for (int p = 1; p < S; ++p) {
        const float* ov = reinterpret_cast<const float*>(smem) + (size_t)(wave + p) * AREA;
        for (int t = 0; t < KS; ++t) sel.insert(ov[(PEND - G::LPQ * T + t) * G::COLS + sel.col]);
      }
      sel.refresh_thr();
    }
  }
  if (part != 0) return;
  const float vk = sel.rank_value(a.k), vk1 = sel.rank_value(a.k + 1);       // ranks k+1 and k+2 (KS >= k+2)
  const int need = a.k + 1 - sel.count_above(vk1);      // neighbours that EQUAL the (k+2)-th value: 0 unless tied
  sel.compact(vk1, need);
  if (S > 1) {                                           // append the other waves' qualifying entries
    int ne = 0;
    for (int i = 0; i < sel.cnt; ++i) ne += sel.lv[i * G::COLS + sel.col] == vk1 ? 1 : 0;
    for (int p = 1; p < S; ++p) {
      const float* ov = reinterpret_cast<const float*>(smem) + (size_t)(wave + p) * AREA;
      const int* oi = reinterpret_cast<const int*>(ov + (PEND + 1) * G::COLS);
      const int oc = oi[(PEND - 1) * G::COLS + sel.col];
      for (int i = 0; __any(i < oc); ++i) {
        const int ii = min(i, PEND - 1);
        const float d = ov[ii * G::COLS + sel.col];
        const int j = oi[ii * G::COLS + sel.col];
        const bool eq = d == vk1 && ne < need;
        const bool keep = i < oc && (d > vk1 || eq) && sel.cnt < PEND;
        if (keep) { sel.lv[sel.cnt * G::COLS + sel.col] = d; sel.li[sel.cnt * G::COLS + sel.col] = j; }
        sel.cnt += keep ? 1 : 0;
        ne += (keep && eq) ? 1 : 0;
      }
    }
  }
  // rank 0 = the largest value (the point itself): dropped.  When that value is SHARED (duplicate points, or a neighbour so
  // close that its distance rounds to the point's own), WHICH of the tied entries Tensor.topk returns first is an outcome of
  // its sort (util.py:159 then drops that one and keeps the others): such a row is replayed like a boundary tie (best_shared
  // below; tiebreak_row sorts the kept entries the way ATen does).  Without tie_scratch: the first logged is dropped.
  // (Whether it is shared is read off the sorted value list: its two best entries are equal.)
  // (-inf == -inf is no tie: a query with fewer than two finite scores -- its own coordinate non-finite -- has nothing to replay)
  const bool best_shared = sel.rank_value(0) == sel.rank_value(1) && sel.rank_value(1) > VCR_NEG_INF;
  int imax = 0;
  float vmax = VCR_NEG_INF;
  if (perm) {
    // (the plain scan logs in index order, so "the first logged" is the LOWEST point index among the largest values)
    for (int i = sel.sg; i < sel.cnt; i += G::LPQ) sel.li[i * G::COLS + sel.col] = perm[sel.li[i * G::COLS + sel.col]];
    int jmax = 0x7fffffff;
    for (int i = 0; __any(i < sel.cnt); ++i) {
      const int ic = min(i, PEND - 1);
      const float d = i < sel.cnt ? sel.lv[ic * G::COLS + sel.col] : VCR_NEG_INF;
      const int j = sel.li[ic * G::COLS + sel.col];
      if (d > vmax || (d == vmax && i < sel.cnt && j < jmax)) { vmax = d; imax = i; jmax = j; }
    }
  } else {
  for (int i = 0; __any(i < sel.cnt); ++i) {
    const float d = i < sel.cnt ? sel.lv[min(i, PEND - 1) * G::COLS + sel.col] : VCR_NEG_INF;
    if (d > vmax) { vmax = d; imax = i; }
  }
  }
  if (q < a.N) {
    if (perm) q = perm[q];
    int32_t* o = a.idx + ((size_t)b * a.N + q) * a.k;
    for (int i = sel.sg; i < sel.cnt && i <= a.k; i += G::LPQ)
      if (i != imax) o[i - (i > imax ? 1 : 0)] = sel.li[i * G::COLS + sel.col];
    // A short list -- NaN scores never pass the filter: the query's own coordinate is non-finite, or its cloud has fewer than
    // k + 1 finite points -- leaves slots unwritten: they take the query's own index, so that every slot is a row of its cloud.
    for (int i = min(sel.cnt, a.k + 1) - (sel.cnt > 0 ? 1 : 0) + sel.sg; i < a.k; i += G::LPQ) o[i] = q;
    if (sel.sg == 0 && ((vk1 == vk && vk1 > VCR_NEG_INF) || best_shared)) {
      if (blk_ties) {                                    // replayed by this very workgroup (replay_block_ties)
        const int pos = atomicAdd(&blk_ties[0], 1);
        if (pos < BLK_TIES) blk_ties[1 + pos] = b * a.N + q;
      } else {
        report_tie(a.tie_scratch, a.tie_cap, b * a.N + q);
      }
    }
  }
}

}  // namespace

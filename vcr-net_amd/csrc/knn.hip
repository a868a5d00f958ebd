// Kernel 1: fused pairwise-distance + top-k (util/util.py:143-160).  The N x N distance matrix is never written: distances are produced
// tile by tile in registers and filtered against each query's current (k+2)-th best value; survivors are logged per query in LDS
// (knn_select.h).  D_ij = (-sq_j + 2 x_i.x_j) - sq_i (the association of util.py:157-158); idx = top-(k+1) of D_i. by value, rank 0
// dropped (util.py:159), written as a SET; rows with an exact tie at the boundary or at the best value are replayed (knn_tiebreak.h).
// Bit-exactness: every body forms the dot product as a k-ASCENDING fma chain, then -sq_j/2 as one more k-step, then 2 acc - sq_i
// (doubling is exact): with the pointwise kernel's reference-ordered features and norms the distance matrix is BIT-IDENTICAL to the
// reference's (CPU sgemm = k-ascending fma chain; verified), so every body and launch form gives the same sets.
// Three bodies; knn_plan() decides which one a search runs, pair_form() whether the two searches of a pass share a launch:
//   knn64c_body  16-query waves on v_mfma_f32_16x16x4_f32, four unsplit waves: feature rows (C == 64) from 1024 groups of 16 queries
//                up, every unsplit Cartesian search (C == 4: ONE MFMA per tile), the fused knn_pair_kernel, the ordered search.
//   knn64_body   32-query waves on v_mfma_f32_32x32x2_f32 (C == 64), S = 1 / 2 / 4 waves splitting a query group's candidates: small grids.
//   knn3_body    Cartesian rows on the VALU, one DPP quad per query, S = 2 / 4: the small Cartesian grids.
#include "common.h"
#include "vcr_internal.h"
#include "knn_tiebreak.h"
#include "knn_select.h"

namespace {

constexpr int TILE = 32;            // candidates per MFMA tile of the 32-query body
constexpr int KNN_MAX_N = 131072;                       // points per cloud the kNN entry points accept: the largest size that is validated
                                                         // (sampled rows at N = 70 001 and 131 072, tests/test_hip_kernels.py; beyond: VCR_EUNSUPPORTED
                                                         // rather than an unvalidated result).  The whole forward keeps its own, lower limit: forward.hip
static bool knn_rows_overflow(const vcr_knn_args* a) { return (long long)a->B * a->N >= (1ll << 31); }   // row = b * N + q is an int
constexpr int KNN_ORD_NEAR = 4;                          // tiles on either side of the own one scanned first
constexpr int KNN_ORD_MAX_TILES = 512;                   // the ordered search's wave-uniform tile mask: clouds of up to 8192 points
// "//@probe ..." lines: inert here, uncommented by profiles/experiments/probe_build.py (phase clocks of wave 0).

// ---------------------------------------------------------------- C == 64 (MFMA)
// Workgroup = W waves = W/S query tiles of 32 queries; wave (qt, part) scans candidate tiles part, part+S, ...
// (W = 4, or 2 for k > 20 whose longer logs would otherwise leave one workgroup per CU)
template <int KS, int S, int W>
__device__ __forceinline__ void knn64_body(const vcr_knn_args& a, int bx, int b) {   // block bx of cloud b
  using G = GeomMfma;
  constexpr int PEND = pend_of<G, KS>();
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int half = lane >> 5, col = lane & 31;
  const int qt = wave / S, part = wave % S;
  const int q0 = (bx * (W / S) + qt) * 32;       // this wave's 32 queries (may lie beyond N: clamped, not written)
  float* lv = reinterpret_cast<float*>(smem) + wave * (2 * (PEND + 1) * 32);
  Selector<G, KS> sel;

  const float* xb = a.x + (size_t)b * a.N * a.ldx;
  const float* sqb = a.sq + (size_t)b * a.N;
  const int q = min(q0 + col, a.N - 1);
  // query fragment: this lane supplies B[k][col] with k = 2s + half for MFMA step s, i.e. the NATURAL k
  // order: the MFMA result is then bit-for-bit the k-ascending fma chain that the reference's CPU sgemm
  // produces (verified against torch.matmul), and with the exact |x|^2 association of the pointwise kernel
  // the whole distance matrix -- hence every top-k set -- equals the reference's.
  // Loads stay 16 B wide: both lanes of a row fetch the whole row and each keeps its parity.
  auto pick = [&](const f32x4* raw, float* dst) {
#pragma unroll
    for (int st = 0; st < 32; ++st) dst[st] = half ? raw[st >> 1][(st & 1) * 2 + 1] : raw[st >> 1][(st & 1) * 2];
  };
  float qf[32];
  {
    f32x4 raw[16];
#pragma unroll
    for (int m = 0; m < 16; ++m) raw[m] = ld4(xb + (size_t)q * a.ldx + 4 * m);
    pick(raw, qf);
  }
  const float sq_q = sqb[q];

  const int ntiles = (a.N + TILE - 1) / TILE;
  //@probe VCR_PROBE_ACC_DECL;
  // walk candidate tiles t0, t0 + S, ... < t1: operands prefetched one tile ahead as raw rows (64 VGPRs), the MFMA
  // chain, then body(tile, acc)
  auto scan_tiles = [&](int t0, int t1, auto&& body) {
    float cf[32];
    float csq = 0.f;
    if (t0 < t1) {
      const int c = min(t0 * TILE + col, a.N - 1);
      f32x4 raw[16];
#pragma unroll
      for (int m = 0; m < 16; ++m) raw[m] = ld4(xb + (size_t)c * a.ldx + 4 * m);
      pick(raw, cf);
      csq = sqb[c];
    }
    for (int tile = t0; tile < t1; tile += S) {
      f32x4 nraw[16];
      float nsq = 0.f;
      if (tile + S < t1) {
        const int c = min((tile + S) * TILE + col, a.N - 1);
#pragma unroll
        for (int m = 0; m < 16; ++m) nraw[m] = ld4(xb + (size_t)c * a.ldx + 4 * m);
        nsq = sqb[c];
      }
      f32x16 acc = {0};
#pragma unroll
      for (int st = 0; st < 32; ++st) acc = mfma32(cf[st], qf[st], acc);
      // 33rd k-step: A[cand][k*] = -sq_cand/2 (half 0), B[k*][q] = 1  ->  acc = dot - sq_j/2, rounded once
      acc = mfma32(half == 0 ? -0.5f * csq : 0.f, half == 0 ? 1.f : 0.f, acc);
      // hipcc (ROCm 7.2) under-pads the MFMA -> v_accvgpr_read hazard of this 16-pass instruction when the
      // accumulator lands in AGPRs (seen in the k = 40 build: register 15, the last one written, was read stale).
      // Tie the wait states to the accumulator itself so they cannot be scheduled away.
      if (KS > 22) asm volatile("s_nop 15\n\ts_nop 7" : "+v"(acc));
      //@probe VCR_PROBE_ACC(0);                                            // prefetch issue + MFMA chain
      body(tile, acc);
      if (tile + S < t1) {
        pick(nraw, cf);
        csq = nsq;
      }
      //@probe VCR_PROBE_ACC(3);                                            // operand pick (waits for the prefetched rows)
    }
  };
  // the selection proper: filter against sel.thr, log, drain
  auto select_body = [&](int tile, const f32x16& acc) {
    const int jbase = tile * TILE;
    const bool ragged = jbase + TILE > a.N;              // only the last tile can hold rows beyond N
    // two steps of 16 rows per query (8 per lane): the log has room for 16 new entries, never for 32
#pragma unroll
    for (int hs = 0; hs < 2; ++hs) {
      sel.make_room();
      //@probe VCR_PROBE_ACC(2);
      float dd[8];
      unsigned m = 0;
#pragma unroll
      for (int r = 0; r < 8; ++r) {
        dd[r] = 2.f * acc[8 * hs + r] - sq_q;            // (-sq_j + 2 dot) - sq_i
        m |= dd[r] > sel.thr ? (1u << r) : 0u;
      }
      if (ragged) {
#pragma unroll
        for (int r = 0; r < 8; ++r) m &= (jbase + acc_row(8 * hs + r, half) < a.N) ? ~0u : ~(1u << r);
      }
      const unsigned om = (unsigned)G::from_seg((int)m, half ^ 1);
      //@probe VCR_PROBE_ACC(1);
      if (__any(m != 0)) {                               // the two lanes of a column append to ONE log: upper half first
        const int base = sel.cnt + (half ? __popc(om) : 0);
#pragma unroll
        for (int r = 0; r < 8; ++r) {                    // branch-free: a lane without a survivor in row r writes the trash row
          const int pos = (m & (1u << r)) ? base + __popc(m & ((1u << r) - 1u)) : PEND;
          sel.lv[pos * 32 + col] = dd[r];
          sel.li[pos * 32 + col] = jbase + acc_row(8 * hs + r, half);
        }
      }
      sel.cnt += __popc(m) + __popc(om);
      //@probe VCR_PROBE_ACC(4);
      if (__any(sel.cnt - sel.done > 16)) sel.drain();   // keep the threshold fresh
      //@probe VCR_PROBE_ACC(5);
    }
  };
  // (no sample floor here: a values-only pre-pass over the first candidates was measured a loss at C == 64, where a sampled tile costs
  //  its 33 MFMAs a second time -- figures in profiles/NOTES.md, round 6, the kNN source split; the Cartesian searches keep theirs)
  sel.init(lv, reinterpret_cast<int*>(lv + (PEND + 1) * 32), lane);
  scan_tiles(part, ntiles, select_body);
  sel.drain();
  // (never taken -- no floor, the compiler drops it; without it in the source the S = 1 kernels swap two instructions, NOTES.md)
  if (__any(!sel.floor_held())) {
    sel.init(lv, reinterpret_cast<int*>(lv + (PEND + 1) * 32), lane);
    scan_tiles(part, ntiles, select_body);
  }
  //@probe VCR_PROBE_ACC_FLUSH(threadIdx.x == 0 && blockIdx.y == 0, blockIdx.x);
  finish<G, KS, S>(sel, a, b, q0 + col, wave, part, smem);
}
template <int KS, int S, int W>
__global__ __launch_bounds__(64 * W, 2) void knn64_kernel(vcr_knn_args a) {
  int bx, b;
  xcd_chunk2(bx, b);                                     // a cloud's query tiles share one XCD's L2
  knn64_body<KS, S, W>(a, bx, b);
}

// ---------------------------------------------------------------- C == 64 on v_mfma_f32_16x16x4_f32 (round 3)
// Half-size waves: 16 queries per wave (MFMA columns), candidate tiles of 16 (MFMA rows), four lanes per query.  Twice as
// many, half as wide waves as knn64_body with the SAME selection work per query (one value list, one log), ~100 VGPRs and
// 8 KB of log per wave: four waves per SIMD instead of one or two, so one wave's 17-MFMA distance chain and its LDS /
// scalar-branch latencies run under the other waves' selection code (rocprofv3 counters of the 32-query kernel in the
// one-launch pair: VALU issuing in 30 % of its wave-cycles, 26 % parked at a waitcnt, 32 % waiting to issue).
// k order: MFMA step s multiplies k = 4s .. 4s+3 (lane row q supplies k = 4s + q), i.e. the natural ascending order, so
// the distance is bit-for-bit the same k-ascending fma chain as in knn64_body and in the reference's CPU sgemm; the
// -sq_j/2 term rides as a 17th step.  Operands are read from the natural [N][64] rows as 16-B chunks and transposed
// across the four lane rows of a column in registers (see load_raw / transpose).
// C == 4 (the Cartesian search, rows (x, y, z, |p|^2)): the whole distance is ONE MFMA -- lane row q4 < 3 supplies
// coordinate q4 of its candidate row (A) and of its query (B), lane row 3 supplies -|c|^2 / 2 and 1: the hardware's
// k-ascending chain is ((x x' + y y') + z z') - |c|^2 / 2, exactly the fma chain + norm step of the C = 64 case and of the
// VALU kernel knn3_body (whose (2 dot - |c|^2) - |q|^2 is the same rounding: doubling is exact).  The Cartesian
// search's distances then cost the idle matrix pipe one instruction per 16 x 16 tile instead of 16 VALU FMAs per wave.
template <int KS, int W, int C = 64, bool XT = false, bool ORD = false>
__device__ __forceinline__ void knn64c_body(const vcr_knn_args& a, int bx, int b) {
  using G = GeomCol16;
  static_assert(C == 64 || C == 4, "feature rows of 64 floats or xyz4 rows");
  static_assert(!ORD || C == 4 || XT, "the ranked rows are stored in xt's layout");
  constexpr int NST = C == 64 ? 16 : 1;                  // MFMA steps of the dot product
  constexpr int PEND = pend_of<G, KS>();
  constexpr int CT = 16;                                 // candidates per tile
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int q4 = lane >> 4, col = lane & 15;
  const int q0 = (bx * W + wave) * 16;
  // log [PEND + 4][16]: rows PEND .. PEND+3 swallow the branch-free appends of lanes without a survivor, one row per
  // lane row q4 (the four lanes of a column would otherwise hit one LDS word with four different values)
  constexpr int LROWS = PEND + 4;
  float* lv = reinterpret_cast<float*>(smem) + wave * (2 * LROWS * 16);
  Selector<G, KS> sel;
  // (ORD: the rows in rank order -- vcr_knn_args.xp / sqp; everything below then counts ranks, finish() translates)
  // (an ORD launch may still run ONE of its two searches the plain way -- or single clouds of one: vcr_knn_args.ord_ok)
  const bool ord = ORD && a.perm != nullptr && (C != 64 || !a.ord_ok || a.ord_ok[b] != 0);
  const float* xb = (ord ? a.xp : a.x) + (size_t)b * a.N * a.ldx;
  // (C == 64) rows whose 16-channel groups are stored transposed (vcr_knn_args.xt): lane row q4's chunks 4 g + q4 are its
  // operands of steps 4 g .. 4 g + 3 as they lie -- same addresses, no shuffles
  constexpr bool pre = C == 64 && XT;                  // (a compile-time variant: the launcher picks it when a.xt is set)
  const float* xl = ord ? xb : pre ? a.xt + (size_t)b * a.N * a.ldx : xb;
  const float* sqb = C == 64 ? (ord ? a.sqp : a.sq) + (size_t)b * a.N : nullptr;
  const int q = min(q0 + col, a.N - 1);
  // Operand fetch (C == 64).  MFMA step s needs x[row][4 s + q4] in lane row q4: every fourth float of the row.  Fetched as such
  // (16 x global_load_dword) the texture path sees 4-byte requests -- 8x the requests of knn64_body per byte, and the
  // kernel is bound by them (measured: 145 of a wave's 208 us at N = 1024).  Instead lane row q4 loads the 16-B chunks
  // 4 g + q4 (g = 0..3; four global_load_dwordx4) and a 4 x 4 transpose between lane rows and vector components --
  // v_permlane16_swap on the register pairs (0,1) (2,3), then v_permlane32_swap on (0,2) (1,3) -- leaves
  // component j of chunk register g = x[row][4 (4 g + j) + q4], i.e. the operand of step s = 4 g + j.
  // (C == 4: one float per lane -- element q4 of the xyz4 row; raw[0][0] carries it, raw[0][1] the row's |p|^2)
  auto load_raw = [&](int row, f32x4* raw) {
    if constexpr (C == 64) {
      const float* rp = xl + (size_t)row * a.ldx + 4 * q4;
#pragma unroll
      for (int g = 0; g < 4; ++g) raw[g] = ld4(rp + 16 * g);
    } else {
      const float* rp = xb + (size_t)row * a.ldx;
      raw[0][0] = rp[q4];
    }
  };
  auto swap16 = [](float& x, float& y) {
    const auto r = __builtin_amdgcn_permlane16_swap(__float_as_int(x), __float_as_int(y), false, false);
    x = __int_as_float(r[0]); y = __int_as_float(r[1]);
  };
  auto swap32 = [](float& x, float& y) {
    const auto r = __builtin_amdgcn_permlane32_swap(__float_as_int(x), __float_as_int(y), false, false);
    x = __int_as_float(r[0]); y = __int_as_float(r[1]);
  };
  auto transpose = [&](const f32x4* raw, float* dst) {   // dst[4 g + j] = operand of MFMA step 4 g + j
    if constexpr (C == 4) {
      dst[0] = q4 == 3 ? -0.5f * raw[0][0] : raw[0][0];  // candidate side: (x, y, z, -|c|^2 / 2)
      return;
    }
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      float r0 = raw[g][0], r1 = raw[g][1], r2 = raw[g][2], r3 = raw[g][3];
      if constexpr (!pre) {
        swap16(r0, r1); swap16(r2, r3);
        swap32(r0, r2); swap32(r1, r3);
      }
      dst[4 * g] = r0; dst[4 * g + 1] = r1; dst[4 * g + 2] = r2; dst[4 * g + 3] = r3;
    }
  };
  float qf[NST];
  {
    f32x4 raw[4];
    load_raw(q, raw);
    transpose(raw, qf);
    if constexpr (C == 4) qf[0] = q4 == 3 ? 1.f : raw[0][0];              // query side: (x, y, z, 1)
  }
  const float sq_q = C == 64 ? sqb[q] : xb[(size_t)q * a.ldx + 3];
  const int ntiles = (a.N + CT - 1) / CT;

  sel.init(lv, reinterpret_cast<int*>(lv + LROWS * 16), lane);
  // (tie_inline 2: the replay's row image is in global scratch, only its query row + block scratch need LDS)
  int* blk_ties = a.tie_inline ? reinterpret_cast<int*>(smem + inline_tie_offset((size_t)W * 2 * LROWS * 16 * 4, (KS > 22 && a.tie_inline == 2) ? 0 : a.N)) : nullptr;
  if (blk_ties) {
    if (threadIdx.x == 0) blk_ties[0] = 0;
    __syncthreads();
  }
  //@probe VCR_PROBE_ACC_DECL;
  // Two candidate tiles per step: their two 17-MFMA chains are independent and issue alternately (a dependent
  // v_mfma_f32_16x16x4_f32 chain leaves 8 of every 40 cycles empty), and the next two tiles' rows are in flight meanwhile.
  float cf[2][NST];
  f32x4 nraw[2][C == 64 ? 4 : 1];
  float csq[2] = {0.f, 0.f}, nsq[2] = {0.f, 0.f};
  auto scan_prologue = [&]() {
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int c = min(u * CT + col, a.N - 1);
      load_raw(c, nraw[u]);
      if constexpr (C == 64) csq[u] = sqb[c];
    }
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      transpose(nraw[u], cf[u]);                         // (VALU consumers: the first tiles have arrived before the loop)
      asm volatile("" : "+v"(csq[u]));
    }
  };
  // the selection proper for one tile: 16 new distances per query (4 per lane: candidate rows 4 q4 + r)
  auto select_tile = [&](int tile, const f32x4& acc) {
    sel.make_room();
    //@probe VCR_PROBE_ACC(2);
    const int jbase = tile * CT + 4 * q4;
    float dd[4];
    unsigned m = 0;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      dd[r] = fmaf(2.f, acc[r], -sq_q);                  // (-sq_j + 2 dot) - sq_i: 2 x is exact, so one fma rounds like mul + sub
      m |= (dd[r] > sel.thr && jbase + r < a.N) ? (1u << r) : 0u;
    }
    // the four lanes of a column append to ONE log, in row order 0, 1, 2, 3: exclusive prefix of their survivor counts
    const int c0 = __popc(m);
    const auto pa = __builtin_amdgcn_permlane16_swap(c0, c0, false, false);      // {even row, odd row} of the pair
    const int pair_total = pa[0] + pa[1];
    const auto pb = __builtin_amdgcn_permlane32_swap(pair_total, pair_total, false, false);   // {rows 0+1, rows 2+3}
    const int pre = ((q4 & 1) ? pa[0] : 0) + ((q4 >> 1) ? pb[0] : 0);
    //@probe VCR_PROBE_ACC(1);                                              // distances + filter + prefix
    if (__any(m != 0)) {
      const int base = sel.cnt + pre;
#pragma unroll
      for (int r = 0; r < 4; ++r) {                      // branch-free: a lane without a survivor in row r writes its trash row
        const int pos = (m & (1u << r)) ? base + __popc(m & ((1u << r) - 1u)) : PEND + q4;
        sel.lv[pos * 16 + col] = dd[r];
        sel.li[pos * 16 + col] = jbase + r;
      }
    }
    sel.cnt += pb[0] + pb[1];
    //@probe VCR_PROBE_ACC(4);                                              // log push
    if (__any(sel.cnt - sel.done > 16)) sel.drain();     // keep the threshold fresh
    //@probe VCR_PROBE_ACC(5);
  };
  auto scan_all = [&]() {
  scan_prologue();
  for (int tile = 0; tile < ntiles; tile += 2) {
    const bool more = tile + 2 < ntiles;
    if (more) {
#pragma unroll
      for (int u = 0; u < 2; ++u) {                      // (a tile beyond the last one re-reads the last row: masked in select_tile)
        const int c = min((tile + 2 + u) * CT + col, a.N - 1);
        load_raw(c, nraw[u]);
        if constexpr (C == 64) nsq[u] = sqb[c];
      }
    }
    f32x4 acc[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
#pragma unroll
    for (int st = 0; st < NST; ++st) {
      acc[0] = mfma16(cf[0][st], qf[st], acc[0]);
      acc[1] = mfma16(cf[1][st], qf[st], acc[1]);
    }
    // 17th k-step: A[cand][k*] = -sq_cand/2 (row 0 of the lanes), B[k*][q] = 1  ->  acc = dot - sq_j/2, rounded once
    // (C == 4: the norm is the 4th k of the one MFMA above)
    if constexpr (C == 64) {
#pragma unroll
      for (int u = 0; u < 2; ++u) acc[u] = mfma16(q4 == 0 ? -0.5f * csq[u] : 0.f, q4 == 0 ? 1.f : 0.f, acc[u]);
    }
    //@probe VCR_PROBE_ACC(0);                                              // prefetch issue + MFMA chains
    select_tile(tile, acc[0]);
    if (tile + 1 < ntiles) select_tile(tile + 1, acc[1]);
    if (more) {
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        transpose(nraw[u], cf[u]);                       // the wait for the prefetch sits HERE
        csq[u] = nsq[u];
        asm volatile("" : "+v"(csq[u]));
      }
    }
    //@probe VCR_PROBE_ACC(3);                                              // wait for the prefetched rows + transpose
  }
  };
  // ---- ORD: the ordered search.  Tiles = 16 consecutive RANKS of the cloud's Morton order (compact in coordinate AND feature
  // space).  (1) the 2 NEAR + 1 tiles around the wave's own rank are scanned: the list then holds a valid lower bound thr of every
  // query's final (k + 2)-th value.  (2) the tiles' centroids go through the same MFMA chain as candidates: s = -|q - c|^2; with
  // the tile's radius rho, no row of the tile can score above -(max(0, |q - c| - rho))^2 -- evaluated with the fp32 rounding of
  // the scores priced in (m: 3e-5 of the norms involved, ~4x the worst case of a 64-term fp32 dot product), so a tile is dropped
  // only when every one of its rows would fail the filter `score > thr` for every query of the wave.  (3) the remaining tiles
  // are scanned like any others.  Visiting order and omissions of entries below the final threshold do not change the kept set.
  [[maybe_unused]] auto ordered_scan_impl = [&](auto) {
    constexpr int NEAR = KNN_ORD_NEAR;
    const int T = ntiles, g = q0 / CT;
    int lo = max(0, g - NEAR), hi = min(T, g + NEAR + 1);
    if (hi - lo < 2 * NEAR + 1) { if (lo == 0) hi = min(T, 2 * NEAR + 1); else lo = max(0, T - (2 * NEAR + 1)); }
    // the two-tile step of scan_all over a tile sequence (next() = the next tile, -1 at the end; wave-uniform); see under ordered_scan
    auto scan_seq = [&](auto&& next) {
      int tA = next(), tB = tA >= 0 ? next() : -1;
      if (tA < 0) return;
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const int c = min((u ? max(tB, 0) : tA) * CT + col, a.N - 1);
        load_raw(c, nraw[u]);
        if constexpr (C == 64) csq[u] = sqb[c];
      }
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        transpose(nraw[u], cf[u]);
        asm volatile("" : "+v"(csq[u]));
      }
      while (tA >= 0) {
        const int nA = next(), nB = nA >= 0 ? next() : -1;
        if (nA >= 0) {
#pragma unroll
          for (int u = 0; u < 2; ++u) {
            const int c = min((u ? max(nB, 0) : nA) * CT + col, a.N - 1);
            load_raw(c, nraw[u]);
            if constexpr (C == 64) nsq[u] = sqb[c];
          }
        }
        f32x4 acc[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
#pragma unroll
        for (int st = 0; st < NST; ++st) {
          acc[0] = mfma16(cf[0][st], qf[st], acc[0]);
          acc[1] = mfma16(cf[1][st], qf[st], acc[1]);
        }
        if constexpr (C == 64) {
#pragma unroll
          for (int u = 0; u < 2; ++u) acc[u] = mfma16(q4 == 0 ? -0.5f * csq[u] : 0.f, q4 == 0 ? 1.f : 0.f, acc[u]);
        }
        select_tile(tA, acc[0]);
        if (tB >= 0) select_tile(tB, acc[1]);
        if (nA >= 0) {
#pragma unroll
          for (int u = 0; u < 2; ++u) {
            transpose(nraw[u], cf[u]);
            csq[u] = nsq[u];
            asm volatile("" : "+v"(csq[u]));
          }
        }
        tA = nA; tB = nB;
      }
    };
    {
      // own tile first, then outwards (g + 1, g - 1, g + 2, ...): along the curve the tiles get closer as the scan approaches
      // the wave's rank -- in rank order every candidate would beat the threshold the previous ones left (a streaming top-k's
      // worst case: the plain loop over ranked rows takes 1.9x its time over unranked ones)
      int i = 0;
      const int gc = min(max(g, lo), hi - 1);
      scan_seq([&]() {
        while (i < 2 * (2 * NEAR + 1) + 2) {
          const int d = (i + 1) >> 1, t = (i & 1) ? gc + d : gc - d;
          ++i;
          if (t >= lo && t < hi && !(d == 0 && (i & 1) == 0)) return t;
        }
        return -1;
      });
    }
    if (hi - lo >= T) return;
    sel.drain();                                         // thr = the (k + 2)-th best of the near candidates, exactly
    constexpr int NEEDW = KNN_ORD_MAX_TILES / 64;                          // tiles still to visit: one bit each (T <= 512)
    unsigned long long need[NEEDW];
#pragma unroll
    for (int i = 0; i < NEEDW; ++i) need[i] = 0ull;
    const float* cen = a.cen + (size_t)b * T * a.ldx;
    const float* crad = a.cen_rad + (size_t)b * T;
    const float* cmax = a.cen_sqmax + (size_t)b * T;
    // (two centroid tiles in flight: fetched one iteration ahead, unconditionally -- past the last one the last again --, so that
    //  the loop is not a chain of exposed memory round trips; 64 x 4096, k = 40: 1846 -> 1795 us)
    struct CenTile { f32x4 raw[C == 64 ? 4 : 1]; float cs, rd[4], mx[4]; };
    auto cfetch = [&](int ct, CenTile& f) {
      const int crow = min(ct * CT + col, T - 1);
      if constexpr (C == 64) {
        const float* rp = cen + (size_t)crow * a.ldx + 4 * q4;
#pragma unroll
        for (int gq = 0; gq < 4; ++gq) f.raw[gq] = ld4(rp + 16 * gq);
        f.cs = a.cen_sq[(size_t)b * T + crow];
      } else {
        f.raw[0][0] = cen[(size_t)crow * a.ldx + q4];
        f.cs = 0.f;
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int tc = min(ct * CT + 4 * q4 + r, T - 1);
        f.rd[r] = crad[tc];
        f.mx[r] = cmax[tc];
      }
    };
    auto ceval = [&](int ct, const CenTile& f) {
      float ccf[NST];
      transpose(f.raw, ccf);
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int st = 0; st < NST; ++st) acc = mfma16(ccf[st], qf[st], acc);
      if constexpr (C == 64) acc = mfma16(q4 == 0 ? -0.5f * f.cs : 0.f, q4 == 0 ? 1.f : 0.f, acc);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int t = ct * CT + 4 * q4 + r;
        const float sc = fmaf(2.f, acc[r], -sq_q);       // -|q - centroid|^2 as the kernel computes scores
        const float m = 3e-5f * (sq_q + f.mx[r]) + 1e-30f;
        const float dl = __builtin_sqrtf(fmaxf(0.f, -sc - m)) * 0.999999f;
        const float lbd = fmaxf(0.f, dl - f.rd[r]);
        const float ub = m - lbd * lbd;                  // no row of tile t scores above ub for this query
        const unsigned long long bal = __builtin_amdgcn_ballot_w64(t < T && !(ub < sel.thr));
#pragma unroll
        for (int qg = 0; qg < 4; ++qg)
          if ((bal >> (16 * qg)) & 0xffffull) {
            const int tt = ct * CT + 4 * qg + r;
            need[tt >> 6] |= 1ull << (tt & 63);
          }
      }
    };
    if constexpr (KS > 22) {
      const int nct = (T + CT - 1) / CT;
      CenTile fa, fb;
      cfetch(0, fa);
      for (int ct = 0; ct < nct; ct += 2) {
        cfetch(min(ct + 1, nct - 1), fb);
        ceval(ct, fa);
        cfetch(min(ct + 2, nct - 1), fa);
        if (ct + 1 < nct) ceval(ct + 1, fb);
      }
    } else {
      // (k <= 20: ONE centroid tile at a time -- the second one in flight costs 25 registers, and with them the fourth
      //  workgroup per CU; the lists of 22 are what makes 128 registers possible at all)
      const int nct = (T + CT - 1) / CT;
      CenTile fa;
      for (int ct = 0; ct < nct; ++ct) {
        cfetch(ct, fa);
        ceval(ct, fa);
      }
    }
    for (int t = lo; t < hi; ++t) need[t >> 6] &= ~(1ull << (t & 63));
    {
      // (ascending rank order; nearest-first on either side of the near range measured 10-14 % slower: the two tiles of a step
      // then lie far apart and the scalar bookkeeping per step grows)
      int w = 0;
      unsigned long long cur = need[0];
      scan_seq([&]() {
        while (cur == 0ull && w < NEEDW - 1) cur = need[++w];
        if (cur == 0ull) return -1;
        const int bit = __builtin_ctzll(cur);
        cur &= cur - 1ull;
        return w * 64 + bit;
      });
    }
  };
  // (a generic lambda behind a wrapper, as the code was measured: a plain one is the same search but changes the ORD kernels' register
  // allocation)
  // (The two-tile step stays written out in scan_prologue + scan_all, in scan_seq and, the single chain, in ceval: stated once as
  // fetch2 / take2 / chains it changed the code of the six knn64c_kernel, the four 16-query and the two ordered knn_pair_kernel
  // instantiations (equal resources; s_nop / s_waitcnt moved, the ordered ones -8 / -6 s_waitcnt and a branch less), and their timing
  // against the parent was not measured.  A fix to the prefetch or the norm step goes into all three places.  NOTES.md, round 6.)
  [[maybe_unused]] auto ordered_scan = [&]() { ordered_scan_impl(std::false_type{}); };
  // C == 4: filter floor from a sample (see SampleNet): the first 256 candidates' values only -- 16 MFMAs -- give a
  // threshold the scan proper starts with (the VALU kernel: 75 -> 65 us; distances are one MFMA per tile here, so the
  // pre-pass costs next to nothing.  C == 64 recomputes 17 MFMAs per sampled tile: measured a wash, off).
  if constexpr (C == 4) {
    constexpr int T0 = SAMPLE / CT, R0 = (KS + 1 + G::LPQ - 1) / G::LPQ;     // LPQ * R0 - 1 >= KS
    if (!ord && ntiles >= 2 * T0 + 1) {
      SampleNet<R0> net;
      net.init();
      for (int t = 0; t < T0; ++t) {                     // (full tiles: 16 T0 <= N)
        const float cv = xb[(size_t)(t * CT + col) * a.ldx + q4];
        const f32x4 acc = mfma16(q4 == 3 ? -0.5f * cv : cv, qf[0], f32x4{0.f, 0.f, 0.f, 0.f});
#pragma unroll
        for (int r = 0; r < 4; ++r) net.insert(fmaf(2.f, acc[r], -sq_q));
      }
      sel.init(lv, reinterpret_cast<int*>(lv + LROWS * 16), lane, col_min<G>(net.s[R0 - 1], sel.sg));
    }
  }
  if constexpr (ORD) {
    if (!ord) scan_all();
    else ordered_scan();
  } else {
    scan_all();
  }
  if constexpr (C == 4) {
    sel.drain();
    if (!ord && __any(!sel.floor_held())) {                      // the sample misjudged some query of this wave: scan without a floor
      sel.init(lv, reinterpret_cast<int*>(lv + LROWS * 16), lane);
      scan_all();
    }
  }
  //@probe VCR_PROBE_ACC_FLUSH(threadIdx.x == 0 && blockIdx.y == 0, blockIdx.x);
  finish<G, KS, 1>(sel, a, b, q0 + col, wave, 0, smem, blk_ties, ord ? a.perm + (size_t)b * a.N : nullptr);
  if (blk_ties) {
    // (the slot form exists in the k > 20 kernels only: they run three workgroups per CU and have the registers for it; with it
    //  the k <= 20 kernels, held to 128 registers for their fourth workgroup, spill 32 of them -- 124 -> 142 us at configs[1])
    unsigned char* gwork = nullptr;
    if constexpr (KS > 22) {
      if (a.tie_inline == 2)                               // this workgroup's slot: (cloud, query block) in launch-independent order
        gwork = reinterpret_cast<unsigned char*>(a.tie_work) + ((size_t)b * ((a.N + 16 * W - 1) / (16 * W)) + bx) * 16 * (size_t)a.N;
    }
    replay_block_ties(a, blk_ties, smem, gwork);
  }
}
// (k > 20: the logs of a workgroup take 51 KB, so three workgroups share a CU whatever the registers allow -- the bound
//  says so and the lists of 42 keep their registers: at four waves per SIMD, 128 VGPRs, two spilled to scratch)
template <int KS, int W, bool XT>
__global__ __launch_bounds__(64 * W, (KS > 22 ? 3 : 4)) void knn64c_kernel(vcr_knn_args a) {
  int bx, b;
  xcd_chunk2(bx, b);
  knn64c_body<KS, W, 64, XT>(a, bx, b);
}
// the Cartesian search on the same body (distances = one MFMA per tile): the unsplit (S = 1) kernel of C == 4
template <int KS, int W>
__global__ __launch_bounds__(64 * W, (KS > 22 ? 3 : 4)) void knn3c_kernel(vcr_knn_args a) {
  int bx, b;
  xcd_chunk2(bx, b);
  knn64c_body<KS, W, 4>(a, bx, b);
}

// ---------------------------------------------------------------- C == 4 (xyz4, VALU)
// Wave = 16 queries x 4 lanes (DPP quad = query); lane s of the quad computes the distances of candidates j = 4u + s.
// S waves of a workgroup may split the candidates of a query group (small grids, k <= 20).
template <int KS, int S>
__device__ __forceinline__ void knn3_body(const vcr_knn_args& a, int bx, int b) {
  using G = GeomQuad;
  constexpr int PEND = pend_of<G, KS>();
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int s = lane & 3, qd = lane >> 2;
  const int grp = wave / S, part = wave % S;
  const int q0 = (bx * (4 / S) + grp) * 16;
  float* lv = reinterpret_cast<float*>(smem) + wave * (2 * (PEND + 1) * 16);
  Selector<G, KS> sel;
  const float* xb = a.x + (size_t)b * a.N * a.ldx;
  const int qi = q0 + qd;
  const f32x4 qv = ld4(xb + (size_t)min(qi, a.N - 1) * a.ldx);
  // 16 candidates per step, 4 per lane: j = j0 + 4u + s (the quad reads 64 contiguous bytes per load); the next
  // step's rows are in flight while this one is filtered
  const int nsteps = (a.N + 15) / 16;
  //@probe VCR_PROBE_ACC_DECL;
  auto scan_steps = [&](int s0, int s1, auto&& body) {
    f32x4 c[4], cn[4];
    auto load = [&](f32x4* dst, int st) {
#pragma unroll
      for (int u = 0; u < 4; ++u) dst[u] = ld4(xb + (size_t)min(st * 16 + 4 * u + s, a.N - 1) * a.ldx);
    };
    if (s0 < s1) load(c, s0);
    int it = 0;
    for (int st = s0; st < s1; st += S, ++it) {
      if (st + S < s1) load(cn, st + S);
      float dd[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const float dot = fmaf(qv[2], c[u][2], fmaf(qv[1], c[u][1], qv[0] * c[u][0]));
        dd[u] = (2.f * dot - c[u][3]) - qv[3];
      }
      body(st, it, dd);
#pragma unroll
      for (int u = 0; u < 4; ++u) c[u] = cn[u];
    }
  };
  auto select_body = [&](int st, int it, const float (&dd)[4]) {
    const int j0 = st * 16;
    sel.make_room();
    unsigned m = 0;
#pragma unroll
    for (int u = 0; u < 4; ++u) m |= (dd[u] > sel.thr && j0 + 4 * u + s < a.N) ? (1u << u) : 0u;
    //@probe VCR_PROBE_ACC(0);                                              // distances + filter
    // the quad appends to ONE log: exclusive prefix of the lanes' survivor counts
    const int c0 = __popc(m);
    const int p1 = __builtin_amdgcn_mov_dpp(c0, 0x90, 0xF, 0xF, true);     // lane s <- lane s-1 (lane 0: itself)
    int inc = c0 + (s >= 1 ? p1 : 0);
    const int p2 = __builtin_amdgcn_mov_dpp(inc, 0x44, 0xF, 0xF, true);    // lane s <- lane s-2 (lanes 0, 1: themselves)
    inc += s >= 2 ? p2 : 0;
    const int total = G::from_seg(inc, 3);
    if (__any(m != 0)) {
      const int base = sel.cnt + inc - c0;
#pragma unroll
      for (int u = 0; u < 4; ++u) {                      // branch-free: lanes without a survivor write the trash row
        const int pos = (m & (1u << u)) ? base + __popc(m & ((1u << u) - 1u)) : PEND;
        sel.lv[pos * 16 + qd] = dd[u];
        sel.li[pos * 16 + qd] = j0 + 4 * u + s;
      }
    }
    sel.cnt += total;
    if ((it < 3 && !(sel.thr0 > VCR_NEG_INF)) || __any(sel.cnt - sel.done > 12)) sel.drain();   // no floor: settle the threshold quickly
    //@probe VCR_PROBE_ACC(1);                                              // log + drains
  };
  constexpr int ST0 = SAMPLE / 16, R0 = (KS + 1 + G::LPQ - 1) / G::LPQ;    // LPQ * R0 - 1 >= KS
  const int my_steps = part < nsteps ? (nsteps - part + S - 1) / S : 0;
  float floor0 = VCR_NEG_INF;
  if (my_steps >= 2 * ST0 + 1) {
    SampleNet<R0> net;
    net.init();
    scan_steps(part, part + S * ST0, [&](int, int, const float (&dd)[4]) {
#pragma unroll
      for (int u = 0; u < 4; ++u) net.insert(dd[u]);
    });
    floor0 = col_min<G>(net.s[R0 - 1], s);
  }
  int* blk_ties = (S == 1 && a.tie_inline) ? reinterpret_cast<int*>(smem + inline_tie_offset((size_t)4 * 2 * (PEND + 1) * 16 * 4, a.N)) : nullptr;
  if (blk_ties) {
    if (threadIdx.x == 0) blk_ties[0] = 0;
    __syncthreads();
  }
  sel.init(lv, reinterpret_cast<int*>(lv + (PEND + 1) * 16), lane, floor0);
  scan_steps(part, nsteps, select_body);
  sel.drain();
  if (__any(!sel.floor_held())) {
    sel.init(lv, reinterpret_cast<int*>(lv + (PEND + 1) * 16), lane);
    scan_steps(part, nsteps, select_body);
  }
  //@probe VCR_PROBE_ACC_FLUSH(threadIdx.x == 0 && blockIdx.y == 0, blockIdx.x);
  finish<G, KS, S>(sel, a, b, qi, wave, part, smem, blk_ties);
  if (blk_ties) replay_block_ties(a, blk_ties, smem);
}
template <int KS, int S>
__global__ __launch_bounds__(256, 2) void knn3_kernel(vcr_knn_args a) {
  int bx, b;
  xcd_chunk2(bx, b);
  knn3_body<KS, S>(a, bx, b);
}

// Both kNN graphs of an LPDNet pass in ONE launch (lpdnet_model.py:113,129 -- the feature-space and the Cartesian search
// are independent): the first n64 workgroups run the MFMA kernel's body, the rest the Cartesian one.  Either kernel
// alone is latency-bound at one wave per SIMD (1024 waves on 1024 SIMDs); launched together the second fills the
// first one's idle issue slots, and the pair costs little more than the longer of the two.
template <int KS, bool COL16, bool XT = false, bool ORD = false>
__global__ __launch_bounds__(256, (COL16 ? (KS > 22 || ORD ? 3 : 4) : 2)) void knn_pair_kernel(vcr_knn_args a64, vcr_knn_args a3, int n64, int gx64, int gx3) {
  const int bid = (int)blockIdx.x;
  if (bid < n64) {
    const int lin = xcd_chunk(bid, n64);
    if constexpr (COL16) knn64c_body<KS, 4, 64, XT, ORD>(a64, lin % gx64, lin / gx64);
    else knn64_body<KS, 1, 4>(a64, lin % gx64, lin / gx64);
  } else {
    const int lin = xcd_chunk(bid - n64, (int)gridDim.x - n64);
    knn64c_body<KS, 4, 4, false, ORD>(a3, lin % gx3, lin / gx3);
  }
}

// The same for SMALL grids (a few pairs per call), where both searches run their candidate-split kernels (S64 / S3 waves
// share a group of queries): launched one after the other each is a latency-bound handful of workgroups (63 + 44 us at one
// pair); together they take as long as the longer one.
template <int KS, int S64, int S3>
__global__ __launch_bounds__(256, 2) void knn_pair_small_kernel(vcr_knn_args a64, vcr_knn_args a3, int n64, int gx64, int gx3) {
  const int bid = (int)blockIdx.x;
  if (bid < n64) {
    const int lin = xcd_chunk(bid, n64);
    knn64_body<KS, S64, 4>(a64, lin % gx64, lin / gx64);
  } else {
    const int lin = xcd_chunk(bid - n64, (int)gridDim.x - n64);
    if constexpr (S3 == 1) knn64c_body<KS, 4, 4>(a3, lin % gx3, lin / gx3);   // (unsplit: the MFMA body, as vcr_knn_f32 launches it)
    else knn3_body<KS, S3>(a3, lin % gx3, lin / gx3);
  }
}

}  // namespace

// the tie counter is zeroed by a kernel, not hipMemsetAsync: a memset NODE in a captured HIP graph made replays on the
// default stream hang on this ROCm build (see forward.hip)
__global__ void zero_count_kernel(int32_t* p) { *p = 0; }
static int zero_count(int32_t* p, hipStream_t s) {
  hipLaunchKernelGGL(zero_count_kernel, dim3(1), dim3(1), 0, s, p);
  return VCR_LAUNCH_RC();
}

// LDS of a replay launch: the row image when it fits, else only the query row + block scratch (the image is in tie_work)
static size_t tiebreak_launch_lds(int N) { return tiebreak_lds(N) <= TB_LDS_MAX ? tiebreak_lds(N) : tiebreak_lds(0); }
extern "C" size_t vcr_knn_tie_work_bytes(int N) {
  return (N > 0 && tiebreak_lds(N) > TB_LDS_MAX) ? (size_t)TB_BLOCKS * 16 * (size_t)N : 0;
}
// one 16 N-byte slot per workgroup of the 16-query-wave kernels (64 queries each): with this much tie_work a launch whose rows
// (or lists: k > 20) leave no room for an LDS image replays its tied rows itself (tie_inline 2)
extern "C" size_t vcr_knn_tie_slot_bytes(int B, int N) {
  return (B > 0 && N > 0) ? (size_t)B * ((N + 63) / 64) * 16 * (size_t)N : 0;
}
// the part of vcr_knn_args every caller must pass: through tie_cap (everything behind it is optional, zero = automatic)
static int knn_take(const vcr_knn_args* user, vcr_knn_args* mine) {
  return vcr_take_args(user, mine, offsetof(vcr_knn_args, waves));
}

// Which feature-space kernel: 16-query waves on 16x16x4 MFMAs (knn64c_body) or 32-query waves on 32x32x2 (knn64_body).
// vcr_knn_args.waves: 8 forces the former; 1 / 2 / 4 the latter with that candidate split; 0 = the half-size waves as soon
// as there are 1024 groups of 16 queries (a wave for every SIMD), by measurement on MI355X (profiles/rounds1-3/r3i_bench_knn.txt;
// 16- vs 32-query waves): one-launch pair 32 clouds x 1024: 148 vs 176 us inside the forward; pair 32 x 2048: 452 vs 477;
// 64 x 4096, k = 40: 2.39 vs 2.92 ms; alone they are level at k = 20 (32 x 1024: 112 vs 123 us, 32 x 2048: 315 vs 303).
// Smaller grids keep the 32-query kernels, whose S = 2 / 4 waves split the candidates of a query group.  Results are
// identical either way (same k-ascending fma chain, same selection).
static bool use_col16(const vcr_knn_args* a) {
  if (a->waves == 8 || a->k > 40) return true;           // (k = 41 .. 62: lists of 64, built for the 16-query bodies only)
  if (a->waves != 0) return false;
  return (long)((a->N + 15) / 16) * a->B >= 1024;
}
// Candidate split S of the 32-query and Cartesian kernels: S waves of a workgroup share one group of queries and split its
// candidates.  The selection work grows with the number of lists (S per query), and measured on MI355X a second wave per SIMD
// bought with S = 2 only breaks even, so S stays 1 as soon as that gives every SIMD (1024 of them) one wave; smaller grids
// split to fill the chip.  (the fold of S > 1 waves parks the value lists behind the logs: there is room for that with k <= 20 only)
static int knn_s(const vcr_knn_args* a) {
  if (a->k > 20) return 1;
  if (a->waves == 1 || a->waves == 2 || a->waves == 4) return a->waves;
  const long groups = (long)((a->N + (a->C == 64 ? 31 : 15)) / (a->C == 64 ? 32 : 16)) * a->B;
  return groups >= 1024 ? 1 : groups >= 512 ? 2 : 4;
}
// the ordered search's inputs are all there and the cloud is small enough for the wave's tile mask (256 tiles of 16 ranks)
// (vcr_knn_order_f32 writes the ranked rows and the centroids at pitch C: a padded x keeps the plain scan)
static bool knn_ordered(const vcr_knn_args* a) {
  return a->perm && a->xp && a->cen && a->cen_rad && a->cen_sqmax && (a->C == 4 || (a->sqp && a->cen_sq)) && a->N <= 16 * KNN_ORD_MAX_TILES &&
         a->ldx == a->C &&
         !(((uintptr_t)a->xp | (uintptr_t)a->cen) & 15);
}

namespace {
// How one search runs.  knn_plan() decides it from the search's arguments, and it is the only place that does: every entry
// point below launches what the plans of its searches say.
enum class KnnBody {
  none,      // the arguments name no form (waves or C out of range)
  mfma32,    // knn64_body (C == 64): 32-query waves on 32x32x2 MFMAs, S waves splitting a query group's candidates
  col16,     // knn64c_body: 16-query waves on 16x16x4 MFMAs, four unsplit waves (C == 64: knn64c_kernel, C == 4: knn3c_kernel)
  quad,      // knn3_body (C == 4, S = 2 / 4): DPP quads on the VALU, 16 queries a wave
};
struct KnnPlan {
  vcr_knn_args a;            // what the kernels get: the caller's arguments with tie_inline set, perm cleared unless ord
  KnnBody body;
  int KS, S;                 // value lists of k + 2 entries rounded up to 22 / 42 / 64; waves sharing one group of queries
  bool xt, ord;              // the 16-query feature-space waves read xt; the ordered inputs are complete (knn_ordered)
  long groups;               // groups of queries of the form's wave size, all clouds: what the form was chosen by
  dim3 grid, block; size_t lds;
  bool zero, replay;         // the tie counter is zeroed first; a replay launch follows the search (owed, not deferred)
};
}  // namespace

// Returns the first thing wrong with the arguments (VCR_OK: none).  The form is chosen even for invalid arguments when waves and
// C name one: vcr_knn_pair_f32 decides between one launch and two before it reports which search is at fault.
static int knn_plan(const vcr_knn_args& a, KnnPlan* p) {
  *p = KnnPlan{a};
  const bool waves_ok = a.waves == 0 || a.waves == 1 || a.waves == 2 || a.waves == 4 || a.waves == 8, c_ok = a.C == 64 || a.C == 4;
  int e = VCR_OK;
  if (!a.x || !a.idx || a.B <= 0 || a.N <= 0 || a.k <= 0 || a.k + 1 > a.N) e = VCR_EINVAL;
  else if (a.k > 62 || a.N > KNN_MAX_N || knn_rows_overflow(&a)) e = VCR_EUNSUPPORTED;   // limits of this library (see vcr_hip.h)
  else if (!waves_ok) e = VCR_EINVAL;
  else if (!c_ok) e = VCR_EUNSUPPORTED;
  if (!waves_ok || !c_ok) return e;
  const bool k20 = a.k <= 20;
  p->KS = k20 ? 22 : a.k <= 40 ? 42 : 64;               // one entry more than topk(k + 1): exposes boundary ties
  const bool c16 = a.C == 64 && use_col16(&a);
  p->S = c16 ? 1 : knn_s(&a);
  p->body = c16 || (a.C == 4 && p->S == 1) ? KnnBody::col16 : a.C == 64 ? KnnBody::mfma32 : KnnBody::quad;
  const int W = p->body == KnnBody::mfma32 && !k20 ? 2 : 4, QW = p->body == KnnBody::mfma32 ? 32 : 16;   // waves x queries
  const long QB = (long)QW * (W / p->S);                 // queries of a workgroup
  p->grid = dim3((unsigned)(((long)a.N + QB - 1) / QB), (unsigned)a.B);
  p->block = dim3(64 * W);
  p->groups = ((long)a.N + QW - 1) / QW * a.B;
  p->xt = p->body == KnnBody::col16 && a.C == 64 && a.xt;
  p->ord = knn_ordered(&a);
  if (!p->ord) p->a.perm = nullptr;                      // (incomplete ordered inputs: the search runs the plain way)
  // In-launch tie replay (col16 only: workgroups of four waves of 16 queries, see replay_block_ties).  0: the tied rows go to a
  // replay launch.  1: replayed by the workgroup that found them, row image in its LDS beside nothing else in <= 40 KB (N <= ~2400).
  // 2 (k > 20): likewise, row image in the workgroup's slot of tie_work (the caller gave vcr_knn_tie_slot_bytes(B, N) bytes of it;
  // the slot form is compiled into the k > 20 kernels only).
  int inl = 0;
  if (p->body == KnnBody::col16) {
    const size_t log = (size_t)4 * 2 * ((k20 ? pend_of<GeomCol16, 22>() : pend_of<GeomCol16, 42>()) + 4) * 16 * 4;   // the four logs
    const size_t slots = vcr_knn_tie_slot_bytes(a.B, a.N);
    if (a.tie_scratch && inline_tie_offset(log, a.N) + (1 + BLK_TIES) * 4 <= INLINE_TIE_MAX_LDS) inl = 1;
    else if (a.tie_scratch && !k20 && slots && a.tie_work && a.tie_work_bytes >= slots && !((uintptr_t)a.tie_work & 15)) inl = 2;
    p->lds = inl ? inline_tie_offset(log, inl == 2 ? 0 : a.N) + (1 + BLK_TIES) * 4 : log;
  } else if (p->body == KnnBody::mfma32) {
    p->lds = (size_t)W * 2 * ((k20 ? pend_of<GeomMfma, 22>() : pend_of<GeomMfma, 42>()) + 1) * 32 * 4;
  } else {
    p->lds = (size_t)4 * 2 * (pend_of<GeomQuad, 22>() + 1) * 16 * 4;   // (S > 1: k <= 20)
  }
  p->a.tie_inline = inl;
  p->zero = a.tie_scratch && !a.tie_zeroed;
  p->replay = a.tie_scratch && !a.tie_defer && !inl;
  if (e) return e;
  if ((a.C == 64 ? (!a.sq || a.ldx < 64 || (a.ldx & 3)) : (a.ldx < 4 || (a.ldx & 3))) || (a.tie_scratch && a.tie_cap < 1)) return VCR_EINVAL;
  // a replay is owed (now or deferred) but the rows need global scratch that the caller did not provide: refuse loudly rather
  // than skip the replay silently
  const size_t need = vcr_knn_tie_work_bytes(a.N);
  if (a.tie_scratch && inl != 2 && need && (!a.tie_work || a.tie_work_bytes < need || ((uintptr_t)a.tie_work & 15))) return VCR_EUNSUPPORTED;
  return VCR_OK;
}

static int zero_ties(const KnnPlan& p, hipStream_t s) { return p.zero ? zero_count(p.a.tie_scratch, s) : VCR_OK; }
// rows with an exact tie at the (k+1)-th value: replay libstdc++'s selection on them (knn_tiebreak_kernel); b: a second search or NULL
static int replay(const vcr_knn_args& a, const vcr_knn_args* b, hipStream_t s) {
  const size_t la = tiebreak_launch_lds(a.N), lb = b ? tiebreak_launch_lds(b->N) : 0, lds = la > lb ? la : lb;
  if (b) return vcr_launch<knn_tiebreak2_kernel>(dim3(TB_BLOCKS, 2), dim3(256), lds, s, a, *b);
  return vcr_launch<knn_tiebreak_kernel>(dim3(TB_BLOCKS), dim3(256), lds, s, a);
}

// one search: zero the tie counter, search, replay
static int knn_run(const KnnPlan& p, hipStream_t s) {
  int rc = zero_ties(p, s);
  if (rc) return rc;
#define VCR_K(...) rc = vcr_launch<__VA_ARGS__>(p.grid, p.block, p.lds, s, p.a)
  if (p.body == KnnBody::col16 && p.a.C == 4) { if (p.KS == 22) VCR_K(knn3c_kernel<22, 4>); else if (p.KS == 42) VCR_K(knn3c_kernel<42, 4>); else VCR_K(knn3c_kernel<64, 4>); }
  else if (p.body == KnnBody::col16 && p.xt) { if (p.KS == 22) VCR_K(knn64c_kernel<22, 4, true>); else if (p.KS == 42) VCR_K(knn64c_kernel<42, 4, true>); else VCR_K(knn64c_kernel<64, 4, true>); }
  else if (p.body == KnnBody::col16) { if (p.KS == 22) VCR_K(knn64c_kernel<22, 4, false>); else if (p.KS == 42) VCR_K(knn64c_kernel<42, 4, false>); else VCR_K(knn64c_kernel<64, 4, false>); }
  else if (p.body == KnnBody::mfma32) { if (p.KS == 42) VCR_K(knn64_kernel<42, 1, 2>); else if (p.S == 1) VCR_K(knn64_kernel<22, 1, 4>); else if (p.S == 2) VCR_K(knn64_kernel<22, 2, 4>); else VCR_K(knn64_kernel<22, 4, 4>); }
  else if (p.S == 2) VCR_K(knn3_kernel<22, 2>);
  else VCR_K(knn3_kernel<22, 4>);
#undef VCR_K
  return rc ? rc : p.replay ? replay(p.a, nullptr, s) : VCR_OK;
}

extern "C" int vcr_knn_f32(const vcr_knn_args* ua, vcr_stream_t stream) {
  vcr_knn_args a;
  if (knn_take(ua, &a)) return VCR_EINVAL;
  vcr_stream_scope scope_(stream);
  KnnPlan p;
  const int e = knn_plan(a, &p);
  return e ? e : knn_run(p, (hipStream_t)stream);
}

extern "C" int vcr_knn_ties_inline(const vcr_knn_args* ua) {
  vcr_knn_args a;
  KnnPlan p;
  return (knn_take(ua, &a) == 0 && knn_plan(a, &p) == VCR_OK && p.a.tie_inline) ? 1 : 0;
}

extern "C" int vcr_knn_ties_f32(const vcr_knn_args* ua, const vcr_knn_args* ub, vcr_stream_t stream) {
  vcr_knn_args a, b;
  if (knn_take(ua, &a) || (ub && knn_take(ub, &b))) return VCR_EINVAL;
  vcr_stream_scope scope_(stream);
  KnnPlan pa, pb;
  int e = knn_plan(a, &pa);
  if (!e && ub) e = knn_plan(b, &pb);
  if (e) return e;
  if (!a.tie_scratch || (ub && !b.tie_scratch)) return VCR_EINVAL;
  return replay(pa.a, ub ? &pb.a : nullptr, (hipStream_t)stream);
}

// Feature-space (a64: C == 64) and Cartesian (a3: C == 4) kNN of the same pass as ONE launch, decided on their standalone plans,
// when both have the same k, the automatic Cartesian form (a3.waves == 0) and the same tie handling (tie_scratch or not, tie_defer):
// fused (knn_pair_kernel) when both plans are unsplit four-wave forms with lists of 22 / 42 and >= 1024 query groups each (the
// regime of the path; with 16-query waves the one form that reads the ordered inputs), small (knn_pair_small_kernel) when the
// arguments are valid and the feature-space search splits its candidates by its own choice (small grids).  Anything else: the two
// vcr_knn_f32 calls.  A replay that is not deferred serves both searches at once.
enum class PairForm { separate, fused, small };
static PairForm pair_form(const KnnPlan& p64, const KnnPlan& p3, bool valid) {
  const vcr_knn_args &a64 = p64.a, &a3 = p3.a;
  if (a64.k != a3.k || a3.waves != 0 || (a64.tie_scratch != nullptr) != (a3.tie_scratch != nullptr) || a64.tie_defer != a3.tie_defer)
    return PairForm::separate;
  auto unsplit4 = [](const KnnPlan& p) { return p.body == KnnBody::col16 || (p.body == KnnBody::mfma32 && p.S == 1 && p.block.x == 256); };
  if (unsplit4(p64) && unsplit4(p3) && p64.KS <= 42 && p64.groups >= 1024 && p3.groups >= 1024) return PairForm::fused;
  if (valid && a64.waves == 0 && p64.body == KnnBody::mfma32 && p64.S > 1) return PairForm::small;
  return PairForm::separate;
}
// both plans, and the pair's own requirement: which search is which
static int pair_plans(const vcr_knn_args& a64, const vcr_knn_args& a3, KnnPlan* p64, KnnPlan* p3, int* e64, int* e3) {
  if (!a64.x || !a3.x || !a64.idx || !a3.idx || a64.C != 64 || a3.C != 4) return VCR_EINVAL;
  *e64 = knn_plan(a64, p64);
  *e3 = knn_plan(a3, p3);
  return VCR_OK;
}

extern "C" int vcr_knn_pair_f32(const vcr_knn_args* u64, const vcr_knn_args* u3, vcr_stream_t stream) {
  vcr_knn_args a64, a3;
  if (knn_take(u64, &a64) || knn_take(u3, &a3)) return VCR_EINVAL;
  vcr_stream_scope scope_(stream);
  KnnPlan p64, p3;
  int e64 = VCR_OK, e3 = VCR_OK;
  if (pair_plans(a64, a3, &p64, &p3, &e64, &e3)) return VCR_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  const PairForm form = pair_form(p64, p3, !e64 && !e3);
  if (form == PairForm::separate) {
    const int rc = e3 ? e3 : knn_run(p3, s);
    return rc ? rc : e64 ? e64 : knn_run(p64, s);
  }
  if (e64 || e3) return e64 ? e64 : e3;
  int rc = zero_ties(p64, s);
  if (!rc) rc = zero_ties(p3, s);
  if (rc) return rc;
  const int gx64 = (int)p64.grid.x, gx3 = (int)p3.grid.x, n64 = gx64 * a64.B;
  const dim3 grid(n64 + gx3 * a3.B), block(256);
  const size_t lds = p64.lds > p3.lds ? p64.lds : p3.lds;
  const vcr_knn_args &k64 = p64.a, &k3 = p3.a;
#define VCR_KP(...) rc = vcr_launch<__VA_ARGS__>(grid, block, lds, s, k64, k3, n64, gx64, gx3)
  if (form == PairForm::small) {
    if (p64.S == 4) { if (p3.S == 4) VCR_KP(knn_pair_small_kernel<22, 4, 4>); else if (p3.S == 2) VCR_KP(knn_pair_small_kernel<22, 4, 2>); else VCR_KP(knn_pair_small_kernel<22, 4, 1>); }
    else { if (p3.S == 4) VCR_KP(knn_pair_small_kernel<22, 2, 4>); else if (p3.S == 2) VCR_KP(knn_pair_small_kernel<22, 2, 2>); else VCR_KP(knn_pair_small_kernel<22, 2, 1>); }
  } else if (p64.body == KnnBody::mfma32) {
    VCR_KP(knn_pair_kernel<22, false>);
  } else if ((p64.ord || p3.ord) && p64.xt) {            // searches over the ranked rows (see vcr_knn_args.perm)
    if (p64.KS == 22) VCR_KP(knn_pair_kernel<22, true, true, true>); else VCR_KP(knn_pair_kernel<42, true, true, true>);
  } else if (p64.KS == 22) {
    if (p64.xt) VCR_KP(knn_pair_kernel<22, true, true>); else VCR_KP(knn_pair_kernel<22, true>);
  } else {
    if (p64.xt) VCR_KP(knn_pair_kernel<42, true, true>); else VCR_KP(knn_pair_kernel<42, true>);
  }
#undef VCR_KP
  // whatever was not replayed inside the launch: one replay launch, now or (tie_defer) when the caller asks for it
  if (rc || !(p64.replay || p3.replay)) return rc;
  return p64.replay ? replay(p64.a, p3.replay ? &p3.a : nullptr, s) : replay(p3.a, nullptr, s);
}

// Host-only, library-internal (forward.hip): what the plans say of one search (b == NULL, as vcr_knn_f32 runs it) or of a pair (a64, a3
// as vcr_knn_pair_f32 runs them).  ordered: the pair takes the one form that reads the ordered inputs (which do not change the form);
// inline_a / inline_b: that search replays its tied rows inside its launch.
extern "C" int vcr_knn_forms_(const vcr_knn_args* ua, const vcr_knn_args* ub, int* ordered, int* inline_a, int* inline_b) {
  vcr_knn_args a, b;
  if (knn_take(ua, &a) || (ub && knn_take(ub, &b))) return VCR_EINVAL;
  KnnPlan pa, pb;
  int ea = VCR_OK, eb = VCR_OK;
  if (!ub) ea = knn_plan(a, &pa);
  else if (pair_plans(a, b, &pa, &pb, &ea, &eb)) return VCR_EINVAL;
  if (ea || eb) return ea ? ea : eb;
  if (ordered) *ordered = ub && pair_form(pa, pb, true) == PairForm::fused && pa.body == KnnBody::col16 && pa.xt;
  if (inline_a) *inline_a = pa.a.tie_inline != 0;
  if (inline_b) *inline_b = ub && pb.a.tie_inline != 0;
  return VCR_OK;
}

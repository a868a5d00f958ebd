// The nearest neighbour across two clouds in the 33-d feature space (include/vcr_hip_match.h): for every
// column of a [B,33,Ns] its nearest column of b [B,33,Nt] by brute force in the DIFFERENCE form, one fmaf chain over the 33
// channels in ascending order (build.py: -ffp-contract=off, every fmaf is spelled out):
//   d_c = a_c - b_c;  acc = d_0 * d_0;  acc = fmaf(d_c, d_c, acc), c = 1 .. 32;  best only on acc < best, from (+inf, -1)
// so a tie goes to the lowest index and a NaN / +inf distance never wins: the comparison is the whole non-finite rule.
//
//   featnn_rows_kernel      one lane per column of the SEARCHED side: the 33 channel values, strided by N in [B,33,N], become
//                           one contiguous row of 36 floats (the last three zero, never read by the chain) in the workspace.
//   featnn_scan_kernel<Q>   256 lanes x Q columns of the searching side per lane, their 33 values in registers (read from the
//                           channels-first planes: consecutive lanes, consecutive addresses), against one of the S segments of
//                           the searched side.  The candidate row's address is the same for every lane of the workgroup
//                           (blockIdx and the loop counter alone), so the row arrives through SCALAR loads and the chain's
//                           subtraction takes it as its scalar operand: two vector instructions a channel and query, no LDS, no
//                           barrier -- section 4.8's scan, fed through LDS broadcasts, runs at the LDS's read rate (section 8),
//                           and here a candidate is 33 values, not 3.  Two candidates are in flight per trip.
//   featnn_merge_kernel     one lane per column: folds the S candidates in ascending segment order with the same strict <
//                           (segments ascend in index: the lowest-index rule survives the split) and writes index and d2.
//   featnn_mutual_kernel    one lane per column of a: nn_idx[i] = j stays iff rev[j] == i.
// The reverse direction (rev_idx, mutual) is the same three launches with the roles exchanged.  The merge's geometry depends on
// the column count alone, so every form of the scan returns the same bits.  No atomics.
#include "seg_scan.h"
#include "../../include/vcr_hip_match.h"

namespace {

constexpr int FN_BLOCK = 256;
static_assert(FN_BLOCK == WG_BLOCK, "seg_scan.h serves workgroups of this size");
constexpr int FN_C = VCR_FEAT_NN_C;
constexpr int FN_ROW = 36;                                 // floats per transposed row: 144 B, 16-B aligned
constexpr int FN_MAX_N = 131072;
constexpr int FN_MAX_SPLITS = 128;
constexpr int FN_MIN_SEGMENT = 64;                         // the plan cuts no segment shorter than this (a forced split may)
constexpr int FN_FILL_PER_CU = 16;                         // workgroups per CU the plan cuts the work into, where it can
constexpr SegLimits FN_LIMITS{FN_MIN_SEGMENT, FN_FILL_PER_CU, FN_MAX_SPLITS};

struct FnRows { const float* x; float* rows; int N; long total; };      // total = B N

__global__ __launch_bounds__(FN_BLOCK) void featnn_rows_kernel(FnRows p) {
  const long g = (long)blockIdx.x * FN_BLOCK + threadIdx.x;
  if (g >= p.total) return;
  const long b = g / p.N;
  const int n = (int)(g - b * p.N);
  const float* x = p.x + (size_t)b * FN_C * p.N + n;
  float* row = p.rows + (size_t)g * FN_ROW;
#pragma unroll
  for (int c4 = 0; c4 < FN_ROW / 4; ++c4) {
    f32x4 v;
#pragma unroll
    for (int u = 0; u < 4; ++u) v[u] = 4 * c4 + u < FN_C ? x[(size_t)(4 * c4 + u) * p.N] : 0.f;
    st4(row + 4 * c4, v);
  }
}

struct FnScan {
  const float* q; const float* rows;                       // the searching side [B,33,Nq], the searched side's rows [B,Nc,36]
  int B, Nq, Nc, S, seg_len, nblk;                         // nblk: workgroups per cloud and segment = ceil(Nq / (256 Q))
  float* part_d2; int* part_idx;                           // [S][B][Nq]
};

template <int Q>
__global__ __launch_bounds__(FN_BLOCK) void featnn_scan_kernel(FnScan p) {
  const int t = threadIdx.x;
  int s, blk, b;
  seg_workgroup(blockIdx.x, p.S, p.nblk, &s, &blk, &b);
  const int Nq = p.Nq, Nc = p.Nc;
  const float* __restrict__ qx = p.q + (size_t)b * FN_C * Nq;

  float a[Q][FN_C], best[Q];
  int bi[Q];
#pragma unroll
  for (int q = 0; q < Q; ++q) {
    const int n = blk * (FN_BLOCK * Q) + q * FN_BLOCK + t;
    const int c = n < Nq ? n : Nq - 1;                     // a lane without a column scans a copy of the last one, stores nothing
#pragma unroll
    for (int ch = 0; ch < FN_C; ++ch) a[q][ch] = qx[(size_t)ch * Nq + c];
    best[q] = __builtin_huge_valf();
    bi[q] = -1;
  }

  int lo, hi;
  seg_range(s, p.seg_len, Nc, &lo, &hi);
  const float* __restrict__ rows = p.rows + (size_t)b * Nc * FN_ROW;   // (workgroup-uniform, like j below: scalar loads)

  auto candidate = [&](int j) {
    const float* __restrict__ row = rows + (size_t)j * FN_ROW;
#pragma unroll
    for (int q = 0; q < Q; ++q) {
      const float d0 = a[q][0] - row[0];
      float acc = d0 * d0;
#pragma unroll
      for (int ch = 1; ch < FN_C; ++ch) {
        const float d = a[q][ch] - row[ch];
        acc = fmaf(d, d, acc);
      }
      const bool take = acc < best[q];
      best[q] = take ? acc : best[q];
      bi[q] = take ? j : bi[q];
    }
  };
  int j = lo;
  for (; j + 1 < hi; j += 2) { candidate(j); candidate(j + 1); }       // ascending: the strict < keeps the lowest index
  if (j < hi) candidate(j);

  const size_t out = ((size_t)s * p.B + b) * (size_t)Nq;
#pragma unroll
  for (int q = 0; q < Q; ++q) {
    const int n = blk * (FN_BLOCK * Q) + q * FN_BLOCK + t;
    if (n < Nq) { p.part_d2[out + n] = best[q]; p.part_idx[out + n] = bi[q]; }
  }
}

struct FnMerge { const float* part_d2; const int* part_idx; int B, N, S; long total; int* idx; float* d2; };   // total = B N

__global__ __launch_bounds__(FN_BLOCK) void featnn_merge_kernel(FnMerge p) {
  const long g = (long)blockIdx.x * FN_BLOCK + threadIdx.x;
  if (g >= p.total) return;
  float best;
  int bi;
  // the candidates [S][B][N] as ONE cloud of B N columns: (s B + b) N + n = s (B N) + g, and B N < 2^31
  nn_fold(p.part_d2, p.part_idx, 1, (int)p.total, p.S, 0, (int)g, &best, &bi);
  p.idx[g] = bi;
  if (p.d2) p.d2[g] = best;
}

struct FnMutual { int* nn_idx; const int* rev; int Ns, Nt; long total; };   // total = B Ns

__global__ __launch_bounds__(FN_BLOCK) void featnn_mutual_kernel(FnMutual p) {
  const long g = (long)blockIdx.x * FN_BLOCK + threadIdx.x;
  if (g >= p.total) return;
  const long b = g / p.Ns;
  const int i = (int)(g - b * p.Ns);
  const int j = p.nn_idx[g];
  if (j >= 0 && p.rev[(size_t)b * p.Nt + j] != i) p.nn_idx[g] = -1;
}

// How one call runs: fn_plan() validates the arguments and decides the form from them and the CU count, and it is the only
// place that does.  A direction is Q and the scan's split; the reverse one exists when rev_idx or mutual asks for it.
struct FnDir { int Q; SegSplit scan; };
struct FnPlan {
  vcr_feat_nn_args a;
  bool reverse;
  FnDir fwd, rev;
  size_t rows_b, rows_a, part_d2, part_idx, rev_buf, bytes;    // workspace offsets: b's rows | a's rows | candidates | rev
};

int fn_dir(int B, int Nq, int Nc, int fq, int fs, int cu, FnDir* d) {
  // Measured (profiles/match_bench.txt, every Q forced at three shapes): more columns per lane amortise the scalar loads of a
  // candidate row and pack two chains into one v_pk_fma_f32 -- four beat one by 10 % at 16 x 16 384 and 1 x 131 072 rows, at
  // three waves per SIMD -- but only while the searched side can still be cut into `fill` workgroups; at 16 x 1 024 rows,
  // where it cannot, one column per lane (four times the workgroups) is 19-26 % faster.  So the plan takes the most columns per
  // lane that leave `fill` workgroups within reach, then cuts the searched side until they exist, into segments of at least
  // FN_MIN_SEGMENT rows (seg_split, under FN_LIMITS).
  d->Q = fq ? fq : seg_fills(B, Nq, Nc, 4, cu, FN_LIMITS) ? 4 : seg_fills(B, Nq, Nc, 2, cu, FN_LIMITS) ? 2 : 1;
  return seg_split(B, Nq, Nc, d->Q, fs, cu, FN_LIMITS, &d->scan);
}

int fn_plan(const vcr_feat_nn_args& a, int cu, FnPlan* p) {
  *p = FnPlan{a};
  if (!a.a || !a.b || !a.nn_idx || a.B < 1 || a.Ns < 1 || a.Nt < 1) return VCR_EINVAL;
  int fq, fs;
  if (seg_variant(a.variant, SEG_Q_124, FN_LIMITS, &fq, &fs)) return VCR_EINVAL;
  if (a.C != FN_C) return VCR_EUNSUPPORTED;
  const int Nmax = a.Ns > a.Nt ? a.Ns : a.Nt;
  if (a.Ns > FN_MAX_N || a.Nt > FN_MAX_N || (long)a.B * Nmax >= (1L << 31)) return VCR_EUNSUPPORTED;
  p->reverse = a.mutual != 0 || a.rev_idx != nullptr;
  int e = fn_dir(a.B, a.Ns, a.Nt, fq, fs, cu, &p->fwd);
  if (e) return e;
  p->rev = FnDir{};
  if (p->reverse && (e = fn_dir(a.B, a.Nt, a.Ns, fq, fs, cu, &p->rev))) return e;
  size_t cand = (size_t)p->fwd.scan.S * a.B * a.Ns;
  if (p->reverse && (size_t)p->rev.scan.S * a.B * a.Nt > cand) cand = (size_t)p->rev.scan.S * a.B * a.Nt;
  p->rows_b = 0;
  p->rows_a = ws_up((size_t)a.B * a.Nt * FN_ROW * 4);
  p->part_d2 = p->rows_a + (p->reverse ? ws_up((size_t)a.B * a.Ns * FN_ROW * 4) : 0);
  p->part_idx = p->part_d2 + ws_up(cand * 4);
  p->rev_buf = p->part_idx + ws_up(cand * 4);
  p->bytes = p->rev_buf + (p->reverse && !a.rev_idx ? ws_up((size_t)a.B * a.Nt * 4) : 0);
  return VCR_OK;
}

unsigned fn_grid(long lanes) { return (unsigned)((lanes + FN_BLOCK - 1) / FN_BLOCK); }     // lanes < 2^31

// One direction: the searched side's rows, the scan the plan says, the merge
int fn_search(const FnDir& d, const float* q, const float* c, int B, int Nq, int Nc, float* rows, float* part_d2, int* part_idx,
              int* idx, float* d2, hipStream_t s) {
  int e;
  const FnRows r{c, rows, Nc, (long)B * Nc};
  hipLaunchKernelGGL(featnn_rows_kernel, dim3(fn_grid(r.total)), dim3(FN_BLOCK), 0, s, r);
  if ((e = VCR_LAUNCH_RC())) return e;
  const FnScan sc{q, rows, B, Nq, Nc, d.scan.S, d.scan.seg_len, d.scan.nblk, part_d2, part_idx};
  switch (d.Q) {
    case 4: hipLaunchKernelGGL(featnn_scan_kernel<4>, dim3(d.scan.grid), dim3(FN_BLOCK), 0, s, sc); break;
    case 2: hipLaunchKernelGGL(featnn_scan_kernel<2>, dim3(d.scan.grid), dim3(FN_BLOCK), 0, s, sc); break;
    default: hipLaunchKernelGGL(featnn_scan_kernel<1>, dim3(d.scan.grid), dim3(FN_BLOCK), 0, s, sc); break;
  }
  if ((e = VCR_LAUNCH_RC())) return e;
  const FnMerge mg{part_d2, part_idx, B, Nq, d.scan.S, (long)B * Nq, idx, d2};
  hipLaunchKernelGGL(featnn_merge_kernel, dim3(fn_grid(mg.total)), dim3(FN_BLOCK), 0, s, mg);
  return VCR_LAUNCH_RC();
}

int fn_take(const vcr_feat_nn_args* user, vcr_feat_nn_args* mine) {
  return vcr_take_args(user, mine, offsetof(vcr_feat_nn_args, variant));
}

}  // namespace

extern "C" int vcr_feat_nn_form(const vcr_feat_nn_args* ua, int cu_count, int* queries_per_lane, int* target_splits) {
  vcr_feat_nn_args a;
  FnPlan p;
  if (fn_take(ua, &a) || cu_count < 0) return VCR_EINVAL;
  const int e = fn_plan(a, cu_count ? cu_count : vcr_cu_count(), &p);
  if (e) return e;
  if (queries_per_lane) *queries_per_lane = p.fwd.Q;
  if (target_splits) *target_splits = p.fwd.scan.S;
  return VCR_OK;
}

extern "C" size_t vcr_feat_nn_workspace_bytes(const vcr_feat_nn_args* ua, int cu_count) {
  vcr_feat_nn_args a;
  FnPlan p;
  if (fn_take(ua, &a) || cu_count < 0) return 0;
  return fn_plan(a, cu_count ? cu_count : vcr_cu_count(), &p) ? 0 : p.bytes;
}

extern "C" int vcr_feat_nn_f32(const vcr_feat_nn_args* ua, void* workspace, size_t workspace_bytes, vcr_stream_t stream) {
  vcr_feat_nn_args a;
  if (fn_take(ua, &a)) return VCR_EINVAL;
  FnPlan p;
  int e = fn_plan(a, 1, &p);                               // the argument checks need no device
  if (e) return e;
  if (!workspace || (((uintptr_t)workspace) & 15)) return VCR_EINVAL;
  vcr_stream_scope scope_(stream);
  e = fn_plan(a, vcr_cu_count(), &p);
  if (e) return e;
  if (workspace_bytes < p.bytes) return VCR_EWORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  unsigned char* w = reinterpret_cast<unsigned char*>(workspace);
  float* part_d2 = reinterpret_cast<float*>(w + p.part_d2);
  int* part_idx = reinterpret_cast<int*>(w + p.part_idx);
  if ((e = fn_search(p.fwd, a.a, a.b, a.B, a.Ns, a.Nt, reinterpret_cast<float*>(w + p.rows_b), part_d2, part_idx, a.nn_idx,
                     a.nn_d2, s)))
    return e;
  if (!p.reverse) return VCR_OK;
  int* rev = a.rev_idx ? a.rev_idx : reinterpret_cast<int*>(w + p.rev_buf);
  if ((e = fn_search(p.rev, a.b, a.a, a.B, a.Nt, a.Ns, reinterpret_cast<float*>(w + p.rows_a), part_d2, part_idx, rev, nullptr, s)))
    return e;
  if (!a.mutual) return VCR_OK;
  const FnMutual mu{a.nn_idx, rev, a.Ns, a.Nt, (long)a.B * a.Ns};
  hipLaunchKernelGGL(featnn_mutual_kernel, dim3(fn_grid(mu.total)), dim3(FN_BLOCK), 0, s, mu);
  return VCR_LAUNCH_RC();
}

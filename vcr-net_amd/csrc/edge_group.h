// Group geometry of the EdgeConv kernels (edgeconv.hip, edgeconv_bf16x3.hip, edgechain.hip), and the host side the two
// EdgeConv entry points share.
//
// 160 edge rows = 5 MFMA tiles of 32 rows = G = 160 / k whole points for k = 20 (G = 8) and k = 40 (G = 4): a tile then spans
// several points, and the row -> point map is a compile-time function of (tile, accumulator register, lane half), so the
// max over a point's edges folds into G per-point registers with static indexing.
//
// What is shared here compiles to the instruction stream the kernels had with their own copies (device-only assembly
// compared file by file).  Deliberately NOT shared: the W2-slice register load (`wf[g] = ld4(p.w2 + ...)`, four kernels) --
// behind a function that takes the array by reference it changes address arithmetic and register allocation of the
// hand-scheduled kernels (1 656 lines of edgeconv.hip's assembly), which sit on register cliffs; edgechain.hip's fold_tile,
// which is edge_fold over a tile's 16 registers written out -- as a loop over edge_fold the k = 20 chain kernel's selects and
// maxima come out in another order (60 lines); the gather / commit lambdas, whose load order IS each kernel's schedule; and
// edgeconv_bf16x3's x1 fold over 8-row slabs (another map: build rows, not accumulator rows).
#pragma once
#include "common.h"

// Points per 5-tile group for the k the static row -> point maps exist for; 0: no such map (the padded kernel, or refused).
constexpr __host__ __device__ int edge_group_points(int k) { return k == 20 || k == 40 ? 160 / k : 0; }

// Accumulator register r of tile t (0..4 inside the group) -> the per-point maxima pm[G].  The register holds edge row
// 32 t + acc_row(r, 0) in lane half 0 and the row 4 below in half 1; where the two belong to different points each half
// offers `lowest` to the other's point: -inf for maxima taken before the bias, 0 for post-ReLU values.  t and r must be
// constants after unrolling (static indexing of pm).
template <int KE, int G>
__device__ __forceinline__ void edge_fold(float v, int t, int r, int half, float lowest, float (&pm)[G]) {
  static_assert(G == edge_group_points(KE), "G points of KE edges fill five 32-row tiles");
  const int row0 = 32 * t + acc_row(r, 0), row1 = row0 + 4;
  const int p0 = row0 / KE, p1 = row1 / KE;
  if (p0 == p1) {
    pm[p0] = fmaxf(pm[p0], v);
  } else {
    pm[p0] = fmaxf(pm[p0], half ? lowest : v);
    pm[p1] = fmaxf(pm[p1], half ? v : lowest);
  }
}

__device__ __forceinline__ f32x4 max4(f32x4 a, f32x4 b) { return f32x4{fmaxf(a[0], b[0]), fmaxf(a[1], b[1]), fmaxf(a[2], b[2]), fmaxf(a[3], b[3])}; }
__device__ __forceinline__ f32x4 relu4(f32x4 v) { return f32x4{fmaxf(v[0], 0.f), fmaxf(v[1], 0.f), fmaxf(v[2], 0.f), fmaxf(v[3], 0.f)}; }

// ---- host side of vcr_edgeconv_f32 / vcr_edgeconv_bf16x3_f32: check, plan (edgeconv.hip), run (each file its own kernels)
enum class EdgeconvForm { PADDED, PACKED, PIPE, BF16X3 };
struct EdgeconvPlan { EdgeconvForm form; int grid; };
int edgeconv_check(const vcr_edgeconv_args* a, bool bf16x3);          // the VCR_E* code of either entry point
EdgeconvPlan edgeconv_plan(const vcr_edgeconv_args& a, bool bf16x3);  // of checked arguments

// The one brute-force nearest-neighbour scan of the full clouds and the plan that fixes its form, shared by
// nnscore.hip (vcr_nn_score_f32) and refine.hip (vcr_refine_f32, which runs it once per round behind a per-cloud gate).
#pragma once
#include "seg_scan.h"
#include "../../include/vcr_hip_score.h"

namespace {

constexpr int NN_BLOCK = 256;
static_assert(NN_BLOCK == WG_BLOCK, "seg_scan.h and wg_scan.h serve workgroups of this size");
constexpr int NN_TILE = 1024;                              // target points per LDS tile: 3 planes x 4 KB
constexpr int NN_MAX_N = 131072;                           // the kNN / FPS entry points' limit (vcr_hip.h)
constexpr int NN_MAX_SPLITS = 128;
constexpr int NN_MIN_SEGMENT = 256;                        // the plan cuts no segment shorter than this (a forced split may)
constexpr int NN_FILL_PER_CU = 64;                         // workgroups per CU the plan cuts the work into, where it can
constexpr SegLimits NN_LIMITS{NN_MIN_SEGMENT, NN_FILL_PER_CU, NN_MAX_SPLITS};

struct NnPartial { double sum; int count; int pad; };      // one per 256 source points
static_assert(sizeof(NnPartial) == 16, "workspace layout");

struct NnScan {
  const float* src; const float* tgt; const float* R; const float* t;
  int B, Ns, Nt, S, seg_len, nblk;                         // nblk: workgroups per cloud and segment = ceil(Ns / (256 Q))
  float* part_d2; int* part_idx;                           // [S][B][Ns]
  const int* live;                                         // optional [B]: a cloud whose word is 0 is skipped (vcr_refine_f32)
};

template <int Q>
__global__ __launch_bounds__(NN_BLOCK) void nn_scan_kernel(NnScan p) {
  __shared__ __attribute__((aligned(16))) float lx[NN_TILE], ly[NN_TILE], lz[NN_TILE];
  const int t = threadIdx.x;
  int s, blk, b;
  seg_workgroup(blockIdx.x, p.S, p.nblk, &s, &blk, &b);
  if (p.live && !p.live[b]) return;                        // (workgroup-uniform, before the first barrier)
  const int Ns = p.Ns, Nt = p.Nt;
  const float* __restrict__ sx = p.src + (size_t)b * 3 * Ns;
  const float* __restrict__ tx = p.tgt + (size_t)b * 3 * Nt;

  float px[Q], py[Q], pz[Q], best[Q];
  int bi[Q];
  float r[9] = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f}, tr[3] = {0.f, 0.f, 0.f};
  if (p.R) {
    for (int i = 0; i < 9; ++i) r[i] = p.R[(size_t)b * 9 + i];
    for (int i = 0; i < 3; ++i) tr[i] = p.t[(size_t)b * 3 + i];
  }
#pragma unroll
  for (int q = 0; q < Q; ++q) {
    const int n = blk * (NN_BLOCK * Q) + q * NN_BLOCK + t;
    const int c = n < Ns ? n : Ns - 1;                     // a lane without a point scans a copy of the last one, stores nothing
    const float x = sx[c], y = sx[Ns + c], z = sx[2 * (size_t)Ns + c];
    if (p.R) {                                             // pose_step_kernel's expression (forward.hip), bit for bit
      px[q] = fmaf(r[2], z, fmaf(r[1], y, r[0] * x)) + tr[0];
      py[q] = fmaf(r[5], z, fmaf(r[4], y, r[3] * x)) + tr[1];
      pz[q] = fmaf(r[8], z, fmaf(r[7], y, r[6] * x)) + tr[2];
    } else {
      px[q] = x; py[q] = y; pz[q] = z;
    }
    best[q] = __builtin_huge_valf();
    bi[q] = -1;
  }

  int lo, hi;
  seg_range(s, p.seg_len, Nt, &lo, &hi);
  const float nan = __uint_as_float(0x7FC00000u);
  for (int t0 = lo; t0 < hi; t0 += NN_TILE) {                         // (workgroup-uniform: the barriers are met by all)
    const int cnt = hi - t0 < NN_TILE ? hi - t0 : NN_TILE;
    const int cnt4 = (cnt + 3) & ~3;                                  // <= NN_TILE; the tail is NaN: its d2 never wins
    __syncthreads();                                                  // the previous tile has been read
    for (int i = t; i < cnt4; i += NN_BLOCK) {
      const bool in = i < cnt;
      const int g = t0 + (in ? i : 0);
      lx[i] = in ? tx[g] : nan;
      ly[i] = in ? tx[Nt + g] : nan;
      lz[i] = in ? tx[2 * (size_t)Nt + g] : nan;
    }
    __syncthreads();
    for (int j = 0; j < cnt4; j += 4) {
      const f32x4 X = ld4(lx + j), Y = ld4(ly + j), Z = ld4(lz + j);  // one address for every lane: broadcast reads
#pragma unroll
      for (int u = 0; u < 4; ++u) {
#pragma unroll
        for (int q = 0; q < Q; ++q) {
          const float dx = px[q] - X[u], dy = py[q] - Y[u], dz = pz[q] - Z[u];
          const float d2 = fmaf(dz, dz, fmaf(dy, dy, dx * dx));
          const bool take = d2 < best[q];
          best[q] = take ? d2 : best[q];
          bi[q] = take ? t0 + j + u : bi[q];
        }
      }
    }
  }
  const size_t row = ((size_t)s * p.B + b) * (size_t)Ns;
#pragma unroll
  for (int q = 0; q < Q; ++q) {
    const int n = blk * (NN_BLOCK * Q) + q * NN_BLOCK + t;
    if (n < Ns) { p.part_d2[row + n] = best[q]; p.part_idx[row + n] = bi[q]; }
  }
}

// How one call runs.  nn_plan() validates the arguments and decides the form from them and the CU count, and it is the only
// place that does: the entry point launches what the plan says, vcr_nn_score_form and _workspace_bytes answer from it.
struct NnPlan {
  vcr_nn_score_args a;
  int Q;
  SegSplit scan;
  unsigned merge_grid;
  int nblk;                                                // workgroups per cloud of the merge
  size_t part_bytes, partial_off, bytes;                   // workspace: part_d2 | part_idx | partials
};

}  // namespace

static int nn_plan(const vcr_nn_score_args& a, int cu, NnPlan* p) {
  *p = NnPlan{a};
  if (!a.src || !a.tgt || !a.fitness || !a.rmse || a.B < 1 || a.Ns < 1 || a.Nt < 1) return VCR_EINVAL;
  if ((a.R == nullptr) != (a.t == nullptr)) return VCR_EINVAL;
  if (!(a.max_dist >= 0.f) || a.max_dist == __builtin_huge_valf()) return VCR_EINVAL;      // negative, NaN, +inf
  int fq, fs;
  if (seg_variant(a.variant, SEG_Q_124, NN_LIMITS, &fq, &fs)) return VCR_EINVAL;
  if (a.Ns > NN_MAX_N || a.Nt > NN_MAX_N || (long)a.B * (a.Ns > a.Nt ? a.Ns : a.Nt) >= (1L << 31)) return VCR_EUNSUPPORTED;
  // Measured (profiles/nnscore_bench.txt, every Q x S forced at four shapes): one point per lane wins at every shape -- at an
  // equal number of workgroups two per lane lose 10-15 % (65 VGPRs, seven waves per SIMD) and four 4-8 % -- and the scan keeps
  // gaining until a CU has been dealt about 64 workgroups, eight rounds of the eight (32 waves) it holds.  So the plan takes
  // Q = 1 and cuts the target (seg_split, under NN_LIMITS); Q = 2 / 4 stay as forced forms.
  p->Q = fq ? fq : 1;
  const int e = seg_split(a.B, a.Ns, a.Nt, p->Q, fs, cu, NN_LIMITS, &p->scan);
  if (e) return e;
  p->nblk = (a.Ns + NN_BLOCK - 1) / NN_BLOCK;
  p->merge_grid = (unsigned)((long)a.B * p->nblk);
  p->part_bytes = ws_up((size_t)p->scan.S * a.B * a.Ns * 4);
  p->partial_off = 2 * p->part_bytes;
  p->bytes = p->partial_off + ws_up((size_t)a.B * p->nblk * sizeof(NnPartial));
  return VCR_OK;
}

// The scan the plan says, on the stream (the workspace's first two parts are its candidates)
static int nn_scan_launch(const NnPlan& p, void* workspace, const int* live, hipStream_t s) {
  unsigned char* w = reinterpret_cast<unsigned char*>(workspace);
  const vcr_nn_score_args& a = p.a;
  const NnScan sc{a.src, a.tgt, a.R, a.t, a.B, a.Ns, a.Nt, p.scan.S, p.scan.seg_len, p.scan.nblk,
                  reinterpret_cast<float*>(w), reinterpret_cast<int*>(w + p.part_bytes), live};
  switch (p.Q) {
    case 4: hipLaunchKernelGGL(nn_scan_kernel<4>, dim3(p.scan.grid), dim3(NN_BLOCK), 0, s, sc); break;
    case 2: hipLaunchKernelGGL(nn_scan_kernel<2>, dim3(p.scan.grid), dim3(NN_BLOCK), 0, s, sc); break;
    default: hipLaunchKernelGGL(nn_scan_kernel<1>, dim3(p.scan.grid), dim3(NN_BLOCK), 0, s, sc); break;
  }
  return VCR_LAUNCH_RC();
}

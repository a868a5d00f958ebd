// The one brute-force nearest-neighbour scan of the full clouds and the plan that fixes its form, shared by
// nnscore.hip (vcr_nn_score_f32) and refine.hip (vcr_refine_f32, which runs it once per round behind a per-cloud gate).
#pragma once
#include "common.h"
#include "../../include/vcr_hip_score.h"

namespace {

constexpr int NN_BLOCK = 256;
constexpr int NN_TILE = 1024;                              // target points per LDS tile: 3 planes x 4 KB
constexpr int NN_MAX_N = 131072;                           // the kNN / FPS entry points' limit (vcr_hip.h)
constexpr int NN_MAX_SPLITS = 128;
constexpr int NN_MIN_SEGMENT = 256;                        // the plan cuts no segment shorter than this (a forced split may)
constexpr int NN_FILL_PER_CU = 64;                         // workgroups per CU the plan cuts the work into, where it can

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
  const unsigned bid = blockIdx.x;
  const int s = (int)(bid % (unsigned)p.S);
  const unsigned rest = bid / (unsigned)p.S;
  const int blk = (int)(rest % (unsigned)p.nblk), b = (int)(rest / (unsigned)p.nblk);
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

  const long seg_lo = (long)s * p.seg_len;
  const int lo = seg_lo < Nt ? (int)seg_lo : Nt;
  const int hi = Nt - lo < p.seg_len ? Nt : lo + p.seg_len;           // [lo, hi) is inside [0, Nt]; empty past the cloud's end
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

// One source point's neighbour from its S candidates, ascending segments = ascending target index: the strict < keeps the
// lowest index among equals, as inside a segment.
__device__ __forceinline__ void nn_fold(const float* part_d2, const int* part_idx, int B, int Ns, int S, int b, int n,
                                        float* best_out, int* bi_out) {
  float best = __builtin_huge_valf();
  int bi = -1;
  for (int s = 0; s < S; ++s) {
    const size_t at = ((size_t)s * B + b) * (size_t)Ns + n;
    const float d2 = part_d2[at];
    const int i = part_idx[at];
    const bool take = d2 < best;
    best = take ? d2 : best;
    bi = take ? i : bi;
  }
  *best_out = best; *bi_out = bi;
}

// How one call runs.  nn_plan() validates the arguments and decides the form from them and the CU count, and it is the only
// place that does: the entry point launches what the plan says, vcr_nn_score_form and _workspace_bytes answer from it.
struct NnPlan {
  vcr_nn_score_args a;
  int Q, S, seg_len;
  unsigned scan_grid, merge_grid;
  int nblk_scan, nblk;                                     // workgroups per cloud: of the scan (and segment), of the merge
  size_t part_bytes, partial_off, bytes;                   // workspace: part_d2 | part_idx | partials
};

inline size_t nn_up(size_t v) { return (v + 255) & ~(size_t)255; }

}  // namespace

static int nn_plan(const vcr_nn_score_args& a, int cu, NnPlan* p) {
  *p = NnPlan{a};
  if (!a.src || !a.tgt || !a.fitness || !a.rmse || a.B < 1 || a.Ns < 1 || a.Nt < 1) return VCR_EINVAL;
  if ((a.R == nullptr) != (a.t == nullptr)) return VCR_EINVAL;
  if (!(a.max_dist >= 0.f) || a.max_dist == __builtin_huge_valf()) return VCR_EINVAL;      // negative, NaN, +inf
  const int fq = a.variant & 0xF, fs = (a.variant >> 8) & 0xFF;
  if ((a.variant & ~0xFF0F) || (fq != 0 && fq != 1 && fq != 2 && fq != 4) || fs > NN_MAX_SPLITS) return VCR_EINVAL;
  if (a.Ns > NN_MAX_N || a.Nt > NN_MAX_N || (long)a.B * (a.Ns > a.Nt ? a.Ns : a.Nt) >= (1L << 31)) return VCR_EUNSUPPORTED;
  if (cu < 1) cu = 1;
  auto groups = [&](int q) { return (long)a.B * ((a.Ns + NN_BLOCK * q - 1) / (NN_BLOCK * q)); };
  // Measured (profiles/nnscore_bench.txt, every Q x S forced at four shapes): one point per lane wins at every shape -- at an
  // equal number of workgroups two per lane lose 10-15 % (65 VGPRs, seven waves per SIMD) and four 4-8 % -- and the scan keeps
  // gaining until a CU has been dealt about 64 workgroups, eight rounds of the eight (32 waves) it holds.  So the plan takes
  // Q = 1 and cuts the target; Q = 2 / 4 stay as forced forms.
  const long fill = (long)NN_FILL_PER_CU * cu;
  const long whole = a.Nt / NN_MIN_SEGMENT;                // (rounded down: a segment, ceil(Nt / S) points, is never shorter)
  const long most = whole < 1 ? 1 : whole < NN_MAX_SPLITS ? whole : NN_MAX_SPLITS;
  const int Q = fq ? fq : 1;
  // S: 1 whenever the source alone fills the CUs; else the target is cut until `fill` workgroups exist, into segments of at
  // least NN_MIN_SEGMENT points
  int S = fs;
  if (!S) {
    S = 1;
    if (groups(Q) < fill) {
      const long want = (fill + groups(Q) - 1) / groups(Q);
      S = (int)(want < most ? want : most);
    }
  }
  p->Q = Q; p->S = S;
  p->seg_len = (a.Nt + S - 1) / S;
  p->nblk_scan = (a.Ns + NN_BLOCK * Q - 1) / (NN_BLOCK * Q);
  p->nblk = (a.Ns + NN_BLOCK - 1) / NN_BLOCK;
  const long scan = groups(Q) * S;
  if (scan >= (1L << 31)) return VCR_EUNSUPPORTED;
  p->scan_grid = (unsigned)scan;
  p->merge_grid = (unsigned)((long)a.B * p->nblk);
  p->part_bytes = nn_up((size_t)S * a.B * a.Ns * 4);
  p->partial_off = 2 * p->part_bytes;
  p->bytes = p->partial_off + nn_up((size_t)a.B * p->nblk * sizeof(NnPartial));
  return VCR_OK;
}

// The scan the plan says, on the stream (the workspace's first two parts are its candidates)
static int nn_scan_launch(const NnPlan& p, void* workspace, const int* live, hipStream_t s) {
  unsigned char* w = reinterpret_cast<unsigned char*>(workspace);
  const vcr_nn_score_args& a = p.a;
  const NnScan sc{a.src, a.tgt, a.R, a.t, a.B, a.Ns, a.Nt, p.S, p.seg_len, p.nblk_scan,
                  reinterpret_cast<float*>(w), reinterpret_cast<int*>(w + p.part_bytes), live};
  switch (p.Q) {
    case 4: hipLaunchKernelGGL(nn_scan_kernel<4>, dim3(p.scan_grid), dim3(NN_BLOCK), 0, s, sc); break;
    case 2: hipLaunchKernelGGL(nn_scan_kernel<2>, dim3(p.scan_grid), dim3(NN_BLOCK), 0, s, sc); break;
    default: hipLaunchKernelGGL(nn_scan_kernel<1>, dim3(p.scan_grid), dim3(NN_BLOCK), 0, s, sc); break;
  }
  return VCR_LAUNCH_RC();
}

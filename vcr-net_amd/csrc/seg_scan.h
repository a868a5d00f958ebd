// The frame of a brute-force scan that is cut into segments, written once for nn_scan_kernel (nn_scan.h),
// voxel_scan_kernel, outlier_count_kernel and featnn_scan_kernel: B clouds, per cloud Nq searching points -- 256 Q of them a
// workgroup -- against Nc searched ones cut into S segments of seg_len.  One workgroup per (cloud, block, segment); a
// (segment, point) candidate goes to the workspace at [s][b][n] and a merge folds the S of a point.  The scan kernels keep
// their own bodies -- what they stage, load and do per pair differs, and their loops were tuned apart.
//
// The contract every one of them keeps: the searched points are met in ASCENDING index inside a segment, segments ascend in
// index, and a candidate replaces the best only on a strict <.  So the lowest index wins among equals, a NaN never wins, and
// any S returns the same bits.
#pragma once
#include "wg_scan.h"

namespace {

// ------------------------------------------------------------------------------------------------------------------ the host

inline size_t ws_up(size_t v) { return (v + 255) & ~(size_t)255; }     // a workspace part's size: the next one starts 256-B aligned

// What a caller has measured for its scan: the plan cuts no segment shorter than min_segment (a forced split may), cuts until
// a CU has been dealt fill_per_cu workgroups where it can, and into max_splits segments at the most (forced ones included).
struct SegLimits { int min_segment, fill_per_cu, max_splits; };

constexpr unsigned SEG_Q_1 = 1u << 0 | 1u << 1;            // the forced Q a caller serves, one bit each: the plan's (0) or 1 ...
constexpr unsigned SEG_Q_124 = SEG_Q_1 | 1u << 2 | 1u << 4;            // ... or 1, 2, 4

// variant = forced Q | forced S << 8 (VCR_NN_SCORE_VARIANT), 0 = the plan's: VCR_EINVAL for a bit outside the two fields, a Q
// the caller does not serve, more than max_splits segments
inline int seg_variant(int variant, unsigned q_served, const SegLimits& lim, int* forced_Q, int* forced_S) {
  const int fq = variant & 0xF, fs = (variant >> 8) & 0xFF;
  if ((variant & ~0xFF0F) || !((q_served >> fq) & 1u) || fs > lim.max_splits) return VCR_EINVAL;
  *forced_Q = fq; *forced_S = fs;
  return VCR_OK;
}

inline long seg_groups(int B, int Nq, int Q) { return (long)B * ((Nq + WG_BLOCK * Q - 1) / (WG_BLOCK * Q)); }
inline long seg_fill(int cu, const SegLimits& lim) { return (long)lim.fill_per_cu * (cu < 1 ? 1 : cu); }
// The most segments the plan cuts Nc into
inline long seg_most(int Nc, const SegLimits& lim) {
  const long whole = Nc / lim.min_segment;                 // (rounded down: a segment, ceil(Nc / S) points, is never shorter)
  return whole < 1 ? 1 : whole < lim.max_splits ? whole : lim.max_splits;
}
// Whether Q points per lane leave `fill` workgroups within the plan's reach (for a caller that chooses its Q by that)
inline bool seg_fills(int B, int Nq, int Nc, int Q, int cu, const SegLimits& lim) {
  return seg_groups(B, Nq, Q) * seg_most(Nc, lim) >= seg_fill(cu, lim);
}

struct SegSplit { int S, seg_len, nblk; unsigned grid; };  // nblk: workgroups per cloud and segment = ceil(Nq / (256 Q))

// S: the forced one; else 1 whenever the searching side alone fills the CUs; else the searched side is cut until `fill`
// workgroups exist, into segments of at least min_segment points.  VCR_EUNSUPPORTED when the grid reaches 2^31.
inline int seg_split(int B, int Nq, int Nc, int Q, int forced_S, int cu, const SegLimits& lim, SegSplit* out) {
  const long groups = seg_groups(B, Nq, Q), fill = seg_fill(cu, lim), most = seg_most(Nc, lim);
  int S = forced_S;
  if (!S) {
    S = 1;
    if (groups < fill) {
      const long want = (fill + groups - 1) / groups;
      S = (int)(want < most ? want : most);
    }
  }
  const long grid = groups * S;
  if (grid >= (1L << 31)) return VCR_EUNSUPPORTED;
  *out = SegSplit{S, (Nc + S - 1) / S, (Nq + WG_BLOCK * Q - 1) / (WG_BLOCK * Q), (unsigned)grid};
  return VCR_OK;
}

// ---------------------------------------------------------------------------------------------------------------- the device

// blockIdx.x -> (segment, block of 256 Q searching points, cloud): the segments of a block are neighbours in the grid
__device__ __forceinline__ void seg_workgroup(unsigned bid, int S, int nblk, int* s, int* blk, int* b) {
  *s = (int)(bid % (unsigned)S);
  const unsigned rest = bid / (unsigned)S;
  *blk = (int)(rest % (unsigned)nblk); *b = (int)(rest / (unsigned)nblk);
}

// Segment s of N searched points: [lo, hi) is inside [0, N]; empty past the cloud's end (a forced S may leave such segments)
__device__ __forceinline__ void seg_range(int s, int seg_len, int N, int* lo, int* hi) {
  const long seg_lo = (long)s * seg_len;
  *lo = seg_lo < N ? (int)seg_lo : N;
  *hi = N - *lo < seg_len ? N : *lo + seg_len;
}

// One searching point's neighbour from its S candidates at [s][b][n], ascending segments = ascending index: the strict < keeps
// the lowest index among equals, as inside a segment.
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

}  // namespace

/*
 * vcr_hip_consistency.h -- a pose from mostly wrong correspondences: pairwise length-consistency voting
 * (the pruning of TEASER, the second-order measure of SC2-PCR) over the pair list of vcr_ransac_f32.  A rigid motion keeps
 * distances, so two right pairs (s_a, t_a), (s_b, t_b) satisfy |s_a - s_b| = |t_a - t_b| and two unrelated pairs almost never
 * do.  No draws, no trial budget; every intermediate but the pose is an integer.  An extension of vcr_hip_match.h (same
 * library, same conventions, same error codes); it adds no symbol to that header, to vcr_hip.h or to its other extensions and
 * moves none of their layouts, so VCR_ABI_VERSION is unchanged.
 *
 * vcr_consistency_f32 -- per cloud, independently of the batch: the result is a function of one cloud pair's inputs alone,
 * the same bits in every B, every batch and every launch form.
 *   pairs       vcr_ransac_f32's pair list (vcr_hip_match.h): the source indices i with 0 <= corr[i] < Nt, ascending:
 *               pair_0 .. pair_{M-1}; s_a is the source point of pair a, t_a its partner
 *   compatible  (a, b), a != b:  ds2, dt2 = vcr_hip_match.h's fmaf(dz, dz, fmaf(dy, dy, dx * dx)) of the fp32 differences of the
 *               two source points and of their two partners;  ds = sqrt(ds2), dt = sqrt(dt2), the correctly rounded fp32
 *               square roots;  min_len2 = min_length * min_length (fp32).  The pair of pairs is compatible iff
 *                 fabsf(ds - dt) <= tau && ds2 >= min_len2 && dt2 >= min_len2
 *               (fp32; a NaN fails).  The relation is symmetric: (x - y)^2 and (y - x)^2 are the same bits.
 *   degree      deg[a] = the number of b in 0 .. M - 1, b != a, compatible with a
 *   kept        P = min(M, keep).  The pairs in the order of DESCENDING degree, among equal degrees the LOWER position in the
 *               pair list first (a stable sort of 0x1FFFF - deg); the first P of them are kept and numbered r = 0 .. P - 1
 *   adjacency   adj[r] = the row of bits c = 0 .. keep - 1: bit c is set iff c < P, c != r and kept c is compatible with kept r
 *               (bit c of the row is bit c % 64 of its 64-bit word c / 64); rows r >= P are zero
 *   seeds       the first S = min(P, seeds) ranks.  For seed r:  w[r][c] = popcount(adj[r] & adj[c]) where bit c of adj[r] is
 *               set, else 0 -- the kept pairs compatible with BOTH;  wmax[r] = the largest w[r][c]
 *   members     of seed r: r itself, and every c with bit c of adj[r] set and (float)w[r][c] >= ratio * (float)wmax[r]
 *               (an fp32 product); n_r is their number
 *   status 1    n_r < 3 (and every slot r >= S): no pose
 *   solve       vcr_hip_refine.h's step on the n_r members (source point p_c, partner q_c), the fp32 values widened to fp64.
 *               Sum order: chain l = 0 .. 63 starts at +0 and adds the members c with c % 64 == l in ASCENDING c (a rank that
 *               is no member adds nothing); the 64 chains are folded by the butterfly v_l += v_{l ^ o}, o = 32, 16, 8, 4, 2, 1.
 *               The fifteen sums S_p, S_q, S_pq = sum p q^T (the products are exact);  inv_n = 1.0 / (double)n_r;
 *               H = S_pq - (S_p S_q^T) * inv_n;  the one-sided Jacobi and the tail of vcr_rigid_svd_f32's solve;
 *               t = S_q * inv_n - R (S_p * inv_n);  a non-finite sum: R, t are NaN.  pose32 = round32(R, t)
 *   status 3    pose32 holds a non-finite value
 *   status 0    valid: count_r = the number of ALL M pairs with d2 <= max_dist * max_dist (the fp32 product) under pose32, d2 by
 *               vcr_hip_score.h's `moved source` and `distance` expressions against the pair's partner -- vcr_ransac_f32's count
 *   best        the valid seed with the highest count, among equal counts the LOWEST r.  None valid (M == 0 included):
 *               best_seed = -1, R = I, t = 0, inliers = 0
 * seed_pose holds pose32 for a seed of status 0 or 3 and twelve zeros for status 1; seed_inliers is -1 for a seed that is not
 * valid; seed_members is n_r (0 for a slot r >= S); member holds the members' bits in adj's layout (zero for r >= S).
 * Against SC2-PCR: the seeds are the highest first-order degrees, not the leading eigenvector's non-maxima; a seed's consensus
 * set is a threshold on its second-order row, not a fixed top-k; the hypothesis is one unweighted rigid fit.  Against TEASER:
 * no maximum clique is sought; the degree ranks the pairs.
 */
#ifndef VCR_HIP_CONSISTENCY_H
#define VCR_HIP_CONSISTENCY_H

#include "../vcr_hip_match.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VCR_CONSISTENCY_MAX_KEEP 4096     /* keep: 64 ... 4096, a multiple of 64 (a row of bits is at most one word a lane) */
#define VCR_CONSISTENCY_PRETEST_ON 0x10   /* variant bits: the degree pass with ... */
#define VCR_CONSISTENCY_PRETEST_OFF 0x20  /* ... and without the pre-test; both set: VCR_EINVAL */

/* variant: VCR_NN_SCORE_VARIANT's encoding for the degree pass (pairs per lane: 1, 2 or 4; splits of the streamed side:
 * 1 ... 128), 0 = the plan decides; beside its two fields VCR_CONSISTENCY_PRETEST_ON or _OFF forces the pre-test, which decides
 * a test from the raw hardware square roots wherever the rounding cannot matter, and neither leaves it to the plan.  Every
 * form returns the same bits: the decisions are the definition's and the partial counts are integers.
 * B, Ns, Nt < 1, a missing src, tgt, corr, R_out or t_out, tau or max_dist negative or not finite, min_length negative or not
 * finite, ratio outside [0, 1] or NaN, keep outside 64 ... 4096 or no multiple of 64, seeds outside 1 ... keep, a bad variant:
 * a stop_after outside 0 ... 2: VCR_EINVAL.  Ns or Nt > 131 072, B * max(Ns, Nt) >= 2^31, B * keep >= 2^30: VCR_EUNSUPPORTED. */
typedef struct {
  uint32_t struct_bytes;        /* sizeof(vcr_consistency_args) as the CALLER was compiled (see vcr_fps_args); the mandatory
                                   part ends behind t_out: 0, shorter than that or longer than this library knows: VCR_EINVAL */
  const float* src; const float* tgt;   /* [B,3,Ns], [B,3,Nt] channels-first fp32, contiguous */
  const int* corr;              /* [B,Ns]: the target index per source point; outside [0, Nt) = none */
  int B, Ns, Nt;
  float tau;                    /* finite, >= 0: the length tolerance */
  float min_length;             /* finite, >= 0: both lengths of a compatible pair of pairs are at least this */
  float max_dist;               /* finite, >= 0: the inlier distance of the count */
  float ratio;                  /* in [0, 1] */
  int keep;                     /* 64 ... VCR_CONSISTENCY_MAX_KEEP, a multiple of 64 */
  int seeds;                    /* 1 ... keep */
  float* R_out; float* t_out;   /* [B,3,3], [B,3], mandatory */
  int* best_seed; int* inliers; int* pairs;    /* optional [B] each; pairs = M */
  int* deg;                     /* optional [B,Ns]: in the SOURCE's numbering, -1 for a point without a pair */
  int* kept;                    /* optional [B,keep]: source indices by rank, -1 behind P */
  uint64_t* adj;                /* optional [B,keep,keep/64] */
  int* seed_status;             /* optional [B,seeds] */
  int* seed_members;            /* optional [B,seeds]: n_r */
  int* seed_inliers;            /* optional [B,seeds]: count_r, -1 for a seed that is not valid */
  float* seed_pose;             /* optional [B,seeds,12]: R row-major, then t */
  uint64_t* member;             /* optional [B,seeds,keep/64] */
  int variant;                  /* 0 = plan decides; otherwise forces a form of the degree pass (tests, benchmarks) */
  int stop_after;               /* 0: the whole call.  1: return behind the degree pass (deg, pairs alone are written; R_out and
                                   t_out are not).  2: behind kept (deg, pairs, kept).  Anything else: VCR_EINVAL */
} vcr_consistency_args;

/* Bytes of workspace vcr_consistency_f32 needs for these arguments (their variant included) on a device of cu_count compute
 * units; 0 for arguments the call would refuse.  cu_count 0 = the current device's; with an explicit cu_count nothing
 * touches a device. */
size_t vcr_consistency_workspace_bytes(const vcr_consistency_args*, int cu_count);
/* Asynchronous on the stream: no host synchronisation, no allocation, no atomic hands out a slot; fourteen launches.
 * workspace: device memory, 16-B aligned, at least vcr_consistency_workspace_bytes(args, 0) bytes (VCR_EWORKSPACE below
 * that); its contents need not be initialised. */
int    vcr_consistency_f32(const vcr_consistency_args*, void* workspace, size_t workspace_bytes, vcr_stream_t);
/* Host-only query (nothing is launched): the form of the degree pass -- pairs per lane, splits of the streamed side, whether
 * the pre-test runs (0 / 1); each pointer may be null. */
int    vcr_consistency_form(const vcr_consistency_args*, int cu_count, int* pairs_per_lane, int* splits, int* pretest);

#ifdef __cplusplus
}
#endif
#endif

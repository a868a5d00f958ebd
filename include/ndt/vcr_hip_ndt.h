/*
 * vcr_hip_ndt.h -- registering a scan to a voxel map of Gaussians: the Normal Distributions Transform,
 * point to distribution (Magnusson's P2D-NDT, PCL's NormalDistributionsTransform).  The target becomes, once, one Gaussian per
 * occupied voxel; a round looks up the voxel of every moved source point and its face neighbours and adds a smooth score with
 * its exact gradient and Hessian -- no neighbour search, no normals, no correspondence cap.  An extension of
 * vcr_hip_voxel_sort.h (same library, same conventions, same error codes); it adds no symbol to that header, to vcr_hip.h or to
 * its other extensions and moves none of their layouts, so VCR_ABI_VERSION is unchanged.
 *
 * vcr_ndt_map_f32 -- per cloud of tgt, independently of the batch; every bit is defined.  h = (double)resolution.
 *   voxels      vcr_hip_voxel.h's, word for word: the finite points, origin_c = (double)lo_c - 0.5 h, the fp64 cell, the voxels
 *               numbered in order of first appearance, the too-fine rule.  members / voxel_start are vcr_voxel_sort_f32's
 *   mean        mu_c(v) = s / (double)n, s the fp64 sum of the n members' coordinates in ascending member order that STARTS AS
 *               the first member: the voxel grid's own mean before its fp32 rounding
 *   covariance  C = six fp64 sums (xx, xy, xz, yy, yz, zz) of the products of d_c = (double)x_c - mu_c, in ascending member
 *               order, starting from 0, each divided by (double)(n - 1).  TWO passes: PCL's one pass sum(x x^T) - n mu mu^T
 *               cancels for a voxel far from the origin and is deliberately not the definition
 *   eigenpairs  C finite and not all zero: the cyclic Jacobi sweeps of the normals (vcr_hip_plane.h: rotations (0,1), (0,2),
 *               (1,2), at most 16 sweeps, stop on three exact zeros); the eigenvalues l_c are the diagonal, V the columns
 *   floor       l_max = the largest l_c; floor = min_eig_ratio * l_max; every l_c < floor is raised to floor (PCL: 0.01)
 *   inv_cov     A = V diag(1 / l) V^T: A_ij = ((v_i0 * (1 / l_0)) * v_j0 + (v_i1 * (1 / l_1)) * v_j1) + (v_i2 * (1 / l_2)) * v_j2,
 *               the six entries 00, 01, 02, 11, 12, 22
 *   valid       n >= min_points, C finite and not all zero, l_max > 0 and the six entries of A finite.  inv_cov of any
 *               other voxel is NaN; its mean is still its mean
 *   outputs     indexed by voxel number; slots v >= count hold NaN (mean, inv_cov) and 0 (valid, voxel_points).  A cloud
 *               without a finite point: count 0, origin NaN.  Too fine: count -1.  In both every later lookup misses
 *   lookup      key(v) = cx | cy << 21 | cz << 42 of the voxel's cell.  Per cloud a table of T = 2^ceil(log2(2 V + 2)) slots,
 *               V = max(count, 0), in the first T of the cloud's vcr_ndt_table_slots(Nt) words of table_keys / table_vals:
 *               open addressing from slot (key * 0x9E3779B97F4A7C15) >> (64 - log2 T), linear probing, every voxel (valid
 *               or not) entered by a 64-bit compare-and-swap on the key word; an empty word is all ones.  Keys are
 *               unique, so WHAT a lookup returns does not depend on who won which slot; the table's words themselves are
 *               the one output of this header that is not defined to the bit (and the sorted alternative was not built)
 * One lane per voxel computes the statistics: a voxel's members are walked serially, twice, as section 4.21's mean walks
 * them once.  A voxel that holds the whole cloud is one lane's 2 n dependent gathers: choose h for tens of points a voxel.
 *
 * vcr_ndt_derivatives_f32 -- score, gradient and Hessian of a scan at a pose; also the loop's round.
 *   moved point p_c = fmaf(r[3c+2], z, fmaf(r[3c+1], y, r[3c] * x)) + t[c]: vcr_hip_score.h's fp32 expression, bit for bit
 *   cell        floor(((double)p_c - origin_c) / h) with the TARGET's origin; a point with a cell outside [0, 2^21) on any
 *               axis, or with a non-finite coordinate, misses altogether
 *   cells read  neighbors = 1: the point's cell (PCL's DIRECT1); neighbors = 7: own, -x, +x, -y, +y, -z, +z (DIRECT7); a
 *               neighbour outside [0, 2^21) is skipped.  Only valid voxels count
 *   per (point, voxel), all fp64, no fused multiply-add, with P = (double)p, a_ij the voxel's inv_cov:
 *               r = P - mu;  Ar_i = (a_i0 r_0 + a_i1 r_1) + a_i2 r_2;  q = (r_0 Ar_0 + r_1 Ar_1) + r_2 Ar_2;
 *               e = exp((-(d2 * 0.5)) * q) -- the ONE value that is the math library's and not spelled out;  w = d2 * e
 *               Jdot(a, v) = v_2 P_1 - v_1 P_2 (a = 0), v_0 P_2 - v_2 P_0 (a = 1), v_1 P_0 - v_0 P_1 (a = 2), v_{a-3} (a >= 3):
 *               J_a . v for the chart's J_a = e_a x p (a < 3), e_{a-3} beyond
 *               u_a = Jdot(a, Ar);  AJ_a,i = Jdot(a, row i of A);  JAJ_ab = Jdot(b, AJ_a)
 *               rAS_00 = -(Ar_1 P_1 + Ar_2 P_2), rAS_11 = -(Ar_0 P_0 + Ar_2 P_2), rAS_22 = -(Ar_0 P_0 + Ar_1 P_1),
 *               rAS_01 = Ar_0 P_1, rAS_02 = Ar_0 P_2, rAS_12 = Ar_1 P_2: r^T A S_ab, S_ab = e_b x (e_a x p) for a <= b < 3
 *               f = f - e;  g_a = g_a + w * u_a;  H_ab = H_ab + w * (((-d2) * (u_a * u_b) + JAJ_ab) + rAS_ab)  (a <= b < 3),
 *               H_ab = H_ab + w * ((-d2) * (u_a * u_b) + JAJ_ab) otherwise: PCL's Hessian in this chart.  The S term was
 *               held to central second differences with the voxel assignment frozen and needed no correction
 *   chart       the pose moves by (euler(x) R, euler(x) t + x[3:6]) at x = 0, euler(x) = Rz(x2) Ry(x1) Rx(x0)
 *   values      per point 29: f, hit (1 if at least one valid voxel was read), g (6), the upper triangle of H by rows (21); a
 *               lane starts them at +0 and adds its voxels in cell order
 *   sum order   per 256 consecutive source points (lanes past Ns add zeros): the wave butterfly v_l += v_{l ^ o}, o = 32 ... 1,
 *               then the four waves ascending, then the partials ascending from +0 -- the refinements' order
 *   d1, d2      PCL's constants from outlier_ratio o and h, computed by the CALLER in fp64:  c1 = 10 (1 - o), c2 = o / h^3,
 *               d3 = -log(c2), d1 = -log(c1 + c2) - d3, d2 = -2 log((-log(c1 exp(-1/2) + c2) - d3) / d1)
 *
 * vcr_ndt_f32 -- Levenberg-Marquardt on f, one call, every round enqueued, no host synchronisation.
 *   state       per cloud fp64: the pose (R, t), the accepted f, g, H, lambda, nu.  Round 0 evaluates the start pose;
 *               lambda = 1e-5 * max_a |H_aa|, nu = 2
 *   trial       (H + lambda I) x = -g by the point-to-plane fit's Cholesky and pivot rule.  Pivot test failed: lambda *= nu,
 *               nu *= 2, the trial is spent and the round's launches do no work for the cloud.  Otherwise the trial pose is
 *               (euler(x) R, euler(x) t + x[3:6]) in fp64 and the round evaluates f, g, H at its fp32 rounding
 *   accept      f_trial < f, strictly: the trial pose and its sums become the state, iterations += 1, lambda *= 1.0 / 3.0,
 *               nu = 2.  Otherwise lambda *= nu, nu *= 2
 *   stops       status 0: an accepted step with max |x[0:3]| < rot_epsilon and max |x[3:6]| < trans_epsilon (converged = 1);
 *               1: max_iterations accepted steps;  2: max_trials rounds;  3: an evaluation with hits < 3;  4: one with a
 *               non-finite sum -- at 3 and 4 the accepted pose stays (the start pose when it is round 0's)
 *   returned    R_out, t_out = the fp32 rounding of the state's pose; score = f; probability = ((-d1) * (-f)) / (double)Ns;
 *               hits, iterations, trials, converged, status; g, H; trace[0] = round 0's f, trace[k] = the f round k
 *               accepted, NaN for a round that accepted none
 *   invariant   score, hits, g, H are vcr_ndt_derivatives_f32's for (R_out, t_out), bit for bit; a cloud's result does not
 *               depend on its batch
 */
#ifndef VCR_HIP_NDT_H
#define VCR_HIP_NDT_H

#include "../vcr_hip_voxel_sort.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VCR_NDT_VALUES 29          /* f, hits, g (6), H (21) */
#define VCR_NDT_STATE_BYTES 512    /* per cloud, in the workspace */
#define VCR_NDT_CONVERGED 0
#define VCR_NDT_MAX_ITERATIONS 1
#define VCR_NDT_MAX_TRIALS 2
#define VCR_NDT_NO_HITS 3
#define VCR_NDT_NOT_FINITE 4

/* B, Nt < 1, a missing pointer, resolution not finite or <= 0, min_points < 3, min_eig_ratio outside (0, 1] or NaN:
 * VCR_EINVAL.  Nt > 131 072 or B * Nt >= 2^31: VCR_EUNSUPPORTED.  The derivative calls read tgt's fields as their map and
 * ignore tgt, min_points and min_eig_ratio. */
typedef struct {
  uint32_t struct_bytes;        /* sizeof(vcr_ndt_map_args) as the CALLER was compiled (see vcr_fps_args); every field is
                                   mandatory: anything but this library's size is VCR_EINVAL */
  const float* tgt;             /* [B,3,Nt] channels-first fp32, contiguous */
  int B, Nt;
  float resolution;             /* the voxel's edge */
  int min_points;               /* >= 3 (PCL: 6) */
  double min_eig_ratio;         /* in (0, 1] (PCL: 0.01) */
  double* mean;                 /* [B,3,Nt] */
  double* inv_cov;              /* [B,6,Nt] */
  int* valid;                   /* [B,Nt] */
  int* count;                   /* [B] */
  int* voxel_points;            /* [B,Nt] */
  double* origin;               /* [B,3] */
  uint64_t* table_keys;         /* [B, vcr_ndt_table_slots(Nt)] */
  int* table_vals;              /* [B, vcr_ndt_table_slots(Nt)] */
} vcr_ndt_map_args;

/* 2^ceil(log2(2 Nt + 2)): the slots a cloud of Nt points reserves; 0 for Nt outside 1 ... 131 072. */
int    vcr_ndt_table_slots(int Nt);

/* With up(v) = v rounded up to a multiple of 256:  up(12 B Nt) + 2 up(4 B Nt) + vcr_voxel_sort_workspace_bytes (the means
 * the grid rounds to fp32, the member lists and where each voxel's begin, and the sort's own); 0 for arguments the call would
 * refuse; cu_count >= 0 is accepted and ignored. */
size_t vcr_ndt_map_workspace_bytes(const vcr_ndt_map_args*, int cu_count);
/* Asynchronous on the stream: no host synchronisation, no allocation; the sort's launches and three more.  workspace: device
 * memory, 16-B aligned, at least _workspace_bytes (VCR_EWORKSPACE below that); its contents need not be initialised.  Every
 * slot of every output is written. */
int    vcr_ndt_map_f32(const vcr_ndt_map_args*, void* workspace, size_t workspace_bytes, vcr_stream_t);
/* Host-only: lanes per voxel (1) and the table slots per cloud. */
int    vcr_ndt_map_form(const vcr_ndt_map_args*, int cu_count, int* lanes_per_voxel, int* table_slots);

/* B, Ns < 1 (B is the map's), a missing src, neighbors not 1 or 7, d1 or d2 not finite or d2 <= 0, one of R and t without the
 * other, a variant outside 0 ... 1, max_iterations or max_trials < 0, an epsilon negative or NaN: VCR_EINVAL.  Ns > 131 072 or
 * B * Ns >= 2^31: VCR_EUNSUPPORTED.  _derivatives_ needs score, hits, g and H and ignores what follows H; vcr_ndt_f32 needs
 * R_out and t_out and takes every other output as optional. */
typedef struct {
  uint32_t struct_bytes;        /* sizeof(vcr_ndt_args) as the CALLER was compiled; the mandatory part ends behind H: 0, shorter
                                   than that or longer than this library knows: VCR_EINVAL */
  const float* src;             /* [B,3,Ns] channels-first fp32, contiguous */
  int Ns;
  const float* R; const float* t;   /* [B,3,3], [B,3]; both NULL = the identity */
  int neighbors;                /* 1 or 7 */
  double d1, d2;
  int variant;                  /* 0 = the plan decides; 1 forces a lane per point, the one form built: every form returns the
                                   same bits */
  double* e_stage;              /* optional [B,Ns,7]: e per (point, cell) in cell order, NaN where no valid voxel was read */
  int* voxel_stage;             /* optional [B,Ns,7]: the valid voxel read, -1 where none */
  double* score;                /* [B]: f */
  int* hits;                    /* [B] */
  double* g;                    /* [B,6] */
  double* H;                    /* [B,21]: the upper triangle by rows */
  int max_iterations;           /* accepted steps */
  int max_trials;               /* rounds behind round 0 */
  double rot_epsilon, trans_epsilon;
  float* R_out; float* t_out;   /* [B,3,3], [B,3] */
  float* R_ba; float* t_ba;     /* optional: the inverse, as vcr_refine_f32's */
  double* probability;          /* optional [B] */
  int* iterations; int* trials; int* converged; int* status;   /* optional [B] each */
  double* trace;                /* optional [B, max_trials + 1] */
} vcr_ndt_args;

/* With nblk = ceil(Ns / 256):  up(VCR_NDT_STATE_BYTES B) + up(8 VCR_NDT_VALUES B nblk), the same for both calls; 0 for arguments
 * the call would refuse; with an explicit cu_count nothing touches a device (the form does not depend on it). */
size_t vcr_ndt_derivatives_workspace_bytes(const vcr_ndt_map_args*, const vcr_ndt_args*, int cu_count);
size_t vcr_ndt_workspace_bytes(const vcr_ndt_map_args*, const vcr_ndt_args*, int cu_count);
/* Asynchronous on the stream: no host synchronisation, no allocation, no atomic.  Three launches (_derivatives_);
 * 2 (max_trials + 1) + 2 (vcr_ndt_f32), whose shapes depend on (B, Ns) alone: the launches of a stopped cloud return at once. */
int    vcr_ndt_derivatives_f32(const vcr_ndt_map_args*, const vcr_ndt_args*, void* workspace, size_t workspace_bytes, vcr_stream_t);
int    vcr_ndt_f32(const vcr_ndt_map_args*, const vcr_ndt_args*, void* workspace, size_t workspace_bytes, vcr_stream_t);
/* Host-only: lanes per point (1), nblk, and the launches the call enqueues. */
int    vcr_ndt_derivatives_form(const vcr_ndt_map_args*, const vcr_ndt_args*, int cu_count, int* lanes_per_point, int* nblk, int* launches);
int    vcr_ndt_form(const vcr_ndt_map_args*, const vcr_ndt_args*, int cu_count, int* lanes_per_point, int* nblk, int* launches);

#ifdef __cplusplus
}
#endif
#endif

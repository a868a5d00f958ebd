/*
 * vcr_hip_orient.h -- consistent orientation of a cloud's normals: the tangent-plane propagation of
 * Hoppe et al. 1992, Open3D's orient_normals_consistent_tangent_plane, on a fixed-width neighbour list.  An extension of
 * vcr_hip.h (same library, same conventions, same error codes); it adds no symbol to that header or to its other extensions and
 * moves none of their layouts, so VCR_ABI_VERSION is unchanged.
 *
 * Per cloud b:
 *   xyz          float [B,3,N] channels-first (the reference point's rule reads z alone)
 *   normals      float [B,3,N] channels-first; they need not be unit vectors
 *   idx          int32 [B,N,k]: row i lists neighbours of point i, as vcr_grid_knn_f32 or vcr_knn_f32 write them; any caller may
 *                build them
 *
 * The definition, free of any order and exact to the bit:
 *   graph        an undirected edge {i, j} wherever j is in row i or i is in row j.  An entry equal to i or outside [0, N) is
 *                IGNORED.  Rows need not be symmetric: the closure is the definition.  An index listed twice is one edge
 *   weight       d = fmaf(nz_i, nz_j, fmaf(ny_i, ny_j, nx_i * nx_j)) in fp32 -- the same bits from either end --, w = 1 - |d|
 *                in fp32 where that is above 0, else 0; a d that is not finite gives w = 1.0f.  So 0 <= w <= 1
 *   reverses     the edge reverses iff d is finite and d < 0 (a NaN, an infinity and -0.0 do not reverse)
 *   order        of edges: (w, lo, hi) with lo = min(i, j), hi = max(i, j), strict and total.  The bits of a float in [0, 1]
 *                are below 2^30 and an index is below 2^17, so (bits of w) << 34 | lo << 17 | hi is ONE 64-bit key with
 *                exactly this order
 *   forest       the minimum spanning forest of the graph under that order; the order is strict, so it is unique
 *   reference    per tree the member with the largest z, the lowest index among equals; -0.0 equals 0.0, and a z that is not
 *                finite ranks below every finite one (equal among themselves)
 *   flip         flip[v] = (the number of reversing edges on the tree path from v to its tree's reference, mod 2) XOR
 *                (nz[reference] < 0; a NaN and -0.0 are not below 0): Open3D's rule, the top point looks up
 *   oriented     n where flip is 0, and n with the sign bit of each of its three components inverted where it is 1
 *   ref          the reference point of v's tree;  n_trees: the number of trees
 * The result is a function of the inputs alone: every B, every batch and every launch form return the same bits, and every
 * slot of every output is written.  A kNN graph may be disconnected; each tree is then oriented on its own (Open3D adds the
 * edges of a Delaunay triangulation to connect it; this library does not).
 *
 * vcr_orient_tangent_f32 is asynchronous on the stream: no host synchronisation, no allocation.  Boruvka's rounds on the packed
 * keys: every round each tree takes the least edge that leaves it (a 64-bit atomic minimum per tree, fed from both ends of every
 * edge), hooks its root under the other tree's (of two trees that chose the same edge the lower root stays) and every vertex is
 * pointed at its new root, with the parity of the reversing edges on the way, by path halving.  ceil(log2 N) rounds of three
 * launches are enqueued; a device flag lets the launches behind the last round that hooked anything return at once.
 *
 * Launch forms (variant): 0 = the plan decides, VCR_ORIENT_ROUNDS = every round three launches (serves every N; today the
 * plan's answer everywhere), VCR_ORIENT_ONE_LAUNCH = all rounds in one launch, a workgroup a cloud: NOT BUILT, it returns
 * VCR_EUNSUPPORTED.
 */
#ifndef VCR_HIP_ORIENT_H
#define VCR_HIP_ORIENT_H

#include "../vcr_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VCR_ORIENT_MAX_N 131072
#define VCR_ORIENT_ROUNDS 1
#define VCR_ORIENT_ONE_LAUNCH 2

/* B < 1, k < 1, a missing mandatory pointer (flip, ref and n_trees are optional), a variant other than 0, VCR_ORIENT_ROUNDS or
 * VCR_ORIENT_ONE_LAUNCH, a bad struct_bytes, a workspace that is NULL, short or not 256-B aligned: VCR_EINVAL.  N outside
 * [1, 131 072], B * N >= 2^31, B * N * k >= 2^31 or variant VCR_ORIENT_ONE_LAUNCH: VCR_EUNSUPPORTED. */
typedef struct {
  uint32_t struct_bytes;        /* sizeof(vcr_orient_tangent_args) as the CALLER was compiled (see vcr_fps_args); the mandatory
                                   part ends behind oriented: 0, shorter than that or longer than this library knows: VCR_EINVAL */
  const float* xyz;             /* [B,3,N] channels-first */
  const float* normals;         /* [B,3,N] channels-first */
  const int* idx;               /* [B,N,k] */
  int B, N, k;
  int variant;                  /* 0 = the plan decides; VCR_ORIENT_ROUNDS / VCR_ORIENT_ONE_LAUNCH force a form */
  float* oriented;              /* out [B,3,N]; it may alias nothing */
  int* flip;                    /* optional out [B,N]: 1 where the normal was negated, else 0 */
  int* ref;                     /* optional out [B,N]: the reference point of the point's tree */
  int* n_trees;                 /* optional out [B] */
} vcr_orient_tangent_args;

/* 0 for arguments vcr_orient_tangent_f32 refuses.  cu_count is accepted and not used today (>= 0). */
size_t vcr_orient_tangent_workspace_bytes(const vcr_orient_tangent_args*, int cu_count);
int vcr_orient_tangent_f32(const vcr_orient_tangent_args*, void* workspace, size_t workspace_bytes, vcr_stream_t);

#ifdef __cplusplus
}
#endif
#endif

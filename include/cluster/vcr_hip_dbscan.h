/*
 * vcr_hip_dbscan.h -- density clustering over neighbourhoods given as ragged rows: DBSCAN as the
 * connected components of the core points' graph, on the CSR rows vcr_grid_radius_f32 writes (vcr_hip_radius.h), and the
 * compaction of a cloud to its largest cluster.  An extension of vcr_hip.h (same library, same conventions, same error codes); it
 * adds no symbol to that header or to its other extensions and moves none of their layouts, so VCR_ABI_VERSION is unchanged.
 *
 * The rows are those of vcr_hip_rows.h.  Per cloud b:
 *   idx          int32 [B,capacity]; row_start int64 [B,N+1]; total int64 [B] -- exactly what vcr_grid_radius_f32 writes, but any
 *                caller may build them.  Point i's row is idx[b, row_start[b,i] ... row_start[b,i+1])
 *   entry        an entry outside [0, N) or equal to i is IGNORED: it is no neighbour and does not count.  L_i is the number of
 *                row i's entries that are not ignored (an index listed twice counts twice)
 *   no radius    the kernels know no radius and re-test no distance: the row IS the neighbourhood
 *   served       cloud b is served iff 0 <= total[b] <= capacity, row_start[b,0] == 0, row_start[b,N] == total[b] and
 *                row_start[b,i] <= row_start[b,i+1] for every i.  A cloud that is not served (one vcr_grid_radius_f32 left as
 *                -1s because it did not fit, say) comes back with every label -2, n_clusters -1, every core flag and every size 0;
 *                no idx entry of it is read.  The other clouds of the batch are unaffected
 *
 * The definition, free of any order:
 *   core         i is a core point iff L_i + 1 >= min_points (the point counts itself, as in Open3D's cluster_dbscan and
 *                scikit-learn's min_samples) and, where xyz is given, its three coordinates are finite
 *   clusters     the connected components of the undirected graph with an edge {i, j} whenever i is core, j is in row i and j is
 *                core.  Rows need not be symmetric: the closure is the definition.  The component whose lowest index is the c-th
 *                smallest among all components' lowest indices has label c, from 0; n_clusters is their number
 *   border       a point that is not core takes the smallest label among the core entries of ITS OWN row, -1 (noise) if it has
 *                none; a point with a non-finite coordinate is always -1
 * On symmetric rows this is the sequential algorithm of Open3D and scikit-learn (seeds in index order, every cluster expanded
 * fully before the next: a border point two clusters reach goes to the lower label).  The result is a function of the rows
 * alone: every B, every launch form and every batch returns the same bits, and every slot of every output is written.
 *
 * vcr_rows_dbscan_f32 is asynchronous on the stream: no host synchronisation, no allocation.  Eight launches: the check of
 * row_start (two), the core flags, the hook (a lock-free union-find whose roots are the components' lowest indices), the flatten,
 * the ordered rank of the roots (two), and the labels.
 *
 * Launch forms.  The three passes that walk rows (core flags, hook, labels) have two forms that return the same bits:
 *   VCR_DBSCAN_LANE   a lane a row
 *   VCR_DBSCAN_WAVE   a wave a row: the row's entries are dealt to the wave's 64 lanes; the count and the border minimum are
 *                     wave reductions of integers
 * vcr_rows_dbscan_form decides from the row length the host can see without a synchronisation, est = capacity / N: the core
 * flags and the hook take the wave form where est >= VCR_DBSCAN_WAVE_HOOK, the labels where est >= VCR_DBSCAN_WAVE_LABEL;
 * variant forces either form for all three.  As measured the hook's wave form won only where the
 * lane form has too few waves to hide its loads -- one cloud of 131 072 points with about 12 entries a row, x1.2-x1.7 -- and lost
 * up to 30 times on rows of 100 entries (64 lanes hooking into one tree at once); the labels' wave form won nowhere.  Both
 * thresholds lie above every row the limits allow and only variant reaches the wave forms.
 *
 * vcr_cluster_largest_f32 keeps the members of the cluster with the most points (sizes' largest slot, the lowest label among
 * equals), compacted in ascending index order by the outlier filters' tail: the (points, count, index) of vcr_hip_outlier.h.  A
 * cloud whose sizes are all 0 or less (no cluster, or not served) gives count 0.
 */
#ifndef VCR_HIP_DBSCAN_H
#define VCR_HIP_DBSCAN_H

#include "../vcr_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VCR_DBSCAN_MAX_N 131072
#define VCR_DBSCAN_LANE 1
#define VCR_DBSCAN_WAVE 2
#define VCR_DBSCAN_WAVE_HOOK 131072       /* est at and above which the core flags and the hook take the wave form: no row is that
                                             long -- the form lost wherever rows are long */
#define VCR_DBSCAN_WAVE_LABEL 131072      /* ... and the labels: its wave form won no measurement */
#define VCR_DBSCAN_NOISE (-1)
#define VCR_DBSCAN_NOT_SERVED (-2)

/* B < 1, a missing mandatory pointer (idx may be NULL where capacity == 0; xyz, core and sizes are optional), capacity < 0,
 * min_points < 1, a variant other than 0, VCR_DBSCAN_LANE or VCR_DBSCAN_WAVE, a bad struct_bytes, a workspace that is NULL,
 * short or not 256-B aligned: VCR_EINVAL.  N outside [1, 131 072], B * N >= 2^31 or B * capacity >= 2^31: VCR_EUNSUPPORTED. */
typedef struct {
  uint32_t struct_bytes;        /* sizeof(vcr_rows_dbscan_args) as the CALLER was compiled (see vcr_fps_args); the mandatory part
                                   ends behind n_clusters: 0, shorter than that or longer than this library knows: VCR_EINVAL */
  const float* xyz;             /* optional [B,3,N] channels-first: the finiteness rule alone reads it */
  const int* idx;               /* [B,capacity] */
  const int64_t* row_start;     /* [B,N+1] */
  const int64_t* total;         /* [B] */
  int B, N, capacity;
  int min_points;               /* >= 1 */
  int variant;                  /* 0 = vcr_rows_dbscan_form decides; VCR_DBSCAN_LANE / VCR_DBSCAN_WAVE force a form */
  int* labels;                  /* out [B,N]: the cluster, -1 noise, -2 not served */
  int* n_clusters;              /* out [B]: -1 not served */
  int* core;                    /* optional out [B,N]: 1 / 0 */
  int* sizes;                   /* optional out [B,N]: slot c the members of cluster c, border points included; 0 behind n_clusters */
} vcr_rows_dbscan_args;

/* 0 for arguments vcr_rows_dbscan_f32 refuses.  cu_count is accepted and not used today (>= 0). */
size_t vcr_rows_dbscan_workspace_bytes(const vcr_rows_dbscan_args*, int cu_count);
int vcr_rows_dbscan_f32(const vcr_rows_dbscan_args*, void* workspace, size_t workspace_bytes, vcr_stream_t);
/* Host-only query (nothing is launched), the one place that decides: the form of the hook (and the core flags) and of the labels.
 * The pointers of the args are not looked at.  cu_count < 0: VCR_EINVAL.  Either result pointer may be NULL. */
int vcr_rows_dbscan_form(const vcr_rows_dbscan_args*, int cu_count, int* hook_form, int* label_form);

/* B < 1, a missing pointer (index is optional), a bad struct_bytes, a workspace that is NULL, short or not 256-B aligned: VCR_EINVAL.
 * N outside [1, 131 072] or B * N >= 2^31: VCR_EUNSUPPORTED. */
typedef struct {
  uint32_t struct_bytes;        /* the mandatory part ends behind count */
  const float* xyz;             /* [B,3,N] channels-first */
  const int* labels;            /* [B,N] as vcr_rows_dbscan_f32 wrote them */
  const int* sizes;             /* [B,N] likewise */
  int B, N;
  float* points;                /* out [B,3,N]: the kept points in ascending index order, NaN behind them */
  int* count;                   /* out [B] */
  int* index;                   /* optional out [B,N]: the kept points' indices, -1 behind them */
} vcr_cluster_largest_args;

size_t vcr_cluster_largest_workspace_bytes(const vcr_cluster_largest_args*, int cu_count);
int vcr_cluster_largest_f32(const vcr_cluster_largest_args*, void* workspace, size_t workspace_bytes, vcr_stream_t);

#ifdef __cplusplus
}
#endif
#endif

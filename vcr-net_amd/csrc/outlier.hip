// Removing a cloud's stray points (include/vcr_hip_outlier.h): Open3D's statistical and radius outlier
// filters.  Both decide a keep flag per point and end in the same tail, which compacts the kept points in ascending order.
//
// vcr_outlier_stat_f32, seven launches (the neighbours are the caller's: no search):
//   outlier_dist_kernel     one lane per point: its k neighbours' rows (one 16-B load each, the index checked against [0, N)
//                           first), the fp64 distances summed in idx's order, mean_dist; per 256 points the (count, sum) of the
//                           valid ones in sum_d2's order
//   outlier_mu_kernel       one workgroup per cloud: the partials ascending, n and mu
//   outlier_dev_kernel      one lane per point: the squared deviation from mu, one partial per 256 points in the same order
//   outlier_sigma_kernel    one workgroup per cloud: var, sigma, thr
//   outlier_mark_kernel     one lane per point: keep, one count of them per 256 points (ballot + popcount)
//   outlier_offsets_kernel  one workgroup per cloud: the exclusive scan of those counts, count[b]
//   outlier_write_kernel    one lane per point writes ONE slot of points / index: a kept point its own (the block's offset + its
//                           rank among the block's kept), a dropped one the padding of slot count + (its rank among the dropped)
// vcr_outlier_radius_f32, four launches (the scan is cut as nn_plan cuts (B, N, N); vcr_outlier_radius_args.variant forces S):
//   outlier_count_kernel    nn_scan_kernel<1>'s structure (nn_scan.h) on the cloud against itself: tiles of NN_TILE points
//                           through three LDS planes, a NaN tail, broadcast ds_read_b128; per pair the distance, one compare and
//                           one add; a count per (segment, point)
//   outlier_merge_kernel    one lane per point: the S counts added (integers: any S gives the same bits), c_i, keep, the count
//                           of kept per 256 points
//   outlier_offsets_kernel, outlier_write_kernel   as above
// The tail -- mark, offsets, write -- lives in outlier_tail.h, which radius.hip includes too (the radius filter on the grid).
// No atomics, no scratch, no loop whose trip count depends on anything but N, k, S and a tile index.
#include "outlier_tail.h"
#include "outlier_flags.h"

namespace {

typedef float f32x2 __attribute__((ext_vector_type(2)));

struct OlDist {
  const float* xyz4; const int* idx; int N, k, nblk;
  float* mean; float* mean_out;                            // [B][N]: the workspace's plane, the optional output
  double* psum; int* pcnt;                                 // [B][nblk]
};

__global__ __launch_bounds__(NN_BLOCK) void outlier_dist_kernel(OlDist p) {
  __shared__ double wsum[NN_BLOCK / 64];
  __shared__ int wcnt[NN_BLOCK / 64];
  const int t = threadIdx.x;
  const int b = (int)(blockIdx.x / (unsigned)p.nblk), blk = (int)(blockIdx.x % (unsigned)p.nblk);
  const int i = blk * NN_BLOCK + t, N = p.N, k = p.k;
  double v = 0.;
  int c = 0;
  if (i < N) {
    const size_t o = (size_t)b * N + i;
    const float* rows = p.xyz4 + (size_t)b * N * 4;
    const int* nb = p.idx + o * k;
    const f32x4 me = ld4(rows + (size_t)i * 4);
    double s = 0.;
#pragma unroll 4
    for (int j = 0; j < k; ++j) {
      int r = nb[j];
      r = (unsigned)r < (unsigned)N ? r : i;               // an entry outside [0, N) reads as the row itself
      const f32x4 q = ld4(rows + (size_t)r * 4);
      const double dx = (double)(q[0] - me[0]), dy = (double)(q[1] - me[1]), dz = (double)(q[2] - me[2]);
      s += sqrt((dx * dx + dy * dy) + dz * dz);
    }
    const float m = (float)(s / (double)(k + 1));
    p.mean[o] = m;
    if (p.mean_out) p.mean_out[o] = m;
    if (ol_finite(m)) { v = (double)m; c = 1; }
  }
  double sum = 0.;
  int cnt = 0;
  wg_sum_count(v, c, t, wsum, wcnt, &sum, &cnt);
  if (t == 0) { p.psum[(size_t)b * p.nblk + blk] = sum; p.pcnt[(size_t)b * p.nblk + blk] = cnt; }
}

__global__ __launch_bounds__(NN_BLOCK) void outlier_mu_kernel(const double* psum, const int* pcnt, int nblk, OlStat* st) {
  __shared__ double ls[NN_BLOCK];
  __shared__ int lc[NN_BLOCK];
  const int t = threadIdx.x, b = blockIdx.x;
  double sum = 0.;
  int n = 0;
  psum += (size_t)b * nblk; pcnt += (size_t)b * nblk;
  wg_fold(nblk, [&](int i, double* s, int* c) { *s = psum[i]; *c = pcnt[i]; }, t, ls, lc, &sum, &n);
  if (t == 0) {
    st[b].n = n;
    st[b].mu = sum / (double)n;                            // (n = 0: 0 / 0, the NaN the header promises)
  }
}

struct OlDev { const float* mean; const OlStat* st; int N, nblk; double* pdev; };

__global__ __launch_bounds__(NN_BLOCK) void outlier_dev_kernel(OlDev p) {
  __shared__ double wsum[NN_BLOCK / 64];
  __shared__ int wcnt[NN_BLOCK / 64];
  const int t = threadIdx.x;
  const int b = (int)(blockIdx.x / (unsigned)p.nblk), blk = (int)(blockIdx.x % (unsigned)p.nblk);
  const int i = blk * NN_BLOCK + t;
  double v = 0.;
  if (i < p.N) {
    const float m = p.mean[(size_t)b * p.N + i];
    if (ol_finite(m)) {
      const double dev = (double)m - p.st[b].mu;
      v = dev * dev;
    }
  }
  double sum = 0.;
  int cnt = 0;
  wg_sum_count(v, 0, t, wsum, wcnt, &sum, &cnt);
  if (t == 0) p.pdev[(size_t)b * p.nblk + blk] = sum;
}

__global__ __launch_bounds__(NN_BLOCK) void outlier_sigma_kernel(const double* pdev, int nblk, float std_ratio, OlStat* st,
                                                                 int* valid, double* stats) {
  __shared__ double ls[NN_BLOCK];
  __shared__ int lc[NN_BLOCK];
  const int t = threadIdx.x, b = blockIdx.x;
  double sum = 0.;
  int unused = 0;
  pdev += (size_t)b * nblk;
  wg_fold(nblk, [&](int i, double* s, int* c) { *s = pdev[i]; *c = 0; }, t, ls, lc, &sum, &unused);
  if (t == 0) {
    const int n = st[b].n;
    const double mu = st[b].mu;
    const double var = sum / (double)(n - 1);
    const double sigma = n < 2 ? 0. : sqrt(var);
    const double thr = mu + (double)std_ratio * sigma;
    st[b].var = var; st[b].sigma = sigma; st[b].thr = thr;
    if (valid) valid[b] = n;
    if (stats) { stats[(size_t)b * 3] = mu; stats[(size_t)b * 3 + 1] = sigma; stats[(size_t)b * 3 + 2] = thr; }
  }
}

struct OlCount {
  const float* xyz;
  int B, N, S, seg_len, nblk;                              // nblk = ceil(N / 256)
  float r2;
  int* part;                                               // [S][B][N]
};

__global__ __launch_bounds__(NN_BLOCK) void outlier_count_kernel(OlCount p) {
  __shared__ __attribute__((aligned(16))) float lx[NN_TILE], ly[NN_TILE], lz[NN_TILE];
  const int t = threadIdx.x;
  int s, blk, b;
  seg_workgroup(blockIdx.x, p.S, p.nblk, &s, &blk, &b);
  const int N = p.N;
  const float* __restrict__ x = p.xyz + (size_t)b * 3 * N;
  const int i = blk * NN_BLOCK + t;
  const float nan = __uint_as_float(0x7FC00000u);
  const float px = i < N ? x[i] : nan, py = i < N ? x[N + i] : nan, pz = i < N ? x[2 * (size_t)N + i] : nan;
  const f32x2 qx = {px, px}, qy = {py, py}, qz = {pz, pz};
  const float r2 = p.r2;
  int c0 = 0, c1 = 0;                                      // the even and the odd points of a tile

  int lo, hi;
  seg_range(s, p.seg_len, N, &lo, &hi);
  for (int t0 = lo; t0 < hi; t0 += NN_TILE) {                          // (workgroup-uniform: the barriers are met by all)
    const int cnt = hi - t0 < NN_TILE ? hi - t0 : NN_TILE;
    const int cnt8 = (cnt + 7) & ~7;                                   // <= NN_TILE; the tail is NaN: its d2 is in no sphere
    __syncthreads();                                                   // the previous tile has been read
    for (int j = t; j < cnt8; j += NN_BLOCK) {
      const bool in = j < cnt;
      const int g = t0 + (in ? j : 0);
      lx[j] = in ? x[g] : nan;
      ly[j] = in ? x[N + g] : nan;
      lz[j] = in ? x[2 * (size_t)N + g] : nan;
    }
    __syncthreads();
    for (int j = 0; j < cnt8; j += 8) {                                // eight points a round: six reads in flight
      const f32x4 X[2] = {ld4(lx + j), ld4(lx + j + 4)}, Y[2] = {ld4(ly + j), ld4(ly + j + 4)},
                  Z[2] = {ld4(lz + j), ld4(lz + j + 4)};               // one address for every lane: broadcast reads
#pragma unroll
      for (int h = 0; h < 2; ++h) {
#pragma unroll
        for (int u = 0; u < 4; u += 2) {                               // two points a packed instruction
          const f32x2 dx = qx - f32x2{X[h][u], X[h][u + 1]}, dy = qy - f32x2{Y[h][u], Y[h][u + 1]},
                      dz = qz - f32x2{Z[h][u], Z[h][u + 1]};
          const f32x2 d2 = __builtin_elementwise_fma(dz, dz, __builtin_elementwise_fma(dy, dy, dx * dx));
          c0 += d2[0] <= r2 ? 1 : 0;
          c1 += d2[1] <= r2 ? 1 : 0;
        }
      }
    }
  }
  if (i < N) p.part[((size_t)s * p.B + b) * (size_t)N + i] = c0 + c1;
}

struct OlMerge {
  const int* part; int B, N, S, nblk, nb_points;
  int* cnt; int* neighbours; int* blkcnt;                  // [B][N], optional [B][N], [B][nblk]
};

__global__ __launch_bounds__(NN_BLOCK) void outlier_merge_kernel(OlMerge p) {
  __shared__ int wcnt[NN_BLOCK / 64];
  const int t = threadIdx.x;
  const int b = (int)(blockIdx.x / (unsigned)p.nblk), blk = (int)(blockIdx.x % (unsigned)p.nblk);
  const int i = blk * NN_BLOCK + t;
  int c = 0;
  if (i < p.N) {
    for (int s = 0; s < p.S; ++s) c += p.part[((size_t)s * p.B + b) * (size_t)p.N + i];
    const size_t o = (size_t)b * p.N + i;
    p.cnt[o] = c;
    if (p.neighbours) p.neighbours[o] = c;
  }
  int kept;
  wg_rank(i < p.N && c > p.nb_points, t, wcnt, &kept);
  if (t == 0) p.blkcnt[(size_t)b * p.nblk + blk] = kept;
}

// How a call runs: the checks, the geometry and the workspace's layout, decided in one place per entry point
struct OlStatPlan {
  vcr_outlier_stat_args a;
  int nblk;
  unsigned point_grid;
  size_t st_off, psum_off, pdev_off, pcnt_off, blk_off, bytes;        // workspace: mean | st | psum | pdev | pcnt | blkcnt
};

struct OlRadiusPlan {
  vcr_outlier_radius_args a;
  SegSplit scan;                                           // (one point per lane: its nblk is the per-point launches' too)
  unsigned point_grid;
  size_t cnt_off, blk_off, bytes;                          // workspace: part | cnt | blkcnt
};

}  // namespace

static int outlier_stat_plan(const vcr_outlier_stat_args& a, OlStatPlan* p) {
  *p = OlStatPlan{a};
  if (!a.xyz4 || !a.idx || !a.points || !a.count || a.B < 1 || a.k < 1 || (((uintptr_t)a.xyz4) & 15)) return VCR_EINVAL;
  if (!(a.std_ratio >= 0.f) || a.std_ratio == __builtin_huge_valf()) return VCR_EINVAL;     // negative, NaN, +inf
  if (a.k > VCR_OUTLIER_MAX_K || a.N < 1 || a.N > NN_MAX_N || (long)a.B * a.N >= (1L << 31)) return VCR_EUNSUPPORTED;
  p->nblk = (a.N + NN_BLOCK - 1) / NN_BLOCK;
  p->point_grid = (unsigned)((long)a.B * p->nblk);
  const size_t parts = (size_t)a.B * p->nblk;
  p->st_off = ws_up((size_t)a.B * a.N * 4);
  p->psum_off = p->st_off + ws_up((size_t)a.B * sizeof(OlStat));
  p->pdev_off = p->psum_off + ws_up(parts * 8);
  p->pcnt_off = p->pdev_off + ws_up(parts * 8);
  p->blk_off = p->pcnt_off + ws_up(parts * 4);
  p->bytes = p->blk_off + ws_up(parts * 4);
  return VCR_OK;
}

static int outlier_stat_take(const vcr_outlier_stat_args* user, vcr_outlier_stat_args* mine) {
  return vcr_take_args(user, mine, offsetof(vcr_outlier_stat_args, index));
}

extern "C" size_t vcr_outlier_stat_workspace_bytes(const vcr_outlier_stat_args* ua, int cu_count) {
  vcr_outlier_stat_args a;
  OlStatPlan p;
  if (outlier_stat_take(ua, &a) || cu_count < 0) return 0;
  return outlier_stat_plan(a, &p) ? 0 : p.bytes;
}

extern "C" int vcr_outlier_stat_f32(const vcr_outlier_stat_args* ua, void* workspace, size_t workspace_bytes,
                                    vcr_stream_t stream) {
  vcr_outlier_stat_args a;
  if (outlier_stat_take(ua, &a)) return VCR_EINVAL;
  OlStatPlan p;
  int e = outlier_stat_plan(a, &p);
  if (e) return e;
  if (!workspace || (((uintptr_t)workspace) & 15)) return VCR_EINVAL;
  if (workspace_bytes < p.bytes) return VCR_EWORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  unsigned char* w = reinterpret_cast<unsigned char*>(workspace);
  float* mean = reinterpret_cast<float*>(w);
  OlStat* st = reinterpret_cast<OlStat*>(w + p.st_off);
  double* psum = reinterpret_cast<double*>(w + p.psum_off);
  double* pdev = reinterpret_cast<double*>(w + p.pdev_off);
  int* pcnt = reinterpret_cast<int*>(w + p.pcnt_off);
  int* blk = reinterpret_cast<int*>(w + p.blk_off);
  const dim3 block(NN_BLOCK), clouds((unsigned)a.B), points(p.point_grid);

  const OlDist ds{a.xyz4, a.idx, a.N, a.k, p.nblk, mean, a.mean_dist, psum, pcnt};
  hipLaunchKernelGGL(outlier_dist_kernel, points, block, 0, s, ds);
  if ((e = VCR_LAUNCH_RC())) return e;
  hipLaunchKernelGGL(outlier_mu_kernel, clouds, block, 0, s, psum, pcnt, p.nblk, st);
  if ((e = VCR_LAUNCH_RC())) return e;
  const OlDev dv{mean, st, a.N, p.nblk, pdev};
  hipLaunchKernelGGL(outlier_dev_kernel, points, block, 0, s, dv);
  if ((e = VCR_LAUNCH_RC())) return e;
  hipLaunchKernelGGL(outlier_sigma_kernel, clouds, block, 0, s, pdev, p.nblk, a.std_ratio, st, a.valid, a.stats);
  if ((e = VCR_LAUNCH_RC())) return e;
  const OlTail tl{mean, st, nullptr, 0, a.xyz4, nullptr, a.N, p.nblk, blk, a.points, a.count, a.index};
  hipLaunchKernelGGL(outlier_mark_kernel, points, block, 0, s, tl);
  if ((e = VCR_LAUNCH_RC())) return e;
  return ol_compact(tl, a.B, p.point_grid, s);
}

// The scan is cut as nn_plan cuts B clouds of N points against themselves, one point per lane, as voxel_plan does
static int outlier_radius_plan(const vcr_outlier_radius_args& a, int cu, OlRadiusPlan* p) {
  *p = OlRadiusPlan{a};
  if (!a.xyz || !a.points || !a.count || a.B < 1 || a.nb_points < 0) return VCR_EINVAL;
  if (!(a.radius > 0.f) || a.radius == __builtin_huge_valf()) return VCR_EINVAL;             // <= 0, NaN, +inf
  int fq, fs;
  if (seg_variant(a.variant, SEG_Q_1, NN_LIMITS, &fq, &fs)) return VCR_EINVAL;
  if (a.N < 1 || a.N > NN_MAX_N || (long)a.B * a.N >= (1L << 31)) return VCR_EUNSUPPORTED;
  const int e = seg_split(a.B, a.N, a.N, 1, fs, cu, NN_LIMITS, &p->scan);
  if (e) return e;
  p->point_grid = (unsigned)((long)a.B * p->scan.nblk);
  const size_t BN = (size_t)a.B * a.N;
  p->cnt_off = ws_up((size_t)p->scan.S * BN * 4);
  p->blk_off = p->cnt_off + ws_up(BN * 4);
  p->bytes = p->blk_off + ws_up((size_t)a.B * p->scan.nblk * 4);
  return VCR_OK;
}

static int outlier_radius_take(const vcr_outlier_radius_args* user, vcr_outlier_radius_args* mine) {
  return vcr_take_args(user, mine, offsetof(vcr_outlier_radius_args, index));
}

extern "C" int vcr_outlier_radius_form(const vcr_outlier_radius_args* ua, int cu_count, int* points_per_lane, int* splits) {
  vcr_outlier_radius_args a;
  OlRadiusPlan p;
  if (outlier_radius_take(ua, &a) || cu_count < 0) return VCR_EINVAL;
  const int e = outlier_radius_plan(a, cu_count ? cu_count : vcr_cu_count(), &p);
  if (e) return e;
  if (points_per_lane) *points_per_lane = 1;
  if (splits) *splits = p.scan.S;
  return VCR_OK;
}

extern "C" size_t vcr_outlier_radius_workspace_bytes(const vcr_outlier_radius_args* ua, int cu_count) {
  vcr_outlier_radius_args a;
  OlRadiusPlan p;
  if (outlier_radius_take(ua, &a) || cu_count < 0) return 0;
  return outlier_radius_plan(a, cu_count ? cu_count : vcr_cu_count(), &p) ? 0 : p.bytes;
}

extern "C" int vcr_outlier_radius_f32(const vcr_outlier_radius_args* ua, void* workspace, size_t workspace_bytes,
                                      vcr_stream_t stream) {
  vcr_outlier_radius_args a;
  if (outlier_radius_take(ua, &a)) return VCR_EINVAL;
  // the argument checks need no device: only a call that passes them asks for the CU count
  OlRadiusPlan p;
  int e = outlier_radius_plan(a, 1, &p);
  if (e) return e;
  if (!workspace || (((uintptr_t)workspace) & 15)) return VCR_EINVAL;
  vcr_stream_scope scope_(stream);
  e = outlier_radius_plan(a, vcr_cu_count(), &p);
  if (e) return e;
  if (workspace_bytes < p.bytes) return VCR_EWORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  unsigned char* w = reinterpret_cast<unsigned char*>(workspace);
  int* part = reinterpret_cast<int*>(w);
  int* cnt = reinterpret_cast<int*>(w + p.cnt_off);
  int* blk = reinterpret_cast<int*>(w + p.blk_off);

  const OlCount sc{a.xyz, a.B, a.N, p.scan.S, p.scan.seg_len, p.scan.nblk, a.radius * a.radius, part};
  hipLaunchKernelGGL(outlier_count_kernel, dim3(p.scan.grid), dim3(NN_BLOCK), 0, s, sc);
  if ((e = VCR_LAUNCH_RC())) return e;
  const OlMerge mg{part, a.B, a.N, p.scan.S, p.scan.nblk, a.nb_points, cnt, a.neighbours, blk};
  hipLaunchKernelGGL(outlier_merge_kernel, dim3(p.point_grid), dim3(NN_BLOCK), 0, s, mg);
  if ((e = VCR_LAUNCH_RC())) return e;
  const OlTail tl{nullptr, nullptr, cnt, a.nb_points, nullptr, a.xyz, a.N, p.scan.nblk, blk, a.points, a.count, a.index};
  return ol_compact(tl, a.B, p.point_grid, s);
}

// The tail alone, on keep flags the caller computed (outlier_flags.h): a flag is a count held against nb_points = 0
int outlier_compact_flags(const int* flags, const float* xyz, int B, int N, int* blkcnt, float* points, int* count, int* index,
                          hipStream_t s) {
  const int nblk = (N + NN_BLOCK - 1) / NN_BLOCK;
  const unsigned point_grid = (unsigned)((long)B * nblk);
  const OlTail tl{nullptr, nullptr, flags, 0, nullptr, xyz, N, nblk, blkcnt, points, count, index};
  hipLaunchKernelGGL(outlier_mark_kernel, dim3(point_grid), dim3(NN_BLOCK), 0, s, tl);
  const int e = VCR_LAUNCH_RC();
  return e ? e : ol_compact(tl, B, point_grid, s);
}

// The dominant plane of a cloud by RANSAC and the split along it (include/segment/vcr_hip_segment.h): Open3D's
// segment_plane with ransac_n = 3, every trial run.  No host synchronisation:
//   plane_mark / plane_offsets / plane_gather   the candidates (finite, mask != 0), ascending, gathered ONCE into contiguous 16-B
//                          rows (x, y, z, index): a count per 256 points (ballot + popcount), their exclusive scan, the rows
//   plane_trial_kernel     a lane a trial: corr_pairs.h's draws, the fp64 cross product, status, n32 and p0; count 0 (or -1)
//   plane_count_*_kernel   THE hot path, T x M tests of six instructions, in two forms (the header): a lane a trial over a range
//                          of candidates that arrive through scalar loads, or a lane four candidates over 64 trials whose values
//                          arrive through scalar loads.  Integer atomic adds onto the trial kernel's zeros: exact in any order
//   plane_best_kernel      ransac_best_kernel's 64-bit key, a workgroup a cloud
//   plane_flags_kernel     a lane a point: the winner's inlier flag, and the block's nine fp64 sums in the header's order
//   plane_refit_kernel     a workgroup a cloud: the blocks' sums ascending, then one lane's Jacobi (normals_point.h) and the outputs
//   plane_invert_kernel    the split's second set of keep flags; both sides go through outlier.hip's tail (outlier_flags.h)
// Every result is a function of the cloud alone; no kernel waits for another workgroup.
#include "corr_pairs.h"
#include "normals_point.h"
#include "outlier_flags.h"
#include "../../include/segment/vcr_hip_segment.h"

namespace {

constexpr int SG_BLOCK = RS_BLOCK;                         // 256: wg_scan.h's workgroup
constexpr int SG_PP = VCR_PLANE_POINT_PER_LANE;
constexpr int SG_TILE = SG_BLOCK * SG_PP;                  // candidates a workgroup of the POINT form holds at a time

__device__ __forceinline__ bool sg_finite(float v) { return fabsf(v) < __builtin_huge_valf(); }

struct SgCand {
  const float* xyz; const int* mask; int N, nblk;
  int* blkcnt;                                             // [B][nblk]: counts, then (in place) their exclusive scan
  float* rows;                                             // [B][N][4]
  int* M;                                                  // [B]
  int* candidates;                                         // optional [B]
};

__device__ __forceinline__ bool sg_candidate(const SgCand& p, int b, int i, f32x4* row) {
  if (i >= p.N) return false;
  const float* pl = p.xyz + (size_t)b * 3 * p.N;
  const float x = pl[i], y = pl[p.N + i], z = pl[2 * (size_t)p.N + i];
  *row = f32x4{x, y, z, __int_as_float(i)};
  return sg_finite(x) && sg_finite(y) && sg_finite(z) && (!p.mask || p.mask[(size_t)b * p.N + i] != 0);
}

__global__ __launch_bounds__(SG_BLOCK) void plane_mark_kernel(SgCand p) {
  __shared__ int wcnt[WG_WAVES];
  const int t = threadIdx.x;
  const int b = (int)(blockIdx.x / (unsigned)p.nblk), blk = (int)(blockIdx.x % (unsigned)p.nblk);
  f32x4 row;
  int kept;
  wg_rank(sg_candidate(p, b, blk * SG_BLOCK + t, &row), t, wcnt, &kept);
  if (t == 0) p.blkcnt[(size_t)b * p.nblk + blk] = kept;
}

__global__ __launch_bounds__(SG_BLOCK) void plane_offsets_kernel(SgCand p) {
  __shared__ int wtot[WG_WAVES];
  const int b = blockIdx.x;
  const int M = wg_offsets(p.blkcnt + (size_t)b * p.nblk, p.nblk, wtot);
  if (threadIdx.x == 0) {
    p.M[b] = M;
    if (p.candidates) p.candidates[b] = M;
  }
}

__global__ __launch_bounds__(SG_BLOCK) void plane_gather_kernel(SgCand p) {
  __shared__ int wcnt[WG_WAVES];
  const int t = threadIdx.x;
  const int b = (int)(blockIdx.x / (unsigned)p.nblk), blk = (int)(blockIdx.x % (unsigned)p.nblk);
  f32x4 row;
  const bool has = sg_candidate(p, b, blk * SG_BLOCK + t, &row);
  int kept;
  const int rank = wg_rank(has, t, wcnt, &kept);
  if (has)                                                 // the block's offset + the rank: < M <= N
    st4(p.rows + ((size_t)b * p.N + p.blkcnt[(size_t)b * p.nblk + blk] + rank) * 4, row);
}

struct SgWork {                                            // per cloud b (status, plane and count: the caller's where given)
  const float* rows;                                       // [B][N][4]
  const int* M;                                            // [B]
  int* status;                                             // [B][T]
  float* plane;                                            // [B][T][8]
  int* count;                                              // [B][T]
  int N, T;
};

struct SgTrial { SgWork w; unsigned seed; int* picks; };

__global__ __launch_bounds__(SG_BLOCK) void plane_trial_kernel(SgTrial p) {
  const unsigned per = (unsigned)((p.w.T + SG_BLOCK - 1) / SG_BLOCK);
  const int b = (int)(blockIdx.x / per);
  const int trial = (int)((blockIdx.x % per) * SG_BLOCK + threadIdx.x);
  if (trial >= p.w.T) return;
  const int M = p.w.M[b];
  const float* rows = p.w.rows + (size_t)b * p.w.N * 4;
  const size_t slot = (size_t)b * p.w.T + trial;
  int status = 0, pick[3] = {-1, -1, -1};
  f32x4 q[3];
  if (M < 1) {
    status = 1;
  } else {
    unsigned at[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      at[j] = rs_pick(p.seed, trial, j, M);                // < M
      q[j] = ld4(rows + (size_t)at[j] * 4);
      pick[j] = __float_as_int(q[j][3]);
    }
    if (at[0] == at[1] || at[0] == at[2] || at[1] == at[2]) status = 1;
  }
  f32x4 nrm = {0.f, 0.f, 0.f, 0.f}, org = {0.f, 0.f, 0.f, 0.f};
  if (status == 0) {
    const double ax = (double)(q[1][0] - q[0][0]), ay = (double)(q[1][1] - q[0][1]), az = (double)(q[1][2] - q[0][2]);
    const double bx = (double)(q[2][0] - q[0][0]), by = (double)(q[2][1] - q[0][1]), bz = (double)(q[2][2] - q[0][2]);
    const double nx = ay * bz - az * by, ny = az * bx - ax * bz, nz = ax * by - ay * bx;     // the products are exact
    const double nn = (nx * nx + ny * ny) + nz * nz;
    const double aa = (ax * ax + ay * ay) + az * az, bb = (bx * bx + by * by) + bz * bz;
    if (nn > 0x1p-40 * (aa * bb)) {                        // a NaN fails
      const double len = sqrt(nn);
      nrm = f32x4{(float)(nx / len), (float)(ny / len), (float)(nz / len), 0.f};
      org = f32x4{q[0][0], q[0][1], q[0][2], 0.f};
    } else {
      status = 2;
    }
  }
  p.w.status[slot] = status;
  st4(p.w.plane + slot * 8, nrm);
  st4(p.w.plane + slot * 8 + 4, org);
  p.w.count[slot] = status == 0 ? 0 : -1;                  // the zero the count kernels add onto
  if (p.picks)
#pragma unroll
    for (int j = 0; j < 3; ++j) p.picks[slot * 3 + j] = pick[j];
}

// the header's `distance` and `inlier`
__device__ __forceinline__ bool sg_inlier(float nx, float ny, float nz, float ox, float oy, float oz, float x, float y, float z,
                                          float thr) {
  const float rx = x - ox, ry = y - oy, rz = z - oz;
  return fabsf(fmaf(nz, rz, fmaf(ny, ry, nx * rx))) <= thr;
}

struct SgCount { SgWork w; float thr; int splits; };

// the range of candidates split s of cloud b walks: [lo, hi)
__device__ __forceinline__ void sg_range(int M, int splits, int s, int* lo, int* hi) {
  const int len = (M + splits - 1) / splits;               // splits <= 512, M <= 131 072: no overflow
  *lo = s * len < M ? s * len : M;
  *hi = *lo + len < M ? *lo + len : M;
}

// TRIAL form: grid = B x ceil(T / 256) x splits
__global__ __launch_bounds__(SG_BLOCK) void plane_count_trial_kernel(SgCount p) {
  const unsigned tiles = (unsigned)((p.w.T + SG_BLOCK - 1) / SG_BLOCK);
  const int s = (int)(blockIdx.x % (unsigned)p.splits);
  const int tile = (int)((blockIdx.x / (unsigned)p.splits) % tiles);
  const int b = (int)(blockIdx.x / ((unsigned)p.splits * tiles));
  const int trial = tile * SG_BLOCK + (int)threadIdx.x;
  int lo, hi;
  sg_range(p.w.M[b], p.splits, s, &lo, &hi);
  if (trial >= p.w.T) return;
  const size_t slot = (size_t)b * p.w.T + trial;
  if (p.w.status[slot] != 0) return;
  const f32x4 nrm = ld4(p.w.plane + slot * 8), org = ld4(p.w.plane + slot * 8 + 4);
  const float* __restrict__ rows = p.w.rows + (size_t)b * p.w.N * 4;      // (workgroup-uniform, like j: scalar loads)
  int count = 0;
  for (int j = lo; j < hi; ++j) {
    const float* __restrict__ r = rows + (size_t)j * 4;
    count += sg_inlier(nrm[0], nrm[1], nrm[2], org[0], org[1], org[2], r[0], r[1], r[2], p.thr) ? 1 : 0;
  }
  if (count) atomicAdd(p.w.count + slot, count);
}

// POINT form: grid = B x ceil(T / 64) x splits
__global__ __launch_bounds__(SG_BLOCK) void plane_count_point_kernel(SgCount p) {
  const unsigned tiles = (unsigned)((p.w.T + 63) / 64);
  const int s = (int)(blockIdx.x % (unsigned)p.splits);
  const int tile = (int)((blockIdx.x / (unsigned)p.splits) % tiles);
  const int b = (int)(blockIdx.x / ((unsigned)p.splits * tiles));
  const int lane = (int)(threadIdx.x & 63);
  const int t0 = tile * 64, nt = p.w.T - t0 < 64 ? p.w.T - t0 : 64;
  int lo, hi;
  sg_range(p.w.M[b], p.splits, s, &lo, &hi);
  const float* rows = p.w.rows + (size_t)b * p.w.N * 4;
  const float* __restrict__ planes = p.w.plane + ((size_t)b * p.w.T + t0) * 8;   // (workgroup-uniform, like u: scalar loads)
  const float nan = __uint_as_float(0x7FC00000u);
  int acc = 0;                                             // the count of trial t0 + lane in this wave's candidates
  for (int c0 = lo; c0 < hi; c0 += SG_TILE) {              // (workgroup-uniform)
    float x[SG_PP], y[SG_PP], z[SG_PP];
#pragma unroll
    for (int k = 0; k < SG_PP; ++k) {
      const int j = c0 + k * SG_BLOCK + (int)threadIdx.x;
      x[k] = nan; y[k] = 0.f; z[k] = 0.f;                  // a slot behind the range is nobody's inlier: its d is NaN
      if (j < hi) {
        const f32x4 r = ld4(rows + (size_t)j * 4);
        x[k] = r[0]; y[k] = r[1]; z[k] = r[2];
      }
    }
    for (int u = 0; u < nt; ++u) {
      const float* __restrict__ pl = planes + (size_t)u * 8;
      const float nx = pl[0], ny = pl[1], nz = pl[2], ox = pl[4], oy = pl[5], oz = pl[6];
      int c = 0;
#pragma unroll
      for (int k = 0; k < SG_PP; ++k) c += __popcll(__ballot(sg_inlier(nx, ny, nz, ox, oy, oz, x[k], y[k], z[k], p.thr)));
      acc += lane == u ? c : 0;
    }
  }
  const size_t slot = (size_t)b * p.w.T + t0 + lane;
  if (lane < nt && acc && p.w.status[slot] == 0) atomicAdd(p.w.count + slot, acc);
}

struct SgBest {
  SgWork w;
  int* best;                                               // [B]
  float* win;                                              // [B][8]: the winner's row of plane, zeros without one
  int* best_trial; int* count;                             // the caller's: optional, mandatory
};

__global__ __launch_bounds__(SG_BLOCK) void plane_best_kernel(SgBest p) {
  __shared__ u64 wbest[WG_WAVES];
  const int t = threadIdx.x, b = blockIdx.x;
  const int* count = p.w.count + (size_t)b * p.w.T;
  u64 key = 0;                                             // a valid trial's key is above 0xFFF00000
  for (int i = t; i < p.w.T; i += SG_BLOCK) {
    const int c = count[i];
    const u64 k = c >= 0 ? ((u64)(unsigned)c << 32) | (u64)(0xFFFFFFFFu - (unsigned)i) : 0ull;
    key = k > key ? k : key;
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    const u64 other = __shfl_xor(key, o, 64);
    key = other > key ? other : key;
  }
  if ((t & 63) == 0) wbest[t >> 6] = key;
  __syncthreads();
  if (t != 0) return;
  for (int w = 1; w < WG_WAVES; ++w) key = wbest[w] > key ? wbest[w] : key;
  int best = -1, inl = 0;
  f32x4 nrm = {0.f, 0.f, 0.f, 0.f}, org = {0.f, 0.f, 0.f, 0.f};
  if (key != 0ull) {
    best = (int)(0xFFFFFFFFu - (unsigned)(key & 0xFFFFFFFFull));
    inl = (int)(key >> 32);
    nrm = ld4(p.w.plane + ((size_t)b * p.w.T + best) * 8);
    org = ld4(p.w.plane + ((size_t)b * p.w.T + best) * 8 + 4);
  }
  p.best[b] = best;
  st4(p.win + (size_t)b * 8, nrm);
  st4(p.win + (size_t)b * 8 + 4, org);
  p.count[b] = inl;
  if (p.best_trial) p.best_trial[b] = best;
}

struct SgFlags {
  const float* xyz; const int* mask; int N, nblk; float thr;
  const int* best; const float* win;
  int* inlier;                                             // [B][N]
  double* part;                                            // [B][nblk][9]
};

__global__ __launch_bounds__(SG_BLOCK) void plane_flags_kernel(SgFlags p) {
  __shared__ double wsum[WG_WAVES][9];
  const int t = threadIdx.x;
  const int b = (int)(blockIdx.x / (unsigned)p.nblk), blk = (int)(blockIdx.x % (unsigned)p.nblk);
  const int i = blk * SG_BLOCK + t;
  const f32x4 nrm = ld4(p.win + (size_t)b * 8), org = ld4(p.win + (size_t)b * 8 + 4);
  NmSums s;
  if (i < p.N) {
    const float* pl = p.xyz + (size_t)b * 3 * p.N;
    const f32x4 v = {pl[i], pl[p.N + i], pl[2 * (size_t)p.N + i], 0.f};
    const bool in = p.best[b] >= 0 && sg_finite(v[0]) && sg_finite(v[1]) && sg_finite(v[2]) &&
                    (!p.mask || p.mask[(size_t)b * p.N + i] != 0) &&
                    sg_inlier(nrm[0], nrm[1], nrm[2], org[0], org[1], org[2], v[0], v[1], v[2], p.thr);
    p.inlier[(size_t)b * p.N + i] = in ? 1 : 0;
    if (in) s.add(v, org);
  }
  double v9[9] = {s.sx, s.sy, s.sz, s.sxx, s.sxy, s.sxz, s.syy, s.syz, s.szz};
#pragma unroll
  for (int k = 0; k < 9; ++k) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v9[k] += __shfl_xor(v9[k], o, 64);
    if ((t & 63) == 0) wsum[t >> 6][k] = v9[k];
  }
  __syncthreads();
  if (t < 9) p.part[((size_t)b * p.nblk + blk) * 9 + t] = ((wsum[0][t] + wsum[1][t]) + wsum[2][t]) + wsum[3][t];
}

struct SgRefit {
  const double* part; int nblk;
  const int* best; const float* win; const int* count;
  float* plane; float* point; double* sums;                // [B][4], optional [B][3], optional [B][9]
};

__global__ __launch_bounds__(SG_BLOCK) void plane_refit_kernel(SgRefit p) {
  __shared__ double stage[SG_BLOCK * 9];
  __shared__ double tot[9];
  const int t = threadIdx.x, b = blockIdx.x;
  const double* part = p.part + (size_t)b * p.nblk * 9;
  double acc = 0.;                                         // thread k < 9: the k-th sum, the blocks ascending
  for (int c0 = 0; c0 < p.nblk; c0 += SG_BLOCK) {          // (workgroup-uniform)
    const int m = p.nblk - c0 < SG_BLOCK ? p.nblk - c0 : SG_BLOCK;
    __syncthreads();
    for (int e = t; e < m * 9; e += SG_BLOCK) stage[e] = part[(size_t)c0 * 9 + e];
    __syncthreads();
    if (t < 9)
      for (int i = 0; i < m; ++i) acc += stage[i * 9 + t];
  }
  if (t < 9) tot[t] = acc;
  __syncthreads();
  if (t != 0) return;
  const int best = p.best[b], cnt = p.count[b];
  const float nan = __uint_as_float(0x7FC00000u);
  float n0 = nan, n1 = nan, n2 = nan, d = nan, q0 = nan, q1 = nan, q2 = nan;
  if (best >= 0) {
    const f32x4 trial = ld4(p.win + (size_t)b * 8), org = ld4(p.win + (size_t)b * 8 + 4);
    n0 = trial[0]; n1 = trial[1]; n2 = trial[2];
    double qx = (double)org[0], qy = (double)org[1], qz = (double)org[2];
    if (cnt >= 3) {
      const double m = (double)cnt;
      const double mx = tot[0] / m, my = tot[1] / m, mz = tot[2] / m;
      double a00 = tot[3] / m - mx * mx, a01 = tot[4] / m - mx * my, a02 = tot[5] / m - mx * mz;
      double a11 = tot[6] / m - my * my, a12 = tot[7] / m - my * mz, a22 = tot[8] / m - mz * mz;
      const bool finite = __builtin_isfinite(a00) && __builtin_isfinite(a01) && __builtin_isfinite(a02) && __builtin_isfinite(a11) &&
                          __builtin_isfinite(a12) && __builtin_isfinite(a22);
      const bool zero = a00 == 0. && a01 == 0. && a02 == 0. && a11 == 0. && a12 == 0. && a22 == 0.;
      if (finite && !zero) {
        double v00 = 1., v01 = 0., v02 = 0., v10 = 0., v11 = 1., v12 = 0., v20 = 0., v21 = 0., v22 = 1.;
        for (int sweep = 0; sweep < NM_SWEEPS; ++sweep) {   // nm_point's sweeps
          if (a01 == 0. && a02 == 0. && a12 == 0.) break;
          nm_rotate(a00, a11, a01, a02, a12, v00, v01, v10, v11, v20, v21);
          nm_rotate(a00, a22, a02, a01, a12, v00, v02, v10, v12, v20, v22);
          nm_rotate(a11, a22, a12, a01, a02, v01, v02, v11, v12, v21, v22);
        }
        const int c = (a00 <= a11 && a00 <= a22) ? 0 : (a11 <= a22 ? 1 : 2);
        const double e0 = c == 0 ? v00 : c == 1 ? v01 : v02;
        const double e1 = c == 0 ? v10 : c == 1 ? v11 : v12;
        const double e2 = c == 0 ? v20 : c == 1 ? v21 : v22;
        const double len = sqrt((e0 * e0 + e1 * e1) + e2 * e2);
        float f0 = (float)(e0 / len), f1 = (float)(e1 / len), f2 = (float)(e2 / len);
        const double dot = ((double)f0 * (double)trial[0] + (double)f1 * (double)trial[1]) + (double)f2 * (double)trial[2];
        if (dot < 0.) { f0 = -f0; f1 = -f1; f2 = -f2; }
        if (sg_finite(f0) && sg_finite(f1) && sg_finite(f2)) {
          n0 = f0; n1 = f1; n2 = f2;
          qx += mx; qy += my; qz += mz;
        }
      }
    }
    d = (float)(-(((double)n0 * qx + (double)n1 * qy) + (double)n2 * qz));
    q0 = (float)qx; q1 = (float)qy; q2 = (float)qz;
  }
  p.plane[(size_t)b * 4] = n0; p.plane[(size_t)b * 4 + 1] = n1; p.plane[(size_t)b * 4 + 2] = n2; p.plane[(size_t)b * 4 + 3] = d;
  if (p.point) { p.point[(size_t)b * 3] = q0; p.point[(size_t)b * 3 + 1] = q1; p.point[(size_t)b * 3 + 2] = q2; }
  if (p.sums)
    for (int k = 0; k < 9; ++k) p.sums[(size_t)b * 9 + k] = tot[k];
}

__global__ __launch_bounds__(SG_BLOCK) void plane_invert_kernel(const int* inlier, long total, int* flags) {
  const long g = (long)blockIdx.x * SG_BLOCK + threadIdx.x;
  if (g < total) flags[g] = inlier[g] > 0 ? 0 : 1;
}

inline size_t sg_up(size_t v) { return (v + 255) & ~(size_t)255; }
inline int sg_ceil(long a, long b) { return (int)((a + b - 1) / b); }

// What the entry points and the form query ask of the numbers
int sg_numbers(const vcr_plane_ransac_args& a) {
  if (a.B < 1 || a.trials < 1) return VCR_EINVAL;
  if (!(a.distance_threshold >= 0.f) || a.distance_threshold == __builtin_huge_valf()) return VCR_EINVAL;   // negative, NaN, +inf
  const int form = a.variant & 0xFF, splits = a.variant >> 8;
  if (a.variant < 0 || (a.variant != 0 && form != VCR_PLANE_TRIAL && form != VCR_PLANE_POINT) || splits > VCR_PLANE_MAX_SPLITS)
    return VCR_EINVAL;
  if (a.ransac_n != 3 || a.N < 1 || a.N > VCR_PLANE_MAX_N || a.trials > VCR_PLANE_MAX_TRIALS || (long)a.B * a.N >= (1L << 31) ||
      (long)a.B * a.trials >= (1L << 29))
    return VCR_EUNSUPPORTED;
  return VCR_OK;
}

int sg_check(const vcr_plane_ransac_args& a) {
  if (!a.xyz || !a.plane || !a.inlier || !a.count) return VCR_EINVAL;
  if (a.trial_plane && (((uintptr_t)a.trial_plane) & 15)) return VCR_EINVAL;
  return sg_numbers(a);
}

// THE one place that decides the count launch's form and its number of splits
void sg_form(const vcr_plane_ransac_args& a, int cus, int* form, int* splits) {
  const int forced = a.variant & 0xFF, given = a.variant >> 8;
  const int f = forced ? forced
                       : (a.N >= VCR_PLANE_POINT_MIN_N || a.trials >= VCR_PLANE_POINT_MIN_T ? VCR_PLANE_POINT : VCR_PLANE_TRIAL);
  int s = given;
  if (s == 0) {
    if (f == VCR_PLANE_POINT) {
      s = sg_ceil(a.N, SG_TILE);
    } else {
      const long wgs = (long)a.B * sg_ceil(a.trials, SG_BLOCK);
      const int most = a.N / VCR_PLANE_TRIAL_MIN_RANGE > 1 ? a.N / VCR_PLANE_TRIAL_MIN_RANGE : 1;
      s = sg_ceil((long)VCR_PLANE_FILL * (cus > 0 ? cus : 256), wgs);
      s = s > most ? most : s;
    }
    s = s > VCR_PLANE_MAX_SPLITS ? VCR_PLANE_MAX_SPLITS : s;
  }
  *form = f;
  *splits = s;
}

// workspace: rows [B N 4] | M [B] | best [B] | win [B 8] | blkcnt [B nblk] | part [B nblk 9] | status | plane | count (where not given)
struct SgPlan { int nblk; size_t M, best, win, blk, part, status, plane, count, bytes; };

SgPlan sg_plan(const vcr_plane_ransac_args& a) {
  SgPlan p;
  p.nblk = sg_ceil(a.N, SG_BLOCK);
  const size_t BT = (size_t)a.B * a.trials;
  p.M = sg_up((size_t)a.B * a.N * 16);
  p.best = p.M + sg_up((size_t)a.B * 4);
  p.win = p.best + sg_up((size_t)a.B * 4);
  p.blk = p.win + sg_up((size_t)a.B * 32);
  p.part = p.blk + sg_up((size_t)a.B * p.nblk * 4);
  p.status = p.part + sg_up((size_t)a.B * p.nblk * 72);
  p.plane = p.status + (a.trial_status ? 0 : sg_up(BT * 4));
  p.count = p.plane + (a.trial_plane ? 0 : sg_up(BT * 32));
  p.bytes = p.count + (a.trial_count ? 0 : sg_up(BT * 4));
  return p;
}

int sg_take(const vcr_plane_ransac_args* user, vcr_plane_ransac_args* mine) {
  return vcr_take_args(user, mine, offsetof(vcr_plane_ransac_args, point));
}

int sp_take(const vcr_plane_split_args* user, vcr_plane_split_args* mine) {
  return vcr_take_args(user, mine, offsetof(vcr_plane_split_args, plane_index));
}

int sp_check(const vcr_plane_split_args& a) {
  if (!a.xyz || !a.inlier || !a.plane_points || !a.plane_count || !a.rest_points || !a.rest_count || a.B < 1) return VCR_EINVAL;
  if (a.N < 1 || a.N > VCR_PLANE_MAX_N || (long)a.B * a.N >= (1L << 31)) return VCR_EUNSUPPORTED;
  return VCR_OK;
}

// workspace: flags [B N] | blkcnt [B nblk]
struct SpPlan { size_t blk, bytes; };

SpPlan sp_plan(int B, int N) {
  SpPlan p;
  p.blk = sg_up((size_t)B * N * 4);
  p.bytes = p.blk + sg_up((size_t)B * sg_ceil(N, SG_BLOCK) * 4);
  return p;
}

}  // namespace

extern "C" int vcr_plane_ransac_form(const vcr_plane_ransac_args* ua, int cu_count, int* form, int* splits) {
  vcr_plane_ransac_args a;
  if (sg_take(ua, &a) || cu_count < 0) return VCR_EINVAL;
  const int e = sg_numbers(a);
  if (e) return e;
  int f, s;
  sg_form(a, cu_count, &f, &s);
  if (form) *form = f;
  if (splits) *splits = s;
  return VCR_OK;
}

extern "C" size_t vcr_plane_ransac_workspace_bytes(const vcr_plane_ransac_args* ua, int cu_count) {
  vcr_plane_ransac_args a;
  if (sg_take(ua, &a) || cu_count < 0 || sg_check(a)) return 0;
  return sg_plan(a).bytes;
}

extern "C" int vcr_plane_ransac_f32(const vcr_plane_ransac_args* ua, void* workspace, size_t workspace_bytes, vcr_stream_t stream) {
  vcr_plane_ransac_args a;
  if (sg_take(ua, &a)) return VCR_EINVAL;
  int e = sg_check(a);
  if (e) return e;
  const SgPlan pl = sg_plan(a);
  if (!workspace || (((uintptr_t)workspace) & 255) || workspace_bytes < pl.bytes) return VCR_EINVAL;
  vcr_stream_scope scope(stream);
  hipStream_t s = (hipStream_t)stream;
  unsigned char* w = reinterpret_cast<unsigned char*>(workspace);
  float* rows = reinterpret_cast<float*>(w);
  int* M = reinterpret_cast<int*>(w + pl.M);
  int* best = reinterpret_cast<int*>(w + pl.best);
  float* win = reinterpret_cast<float*>(w + pl.win);
  int* blk = reinterpret_cast<int*>(w + pl.blk);
  double* part = reinterpret_cast<double*>(w + pl.part);
  const int B = a.B, N = a.N, T = a.trials;
  const SgWork wk{rows, M, a.trial_status ? a.trial_status : reinterpret_cast<int*>(w + pl.status),
                  a.trial_plane ? a.trial_plane : reinterpret_cast<float*>(w + pl.plane),
                  a.trial_count ? a.trial_count : reinterpret_cast<int*>(w + pl.count), N, T};
  const dim3 block(SG_BLOCK), clouds((unsigned)B), points((unsigned)((long)B * pl.nblk));      // (B N < 2^31)
  int form, splits;
  sg_form(a, vcr_cu_count(), &form, &splits);

  const SgCand cd{a.xyz, a.mask, N, pl.nblk, blk, rows, M, a.candidates};
  hipLaunchKernelGGL(plane_mark_kernel, points, block, 0, s, cd);
  if ((e = VCR_LAUNCH_RC())) return e;
  hipLaunchKernelGGL(plane_offsets_kernel, clouds, block, 0, s, cd);
  if ((e = VCR_LAUNCH_RC())) return e;
  hipLaunchKernelGGL(plane_gather_kernel, points, block, 0, s, cd);
  if ((e = VCR_LAUNCH_RC())) return e;
  hipLaunchKernelGGL(plane_trial_kernel, dim3((unsigned)((long)B * sg_ceil(T, SG_BLOCK))), block, 0, s,      // (B T < 2^29)
                     SgTrial{wk, a.seed, a.trial_picks});
  if ((e = VCR_LAUNCH_RC())) return e;
  const SgCount ct{wk, a.distance_threshold, splits};
  if ((long)B * sg_ceil(T, 64) * splits >= (1L << 31)) return VCR_EUNSUPPORTED;      // (forced splits only: the plan's stay below)
  if (form == VCR_PLANE_POINT)
    hipLaunchKernelGGL(plane_count_point_kernel, dim3((unsigned)((long)B * sg_ceil(T, 64) * splits)), block, 0, s, ct);
  else
    hipLaunchKernelGGL(plane_count_trial_kernel, dim3((unsigned)((long)B * sg_ceil(T, SG_BLOCK) * splits)), block, 0, s, ct);
  if ((e = VCR_LAUNCH_RC())) return e;
  hipLaunchKernelGGL(plane_best_kernel, clouds, block, 0, s, SgBest{wk, best, win, a.best_trial, a.count});
  if ((e = VCR_LAUNCH_RC())) return e;
  hipLaunchKernelGGL(plane_flags_kernel, points, block, 0, s,
                     SgFlags{a.xyz, a.mask, N, pl.nblk, a.distance_threshold, best, win, a.inlier, part});
  if ((e = VCR_LAUNCH_RC())) return e;
  hipLaunchKernelGGL(plane_refit_kernel, clouds, block, 0, s, SgRefit{part, pl.nblk, best, win, a.count, a.plane, a.point, a.refit_sums});
  return VCR_LAUNCH_RC();
}

extern "C" size_t vcr_plane_split_workspace_bytes(const vcr_plane_split_args* ua, int cu_count) {
  vcr_plane_split_args a;
  if (sp_take(ua, &a) || cu_count < 0 || sp_check(a)) return 0;
  return sp_plan(a.B, a.N).bytes;
}

extern "C" int vcr_plane_split_f32(const vcr_plane_split_args* ua, void* workspace, size_t workspace_bytes, vcr_stream_t stream) {
  vcr_plane_split_args a;
  if (sp_take(ua, &a)) return VCR_EINVAL;
  int e = sp_check(a);
  if (e) return e;
  const SpPlan pl = sp_plan(a.B, a.N);
  if (!workspace || (((uintptr_t)workspace) & 255) || workspace_bytes < pl.bytes) return VCR_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  unsigned char* w = reinterpret_cast<unsigned char*>(workspace);
  int* flags = reinterpret_cast<int*>(w);
  int* blk = reinterpret_cast<int*>(w + pl.blk);
  const long total = (long)a.B * a.N;
  if ((e = outlier_compact_flags(a.inlier, a.xyz, a.B, a.N, blk, a.plane_points, a.plane_count, a.plane_index, s))) return e;
  hipLaunchKernelGGL(plane_invert_kernel, dim3((unsigned)((total + SG_BLOCK - 1) / SG_BLOCK)), dim3(SG_BLOCK), 0, s, a.inlier, total,
                     flags);
  if ((e = VCR_LAUNCH_RC())) return e;
  return outlier_compact_flags(flags, a.xyz, a.B, a.N, blk, a.rest_points, a.rest_count, a.rest_index, s);
}

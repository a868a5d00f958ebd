// A pose from correspondences (include/vcr_hip_match.h): Open3D's feature-matching RANSAC with
// ransac_n = 3, its edge-length and distance checkers, every trial run.  Four launches, no host synchronisation:
//   ransac_pairs_kernel   (its body: corr_pairs.h, shared with fgr.hip) one workgroup per cloud: the source points with a partner,
//                         ascending, gathered ONCE into contiguous 32-B rows (sx, sy, sz, source index | tx, ty, tz, 0) by a
//                         ballot prefix over chunks of 256; M and a zeroed counter of valid trials behind them.
//   ransac_trial_kernel   one QUAD per trial: the four lanes draw the same three picks and run the integer and fp32 tests
//                         together, then the solve of vcr_refine_f32's step with n = 3 -- svd3.h's quad Jacobi and its tail,
//                         one text for all solves of the library -- the fp32 pose, the distance check of the three picks.  A
//                         valid trial appends itself to the cloud's list (an ordinary atomic add on its counter: the order of
//                         the list decides nothing, a trial's count is its own).
//   ransac_count_kernel   one LANE per valid trial, its pose in twelve registers, over ALL M rows: the row's address is the
//                         same for every lane of the workgroup, so it arrives through scalar loads (section 8's note on
//                         section 4.8's scan: a broadcast through LDS would bind there).  Invalid trials were compacted away.
//   ransac_best_kernel    one workgroup per cloud: the maximum of the 64-bit key (count << 32) | (0xFFFFFFFF - t) over the
//                         valid trials -- the highest count, the lowest trial among equals -- and the outputs.
// Every result is a function of the cloud alone; all writes are plain vector stores.
#include "seg_scan.h"
#include "corr_pairs.h"
#include "svd3.h"
#include "../../include/vcr_hip_match.h"

namespace {

struct RsWork {                                            // the workspace, per cloud b
  float* rows;                                             // [B][Ns][8]
  int* M;                                                  // [B]
  int* nvalid;                                             // [B]
  int* list;                                               // [B][T]: the valid trials, in no particular order
  int* status;                                             // [B][T]   (the caller's arrays where it gave them)
  float* pose;                                             // [B][T][12]
  int* count;                                              // [B][T]
};

__global__ __launch_bounds__(RS_BLOCK) void ransac_pairs_kernel(RsPairs p) { rs_pairs_body(p); }

struct RsTrial {
  RsWork w; int Ns, T; unsigned seed; float max_d2, s2; int edges;
  int* picks;                                              // optional [B][T][3]
};

__global__ __launch_bounds__(RS_BLOCK) void ransac_trial_kernel(RsTrial p) {
  const unsigned per = (unsigned)((4L * p.T + RS_BLOCK - 1) / RS_BLOCK);        // workgroups per cloud
  const int b = (int)(blockIdx.x / per);
  const int trial = (int)(((blockIdx.x % per) * RS_BLOCK + threadIdx.x) >> 2);
  const int li = threadIdx.x & 3;
  if (trial >= p.T) return;                                // (quad-uniform, like everything up to the gather below)
  const int M = p.w.M[b];
  const float* rows = p.w.rows + (size_t)b * p.Ns * 8;
  const size_t slot = (size_t)b * p.T + trial;
  int status = 0, pick[3] = {-1, -1, -1};
  f32x4 s[3], q[3];
  if (M < 1) {
    status = 1;
  } else {
    unsigned at[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      at[j] = rs_pick(p.seed, trial, j, M);
      s[j] = ld4(rows + (size_t)at[j] * 8);
      q[j] = ld4(rows + (size_t)at[j] * 8 + 4);
      pick[j] = __float_as_int(s[j][3]);
    }
    if (at[0] == at[1] || at[0] == at[2] || at[1] == at[2]) {
      status = 1;
    } else if (p.edges) {
      bool ok = true;
#pragma unroll
      for (int e = 0; e < 3; ++e) {
        const int u = e == 2 ? 1 : 0, v = e == 0 ? 1 : 2;  // (0,1), (0,2), (1,2)
        const float ds2 = rs_len2(s[u], s[v]), dt2 = rs_len2(q[u], q[v]);
        ok = ok && ds2 >= p.s2 * dt2 && dt2 >= p.s2 * ds2; // a NaN fails
      }
      status = ok ? 0 : 2;
    }
  }
  float P[12] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (status == 0) {                                       // (quad-uniform)
    double Sp[3], Sq[3], H[9];
    const double inv_n = 1.0 / 3.0;
    bool finite = true;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      Sp[r] = ((double)s[0][r] + (double)s[1][r]) + (double)s[2][r];
      Sq[r] = ((double)q[0][r] + (double)q[1][r]) + (double)q[2][r];
      finite = finite && __builtin_isfinite(Sp[r]) && __builtin_isfinite(Sq[r]);
    }
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const double Spq = ((double)s[0][r] * (double)q[0][c] + (double)s[1][r] * (double)q[1][c]) + (double)s[2][r] * (double)q[2][c];
        finite = finite && __builtin_isfinite(Spq);
        H[3 * r + c] = Spq - (Sp[r] * Sq[c]) * inv_n;
      }
    double a[3], v[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      a[j] = li == 0 ? H[j] : li == 1 ? H[3 + j] : li == 2 ? H[6 + j] : 0.0;
      v[j] = li == j ? 1.0 : 0.0;
    }
    jacobi_sweeps_quad(a, v);
    double A[3][3], V[3][3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {                          // gather the rows (lane i of the quad = row i)
      A[0][j] = quad_get(a[j], 0); A[1][j] = quad_get(a[j], 1); A[2][j] = quad_get(a[j], 2);
      V[0][j] = quad_get(v[j], 0); V[1][j] = quad_get(v[j], 1); V[2][j] = quad_get(v[j], 2);
    }
    if (li != 0) return;
    double R[9];
    svd3_finish(A, V, R);
    const double nan = __builtin_nan("");
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      const double tr = Sq[r] * inv_n - (R[3 * r] * (Sp[0] * inv_n) + R[3 * r + 1] * (Sp[1] * inv_n) + R[3 * r + 2] * (Sp[2] * inv_n));
      P[9 + r] = (float)(finite ? tr : nan);
    }
#pragma unroll
    for (int e = 0; e < 9; ++e) P[e] = (float)(finite ? R[e] : nan);
    bool ok = true;
#pragma unroll
    for (int e = 0; e < 12; ++e) ok = ok && __builtin_isfinite(P[e]);
    if (!ok) {
      status = 3;
    } else {
      bool far = false;
#pragma unroll
      for (int j = 0; j < 3; ++j) far = far || rs_d2(P, s[j][0], s[j][1], s[j][2], q[j][0], q[j][1], q[j][2]) > p.max_d2;
      status = far ? 4 : 0;
    }
  }
  if (li != 0) return;
  p.w.status[slot] = status;
#pragma unroll
  for (int e4 = 0; e4 < 3; ++e4) {
    const f32x4 v4 = {P[4 * e4], P[4 * e4 + 1], P[4 * e4 + 2], P[4 * e4 + 3]};
    st4(p.w.pose + slot * 12 + 4 * e4, v4);
  }
  if (p.picks)
#pragma unroll
    for (int j = 0; j < 3; ++j) p.picks[slot * 3 + j] = pick[j];
  if (status == 0) {
    const int at = atomicAdd(p.w.nvalid + b, 1);           // < T: at most one entry per trial
    p.w.list[(size_t)b * p.T + at] = trial;
  } else {
    p.w.count[slot] = -1;
  }
}

struct RsCount { RsWork w; int Ns, T; float max_d2; };

__global__ __launch_bounds__(RS_BLOCK) void ransac_count_kernel(RsCount p) {
  const unsigned per = (unsigned)((p.T + RS_BLOCK - 1) / RS_BLOCK);
  const int b = (int)(blockIdx.x / per);
  const int g = (int)((blockIdx.x % per) * RS_BLOCK + threadIdx.x);
  const int nvalid = p.w.nvalid[b], M = p.w.M[b];
  if (g >= nvalid) return;                                 // nvalid <= T
  const int trial = p.w.list[(size_t)b * p.T + g];
  const size_t slot = (size_t)b * p.T + trial;
  float P[12];
#pragma unroll
  for (int e4 = 0; e4 < 3; ++e4) {
    const f32x4 v4 = ld4(p.w.pose + slot * 12 + 4 * e4);
#pragma unroll
    for (int u = 0; u < 4; ++u) P[4 * e4 + u] = v4[u];
  }
  const float* __restrict__ rows = p.w.rows + (size_t)b * p.Ns * 8;     // (workgroup-uniform, like j: scalar loads)
  int count = 0;
  for (int j = 0; j < M; ++j) {
    const float* __restrict__ r = rows + (size_t)j * 8;
    count += rs_d2(P, r[0], r[1], r[2], r[4], r[5], r[6]) <= p.max_d2 ? 1 : 0;
  }
  p.w.count[slot] = count;
}

struct RsBest {
  RsWork w; int T;
  float* R_out; float* t_out; int* best_trial; int* inliers;
};

__global__ __launch_bounds__(RS_BLOCK) void ransac_best_kernel(RsBest p) {
  __shared__ u64 wbest[RS_BLOCK / 64];
  const int t = threadIdx.x, b = blockIdx.x;
  const int* count = p.w.count + (size_t)b * p.T;
  u64 key = 0;                                             // a valid trial's key is above 0xFFF00000
  for (int i = t; i < p.T; i += RS_BLOCK) {
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
  for (int w = 1; w < RS_BLOCK / 64; ++w) key = wbest[w] > key ? wbest[w] : key;
  float P[12] = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f};
  int best = -1, inl = 0;
  if (key != 0ull) {
    best = (int)(0xFFFFFFFFu - (unsigned)(key & 0xFFFFFFFFull));
    inl = (int)(key >> 32);
    const float* pose = p.w.pose + ((size_t)b * p.T + best) * 12;
    for (int e = 0; e < 12; ++e) P[e] = pose[e];
  }
  for (int e = 0; e < 9; ++e) p.R_out[(size_t)b * 9 + e] = P[e];
  for (int e = 0; e < 3; ++e) p.t_out[(size_t)b * 3 + e] = P[9 + e];
  if (p.best_trial) p.best_trial[b] = best;
  if (p.inliers) p.inliers[b] = inl;
}

struct RsPlan { size_t rows, M, nvalid, list, status, pose, count, bytes; };

int rs_plan(const vcr_ransac_args& a, RsPlan* p) {
  *p = RsPlan{};
  if (!a.src || !a.tgt || !a.corr || !a.R_out || !a.t_out || a.B < 1 || a.Ns < 1 || a.Nt < 1 || a.trials < 1) return VCR_EINVAL;
  if (!(a.max_dist >= 0.f) || a.max_dist == __builtin_huge_valf()) return VCR_EINVAL;      // negative, NaN, +inf
  if (!(a.similarity >= 0.f && a.similarity <= 1.f)) return VCR_EINVAL;
  const int Nmax = a.Ns > a.Nt ? a.Ns : a.Nt;
  if (a.trials > VCR_RANSAC_MAX_TRIALS || a.Ns > RS_MAX_N || a.Nt > RS_MAX_N || (long)a.B * Nmax >= (1L << 31) ||
      (long)a.B * a.trials >= (1L << 29))
    return VCR_EUNSUPPORTED;
  const size_t BT = (size_t)a.B * a.trials;
  p->rows = 0;
  p->M = ws_up((size_t)a.B * a.Ns * 32);
  p->nvalid = p->M + ws_up((size_t)a.B * 4);
  p->list = p->nvalid + ws_up((size_t)a.B * 4);
  p->status = p->list + ws_up(BT * 4);
  p->pose = p->status + (a.trial_status ? 0 : ws_up(BT * 4));
  p->count = p->pose + (a.trial_pose ? 0 : ws_up(BT * 48));
  p->bytes = p->count + (a.trial_inliers ? 0 : ws_up(BT * 4));
  return VCR_OK;
}

int rs_take(const vcr_ransac_args* user, vcr_ransac_args* mine) {
  return vcr_take_args(user, mine, offsetof(vcr_ransac_args, best_trial));
}

}  // namespace

extern "C" size_t vcr_ransac_workspace_bytes(const vcr_ransac_args* ua, int cu_count) {
  vcr_ransac_args a;
  RsPlan p;
  if (rs_take(ua, &a) || cu_count < 0) return 0;
  return rs_plan(a, &p) ? 0 : p.bytes;                     // (the form does not depend on the device)
}

extern "C" int vcr_ransac_f32(const vcr_ransac_args* ua, void* workspace, size_t workspace_bytes, vcr_stream_t stream) {
  vcr_ransac_args a;
  if (rs_take(ua, &a)) return VCR_EINVAL;
  RsPlan p;
  int e = rs_plan(a, &p);
  if (e) return e;
  if (!workspace || (((uintptr_t)workspace) & 15)) return VCR_EINVAL;
  if (a.trial_pose && (((uintptr_t)a.trial_pose) & 15)) return VCR_EINVAL;     // a pose is read and written 16 B at a time
  if (workspace_bytes < p.bytes) return VCR_EWORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  unsigned char* w = reinterpret_cast<unsigned char*>(workspace);
  const RsWork wk{reinterpret_cast<float*>(w + p.rows), reinterpret_cast<int*>(w + p.M), reinterpret_cast<int*>(w + p.nvalid),
                  reinterpret_cast<int*>(w + p.list),
                  a.trial_status ? a.trial_status : reinterpret_cast<int*>(w + p.status),
                  a.trial_pose ? a.trial_pose : reinterpret_cast<float*>(w + p.pose),
                  a.trial_inliers ? a.trial_inliers : reinterpret_cast<int*>(w + p.count)};
  const int B = a.B, T = a.trials;
  const float max_d2 = a.max_dist * a.max_dist;            // fp32: one rounding
  const RsPairs pr{a.src, a.tgt, a.corr, a.Ns, a.Nt, wk.rows, wk.M, wk.nvalid, a.pairs};
  hipLaunchKernelGGL(ransac_pairs_kernel, dim3((unsigned)B), dim3(RS_BLOCK), 0, s, pr);
  if ((e = VCR_LAUNCH_RC())) return e;
  const RsTrial tr{wk, a.Ns, T, a.seed, max_d2, a.similarity * a.similarity, a.similarity != 0.f ? 1 : 0, a.trial_picks};
  const long per4 = (4L * T + RS_BLOCK - 1) / RS_BLOCK;    // B T < 2^29: the grids stay below 2^31
  hipLaunchKernelGGL(ransac_trial_kernel, dim3((unsigned)(B * per4)), dim3(RS_BLOCK), 0, s, tr);
  if ((e = VCR_LAUNCH_RC())) return e;
  const RsCount ct{wk, a.Ns, T, max_d2};
  const long per = (T + RS_BLOCK - 1) / RS_BLOCK;
  hipLaunchKernelGGL(ransac_count_kernel, dim3((unsigned)(B * per)), dim3(RS_BLOCK), 0, s, ct);
  if ((e = VCR_LAUNCH_RC())) return e;
  const RsBest bs{wk, T, a.R_out, a.t_out, a.best_trial, a.inliers};
  hipLaunchKernelGGL(ransac_best_kernel, dim3((unsigned)B), dim3(RS_BLOCK), 0, s, bs);
  return VCR_LAUNCH_RC();
}

// Kernel 4: centred 3x3 cross-covariance + SVD rigid solve (model/vcrnet_model.py:356-399).
// The reference loops over the batch in Python with one LAPACK call and one host sync (det < 0) per
// sample; here one 256-thread block per sample reduces the means and the covariance (fp64 accumulation of the fp32
// inputs; all six / all nine sums cross the block together: four barriers in total), and the first quad of wave 0 runs
// the one-sided Jacobi SVD in fp64 cooperatively: lane i owns row i of A and V, the column inner products of a
// rotation are summed over the quad with DPP, every lane rotates its own row.  Lane 0 gathers the rows for the tail
// (ordering, rank completion, R = V U^T, determinant rule).
//   H = sum_k (s_k - s_mean)(c_k - c_mean)^T,  H = U S V^T,  R = V U^T,
//   det R < 0  ->  flip the column of V that belongs to the SMALLEST singular value (torch.svd sorts
//   descending, so the reference's V @ diag(1,1,-1) is exactly that; :382-386),  t = -R s_mean + c_mean.
// R = V U^T does not depend on the SVD's sign/order conventions while the singular values are distinct,
// so LAPACK-vs-Jacobi differences do not leak into (R, t).
#include "common.h"
#include "svd3.h"

namespace {

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
// NV sums across the block at once: wave trees, one LDS hand-off, fixed order over the four waves
template <int NV>
__device__ __forceinline__ void block_sums(double (&v)[NV], double* red) {
  const int w = threadIdx.x >> 6;
#pragma unroll
  for (int e = 0; e < NV; ++e) v[e] = wave_sum_f64(v[e]);
  __syncthreads();
  if ((threadIdx.x & 63) == 0)
#pragma unroll
    for (int e = 0; e < NV; ++e) red[w * NV + e] = v[e];
  __syncthreads();
#pragma unroll
  for (int e = 0; e < NV; ++e) v[e] = ((red[e] + red[NV + e]) + red[2 * NV + e]) + red[3 * NV + e];
}

__global__ __launch_bounds__(256) void rigid_svd_kernel(vcr_rigid_svd_args p) {
  __shared__ double red[4 * 9];
  const int b = blockIdx.x, t = threadIdx.x;
  const float* S = p.src + (size_t)b * p.K * p.lds;
  const float* C = p.corr + (size_t)b * p.K * p.ldc;
  double mean[6] = {0, 0, 0, 0, 0, 0};
  for (int i = t; i < p.K; i += 256)
    for (int c = 0; c < 3; ++c) { mean[c] += S[(size_t)i * p.lds + c]; mean[3 + c] += C[(size_t)i * p.ldc + c]; }
  block_sums<6>(mean, red);
  // the reference centres in fp32 (src - src.mean): round the means to fp32 like it does
  float smf[3], cmf[3];
  for (int c = 0; c < 3; ++c) { smf[c] = (float)(mean[c] / p.K); cmf[c] = (float)(mean[3 + c] / p.K); }
  double H[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  for (int i = t; i < p.K; i += 256) {
    float sc[3], cc[3];
    for (int c = 0; c < 3; ++c) { sc[c] = S[(size_t)i * p.lds + c] - smf[c]; cc[c] = C[(size_t)i * p.ldc + c] - cmf[c]; }
    for (int r = 0; r < 3; ++r)
      for (int c = 0; c < 3; ++c) H[3 * r + c] += (double)sc[r] * (double)cc[c];
  }
  block_sums<9>(H, red);
  if (t >= 64) return;                                   // wave 0 finishes; its first quad runs the Jacobi sweeps together
  const int li = t & 3;
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
  if (t == 0) {
    double R[9];
    svd3_finish(A, V, R);
    // a non-finite correspondence or point (the reference's torch.svd raises on it): the whole pose is NaN, stated here
    // rather than left to the sweeps, whose fmax-style tests can squash a NaN
    bool finite = true;
    for (int e = 0; e < 9; ++e) finite = finite && __builtin_isfinite(H[e]);
    for (int c = 0; c < 6; ++c) finite = finite && __builtin_isfinite(mean[c]);
    if (!finite)
      for (int e = 0; e < 9; ++e) R[e] = __builtin_nan("");
    float* Ro = p.R + (size_t)b * 9;
    float* to = p.t + (size_t)b * 3;
    float Rf[9], tf[3];
    for (int e = 0; e < 9; ++e) { Rf[e] = (float)R[e]; Ro[e] = Rf[e]; }
    for (int r = 0; r < 3; ++r) {
      tf[r] = (float)(-(R[3 * r] * smf[0] + R[3 * r + 1] * smf[1] + R[3 * r + 2] * smf[2]) + cmf[r]);
      to[r] = tf[r];
    }
    if (p.R_ba) for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) p.R_ba[(size_t)b * 9 + 3 * r + c] = Rf[3 * c + r];
    if (p.t_ba) for (int r = 0; r < 3; ++r)
      p.t_ba[(size_t)b * 3 + r] = -(Rf[r] * tf[0] + Rf[3 + r] * tf[1] + Rf[6 + r] * tf[2]);
    if (p.H) for (int e = 0; e < 9; ++e) p.H[(size_t)b * 9 + e] = (float)H[e];
  }
}

}  // namespace

extern "C" int vcr_rigid_svd_f32(const vcr_rigid_svd_args* a, vcr_stream_t stream) {
  if (!a || !a->src || !a->corr || !a->R || !a->t) return VCR_EINVAL;
  if (a->B <= 0 || a->K < 3 || a->lds < 3 || a->ldc < 3) return VCR_EINVAL;
  hipLaunchKernelGGL(rigid_svd_kernel, dim3(a->B), dim3(256), 0, (hipStream_t)stream, *a);
  return VCR_LAUNCH_RC();
}

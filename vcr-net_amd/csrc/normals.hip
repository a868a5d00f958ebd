// A normal per point from given neighbours (include/vcr_hip_plane.h): vcr_normals_f32.
//
// One launch, one LANE per point.  The header fixes the nine fp64 sums over the neighbours in idx's order, so a point's rows are
// summed by one lane -- a quad per point would need another order or a serial pass over its lanes -- and the 3 x 3 symmetric
// eigenproblem behind them is a cyclic Jacobi in that lane's registers: six values of C, nine of V, no LDS, no scratch.  A
// neighbour is one 16-B row load; the idx entry is checked against [0, N) before it is used (the one gather of the library fed
// by a caller's indices).
#include "common.h"
#include "normals_point.h"                                  // the arithmetic behind the sums, shared with rows.hip
#include "../../include/vcr_hip_plane.h"

namespace {

constexpr int NM_BLOCK = 256;
constexpr int NM_MAX_N = 131072;                           // the kNN entry points' limit (vcr_hip.h)

struct NmArgs {
  const float* xyz4; const int* idx; int N, k; long total; // total = B N
  const float* view; float* normals; float* curv;
};

__global__ __launch_bounds__(NM_BLOCK) void normals_kernel(NmArgs p) {
  const long g = (long)blockIdx.x * NM_BLOCK + threadIdx.x;
  if (g >= p.total) return;
  const int N = p.N, k = p.k;
  const long b = g / N;
  const int i = (int)(g - b * N);
  const float* rows = p.xyz4 + (size_t)b * N * 4;
  const int* nb = p.idx + (size_t)g * k;
  const f32x4 me = ld4(rows + (size_t)i * 4);
  NmSums s;
#pragma unroll 4
  for (int j = 0; j < k; ++j) {
    int r = nb[j];
    r = (unsigned)r < (unsigned)N ? r : i;                 // an entry outside [0, N) reads as the row itself
    s.add(ld4(rows + (size_t)r * 4), me);
  }
  float n0, n1, n2, cv;
  nm_point(s, (double)(k + 1), me, p.view ? p.view + (size_t)b * 3 : nullptr, n0, n1, n2, cv);
  float* out = p.normals + (size_t)b * 3 * N + i;
  out[0] = n0; out[N] = n1; out[2 * (size_t)N] = n2;
  if (p.curv) p.curv[g] = cv;
}

}  // namespace

static int nm_take(const vcr_normals_args* user, vcr_normals_args* mine) {
  return vcr_take_args(user, mine, offsetof(vcr_normals_args, curvature));
}

extern "C" int vcr_normals_f32(const vcr_normals_args* ua, vcr_stream_t stream) {
  vcr_normals_args a;
  if (nm_take(ua, &a)) return VCR_EINVAL;
  if (!a.xyz4 || !a.idx || !a.normals || a.B < 1 || a.N < 1 || a.k < 1 || (((uintptr_t)a.xyz4) & 15)) return VCR_EINVAL;
  if (a.k > VCR_NORMALS_MAX_K || a.N > NM_MAX_N || (long)a.B * a.N >= (1L << 31)) return VCR_EUNSUPPORTED;
  const long total = (long)a.B * a.N;
  const NmArgs k{a.xyz4, a.idx, a.N, a.k, total, a.viewpoint, a.normals, a.curvature};
  hipLaunchKernelGGL(normals_kernel, dim3((unsigned)((total + NM_BLOCK - 1) / NM_BLOCK)), dim3(NM_BLOCK), 0, (hipStream_t)stream, k);
  return VCR_LAUNCH_RC();
}

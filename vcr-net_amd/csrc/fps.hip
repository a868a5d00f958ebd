// Farthest-point sampling (farthest_point_sample, util/util.py:107-140) as ONE launch: npoint strictly sequential rounds, each
// a pass over the whole cloud plus an arg-max, run inside the kernel by one workgroup of 1024 threads per cloud.
//
// The result is discrete, so the arithmetic is the reference's, operation for operation (every one rounded; build.py compiles
// with -ffp-contract=off, nothing below is an fma):
//   d = (dx*dx + dy*dy) + dz*dz;   dist[n] = d where d < dist[n];   far = the LOWEST n with the largest dist[n].
// A NaN / inf coordinate makes d NaN / inf, `d < dist` false, and the point keeps dist = 1e10: the comparison is the whole
// non-finite rule.  dist[n] therefore always lies in [0, 1e10]; only the barycentre rule of the start point meets NaN / inf
// values, and orders them as torch.max does (NaN above +inf, the first one wins).
//
// Arg-max with the first-index rule in one reduction: the values are non-negative (or a canonical NaN), so their bit patterns
// order like unsigned integers; key = bits(value) << 32 | (0xFFFFFFFF - n), largest key = largest value, lowest n.  Every thread
// folds its own points (ascending n, strict >), a wave folds by shuffles, one LDS slot per wave, ONE workgroup barrier, and
// every wave folds the 16 slots for itself.  The slots are double-buffered: the next round writes the other set.
// The winner's coordinates are re-read through the scalar cache (its index is wave-uniform): ~200 cycles of L2 latency a round.
//
// Two forms (fps_plan picks; vcr_fps_args.variant forces):
//   resident  -- the cloud's x, y, z and dist in registers, R points per thread (n = j * 1024 + thread), loaded once.
//   streaming -- coordinates re-read from L2 every round; dist in registers (R per thread) and, beyond them, LDS (L per thread).
#include "common.h"

namespace {

constexpr int FPS_BLOCK = 1024, FPS_WAVES = FPS_BLOCK / 64;
constexpr int FPS_MAX_N = 131072;                          // the kNN entry points' limit (vcr_hip.h)
constexpr int FPS_SLOT_BYTES = 2 * FPS_WAVES * 8;          // two sets of one 64-bit key per wave
constexpr int FPS_SUM_BYTES = FPS_WAVES * 3 * 8;           // the barycentre's per-wave coordinate sums (fp64)
constexpr int FPS_DIST_OFF = 1024;                         // the streaming form's LDS distances start here (16-B aligned)
static_assert(FPS_SLOT_BYTES + FPS_SUM_BYTES <= FPS_DIST_OFF, "LDS layout");

__device__ __forceinline__ unsigned long long fps_key(float v, int n) {
  return ((unsigned long long)__float_as_uint(v) << 32) | (unsigned long long)(0xFFFFFFFFu - (unsigned)n);
}
__device__ __forceinline__ unsigned long long fps_wave_max(unsigned long long k, int from) {
#pragma unroll
  for (int o = from; o >= 1; o >>= 1) {
    const unsigned long long other = __shfl_xor(k, o, 64);
    k = other > k ? other : k;
  }
  return k;
}
// The workgroup's largest key, in every thread.  `turn` counts the reductions of the launch (the slot set alternates).
__device__ __forceinline__ unsigned long long fps_block_max(unsigned long long k, unsigned long long* slots, int turn) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  unsigned long long* s = slots + (turn & 1) * FPS_WAVES;
  k = fps_wave_max(k, 32);
  if (lane == 0) s[wave] = k;
  lds_barrier();
  return fps_wave_max(s[lane & (FPS_WAVES - 1)], FPS_WAVES / 2);
}

// One round's work on one point: the distance to the chosen point, the running minimum, the thread's running arg-max.
__device__ __forceinline__ float fps_update(float x, float y, float z, float fx, float fy, float fz, float dist) {
  const float dx = x - fx, dy = y - fy, dz = z - fz;
  const float d = (dx * dx + dy * dy) + dz * dz;
  return d < dist ? d : dist;
}

__device__ __forceinline__ float fps_ld(const float* base, unsigned byte_off) {   // uniform base + 32-bit lane offset
  return *reinterpret_cast<const float*>(reinterpret_cast<const char*>(base) + byte_off);
}

template <int R, int L, bool RESIDENT>
__global__ __launch_bounds__(FPS_BLOCK) void fps_kernel(vcr_fps_args a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  unsigned long long* slots = reinterpret_cast<unsigned long long*>(smem);
  double* sums = reinterpret_cast<double*>(smem + FPS_SLOT_BYTES);
  float* ldist = reinterpret_cast<float*>(smem + FPS_DIST_OFF);    // [L][1024], thread t owns column t
  const int t = threadIdx.x, b = blockIdx.x, N = a.N;
  const float* __restrict__ px = a.xyz_cf + (size_t)b * a.cloud_stride;
  const float* __restrict__ py = px + N;
  const float* __restrict__ pz = py + N;
  int32_t* idx = a.idx + (size_t)b * a.npoint;
  float* out = a.out_cf ? a.out_cf + (size_t)b * 3 * a.npoint : nullptr;
  constexpr int XR = RESIDENT ? R : 1;
  float x[XR], y[XR], z[XR], dist[R];
  int turn = 0, far;

#pragma unroll
  for (int j = 0; j < R; ++j) {
    const int n = j * FPS_BLOCK + t;
    dist[j] = n < N ? 1e10f : -1.f;                        // a slot without a point: below every distance, never updated
    if (RESIDENT) {
      const int c = n < N ? n : N - 1;
      x[j] = px[c]; y[j] = py[c]; z[j] = pz[c];
    }
  }
  for (int j = 0; j < L; ++j) ldist[j * FPS_BLOCK + t] = (R + j) * FPS_BLOCK + t < N ? 1e10f : -1.f;

  if (a.start) {
    far = a.start[b];
    far = far < 0 ? 0 : far >= N ? N - 1 : far;
  } else {
    // the reference's start: the point farthest from the barycentre (util.py:125-130).  fp64 sums rounded once.
    double sx = 0., sy = 0., sz = 0.;
    if (RESIDENT) {
#pragma unroll
      for (int j = 0; j < R; ++j) {
        const bool in = j * FPS_BLOCK + t < N;
        sx += in ? (double)x[j] : 0.; sy += in ? (double)y[j] : 0.; sz += in ? (double)z[j] : 0.;
      }
    } else {
      for (int n = t; n < N; n += FPS_BLOCK) { sx += (double)px[n]; sy += (double)py[n]; sz += (double)pz[n]; }
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) { sx += __shfl_xor(sx, o, 64); sy += __shfl_xor(sy, o, 64); sz += __shfl_xor(sz, o, 64); }
    if ((t & 63) == 0) { sums[(t >> 6) * 3] = sx; sums[(t >> 6) * 3 + 1] = sy; sums[(t >> 6) * 3 + 2] = sz; }
    lds_barrier();
    sx = sy = sz = 0.;
    for (int w = 0; w < FPS_WAVES; ++w) { sx += sums[w * 3]; sy += sums[w * 3 + 1]; sz += sums[w * 3 + 2]; }   // fixed order, every thread
    const float cx = (float)sx / (float)N, cy = (float)sy / (float)N, cz = (float)sz / (float)N;
    unsigned long long key = 0;
    auto fold = [&](float xn, float yn, float zn, int n) {
      const float dx = xn - cx, dy = yn - cy, dz = zn - cz;
      float d = (dx * dx + dy * dy) + dz * dz;
      if (d != d) d = __uint_as_float(0x7FC00000u);        // torch.max: a NaN is the largest value, the first one wins
      const unsigned long long k = fps_key(d, n);
      key = k > key ? k : key;
    };
    if (RESIDENT) {
#pragma unroll
      for (int j = 0; j < R; ++j) {
        const int n = j * FPS_BLOCK + t;
        if (n < N) fold(x[j], y[j], z[j], n);
      }
    } else {
      for (int n = t; n < N; n += FPS_BLOCK) fold(px[n], py[n], pz[n], n);
    }
    far = (int)(0xFFFFFFFFu - (unsigned)fps_block_max(key, slots, turn++));
  }

  for (int i = 0;; ++i) {
    far = __builtin_amdgcn_readfirstlane(far);
    const float fx = px[far], fy = py[far], fz = pz[far];
    if (t == 0) {
      idx[i] = far;
      if (out) { out[i] = fx; out[a.npoint + i] = fy; out[2 * a.npoint + i] = fz; }
    }
    if (i == a.npoint - 1) break;
    float best = -2.f;
    int bj = 0;
    // byte offsets of this thread's points, rebuilt every round from a value the compiler cannot see through: hoisted out of the
    // round loop, the streaming form's per-point addresses would be registers it does not have
    unsigned tb = (unsigned)t * 4u;
    const unsigned lastb = (unsigned)(N - 1) * 4u;
    if (!RESIDENT) asm volatile("" : "+v"(tb));
#pragma unroll
    for (int j = 0; j < R; ++j) {
      if (RESIDENT || j * FPS_BLOCK < N) {                 // (wave-uniform: rows of threads beyond a streamed cloud cost nothing)
        float xn, yn, zn;
        if (RESIDENT) { xn = x[j]; yn = y[j]; zn = z[j]; }
        else { const unsigned o = min(tb + (unsigned)j * (FPS_BLOCK * 4u), lastb); xn = fps_ld(px, o); yn = fps_ld(py, o); zn = fps_ld(pz, o); }
        const float dn = fps_update(xn, yn, zn, fx, fy, fz, dist[j]);
        dist[j] = dn;
        if (dn > best) { best = dn; bj = j; }
      }
    }
    for (int j = 0; j < L && (R + j) * FPS_BLOCK < N; ++j) {
      const unsigned o = min(tb + (unsigned)(R + j) * (FPS_BLOCK * 4u), lastb);
      const float xn = fps_ld(px, o), yn = fps_ld(py, o), zn = fps_ld(pz, o);
      const float dn = fps_update(xn, yn, zn, fx, fy, fz, ldist[j * FPS_BLOCK + t]);
      ldist[j * FPS_BLOCK + t] = dn;
      if (dn > best) { best = dn; bj = R + j; }
    }
    // (best < 0: a thread without a point -- key 0 loses to every real key, and thread 0 always holds point 0)
    const unsigned long long key = best >= 0.f ? fps_key(best, bj * FPS_BLOCK + t) : 0ull;
    far = (int)(0xFFFFFFFFu - (unsigned)fps_block_max(key, slots, turn++));
  }
}

// How one call runs.  fps_plan() validates the arguments and decides the form from them, and it is the only place that does:
// the entry point launches what the plan says, vcr_fps_form answers from it.
struct FpsPlan {
  vcr_fps_args a;
  int form;                  // 1 resident, 2 streaming
  int R, L;                  // points per thread: in registers, in LDS (streaming form only)
  dim3 grid, block; size_t lds;
};
constexpr int FPS_RESIDENT = 1, FPS_STREAMING = 2;
// Instantiations, smallest first.  Resident: four registers a point (x, y, z, dist) of the 128 a lane has at four waves per SIMD:
// 20 points is what fits without a spill (98 registers; 24 points spill three).  Streaming: one register a point up to 96, then 32 more in 128 KB of LDS -- 128 points per
// thread = 131 072 = the library's limit.
constexpr int FPS_RES_R[] = {1, 4, 8, 16, 20};
constexpr int FPS_STR_RL[][2] = {{32, 0}, {64, 0}, {96, 32}};
constexpr int FPS_RES_MAX_N = 20 * FPS_BLOCK;

}  // namespace

static int fps_plan(const vcr_fps_args& a, FpsPlan* p) {
  *p = FpsPlan{a};
  if (!a.xyz_cf || !a.idx || a.B < 1 || a.N < 1 || a.npoint < 1 || a.cloud_stride < 3L * a.N) return VCR_EINVAL;
  if (a.variant != 0 && a.variant != FPS_RESIDENT && a.variant != FPS_STREAMING) return VCR_EINVAL;
  if (a.N > FPS_MAX_N || (long)a.B * (a.N > a.npoint ? a.N : a.npoint) >= (1L << 31)) return VCR_EUNSUPPORTED;
  if (a.variant == FPS_RESIDENT && a.N > FPS_RES_MAX_N) return VCR_EUNSUPPORTED;
  p->form = a.variant ? a.variant : a.N <= FPS_RES_MAX_N ? FPS_RESIDENT : FPS_STREAMING;
  if (p->form == FPS_RESIDENT) {
    for (int r : FPS_RES_R) if (a.N <= r * FPS_BLOCK) { p->R = r; break; }
  } else {
    for (auto& rl : FPS_STR_RL) if (a.N <= (rl[0] + rl[1]) * FPS_BLOCK) { p->R = rl[0]; p->L = rl[1]; break; }
  }
  p->grid = dim3((unsigned)a.B);
  p->block = dim3(FPS_BLOCK);
  p->lds = FPS_DIST_OFF + (size_t)p->L * FPS_BLOCK * 4;
  return VCR_OK;
}

static int fps_take(const vcr_fps_args* user, vcr_fps_args* mine) {
  return vcr_take_args(user, mine, offsetof(vcr_fps_args, out_cf));
}

extern "C" int vcr_fps_form(const vcr_fps_args* ua, int* form, int* points_per_thread) {
  vcr_fps_args a;
  FpsPlan p;
  if (fps_take(ua, &a)) return VCR_EINVAL;
  const int e = fps_plan(a, &p);
  if (e) return e;
  if (form) *form = p.form;
  if (points_per_thread) *points_per_thread = p.R + p.L;
  return VCR_OK;
}

extern "C" int vcr_fps_f32(const vcr_fps_args* ua, vcr_stream_t stream) {
  vcr_fps_args a;
  if (fps_take(ua, &a)) return VCR_EINVAL;
  vcr_stream_scope scope_(stream);
  FpsPlan p;
  const int e = fps_plan(a, &p);
  if (e) return e;
  hipStream_t s = (hipStream_t)stream;
#define VCR_F(...) return vcr_launch<fps_kernel<__VA_ARGS__>>(p.grid, p.block, p.lds, s, p.a)
  if (p.form == FPS_RESIDENT) {
    switch (p.R) {
      case 1: VCR_F(1, 0, true);
      case 4: VCR_F(4, 0, true);
      case 8: VCR_F(8, 0, true);
      case 16: VCR_F(16, 0, true);
      default: VCR_F(20, 0, true);
    }
  }
  switch (p.R) {
    case 32: VCR_F(32, 0, false);
    case 64: VCR_F(64, 0, false);
    default: VCR_F(96, 32, false);
  }
#undef VCR_F
}

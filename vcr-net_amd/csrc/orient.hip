// Consistent normal orientation (include/orient/vcr_hip_orient.h): vcr_orient_tangent_f32 -- the minimum
// spanning forest of the neighbour graph under the packed (w, lo, hi) keys by Boruvka's rounds, every round three launches, with
// the parity of the reversing edges carried along; then the trees' reference points and the signs.
//
//   orient_init_kernel      a lane a point: word[i] = up[i] = (i, parity 0), best[i] = none, top[i] = 0; the round flags and
//                           n_trees zeroed
//   orient_pick_kernel      a lane a point: the key of every entry of its row that leaves its tree, folded into best[] of BOTH
//                           trees' roots by a 64-bit atomicMin behind a relaxed pre-read (a key that cannot win is not sent)
//   orient_hook_kernel      a lane a root with a best key: the other tree's root r'; of two roots that chose the same edge the
//                           lower stays; otherwise up[r] = (r', s[a] ^ s[b] ^ reverses(a, b)); says "this round hooked",
//                           one store a wave
//   orient_flatten_kernel   a lane a point: its root in the forest of up[] by path halving on the packed word, the parity
//                           folded in; word[i] = (that root, parity towards it); best[i] = none for the next round
//   orient_top_kernel       a lane a point: (orderable z, inverted index) into top[root] by a 64-bit atomicMax -- one a wave
//                           where the wave's points share a tree
//   orient_out_kernel       a lane a point: ref, flip, the oriented normal; the roots counted into n_trees (one add a workgroup)
//
// State.  word[i] (read by every kernel, written by init and flatten alone) holds (root << 1 | parity): between two rounds
// every vertex points AT its tree's root.  up[] is the forest of the roots: up[r] == (r, 0) while r is a root, and the hook
// writes (r', parity) once, never again -- r is no root afterwards and nothing reads word[] towards it once the flatten has run.
// The hook reads word[] and best[] and writes up[] alone, so it races with nobody.  In the flatten every access to up[] is a
// relaxed agent-scope atomic (the XCDs' L2s are not coherent: such an access is served past them), and
//   (1) the hooks of a round are acyclic: every tree chose its least outgoing edge under ONE strict total order, so a cycle of
//       choices can only be two trees choosing the same edge, and of those the lower root stays
//   (2) a halving store writes to x its grandparent as read, with the two parities added: a true statement about the finished
//       hooks, a proper ancestor of x.  A stale read is an older true statement.  Every step of or_find goes to a proper
//       ancestor in a finite forest, so the loop ends; no lane waits for another
// So the shape of up[] under compression depends on arrival order and (root, parity) of every vertex does not.  Which lane wins
// which atomicMin does not matter either: a minimum is order-free, and with a strict order the forest is unique.
#include "common.h"
#include "../../include/orient/vcr_hip_orient.h"

namespace {

typedef unsigned long long u64;

constexpr int OR_BLOCK = 256;
constexpr u64 OR_NONE = ~0ull;
constexpr int OR_LIVE = 64;                                // ints of round flags in front of the workspace (rounds <= 17)

struct OrState { unsigned* word; unsigned* up; u64* best; u64* top; int* live; };
struct OrInit { OrState s; int N, nblk, nlive; int* n_trees; };
struct OrRound { OrState s; const float* normals; const int* idx; int N, k, nblk, round; };
struct OrTail { OrState s; const float* xyz; const float* normals; int N, nblk; float* oriented; int* flip; int* ref; int* n_trees; };

__device__ __forceinline__ unsigned or_ld(const unsigned* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void or_st(unsigned* p, unsigned v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ u64 or_ld64(const u64* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// blockIdx -> (cloud, point); false behind the cloud's end
__device__ __forceinline__ bool or_mine(int nblk, int N, int& b, int& i) {
  b = (int)(blockIdx.x / (unsigned)nblk);
  i = (int)(blockIdx.x % (unsigned)nblk) * OR_BLOCK + threadIdx.x;
  return i < N;
}

// d of the header: the same bits from either end (a product and two fmaf, each commutative in its factors)
__device__ __forceinline__ float or_dot(const float* n, int N, int i, int j) {
  return fmaf(n[2 * (size_t)N + i], n[2 * (size_t)N + j], fmaf(n[N + i], n[N + j], n[i] * n[j]));
}

__device__ __forceinline__ bool or_finite(float v) { return fabsf(v) < __builtin_huge_valf(); }

__device__ __forceinline__ u64 or_key(float d, int i, int j) {
  const float x = 1.0f - fabsf(d);
  const float w = or_finite(d) ? (x > 0.0f ? x : 0.0f) : 1.0f;
  const unsigned lo = i < j ? i : j, hi = i < j ? j : i;
  return ((u64)__float_as_uint(w) << 34) | ((u64)lo << 17) | (u64)hi;
}

__device__ __forceinline__ unsigned or_reverses(float d) { return or_finite(d) && d < 0.0f ? 1u : 0u; }

// key into *slot where it is smaller: the pre-read keeps a key that cannot win off the atomic unit
__device__ __forceinline__ void or_min(u64* slot, u64 key) {
  if (key < or_ld64(slot)) atomicMin(slot, key);
}

// The root of x in the forest of up[] and the parity of the path to it, with path halving (2)
__device__ __forceinline__ unsigned or_find(unsigned* up, unsigned x, unsigned& parity) {
  unsigned par = 0;
  for (;;) {
    const unsigned P = or_ld(up + x), p = P >> 1;
    if (p == x) break;
    const unsigned G = or_ld(up + p), g = G >> 1;
    if (g == p) { par ^= P & 1u; x = p; break; }
    const unsigned both = (P ^ G) & 1u;
    or_st(up + x, (g << 1) | both);
    par ^= both;
    x = g;
  }
  parity = par;
  return x;
}

// a round behind one that hooked nothing has nothing to do (round 0 always runs)
__device__ __forceinline__ bool or_idle(const OrRound& p) { return p.round > 0 && p.s.live[p.round] == 0; }

__global__ __launch_bounds__(OR_BLOCK) void orient_init_kernel(OrInit p) {
  if (blockIdx.x == 0 && (int)threadIdx.x < p.nlive) p.s.live[threadIdx.x] = 0;
  int b, i;
  if (!or_mine(p.nblk, p.N, b, i)) return;
  const size_t g = (size_t)b * p.N + i;
  p.s.word[g] = (unsigned)i << 1;
  p.s.up[g] = (unsigned)i << 1;
  p.s.best[g] = OR_NONE;
  p.s.top[g] = 0;
  if (p.n_trees && i == 0) p.n_trees[b] = 0;
}

__global__ __launch_bounds__(OR_BLOCK) void orient_pick_kernel(OrRound p) {
  if (or_idle(p)) return;
  int b, i;
  if (!or_mine(p.nblk, p.N, b, i)) return;
  const int N = p.N;
  const size_t base = (size_t)b * N;
  const unsigned* word = p.s.word + base;
  u64* best = p.s.best + base;
  const float* n = p.normals + base * 3;
  const int* row = p.idx + (base + i) * p.k;
  const unsigned ri = word[i] >> 1;
  for (int e = 0; e < p.k; ++e) {
    const int j = row[e];
    if ((unsigned)j >= (unsigned)N || j == i) continue;
    const unsigned rj = word[j] >> 1;
    if (rj == ri) continue;                                // inside the tree
    const u64 key = or_key(or_dot(n, N, i, j), i, j);
    or_min(best + ri, key);
    or_min(best + rj, key);                                // j's tree may not list this edge in any row of its own
  }
}

__global__ __launch_bounds__(OR_BLOCK) void orient_hook_kernel(OrRound p) {
  if (or_idle(p)) return;
  int b, i;
  bool hooked = false;
  if (or_mine(p.nblk, p.N, b, i)) {
    const int N = p.N;
    const size_t base = (size_t)b * N;
    const unsigned* word = p.s.word + base;
    const u64* best = p.s.best + base;
    const u64 key = best[i];
    // a root whose tree an edge leaves (a vertex that is no root holds no key: the flatten cleared it)
    if ((word[i] >> 1) == (unsigned)i && key != OR_NONE) {
      const int a = (int)((key >> 17) & 0x1FFFFu), c = (int)(key & 0x1FFFFu);
      const unsigned wa = word[a], wc = word[c];
      const unsigned other = (wa >> 1) == (unsigned)i ? wc >> 1 : wa >> 1;
      if (!(best[other] == key && (unsigned)i < other)) {  // both chose this edge: the lower root stays (1)
        const unsigned rev = or_reverses(or_dot(p.normals + base * 3, N, a, c));
        or_st(p.s.up + base + i, (other << 1) | (((wa ^ wc) & 1u) ^ rev));
        hooked = true;
      }
    }
  }
  // "this round hooked": one store a wave, not one a root -- they all go to one address
  const unsigned long long any = __ballot(hooked);
  if (any && (int)(threadIdx.x & 63) == __ffsll((long long)any) - 1)
    __hip_atomic_store(p.s.live + p.round + 1, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(OR_BLOCK) void orient_flatten_kernel(OrRound p) {
  if (or_idle(p)) return;
  int b, i;
  if (!or_mine(p.nblk, p.N, b, i)) return;
  const size_t base = (size_t)b * p.N;
  const unsigned w = p.s.word[base + i];
  unsigned par;
  const unsigned root = or_find(p.s.up + base, w >> 1, par);
  p.s.word[base + i] = (root << 1) | ((w & 1u) ^ par);
  p.s.best[base + i] = OR_NONE;
}

// z as an unsigned that orders like the float: 0 for a z that is not finite (below every finite one), -0.0 as 0.0
__device__ __forceinline__ unsigned or_zbits(float z) {
  if (!or_finite(z)) return 0u;
  const unsigned u = __float_as_uint(z == 0.0f ? 0.0f : z);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__global__ __launch_bounds__(OR_BLOCK) void orient_top_kernel(OrTail p) {
  int b, i;
  const bool live = or_mine(p.nblk, p.N, b, i);            // (b is the workgroup's; a wave may end behind the cloud)
  const size_t base = (size_t)b * p.N;
  unsigned root = 0xFFFFFFFFu;
  u64 key = 0;                                             // below every member's key: an inverted index is never 0
  if (live) {
    root = p.s.word[base + i] >> 1;
    key = ((u64)or_zbits(p.xyz[base * 3 + 2 * (size_t)p.N + i]) << 32) | (u64)(0xFFFFFFFFu - (unsigned)i);
  }
  // a wave whose live lanes all sit in ONE tree -- the rule on a connected graph -- sends its maximum once: a tree's members
  // would otherwise queue at one address.  A maximum is order-free, so the slot ends the same either way
  const unsigned long long on = __ballot(live);
  const unsigned first = (unsigned)__shfl((int)root, on ? __ffsll((long long)on) - 1 : 0, 64);
  if (on && __ballot(live && root == first) == on) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
      const u64 other = ((u64)(unsigned)__shfl_xor((int)(key >> 32), o, 64) << 32) | (u64)(unsigned)__shfl_xor((int)(key & 0xFFFFFFFFull), o, 64);
      key = other > key ? other : key;
    }
    if ((threadIdx.x & 63) != 0) return;
    root = first;
  } else if (!live) {
    return;
  }
  u64* slot = p.s.top + base + root;
  if (key > or_ld64(slot)) atomicMax(slot, key);
}

__global__ __launch_bounds__(OR_BLOCK) void orient_out_kernel(OrTail p) {
  int b, i;
  const bool live = or_mine(p.nblk, p.N, b, i);
  const int N = p.N;
  const size_t base = (size_t)b * N;
  bool is_root = false;
  if (live) {
    const unsigned w = p.s.word[base + i];
    is_root = (w >> 1) == (unsigned)i;
    const unsigned ref = 0xFFFFFFFFu - (unsigned)(p.s.top[base + (w >> 1)] & 0xFFFFFFFFull);    // a member of the tree: < N
    const unsigned wr = p.s.word[base + ref];
    const float* n = p.normals + base * 3;
    const unsigned f = ((w ^ wr) & 1u) ^ (n[2 * (size_t)N + ref] < 0.0f ? 1u : 0u);
    float* o = p.oriented + base * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) o[c * (size_t)N + i] = __uint_as_float(__float_as_uint(n[c * (size_t)N + i]) ^ (f << 31));
    if (p.flip) p.flip[base + i] = (int)f;
    if (p.ref) p.ref[base + i] = (int)ref;
  }
  if (p.n_trees) {                                         // (workgroup-uniform)
    const int roots = __syncthreads_count(is_root);
    if (threadIdx.x == 0 && roots) atomicAdd(p.n_trees + b, roots);
  }
}

int or_numbers(int B, int N, int k, int variant) {
  if (B < 1 || k < 1) return VCR_EINVAL;
  if (variant != 0 && variant != VCR_ORIENT_ROUNDS && variant != VCR_ORIENT_ONE_LAUNCH) return VCR_EINVAL;
  if (N < 1 || N > VCR_ORIENT_MAX_N || (long)B * N >= (1L << 31) || (long)B * N * k >= (1L << 31)) return VCR_EUNSUPPORTED;
  if (variant == VCR_ORIENT_ONE_LAUNCH) return VCR_EUNSUPPORTED;      // the one-launch form is not built
  return VCR_OK;
}

int or_check(const vcr_orient_tangent_args& a) {
  if (!a.xyz || !a.normals || !a.idx || !a.oriented) return VCR_EINVAL;
  return or_numbers(a.B, a.N, a.k, a.variant);
}

inline size_t or_up(size_t v) { return (v + 255) & ~(size_t)255; }

// workspace: live [OR_LIVE] | word [B N] | up [B N] | best [B N] (64-bit) | top [B N] (64-bit)
struct OrPlan { int nblk, rounds; size_t word_off, up_off, best_off, top_off, bytes; };

OrPlan or_plan(int B, int N) {
  OrPlan p;
  p.nblk = (N + OR_BLOCK - 1) / OR_BLOCK;
  p.rounds = 0;
  while ((1L << p.rounds) < (long)N) ++p.rounds;           // every round at least halves the trees that have an edge to leave by
  const size_t BN = (size_t)B * N;
  p.word_off = or_up((size_t)OR_LIVE * 4);
  p.up_off = p.word_off + or_up(BN * 4);
  p.best_off = p.up_off + or_up(BN * 4);
  p.top_off = p.best_off + or_up(BN * 8);
  p.bytes = p.top_off + or_up(BN * 8);
  return p;
}

int or_take(const vcr_orient_tangent_args* user, vcr_orient_tangent_args* mine) {
  return vcr_take_args(user, mine, offsetof(vcr_orient_tangent_args, flip));
}

}  // namespace

extern "C" size_t vcr_orient_tangent_workspace_bytes(const vcr_orient_tangent_args* ua, int cu_count) {
  vcr_orient_tangent_args a;
  if (or_take(ua, &a) || cu_count < 0 || or_check(a)) return 0;
  return or_plan(a.B, a.N).bytes;
}

extern "C" int vcr_orient_tangent_f32(const vcr_orient_tangent_args* ua, void* workspace, size_t workspace_bytes,
                                      vcr_stream_t stream) {
  vcr_orient_tangent_args a;
  if (or_take(ua, &a)) return VCR_EINVAL;
  int e = or_check(a);
  if (e) return e;
  const OrPlan pl = or_plan(a.B, a.N);
  if (!workspace || (((uintptr_t)workspace) & 255) || workspace_bytes < pl.bytes) return VCR_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  unsigned char* w = reinterpret_cast<unsigned char*>(workspace);
  const OrState st{reinterpret_cast<unsigned*>(w + pl.word_off), reinterpret_cast<unsigned*>(w + pl.up_off),
                   reinterpret_cast<u64*>(w + pl.best_off), reinterpret_cast<u64*>(w + pl.top_off), reinterpret_cast<int*>(w)};
  const dim3 block(OR_BLOCK), grid((unsigned)((long)a.B * pl.nblk));
  hipLaunchKernelGGL(orient_init_kernel, grid, block, 0, s, OrInit{st, a.N, pl.nblk, pl.rounds + 2, a.n_trees});
  if ((e = VCR_LAUNCH_RC())) return e;
  for (int r = 0; r < pl.rounds; ++r) {
    const OrRound kr{st, a.normals, a.idx, a.N, a.k, pl.nblk, r};
    hipLaunchKernelGGL(orient_pick_kernel, grid, block, 0, s, kr);
    if ((e = VCR_LAUNCH_RC())) return e;
    hipLaunchKernelGGL(orient_hook_kernel, grid, block, 0, s, kr);
    if ((e = VCR_LAUNCH_RC())) return e;
    hipLaunchKernelGGL(orient_flatten_kernel, grid, block, 0, s, kr);
    if ((e = VCR_LAUNCH_RC())) return e;
  }
  const OrTail kt{st, a.xyz, a.normals, a.N, pl.nblk, a.oriented, a.flip, a.ref, a.n_trees};
  hipLaunchKernelGGL(orient_top_kernel, grid, block, 0, s, kt);
  if ((e = VCR_LAUNCH_RC())) return e;
  hipLaunchKernelGGL(orient_out_kernel, grid, block, 0, s, kt);
  return VCR_LAUNCH_RC();
}

// Host-only sweep of the fp32 linear's launch planner (csrc/linear.hip: linear_plan) through the library-internal reporter
// vcr_linear_forms_ and vcr_linear_config: one fixed-size binary record per argument set on stdout, the number of sets on
// stderr.  Two builds of the library plan alike iff their recordings are byte-identical:
//   c++ -O2 -std=c++17 -I include -I vcr-net_amd/csrc profiles/experiments/linear_plan_sweep.cpp -ldl -o /tmp/linear_plan_sweep
//   cmp <(/tmp/linear_plan_sweep old/libvcr_hip.so) <(/tmp/linear_plan_sweep vcr-net_amd/libvcr_hip.so)
// No GPU is needed (the library then plans for 256 CUs); pointers are made-up addresses, never dereferenced on the host.
#include <dlfcn.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <vector>
#include "vcr_internal.h"

typedef decltype(&vcr_linear_forms_) forms_fn;
typedef decltype(&vcr_linear_config) config_fn;
static forms_fn forms;
static config_fn config;
static long nsets = 0;

static void record(const vcr_linear_args* a, const vcr_linear_args* b) {
  int rec[20];
  memset(rec, 0xff, sizeof(rec));                        // (what the reporter leaves alone stays -1)
  rec[0] = forms(a, b, &rec[1], &rec[2], &rec[10]);
  rec[18] = config(a);
  rec[19] = b ? config(b) : 0;
  fwrite(rec, sizeof(rec), 1, stdout);
  ++nsets;
}

// flag sets of one linear: bit 0 residual, 1 stats_out, 2 ln_stats_in, 3 bad ln_nseg, 4 no ln_colsum, 5 segmax_out, 6 segmax
// without relu, 7 y == NULL, 8 y + 4 B, 9 bias + 4 B, 10 residual + 4 B, 11 ln_colsum + 4 B, 12 ldy = N + 1, 13 ldr = N + 2,
// 14 ldx = K + 2, 15 seg_k = 0, 16 ld_segmax = N + 1
static vcr_linear_args make(int M, int N, int K, int flags, int variant) {
  vcr_linear_args a;
  memset(&a, 0, sizeof(a));
  auto bit = [&](int i) { return (flags >> i) & 1; };
  a.x = (const float*)0x10000; a.w = (const float*)0x20000;
  a.bias = (const float*)(uintptr_t)(0x30000 + 4 * bit(9));
  a.y = bit(7) ? nullptr : (float*)(uintptr_t)(0x40000 + 4 * bit(8));
  a.ldx = K + 2 * bit(14); a.ldy = N + bit(12);
  a.M = M; a.N = N; a.K = K; a.relu = bit(5) && !bit(6);
  if (bit(0)) { a.residual = (const float*)(uintptr_t)(0x50000 + 4 * bit(10)); a.ldr = N + 2 * bit(13); }
  if (bit(1)) a.stats_out = (float*)0x60000;
  if (bit(2)) {
    a.ln_stats_in = (const float*)0x70000; a.ln_nseg = bit(3) ? 7 : K / 16;
    a.ln_colsum = bit(4) ? nullptr : (const float*)(uintptr_t)(0x80000 + 4 * bit(11)); a.ln_eps = 1e-6f;
  }
  if (bit(5)) { a.segmax_out = (float*)0x90000; a.ld_segmax = N + bit(16); a.seg_k = bit(15) ? 0 : 20; }
  a.variant = variant;
  return a;
}

int main(int argc, char** argv) {
  void* lib = argc > 1 ? dlopen(argv[1], RTLD_NOW) : nullptr;
  if (!lib) { fprintf(stderr, "usage: linear_plan_sweep libvcr_hip.so   (%s)\n", argc > 1 ? dlerror() : "no library"); return 2; }
  forms = (forms_fn)dlsym(lib, "vcr_linear_forms_");
  config = (config_fn)dlsym(lib, "vcr_linear_config");
  if (!forms || !config) { fprintf(stderr, "reporter not found\n"); return 2; }

  std::vector<int> Ms = {1, 31, 32, 33};
  for (int m = 32; m <= 4096; m += 32) { Ms.push_back(m - 1); Ms.push_back(m); Ms.push_back(m + 1); }
  for (int m = 1024; m <= 131072; m += 1024) for (int d : {-1, 0, 1, 95, 96, 127}) Ms.push_back(m + d);
  const int Ns[] = {3, 64, 256, 510, 512, 1024, 1536, 3072}, Ks[] = {32, 128, 512, 1024, 48};
  std::vector<int> variants;                             // every combination of the nine bits, and the retired selectors
  const int bits[9] = {4, 8, 16, 64, 1024, 2048, 4096, 8192, 16384};
  for (int s = 0; s < 512; ++s) {
    int v = 0;
    for (int i = 0; i < 9; ++i) if (s >> i & 1) v |= bits[i];
    variants.push_back(v);
  }
  for (int v : {1, 32, 128, 256, 512, 1 | 16, 32 | 2048}) variants.push_back(v);
  const int single_bits[] = {0, 4, 8, 16, 64, 1024, 2048, 4096, 8192, 16384, 8 | 16, 64 | 16, 8 | 1024, 16 | 1024, 8 | 64, 2048 | 8, 2048 | 64};
  const int flagsets[] = {0, 1, 2, 3, 4, 6, 7, 4 | 8, 4 | 16, 4 | 1 << 11, 32, 32 | 64, 32 | 128, 32 | 1, 32 | 2, 32 | 4, 32 | 1 << 15,
                          32 | 1 << 16, 128, 256, 512, 1 | 1 << 10, 1 << 12, 1 | 1 << 13, 1 << 14, 2 | 256, 6 | 512, 3 | 1 << 10, 32 | 256,
                          3 | 1 << 12, 7 | 1 << 13};

  // 1. singles, every shape: M x N x K x {plain, residual, residual + statistics, LayerNorm-in} x the single bits
  for (int M : Ms) for (int N : Ns) for (int K : Ks) for (int f : {0, 1, 3, 4, 7}) for (int v : single_bits) {
    const vcr_linear_args a = make(M, N, K, f, v);
    record(&a, nullptr);
  }
  // 2. singles, every flag set and every variant combination at the shapes where the planner changes its mind
  const int Mr[] = {1, 33, 128, 1024, 2048, 3000, 3077, 4096, 8192, 14336, 16383, 16384, 32768, 36864, 65536, 131072};
  for (int M : Mr) for (int N : Ns) for (int K : Ks) for (int f : flagsets) for (int v : variants) {
    const vcr_linear_args a = make(M, N, K, f, v);
    record(&a, nullptr);
  }
  // 3. pairs: the cross product of a reduced set of halves (every quirk DESIGN.md quotes is in it) and of variants per half
  std::vector<vcr_linear_args> halves;
  const int Mp[] = {1, 1024, 2048, 3000, 3077, 8192, 14336, 16383, 16384, 32768, 36864, 65536};
  const int Np[] = {256, 510, 512, 1024}, Kp[] = {512, 128}, Fp[] = {0, 1, 3, 2, 4, 7, 32, 256, 128};
  for (int M : Mp) for (int N : Np) for (int K : Kp) for (int f : Fp) {
    if (K == 128 && (N != 512 || f > 3)) continue;
    halves.push_back(make(M, N, K, f, 0));
  }
  const int Vp[] = {0, 4, 8, 16, 64, 1024, 2048, 4096, 8192, 16384, 8 | 16, 64 | 16, 16 | 1024, 1, 2048 | 4096};
  for (const vcr_linear_args& ha : halves) for (const vcr_linear_args& hb : halves) for (int va : Vp) for (int vb : Vp) {
    if (va && vb && va != vb && (va > 64 || vb > 64) && !(va >= 2048 && vb >= 2048)) continue;   // (mixed: small bits, or two heights)
    vcr_linear_args a = ha, b = hb;
    a.variant = va; b.variant = vb;
    record(&a, &b);
  }
  const vcr_linear_args one = make(2048, 512, 512, 1, 0);
  record(&one, nullptr); record(nullptr, nullptr); record(nullptr, &one);
  fprintf(stderr, "%ld argument sets\n", nsets);
  return 0;
}

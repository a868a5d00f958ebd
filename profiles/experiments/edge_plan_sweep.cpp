// Host-only sweep of the EdgeConv family's launch planners (csrc/edgeconv.hip: edgeconv_check / edgeconv_plan, gathermax_check /
// gathermax_plan) through the library-internal reporters vcr_edgeconv_forms_ and vcr_gathermax_forms_: one fixed-size binary
// record per argument set on stdout, the number of sets on stderr.  Two builds of the library plan alike iff their recordings
// are byte-identical:
//   c++ -O2 -std=c++17 -I include -I vcr-net_amd/csrc profiles/experiments/edge_plan_sweep.cpp -ldl -o /tmp/edge_plan_sweep
//   cmp <(/tmp/edge_plan_sweep old/libvcr_hip.so) <(/tmp/edge_plan_sweep vcr-net_amd/libvcr_hip.so)
// No GPU is needed (the library then plans for 256 CUs); pointers are made-up addresses, never dereferenced on the host.
#include <dlfcn.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <vector>
#include "vcr_internal.h"

typedef decltype(&vcr_edgeconv_forms_) ec_fn;
typedef decltype(&vcr_gathermax_forms_) gm_fn;
static ec_fn ec_forms;
static gm_fn gm_forms;
static long nsets = 0;

static void record_ec(const vcr_edgeconv_args* a, int bf16x3) {
  int rec[6];
  memset(rec, 0xff, sizeof(rec));                        // (what the reporter leaves alone stays -1)
  rec[0] = ec_forms(a, bf16x3, &rec[1], &rec[2]);
  fwrite(rec, sizeof(rec), 1, stdout);
  ++nsets;
}
static void record_gm(const vcr_gathermax_args* a) {
  int rec[6];
  memset(rec, 0xff, sizeof(rec));
  rec[0] = gm_forms(a, &rec[1], &rec[2], &rec[3], &rec[4]);
  fwrite(rec, sizeof(rec), 1, stdout);
  ++nsets;
}

// pointer bits: 0 pq, 1 idx, 2 w2, 3 b2, 4 x1, 5 x2 at + 4 B; pitch digits (base 3): ldpq, ldx1, ldx2 at + 0 / 1 / 2
static vcr_edgeconv_args make_ec(int M, int N, int k, int ptrs, int pitches) {
  vcr_edgeconv_args a;
  memset(&a, 0, sizeof(a));
  auto at = [&](uintptr_t base, int bit) { return base + 4 * ((ptrs >> bit) & 1); };
  a.pq = (const float*)at(0x10000, 0); a.idx = (const int32_t*)at(0x20000, 1);
  a.w2 = (const float*)at(0x30000, 2); a.b2 = (const float*)at(0x40000, 3);
  a.x1 = (float*)at(0x50000, 4); a.x2 = (float*)at(0x60000, 5);
  a.ldpq = 256 + pitches % 3; a.ldx1 = 128 + pitches / 3 % 3; a.ldx2 = 128 + pitches / 9 % 3;
  a.M = M; a.n_per_cloud = N; a.k = k;
  return a;
}

// pointer bits: 0 pq, 1 idx, 2 y at + 4 B, 3 an order list; pitch digits (base 3): ldpq = 2 C + 0 / 1 / 2, ldy = C + 0 / 1 / 2
static vcr_gathermax_args make_gm(int B, int N, int extra, int k, int C, int ptrs, int pitches, int variant) {
  vcr_gathermax_args a;
  memset(&a, 0, sizeof(a));
  auto at = [&](uintptr_t base, int bit) { return base + 4 * ((ptrs >> bit) & 1); };
  a.pq = (const float*)at(0x10000, 0); a.idx = (const int32_t*)at(0x20000, 1); a.y = (float*)at(0x30000, 2);
  if (ptrs & 8) a.order = (const int32_t*)0x40000;
  a.C = C; a.ldpq = 2 * C + pitches % 3; a.ldy = C + pitches / 3 % 3;
  a.k = k; a.M = B * N + extra; a.n_per_cloud = N; a.variant = variant;
  return a;
}

int main(int argc, char** argv) {
  void* lib = argc > 1 ? dlopen(argv[1], RTLD_NOW) : nullptr;
  if (!lib) { fprintf(stderr, "usage: edge_plan_sweep libvcr_hip.so   (%s)\n", argc > 1 ? dlerror() : "no library"); return 2; }
  ec_forms = (ec_fn)dlsym(lib, "vcr_edgeconv_forms_");
  gm_forms = (gm_fn)dlsym(lib, "vcr_gathermax_forms_");
  if (!ec_forms || !gm_forms) { fprintf(stderr, "reporter not found\n"); return 2; }

  // ---- EdgeConv, fp32 and bf16x3 entry: k 1..66 (and 0, -1); M around the group sizes (8 / 4) and the three grid caps
  // (512 slots = 4096 / 2048 points, the padded kernel's 2048 points, the bf16x3 kernel's 1024 groups = 8192 / 4096 points);
  // n_per_cloud dividing M or not; every pointer at + 0 / + 4 B; every pitch at + 0 / + 1 / + 2
  const int Ms[] = {-1, 0, 1, 2, 7, 8, 9, 37, 74, 160, 511, 512, 513, 1023, 1024, 1025, 2044, 2047, 2048, 2049, 2052, 4088, 4092, 4095,
                    4096, 4097, 4100, 4104, 8184, 8191, 8192, 8193, 8200, 32768, 65536};
  for (int bf = 0; bf < 2; ++bf) for (int k = -1; k <= 66; ++k) for (int M : Ms) for (int N : {0, 1, 3, M / 2, M, 1024})
    for (int ptrs = 0; ptrs < 64; ++ptrs) for (int pitches = 0; pitches < 27; ++pitches) {
      const vcr_edgeconv_args a = make_ec(M, N, k, ptrs, pitches);
      record_ec(&a, bf);
    }
  for (int bf = 0; bf < 2; ++bf) for (int k : {7, 20, 33, 40, 65}) {
    record_ec(nullptr, bf);
    for (int null = 0; null < 6; ++null) {               // one NULL pointer at a time
      vcr_edgeconv_args a = make_ec(4096, 1024, k, 0, 0);
      const void** slots[6] = {(const void**)&a.pq, (const void**)&a.idx, (const void**)&a.w2, (const void**)&a.b2,
                               (const void**)&a.x1, (const void**)&a.x2};
      *slots[null] = nullptr;
      record_ec(&a, bf);
    }
    for (int ld : {0, 4, 127, 128, 252, 255, 256, 260, 512}) {   // pitches below their minima
      vcr_edgeconv_args a = make_ec(4096, 1024, k, 0, 0);
      a.ldpq = ld; record_ec(&a, bf);
      a.ldpq = 256; a.ldx1 = ld; record_ec(&a, bf);
      a.ldx1 = 128; a.ldx2 = ld; record_ec(&a, bf);
    }
  }

  // ---- gather-max: cloud sizes around the 32-channel (1066 / 1067) and the 16-channel (2048 / 2049) limits of the LDS forms,
  // cloud counts around the 192-workgroup minimum at every slice count, M a multiple of n_per_cloud or not
  const int Ns[] = {1, 64, 333, 768, 1000, 1024, 1065, 1066, 1067, 1068, 2047, 2048, 2049, 2050, 4096, 5119, 5120, 5121, 10240};
  const int Bs[] = {1, 2, 4, 5, 6, 7, 8, 23, 24, 25, 31, 32, 47, 48, 63, 64, 65, 95, 96, 191, 192, 193, 200, 1000};
  // 1. every k, a few channel counts, the variants the header names (and an unknown one), every pointer combination
  for (int k = -1; k <= 66; ++k) for (int N : Ns) for (int B : Bs) for (int C : {4, 32, 96, 128, 256, 260})
    for (int ptrs = 0; ptrs < 16; ++ptrs) for (int v : {0, 1, 8, 16, 32, 5}) {
      const vcr_gathermax_args a = make_gm(B, N, 0, k, C, ptrs, 0, v);
      record_gm(&a);
    }
  // 2. the packable k and one other: every C in steps of 4 up to 260 (and two that are no multiple of 4), all variants -1..33,
  // one pointer at + 4 B at a time or every pitch combination; M = B N and B N + 1
  for (int k : {20, 40, 7}) for (int N : Ns) for (int B : Bs) for (int C = 0; C <= 266; C += (C < 260 ? 4 : 3))
    for (int v = -1; v <= 33; ++v) {
      for (int ptrs : {1, 2, 4}) {
        const vcr_gathermax_args a = make_gm(B, N, 0, k, C, ptrs, 0, v);
        record_gm(&a);
      }
      for (int pitches = 0; pitches < 9; ++pitches) {
        const vcr_gathermax_args a = make_gm(B, N, 0, k, C, 0, pitches, v);
        record_gm(&a);
      }
      const vcr_gathermax_args a = make_gm(B, N, 1, k, C, 0, 0, v);
      record_gm(&a);
    }
  for (int k : {20, 7}) for (int v : {0, 1, 32}) {
    record_gm(nullptr);
    for (int null = 0; null < 3; ++null) {
      vcr_gathermax_args a = make_gm(32, 1024, 0, k, 256, 0, 0, v);
      const void** slots[3] = {(const void**)&a.pq, (const void**)&a.idx, (const void**)&a.y};
      *slots[null] = nullptr;
      record_gm(&a);
    }
    for (int N : {0, -1}) {
      vcr_gathermax_args a = make_gm(32, 1024, 0, k, 256, 0, 0, v);
      a.n_per_cloud = N; record_gm(&a);
    }
    vcr_gathermax_args a = make_gm(32, 1024, 0, k, 256, 0, 0, v);
    a.ldpq = 508; record_gm(&a);                          // below 2 C
    a.ldpq = 512; a.M = 0; record_gm(&a);
  }
  fprintf(stderr, "%ld argument sets\n", nsets);
  return 0;
}

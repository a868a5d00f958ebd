// The outlier filters' tail (outlier_tail.h: mark, offsets, write) for a caller that brings its own keep flags -- dbscan.hip's
// largest cluster.  Defined in outlier.hip, whose kernels it launches: a file that includes this header compiles none of them.
// Host only, library-internal (C++ linkage, no ABI promise).
//   flags   int32 [B,N]: a point is kept iff its flag is > 0
//   xyz     [B,3,N] channels-first
//   blkcnt  workspace, int32 [B, ceil(N / 256)]
//   points [B,3,N], count [B], index [B,N] (optional): as vcr_outlier_radius_f32 writes them
// Asynchronous on the stream; returns the first launch error.
#pragma once
#include <hip/hip_runtime.h>

int outlier_compact_flags(const int* flags, const float* xyz, int B, int N, int* blkcnt, float* points, int* count, int* index,
                          hipStream_t s);

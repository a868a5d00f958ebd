// The capped nearest neighbour across two clouds on the target's grid (include/vcr_hip_gridnn.h), as the
// files that run it see it: gridnn.hip defines the three host functions below; nnscore.hip and refine_round.h (the three fits)
// call them where their scan siblings call nn_scan_launch.  Host code only, library-internal: no C-ABI promise.
#pragma once
#include <hip/hip_runtime.h>
#include "../../include/vcr_hip_gridnn.h"

enum { GRIDNN_SCORE = 0, GRIDNN_REFINE = 1 };              // the entry point's family: what order = 0 is decided per
constexpr int GRIDNN_ORDER_ROUNDS = 8;                     // searches a call must enqueue for the plan to build the source's order

// One call's grid search: the checked vcr_grid_nn_args with the order resolved, and the layout of the grid's part of the
// workspace (`area`: 256-B aligned, behind the sibling's S = 1 parts): the target's grid | the source's, with order 1
struct GridNnPlan {
  int B, Ns, Nt;
  int order;                                               // 1 = the source's cell order, 2 = index order
  float cell;
  int cells;                                               // G(Nt), the target's cell budget
  size_t src_off, bytes;
};

// VCR_EINVAL for a struct that does not say its size, a cell that is negative, NaN or infinite, an order outside 0 ... 2.
// B, Ns, Nt have passed the sibling's checks; searches: how many the call enqueues (1, or max_iterations + 1).
int gridnn_plan(const vcr_grid_nn_args* user, int family, int searches, int B, int Ns, int Nt, GridNnPlan* p);
// Once a call, in front of round 0: the target's grid (five launches) and, with order 1, the source's permutation (six)
int gridnn_build(const GridNnPlan& p, const float* src, const float* tgt, void* area, hipStream_t s);
// One search: part_d2 / part_idx [B][Ns] in nn_scan_kernel's S = 1 layout, under the pose (R, t; both NULL = identity);
// live: optional [B], a cloud whose word is 0 is skipped
int gridnn_search(const GridNnPlan& p, const float* src, const float* R, const float* t, float cap2, const void* area,
                  float* part_d2, int* part_idx, const int* live, hipStream_t s);

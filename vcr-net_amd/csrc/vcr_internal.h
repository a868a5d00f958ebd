// Library-internal entry points: exported from libvcr_hip.so but NOT part of the C-ABI of include/vcr_hip.h (no version
// promise; the trailing underscore says so).  Host only -- nothing is launched and no device is needed: each reports what a
// family's launch planner makes of a set of arguments.  The forward driver sizes its workspace with them, the tests pin the
// plans DESIGN.md quotes (tests/test_abi.py), the sweeps under profiles/experiments/ compare two builds of the library.
//
// Declared ONCE, here: the file that defines a reporter includes this header, so a definition that disagrees with its
// declaration does not compile; vcrnet_amd/native.py's INTERNAL signature table is held to these prototypes by
// test_ctypes_signatures_match_the_header.  Plain C, like the public header.
#ifndef VCR_INTERNAL_H
#define VCR_INTERNAL_H

#include "../../include/vcr_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Each is documented at its definition. */
/* linear.hip: linear_plan's answer for one (b == NULL) or two linears; form_a / form_b take 8 ints each. */
int vcr_linear_forms_(const vcr_linear_args* a, const vcr_linear_args* b, int* one_launch, int* form_a, int* form_b);
/* knn.hip: knn_plan's answer for one search (b == NULL) or the pair. */
int vcr_knn_forms_(const vcr_knn_args* a, const vcr_knn_args* b, int* ordered, int* inline_a, int* inline_b);
/* attention.hip: sdpa_plan's key split and kernel; the floats of split_work the forward reserves for its attention launches. */
int vcr_sdpa_forms_(const vcr_sdpa_args* a, int* nsplit, int* persistent);
long vcr_sdpa_split_floats_(size_t rows, int heads, int ldo, long nbatch, int nq, int cus);
/* edgeconv.hip: edgeconv_check / edgeconv_plan and gathermax_check / gathermax_plan. */
int vcr_edgeconv_forms_(const vcr_edgeconv_args* a, int bf16x3, int* form, int* grid);
int vcr_gathermax_forms_(const vcr_gathermax_args* a, int* form, int* cs, int* grid, int* lds_bytes);

#ifdef __cplusplus
}
#endif
#endif /* VCR_INTERNAL_H */

// Host build of vartrix_amd/csrc/vtx_call_core.h for tests/test_call_core.py: the functions reduce_count_kernel and reduce_emit_kernel
// are compiled from, one group per call.
#include <stdint.h>

#include "../../vartrix_amd/csrc/vtx_call_core.h"

extern "C" {
uint32_t vtxt_call_of(int32_t rs, int32_t as, int32_t min_score) { return vtxcall::call_of(rs, as, min_score); }
uint32_t vtxt_collapse_of(uint32_t r, uint32_t a, uint32_t k) { return vtxcall::collapse_of(r, a, k); }
// out = (ref, alt, unk) of the group [begin, end)
void vtxt_count_group(const int32_t* ref_score, const int32_t* alt_score, const uint32_t* head_umi, uint32_t begin, uint32_t end,
                      int32_t min_score, int use_umi, uint32_t* out) {
    const vtxcall::Counts c = vtxcall::count_group(ref_score, alt_score, head_umi, begin, end, min_score, use_umi != 0);
    out[0] = c.r; out[1] = c.a; out[2] = c.k;
}
int vtxt_keep_of(uint32_t r, uint32_t a, uint32_t k, int mode) { return vtxcall::keep_of(vtxcall::Counts{r, a, k}, mode) ? 1 : 0; }
// out = (value, ref_value)
void vtxt_values_of(uint32_t r, uint32_t a, uint32_t k, int mode, double* out) { vtxcall::values_of(vtxcall::Counts{r, a, k}, mode, &out[0], &out[1]); }
}

// Host build of vartrix_amd/csrc/vtx_f64_text.h (the per-lane f64 formatter of mtx_len_kernel<true> / mtx_text_kernel<true>) for
// tests/test_f64_text.py: f64_len / f64_put over arrays, and the two value families of the tests generated here (Python would
// take minutes for them).
#include <stdint.h>
#include <string.h>

#include "../../vartrix_amd/csrc/vtx_f64_text.h"

extern "C" {

// len[i] = f64_len(v[i]); text + i * stride gets f64_put's bytes.  The caller fills `text` with a canary first and checks it.
// Returns the number of values whose f64_put did not end exactly f64_len bytes behind its start (must be 0).
uint64_t vtxt_format(const double* v, uint64_t n, uint32_t* len, uint8_t* text, uint32_t stride) {
    uint64_t bad = 0;
    for (uint64_t i = 0; i < n; ++i) {
        len[i] = vtxt::f64_len(v[i]);
        uint8_t* p = text + i * stride;
        if (len[i] && vtxt::f64_put(p, v[i]) != p + len[i]) ++bad;
    }
    return bad;
}

// every a / t for 1 <= t <= tmax, 0 <= a <= t, in that order; returns the count (out may be null to ask for it)
uint64_t vtxt_gen_ratios(uint32_t tmax, double* out) {
    uint64_t n = 0;
    for (uint32_t t = 1; t <= tmax; ++t)
        for (uint32_t a = 0; a <= t; ++a, ++n)
            if (out) out[n] = (double)a / (double)t;
    return n;
}

// emit_coo_kernel's expression for alt_frac: (double)a / ((double)r + a + k) of u32 counters
void vtxt_gen_frac(const uint32_t* a, const uint32_t* r, const uint32_t* k, uint64_t n, double* out) {
    for (uint64_t i = 0; i < n; ++i) out[i] = (double)a[i] / ((double)r[i] + a[i] + k[i]);
}

int vtxt_min_exp2(void) { return vtxt::MIN_EXP2; }
int vtxt_max_exp2(void) { return vtxt::MAX_EXP2; }
uint32_t vtxt_max_len(void) { return vtxt::MAX_LEN; }

}  // extern "C"

// Host build of vartrix_amd/csrc/vtx_csr_dense_core.h for tests/test_csr_dense_core.py: the functions one lane of the CSR x table kernel
// (vtx_csr_dense.hip) runs alone, with the lanes as loops and the exchange between lanes as array reads (lanes.h).
// No device code, no sanitizer: a shared object ctypes loads.
#include "lanes.h"

extern "C" {

uint32_t csrdense_max(void) { return vtxr::DENSE_MAX; }
uint32_t csrdense_unroll(void) { return vtxr::DENSE_UNROLL; }

// count * weight modulo 2^64
uint64_t csrdense_mul(uint32_t count, int32_t w) { return vtxr::dense_mul(count, w); }
uint64_t csrdense_table_index(uint32_t v, uint32_t n_cols, uint32_t h) { return vtxr::dense_table_index(v, n_cols, h); }
uint64_t csrdense_out_index(uint64_t r, uint32_t n_cols, uint32_t h) { return vtxr::dense_out_index(r, n_cols, h); }

// vtx_csr_dense_sum; w_alt or w_ref may be NULL; stores: n_major * n_cols zeroed bytes that count the lanes that store each element
void csrdense_sum(const uint64_t* indptr, uint32_t n_major, const uint32_t* indices, const uint32_t* alt, const uint32_t* ref,
                  const int32_t* w_alt, const int32_t* w_ref, uint32_t n_cols, int64_t* out, uint8_t* stores) {
    csrdense::sum(csrdense::SumIn{indptr, n_major, indices, alt, ref, w_alt, w_ref, n_cols}, out, stores);
}

}

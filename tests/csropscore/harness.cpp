// Host build of vartrix_amd/csrc/vtx_csr_ops_core.h for tests/test_csr_ops_core.py: the functions one lane of the summary and selection
// kernels (vtx_csr_ops.hip) runs alone, with the lanes as loops (lanes.h).  No device code, no sanitizer: a shared object ctypes loads.
#include "lanes.h"

extern "C" {

uint32_t csrops_group_lanes(uint64_t nnz, uint64_t n_major) { return vtxr::group_lanes(nnz, n_major); }

// csr_row_stats_kernel<G>; out: seven arrays of n_major elements (4 x u32, 3 x u64), any of them NULL
void csrops_row_stats(const uint64_t* indptr, uint32_t n_major, const uint32_t* alt, const uint32_t* ref, const uint32_t* unk, uint32_t G,
                      uint32_t* n_entries, uint32_t* n_alt, uint32_t* n_ref, uint32_t* n_both, uint64_t* sum_alt, uint64_t* sum_ref,
                      uint64_t* sum_unk) {
    csrops::row_stats(indptr, n_major, alt, ref, unk, G, csrops::StatsOut{n_entries, n_alt, n_ref, n_both, sum_alt, sum_ref, sum_unk});
}

// vtx_csr_select_plan: sizes = {n_major_out, n_minor_out, nnz_out}
void csrops_plan(const uint64_t* indptr, uint32_t n_major, uint32_t n_minor, const uint32_t* indices, uint64_t nnz, const uint8_t* keep_major,
                 const uint8_t* keep_minor, uint32_t* sizes) {
    csrops::Maps m;
    csrops::scans(indptr, n_major, n_minor, indices, nnz, keep_major, keep_minor, m, sizes);
}

// vtx_csr_select into arrays of the plan's sizes; writes: n_major_out + 1 zeroed bytes that count the stores into indptr_out
void csrops_select(const uint64_t* indptr, uint32_t n_major, uint32_t n_minor, const uint32_t* indices, uint64_t nnz, const uint8_t* keep_major,
                   const uint8_t* keep_minor, uint64_t* indptr_out, uint8_t* writes, uint32_t* indices_out, uint32_t* major_ids, uint32_t* minor_ids,
                   const uint32_t* pay32_in, uint32_t* pay32_out, const uint64_t* pay64_in, uint64_t* pay64_out) {
    csrops::Maps m;
    uint32_t sizes[3];
    csrops::scans(indptr, n_major, n_minor, indices, nnz, keep_major, keep_minor, m, sizes);
    csrops::place(indptr, n_major, n_minor, indices, nnz, keep_major, keep_minor, m, indptr_out, writes, indices_out, major_ids, minor_ids, pay32_in,
                  pay32_out, pay64_in, pay64_out);
}

}

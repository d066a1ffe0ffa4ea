// Host build of vartrix_amd/csrc/vtx_csr_group_core.h for tests/test_csr_group_core.py: the functions one lane of the pseudobulk kernels
// (vtx_csr_group.hip) runs alone, with the lanes as loops and the tile as an array (lanes.h).  No device code, no sanitizer: a shared
// object ctypes loads.
#include "lanes.h"

extern "C" {

uint32_t csrgroup_window(void) { return vtxr::GROUP_WINDOW; }
uint32_t csrgroup_max(void) { return vtxr::GROUP_MAX; }
uint32_t csrgroup_tile_bytes(void) { return (uint32_t)sizeof(vtxr::GroupTile); }

// csr_group_check_kernel: the lowest column with a bad label, 0xFFFFFFFF when there is none
uint32_t csrgroup_first_bad(const uint32_t* group, uint32_t n_minor, uint32_t n_groups) { return csrgroup::first_bad(group, n_minor, n_groups); }

// vtx_csr_group_plan: pos[n_major + 1]; returns nnz_out
uint32_t csrgroup_plan(const uint64_t* indptr, uint32_t n_major, const uint32_t* indices, const uint32_t* group, uint32_t n_groups, uint32_t* pos) {
    std::vector<uint32_t> p;
    csrgroup::count(indptr, n_major, indices, group, n_groups, p);
    for (size_t i = 0; i < p.size(); ++i) pos[i] = p[i];
    return p[n_major];
}

// vtx_csr_group_sum into arrays of the plan's size; stores: nnz_out zeroed bytes that count the lanes that store into each slot
void csrgroup_sum(const uint64_t* indptr, uint32_t n_major, const uint32_t* indices, const uint32_t* alt, const uint32_t* ref, const uint32_t* unk,
                  const uint32_t* group, uint32_t n_groups, uint64_t* indptr_out, uint32_t* indices_out, uint8_t* stores, uint32_t* n_entries,
                  uint32_t* n_alt, uint32_t* n_ref, uint32_t* n_both, uint64_t* sum_alt, uint64_t* sum_ref, uint64_t* sum_unk) {
    std::vector<uint32_t> p;
    csrgroup::count(indptr, n_major, indices, group, n_groups, p);
    csrgroup::fill(indptr, n_major, indices, alt, ref, unk, group, n_groups, p, indptr_out, indices_out,
                   csrgroup::StatsOut{n_entries, n_alt, n_ref, n_both, sum_alt, sum_ref, sum_unk}, stores);
}

}

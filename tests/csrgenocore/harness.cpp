// Host build of vartrix_amd/csrc/vtx_csr_geno_core.h for tests/test_csr_geno_core.py: the functions one lane of the donor tally kernels
// (vtx_csr_geno.hip) runs alone, with the lanes as loops and the exchange between lanes as array reads (lanes.h).  No device code, no
// sanitizer: a shared object ctypes loads.
#include "lanes.h"

extern "C" {

uint32_t csrgeno_max(void) { return vtxr::GENO_MAX; }
uint32_t csrgeno_none(void) { return vtxr::GENO_NONE; }
uint32_t csrgeno_tally_bytes(void) { return (uint32_t)sizeof(vtxr::GenoTally); }

// the lane map of the pass at `base`: Dp; per lane its sub-group, its donor slot and whether it is live (64 values each)
uint32_t csrgeno_lane_map(uint32_t n_donors, uint32_t base, uint32_t* sub, uint32_t* d, uint8_t* live) {
    const uint32_t Dp = vtxr::pass_lanes(n_donors, base);
    for (uint32_t lane = 0; lane < csrgeno::WAVE; ++lane) {
        const vtxr::GenoLane me = vtxr::lane_map(lane, Dp);
        sub[lane] = me.sub; d[lane] = me.d; live[lane] = vtxr::lane_live(base, me.d, n_donors);
    }
    return Dp;
}

// the lane distances of the fold, in order; returns how many
uint32_t csrgeno_fold_strides(uint32_t Dp, uint32_t* strides) {
    uint32_t n = 0;
    for (uint32_t s = vtxr::fold_first(Dp); vtxr::fold_more(s); s = vtxr::fold_next(s)) strides[n++] = s;
    return n;
}

// csr_geno_check_kernel: the lowest flat index of a bad byte, all ones when there is none
uint64_t csrgeno_first_bad(const uint8_t* geno, uint64_t n_bytes) { return csrgeno::first_bad(geno, n_bytes); }

// vtx_csr_geno_tally; stores: n_major * n_donors * 4 zeroed bytes that count the lanes that store each element
void csrgeno_tally(const uint64_t* indptr, uint32_t n_major, const uint32_t* indices, const uint32_t* alt, const uint32_t* ref,
                   const uint8_t* geno, uint32_t n_donors, uint64_t* sum_alt, uint64_t* sum_ref, uint32_t* n_obs, uint8_t* stores) {
    csrgeno::tally<vtxr::DonorHyp>(csrgeno::TallyIn{indptr, n_major, indices, alt, ref, geno, n_donors, nullptr, 0}, csrgeno::TallyOut{sum_alt, sum_ref, n_obs}, stores);
}

}

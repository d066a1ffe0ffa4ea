// Host build of vartrix_amd/csrc/vtx_csr_geno_pair_core.h for tests/test_csr_geno_pair_core.py: the functions one lane of the doublet
// tally kernels (vtx_csr_geno.hip) runs alone, with the lanes as loops and the exchange between lanes as array reads (lanes.h).
// No device code, no sanitizer: a shared object ctypes loads.
#include "lanes.h"

extern "C" {

uint32_t csrgenopair_max(void) { return vtxr::PAIR_MAX; }
uint32_t csrgenopair_classes(void) { return vtxr::PAIR_CLASSES; }
uint32_t csrgenopair_tally_bytes(void) { return (uint32_t)sizeof(vtxr::PairTally); }

// the class of an entry under a pair, from the two genotype bytes
uint32_t csrgenopair_class(uint8_t ga, uint8_t gb) { return vtxr::pair_class(ga, gb); }

// csr_geno_pair_check_kernel: the lowest index of a pair with a donor out of range, all ones when there is none
uint64_t csrgenopair_first_bad(const uint32_t* pairs, uint32_t n_pairs, uint32_t n_donors) { return csrgenopair::first_bad(pairs, n_pairs, n_donors); }

// vtx_csr_geno_pair_tally; stores: n_major * n_pairs * 6 zeroed bytes that count the lanes that store each element
void csrgenopair_tally(const uint64_t* indptr, uint32_t n_major, const uint32_t* indices, const uint32_t* alt, const uint32_t* ref,
                       const uint8_t* geno, uint32_t n_donors, const uint32_t* pairs, uint32_t n_pairs, uint64_t* sum_alt, uint64_t* sum_ref,
                       uint32_t* n_obs, uint8_t* stores) {
    csrgenopair::tally(csrgenopair::TallyIn{indptr, n_major, indices, alt, ref, geno, n_donors, pairs, n_pairs}, csrgenopair::TallyOut{sum_alt, sum_ref, n_obs}, stores);
}

}

// The pair side of vartrix_amd/csrc/vtx_csr_geno.hip on the host: the pair check as a loop, and the tally of ../csrgenocore/lanes.h (the
// one mirror of csr_tally_kernel) over vtxr::PairHyp of vtx_csr_geno_pair_core.h: what harness.cpp (a shared object for ctypes) and
// main.cpp (a stand-alone program, also built under sanitizers) both run.  Host code only.
#ifndef CSRGENOPAIR_LANES_H
#define CSRGENOPAIR_LANES_H
#include "../../vartrix_amd/csrc/vtx_csr_geno_pair_core.h"
#include "../csrgenocore/lanes.h"

namespace csrgenopair {

using csrgeno::NO_BAD;
using csrgeno::TallyIn;
using csrgeno::TallyOut;

// csr_geno_pair_check_kernel: the integer minimum over the lanes
inline uint64_t first_bad(const uint32_t* pairs, uint32_t n_pairs, uint32_t n_donors) {
    uint64_t first = NO_BAD;
    for (uint32_t p = 0; p < n_pairs; ++p)
        if (vtxr::pair_bad(pairs[2 * p], pairs[2 * p + 1], n_donors) && p < first) first = p;
    return first;
}

// csr_tally_kernel<vtxr::PairHyp>.  stores (n_major * n_pairs * 6 bytes, may be NULL) counts the lanes that store each output element.
inline void tally(const TallyIn& in, const TallyOut& out, uint8_t* stores) { csrgeno::tally<vtxr::PairHyp>(in, out, stores); }

}  // namespace csrgenopair
#endif

// The kernels of vartrix_amd/csrc/vtx_csr_geno.hip with the lanes as loops and the exchange between lanes as array reads, over
// vtx_csr_geno_core.h: what harness.cpp (a shared object for ctypes) and main.cpp (a stand-alone program, also built under sanitizers)
// both run.  Host code only.
#ifndef CSRGENO_LANES_H
#define CSRGENO_LANES_H
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "../../vartrix_amd/csrc/vtx_csr_geno_core.h"

namespace csrgeno {

constexpr uint32_t WAVE = vtxr::GENO_WAVE;
constexpr uint64_t NO_BAD = ~0ull;

struct TallyOut {          // n_major * n_donors * 4 elements each; a NULL array is not written
    uint64_t *sum_alt, *sum_ref;
    uint32_t* n_obs;
};

// csr_geno_check_kernel: the integer minimum over the lanes
inline uint64_t first_bad(const uint8_t* geno, uint64_t n_bytes) {
    uint64_t first = NO_BAD;
    for (uint64_t i = 0; i < n_bytes; ++i)
        if (vtxr::geno_bad(geno[i]) && i < first) first = i;
    return first;
}

// csr_geno_tally_kernel.  stores (n_major * n_donors * 4 bytes, may be NULL) counts the lanes that store each output element.
inline void tally(const uint64_t* indptr, uint32_t n_major, const uint32_t* indices, const uint32_t* alt, const uint32_t* ref,
                  const uint8_t* geno, uint32_t n_donors, const TallyOut& out, uint8_t* stores) {
    for (uint64_t r = 0; r < n_major; ++r) {
        const uint64_t begin = indptr[r], end = indptr[r + 1];
        for (uint32_t base = 0; base < n_donors; base += WAVE) {
            const uint32_t Dp = vtxr::pass_lanes(n_donors, base), stride = vtxr::sub_groups(Dp);
            vtxr::GenoTally t[WAVE];
            memset(t, 0xA5, sizeof t);                            // registers hold what the last pass left
            for (uint32_t lane = 0; lane < WAVE; ++lane) {
                const vtxr::GenoLane me = vtxr::lane_map(lane, Dp);
                const bool live = vtxr::lane_live(base, me.d, n_donors);
                t[lane] = vtxr::tally_zero();
                for (uint64_t k = begin + me.sub; k < end; k += stride) {
                    const uint32_t v = indices[k], a = alt[k], f = ref[k];      // every lane loads the entry, only a live one a genotype
                    if (live) vtxr::tally_add(t[lane], vtxr::geno_class(geno[vtxr::geno_index(v, n_donors, base, me.d)]), a, f);
                }
            }
            for (uint32_t s = vtxr::fold_first(Dp); vtxr::fold_more(s); s = vtxr::fold_next(s)) {
                vtxr::GenoTally o[WAVE];
                for (uint32_t lane = 0; lane < WAVE; ++lane) o[lane] = t[lane ^ s];      // __shfl_xor: what the other lane held BEFORE the step
                for (uint32_t lane = 0; lane < WAVE; ++lane) vtxr::tally_merge(t[lane], o[lane]);
            }
            for (uint32_t lane = 0; lane < WAVE; ++lane) {
                const vtxr::GenoLane me = vtxr::lane_map(lane, Dp);
                if (me.sub != 0 || !vtxr::lane_live(base, me.d, n_donors)) continue;
                const uint64_t q = vtxr::tally_index(r, n_donors, base + me.d, 0);
                for (uint32_t g = 0; g < vtxr::GENO_CLASSES; ++g) {
                    if (stores && stores[q + g] < 255) ++stores[q + g];
                    if (out.sum_alt) out.sum_alt[q + g] = t[lane].sum_alt[g];
                    if (out.sum_ref) out.sum_ref[q + g] = t[lane].sum_ref[g];
                    if (out.n_obs) out.n_obs[q + g] = t[lane].n_obs[g];
                }
            }
        }
    }
}

}  // namespace csrgeno
#endif

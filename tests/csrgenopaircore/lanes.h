// The kernels of vartrix_amd/csrc/vtx_csr_geno_pair.hip with the lanes as loops and the exchange between lanes as array reads, over
// vtx_csr_geno_pair_core.h: what harness.cpp (a shared object for ctypes) and main.cpp (a stand-alone program, also built under
// sanitizers) both run.  Host code only.
#ifndef CSRGENOPAIR_LANES_H
#define CSRGENOPAIR_LANES_H
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "../../vartrix_amd/csrc/vtx_csr_geno_pair_core.h"

namespace csrgenopair {

constexpr uint32_t WAVE = vtxr::GENO_WAVE;
constexpr uint64_t NO_BAD = ~0ull;

struct TallyOut {          // n_major * n_pairs * 6 elements each; a NULL array is not written
    uint64_t *sum_alt, *sum_ref;
    uint32_t* n_obs;
};

// csr_geno_pair_check_kernel: the integer minimum over the lanes
inline uint64_t first_bad(const uint32_t* pairs, uint32_t n_pairs, uint32_t n_donors) {
    uint64_t first = NO_BAD;
    for (uint32_t p = 0; p < n_pairs; ++p)
        if (vtxr::pair_bad(pairs[2 * p], pairs[2 * p + 1], n_donors) && p < first) first = p;
    return first;
}

// csr_geno_pair_tally_kernel.  stores (n_major * n_pairs * 6 bytes, may be NULL) counts the lanes that store each output element.
inline void tally(const uint64_t* indptr, uint32_t n_major, const uint32_t* indices, const uint32_t* alt, const uint32_t* ref,
                  const uint8_t* geno, uint32_t n_donors, const uint32_t* pairs, uint32_t n_pairs, const TallyOut& out, uint8_t* stores) {
    for (uint64_t r = 0; r < n_major; ++r) {
        const uint64_t begin = indptr[r], end = indptr[r + 1];
        for (uint32_t base = 0; base < n_pairs; base += WAVE) {
            const uint32_t Dp = vtxr::pass_lanes(n_pairs, base), stride = vtxr::sub_groups(Dp);
            vtxr::PairTally t[WAVE];
            memset(t, 0xA5, sizeof t);                            // registers hold what the last pass left
            for (uint32_t lane = 0; lane < WAVE; ++lane) {
                const vtxr::GenoLane me = vtxr::lane_map(lane, Dp);
                const bool live = vtxr::lane_live(base, me.d, n_pairs);
                uint32_t da = 0, db = 0;
                if (live) { da = pairs[2 * (base + me.d)]; db = pairs[2 * (base + me.d) + 1]; }      // only a live lane loads its pair
                t[lane] = vtxr::pair_tally_zero();
                for (uint64_t k = begin + me.sub; k < end; k += stride) {
                    const uint32_t v = indices[k], a = alt[k], f = ref[k];      // every lane loads the entry, only a live one its two bytes
                    if (live)
                        vtxr::pair_tally_add(t[lane], vtxr::pair_class(geno[vtxr::pair_geno_index(v, n_donors, da)], geno[vtxr::pair_geno_index(v, n_donors, db)]), a, f);
                }
            }
            for (uint32_t s = vtxr::fold_first(Dp); vtxr::fold_more(s); s = vtxr::fold_next(s)) {
                vtxr::PairTally o[WAVE];
                for (uint32_t lane = 0; lane < WAVE; ++lane) o[lane] = t[lane ^ s];      // __shfl_xor: what the other lane held BEFORE the step
                for (uint32_t lane = 0; lane < WAVE; ++lane) vtxr::pair_tally_merge(t[lane], o[lane]);
            }
            for (uint32_t lane = 0; lane < WAVE; ++lane) {
                const vtxr::GenoLane me = vtxr::lane_map(lane, Dp);
                if (me.sub != 0 || !vtxr::lane_live(base, me.d, n_pairs)) continue;
                const uint64_t q = vtxr::pair_tally_index(r, n_pairs, base + me.d, 0);
                for (uint32_t c = 0; c < vtxr::PAIR_CLASSES; ++c) {
                    if (stores && stores[q + c] < 255) ++stores[q + c];
                    if (out.sum_alt) out.sum_alt[q + c] = t[lane].sum_alt[c];
                    if (out.sum_ref) out.sum_ref[q + c] = t[lane].sum_ref[c];
                    if (out.n_obs) out.n_obs[q + c] = t[lane].n_obs[c];
                }
            }
        }
    }
}

}  // namespace csrgenopair
#endif

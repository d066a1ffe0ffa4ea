// The kernels of vartrix_amd/csrc/vtx_csr_geno.hip with the lanes as loops and the exchange between lanes as array reads, over
// vtx_csr_geno_core.h: what harness.cpp (a shared object for ctypes) and main.cpp (a stand-alone program, also built under sanitizers)
// both run.  The tally is a template over the kernel's own hypothesis policies: vtxr::DonorHyp here, vtxr::PairHyp in
// ../csrgenopaircore/, which includes this file.  Host code only.
#ifndef CSRGENO_LANES_H
#define CSRGENO_LANES_H
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "../../vartrix_amd/csrc/vtx_csr_geno_core.h"

namespace csrgeno {

constexpr uint32_t WAVE = vtxr::GENO_WAVE;
constexpr uint64_t NO_BAD = ~0ull;

// what the kernel takes (vtx_geno_in / vtx_geno_pair_in of vtx_device.h, which a host build cannot include); pairs: PairHyp only
struct TallyIn {
    const uint64_t* indptr; uint32_t n_major; const uint32_t* indices; const uint32_t *alt, *ref; const uint8_t* geno; uint32_t n_donors;
    const uint32_t* pairs; uint32_t n_pairs;
};
struct TallyOut {          // n_major * hypotheses * classes elements each; a NULL array is not written
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

// csr_tally_kernel<H>.  stores (n_major * hypotheses * classes bytes, may be NULL) counts the lanes that store each output element.
template <class H> inline void tally(const TallyIn& in, const TallyOut& out, uint8_t* stores) {
    constexpr uint32_t N = H::CLASSES;
    const uint32_t n_hyp = H::count(in);
    for (uint64_t r = 0; r < in.n_major; ++r) {
        const uint64_t begin = in.indptr[r], end = in.indptr[r + 1];
        for (uint32_t base = 0; base < n_hyp; base += WAVE) {
            const uint32_t Dp = vtxr::pass_lanes(n_hyp, base), stride = vtxr::sub_groups(Dp);
            vtxr::ClassTally<N> t[WAVE];
            memset(t, 0xA5, sizeof t);                            // registers hold what the last pass left
            for (uint32_t lane = 0; lane < WAVE; ++lane) {
                const vtxr::GenoLane me = vtxr::lane_map(lane, Dp);
                const bool live = vtxr::lane_live(base, me.d, n_hyp);
                typename H::Lane mine{};
                if (live) mine = H::load(in, base + me.d);        // only a live lane loads its pair
                t[lane] = vtxr::tally_zero<N>();
                for (uint64_t k = begin + me.sub; k < end; k += stride) {
                    const uint32_t v = in.indices[k], a = in.alt[k], f = in.ref[k];      // every lane loads the entry, only a live one a genotype
                    if (live) vtxr::tally_add(t[lane], H::cls(in, mine, v, base + me.d), a, f);
                }
            }
            for (uint32_t s = vtxr::fold_first(Dp); vtxr::fold_more(s); s = vtxr::fold_next(s)) {
                vtxr::ClassTally<N> o[WAVE];
                for (uint32_t lane = 0; lane < WAVE; ++lane) o[lane] = t[lane ^ s];      // __shfl_xor: what the other lane held BEFORE the step
                for (uint32_t lane = 0; lane < WAVE; ++lane) vtxr::tally_merge(t[lane], o[lane]);
            }
            for (uint32_t lane = 0; lane < WAVE; ++lane) {
                const vtxr::GenoLane me = vtxr::lane_map(lane, Dp);
                if (me.sub != 0 || !vtxr::lane_live(base, me.d, n_hyp)) continue;
                const uint64_t q = vtxr::tally_index<N>(r, n_hyp, base + me.d, 0);
                for (uint32_t g = 0; g < N; ++g) {
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

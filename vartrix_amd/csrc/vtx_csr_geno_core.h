// vtx_csr_geno_core.h — what ONE LANE does alone in the tally kernel (vtx_csr_geno.hip): the check of a genotype byte, the lane's place
// in the wavefront (which hypothesis, which entries), an entry's contribution to the lane's 3 N numbers (ClassTally<N>), the fold of the
// lanes that share a hypothesis, and the place of a number in the output.  A hypothesis is a donor here (DonorHyp, N = 4) and a pair of
// donors in vtx_csr_geno_pair_core.h (PairHyp, N = 6); everything below says "donor" and holds for either.
//
// What it serves: the step that produces the donor label pseudobulk (vtx_csr_group_core.h) takes.  Cells of pooled samples are scored
// against the known genotypes of the pooled donors: for every (cell, donor) pair the alt and ref reads of the cell's entries are summed
// by the donor's genotype class at the entry's variant — 0 hom-ref, 1 het, 2 hom-alt, 3 missing.  Every likelihood model in use is a
// linear function of those numbers, so the device adds integers and the floating point stays in a few lines on top (api.assign_donors).
// The reference writes the matrix and stops (src/main.rs:381-389).
//
// The table.  geno[n_minor * n_donors], one byte per (variant, donor), variant-major: the donors of one variant are consecutive.
// A byte is 0, 1, 2 or GENO_NONE; anything else is refused (geno_bad) before a byte of output is written.
//
// The lane map.  One wavefront owns one row (a cell) and, per pass, the donors [base, base + count), count = pass_donors() <= 64.
// Dp = pass_lanes() is the smallest power of two >= count; the wavefront is 64 / Dp sub-groups of Dp lanes, lane = sub * Dp + d.  Lane
// (sub, d) is LIVE when base + d < n_donors and then tallies donor base + d over the entries begin + sub, + 64 / Dp, + 2 * 64 / Dp, ...
// of the row: the Dp lanes of a sub-group load the same entry and Dp consecutive genotype bytes, and only live lanes load one.  The
// tally lives in registers: tally_add selects the class by N predicated additions, never by an index into the arrays (an array
// indexed at run time leaves the registers).  n_donors > 64: the wavefront repeats the row once per 64 donors, at most GENO_MAX_PASSES
// times.
//
// The fold.  The lanes (0, d), (1, d), ... hold partial tallies of one donor; they are exchanged over the lane distances Dp, 2 Dp, ... 32
// (fold_first, fold_next: an xor of the lane number with the distance) and added with tally_merge.  Lanes of one d are all live or all
// dead, a dead lane's tally is zero.  Afterwards every lane holds its donor's total and the live lanes of sub-group 0 store: every
// (row, donor, class) element is written exactly once, by one lane, whether the row has entries or not.  Integer additions only: the
// grouping cannot change a result, there are no atomics and no zeroing pass.
//
// Compiles for the host too (tests/csrgenocore/: the same functions, the lanes as loops, the exchange as array reads, against numpy).
#ifndef VTX_CSR_GENO_CORE_H
#define VTX_CSR_GENO_CORE_H

#include "vtx_csr_ops_core.h"

#ifdef __HIPCC__
#define VTXR_UNROLL _Pragma("unroll")
#define VTXR_STATIC_FN static VTXR_FN                                   // a static member of a hypothesis policy
#else
#define VTXR_UNROLL
#define VTXR_STATIC_FN VTXR_FN                                            // (the host's VTXR_FN is static inline already)
#endif

namespace vtxr {

constexpr uint8_t GENO_NONE = 0xFF;                                       // VTX_GENO_NONE: the donor has no call at this variant
constexpr uint32_t GENO_CLASSES = 4;                                      // hom-ref, het, hom-alt, missing
constexpr uint32_t GENO_WAVE = 64;                                        // lanes that share a row
constexpr uint32_t GENO_MAX_PASSES = 16;                                  // passes over a row, at most
constexpr uint32_t GENO_MAX = GENO_WAVE * GENO_MAX_PASSES;                // the largest n_donors

// the tally of one hypothesis (a donor, a pair of donors) in N classes
template <uint32_t N> struct ClassTally {
    uint64_t sum_alt[N], sum_ref[N];
    uint32_t n_obs[N];                                                    // entries of the class with alt + ref > 0
};
using GenoTally = ClassTally<GENO_CLASSES>;

struct GenoLane { uint32_t sub, d; };

// a byte the call refuses: neither a class nor VTX_GENO_NONE
VTXR_FN bool geno_bad(uint8_t g) { return g > 2 && g != GENO_NONE; }

// the class of a byte that passed the check
VTXR_FN uint32_t geno_class(uint8_t g) { return g == GENO_NONE ? 3u : (uint32_t)g; }

// the donors of the pass that begins at `base` (base < n_donors, a multiple of GENO_WAVE)
VTXR_FN uint32_t pass_donors(uint32_t n_donors, uint32_t base) { return n_donors - base < GENO_WAVE ? n_donors - base : GENO_WAVE; }

// Dp: the lanes of a sub-group, the smallest power of two >= the donors of the pass
VTXR_FN uint32_t pass_lanes(uint32_t n_donors, uint32_t base) {
    const uint32_t count = pass_donors(n_donors, base);
    uint32_t Dp = 1;
    while (Dp < count) Dp *= 2;
    return Dp;
}

VTXR_FN GenoLane lane_map(uint32_t lane, uint32_t Dp) { return GenoLane{lane / Dp, lane % Dp}; }
VTXR_FN bool lane_live(uint32_t base, uint32_t d, uint32_t n_donors) { return base + d < n_donors; }
VTXR_FN uint32_t sub_groups(uint32_t Dp) { return GENO_WAVE / Dp; }       // the stride of a sub-group's walk over the row

// where a live lane's genotype byte is: < n_minor * n_donors, since v < n_minor (the CSR check) and base + d < n_donors
VTXR_FN uint64_t geno_index(uint32_t v, uint32_t n_donors, uint32_t base, uint32_t d) { return (uint64_t)v * n_donors + base + d; }

// (N where it cannot be deduced defaults to the donor's: tally_zero() is a GenoTally)
template <uint32_t N = GENO_CLASSES> VTXR_FN ClassTally<N> tally_zero() { return ClassTally<N>{{}, {}, {}}; }

// one entry into the tally of a hypothesis whose class at the entry's variant is `cls`: every class takes an addition, all but one of
// them of zero.  g is a literal in every step of the unrolled loop: the arrays are never indexed at run time
template <uint32_t N> VTXR_FN void tally_add(ClassTally<N>& t, uint32_t cls, uint32_t alt, uint32_t ref) {
    const uint32_t seen = (alt | ref) != 0u;                              // alt + ref > 0 without the carry
    VTXR_UNROLL
    for (uint32_t g = 0; g < N; ++g) {
        const bool on = cls == g;
        t.sum_alt[g] += on ? alt : 0u;
        t.sum_ref[g] += on ? ref : 0u;
        t.n_obs[g] += on ? seen : 0u;
    }
}

// the partial tally of another lane of the same hypothesis
template <uint32_t N> VTXR_FN void tally_merge(ClassTally<N>& a, const ClassTally<N>& b) {
    for (uint32_t g = 0; g < N; ++g) { a.sum_alt[g] += b.sum_alt[g]; a.sum_ref[g] += b.sum_ref[g]; a.n_obs[g] += b.n_obs[g]; }
}

// the lane distances of the fold: for (s = fold_first(Dp); fold_more(s); s = fold_next(s)) exchange with lane ^ s.  Dp, 2 Dp, ... 32.
VTXR_FN uint32_t fold_first(uint32_t Dp) { return Dp; }
VTXR_FN bool fold_more(uint32_t s) { return s < GENO_WAVE; }
VTXR_FN uint32_t fold_next(uint32_t s) { return s * 2; }

// the element of (row r, hypothesis h of n_hyp, class g of N) in each of the three output arrays
template <uint32_t N = GENO_CLASSES> VTXR_FN uint64_t tally_index(uint64_t r, uint32_t n_hyp, uint32_t h, uint32_t g) { return (r * n_hyp + h) * N + g; }

// The one-donor hypotheses as the tally kernel takes them (vtx_csr_geno.hip: csr_tally_kernel<DonorHyp, ...>; PairHyp is
// vtx_csr_geno_pair_core.h's).  `In` is any struct with the fields of vtx_geno_in (vtx_device.h) that the policy names.
struct DonorHyp {
    static constexpr uint32_t CLASSES = GENO_CLASSES;
    struct Lane {};                                                       // a live lane loads nothing per pass
    template <class In> VTXR_STATIC_FN uint32_t count(const In& in) { return in.n_donors; }
    template <class In> VTXR_STATIC_FN Lane load(const In&, uint32_t) { return Lane{}; }
    // the class of the entry at variant v under donor h, a live lane's
    template <class In> VTXR_STATIC_FN uint32_t cls(const In& in, const Lane&, uint32_t v, uint32_t h) {
        return geno_class(in.geno[geno_index(v, in.n_donors, h, 0)]);
    }
};

}  // namespace vtxr
#endif

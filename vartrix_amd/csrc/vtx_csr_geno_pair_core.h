// vtx_csr_geno_pair_core.h — what is particular to a PAIR of donors in the tally kernel (vtx_csr_geno.hip): the check of a pair, the
// class of an entry under a pair, and the policy PairHyp that hands both to the kernel.  The lane's place in the wavefront, the tally
// (ClassTally<PAIR_CLASSES>: eighteen numbers), its fold and its place in the output are vtx_csr_geno_core.h's, with a pair in a
// donor's place.
//
// What it serves: the two-donor hypotheses next to the one-donor ones of vtx_csr_geno_core.h.  A droplet that holds cells of the donors
// a and b in equal parts shows, at a variant, an alt read with a probability that depends only on the DOSAGE g_a + g_b in 0 .. 4.  So per
// (cell, pair) the alt reads, the ref reads and the informative entries are summed by dosage class; class 5 takes the entries at which
// either donor has no call.  The likelihood is a linear function of those numbers (api.assign_doublets).  It is not a function of the
// one-donor tallies: it needs the joint class of each entry.  The six classes assume a 50 : 50 mixture.
//
// The pairs.  pairs[2 * n_pairs]: the donors (a, b) of pair p at [2 p], [2 p + 1].  Any list: duplicates, both orders, a == b.  A donor
// >= n_donors is refused (pair_bad) before a byte of output is written.  Pair (a, a) carries donor a's one-donor tally on the classes
// 0, 2, 4 and its missing class on 5 — by the rule above, not by a case of its own.
//
// The lane map.  pass_lanes, lane_map, lane_live, sub_groups and the fold distances of vtx_csr_geno_core.h with n_pairs for n_donors: one
// wavefront owns a row and, per pass, the pairs [base, base + count), count <= 64; lane (sub, d) is live when base + d < n_pairs, loads
// its (a, b) once per pass and tallies over the entries begin + sub, + 64 / Dp, ...  Per entry it loads two bytes of the table, both
// inside it (pair_geno_index).  n_pairs > 64: the wavefront repeats the row once per 64 pairs, at most PAIR_MAX_PASSES times.
//
// Compiles for the host too (tests/csrgenopaircore/: the same functions, the lanes as loops, the exchange as array reads, against numpy).
#ifndef VTX_CSR_GENO_PAIR_CORE_H
#define VTX_CSR_GENO_PAIR_CORE_H

#include "vtx_csr_geno_core.h"

namespace vtxr {

constexpr uint32_t PAIR_CLASSES = 6;                                      // dosage 0 .. 4, and 5: either donor without a call
constexpr uint32_t PAIR_NONE_CLASS = 5;
constexpr uint32_t PAIR_MAX_PASSES = 64;                                  // passes over a row, at most
constexpr uint32_t PAIR_MAX = GENO_WAVE * PAIR_MAX_PASSES;                // the largest n_pairs

using PairTally = ClassTally<PAIR_CLASSES>;

// a pair the call refuses: a donor the table has no column for
VTXR_FN bool pair_bad(uint32_t a, uint32_t b, uint32_t n_donors) { return a >= n_donors || b >= n_donors; }

// the class of an entry under a pair, from the two bytes (both passed geno_bad)
VTXR_FN uint32_t pair_class(uint8_t ga, uint8_t gb) { return (ga == GENO_NONE || gb == GENO_NONE) ? PAIR_NONE_CLASS : (uint32_t)ga + (uint32_t)gb; }

// where the byte of a donor is: < n_minor * n_donors, since v < n_minor (the CSR check) and donor < n_donors (the pair check)
VTXR_FN uint64_t pair_geno_index(uint32_t v, uint32_t n_donors, uint32_t donor) { return (uint64_t)v * n_donors + donor; }

// The two-donor hypotheses as the tally kernel takes them (DonorHyp's counterpart).  `In`: the fields of vtx_geno_pair_in (vtx_device.h).
struct PairHyp {
    static constexpr uint32_t CLASSES = PAIR_CLASSES;
    struct Lane { uint32_t a, b; };                                       // a live lane loads its pair once per pass
    template <class In> VTXR_STATIC_FN uint32_t count(const In& in) { return in.n_pairs; }
    template <class In> VTXR_STATIC_FN Lane load(const In& in, uint32_t h) { return Lane{in.pairs[2 * h], in.pairs[2 * h + 1]}; }
    // the class of the entry at variant v under the pair, a live lane's
    template <class In> VTXR_STATIC_FN uint32_t cls(const In& in, const Lane& me, uint32_t v, uint32_t) {
        return pair_class(in.geno[pair_geno_index(v, in.n_donors, me.a)], in.geno[pair_geno_index(v, in.n_donors, me.b)]);
    }
};

}  // namespace vtxr
#endif

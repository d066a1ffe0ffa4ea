// vtx_csr_geno_pair_core.h — what ONE LANE does alone in the doublet tally kernels (vtx_csr_geno_pair.hip): the check of a pair of donors,
// the class of an entry under a pair, an entry's contribution to the lane's eighteen numbers, the merge of the lanes that share a pair,
// and the place of a number in the output.  The lane's place in the wavefront is vtx_csr_geno_core.h's, with a pair in a donor's place.
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
// inside it (pair_geno_index).  The tally lives in registers: pair_tally_add selects the class by six predicated additions, never by an
// index into the arrays.  n_pairs > 64: the wavefront repeats the row once per 64 pairs, at most PAIR_MAX_PASSES times.
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

struct PairTally {
    uint64_t sum_alt[PAIR_CLASSES], sum_ref[PAIR_CLASSES];
    uint32_t n_obs[PAIR_CLASSES];                                         // entries of the class with alt + ref > 0
};

// a pair the call refuses: a donor the table has no column for
VTXR_FN bool pair_bad(uint32_t a, uint32_t b, uint32_t n_donors) { return a >= n_donors || b >= n_donors; }

// the class of an entry under a pair, from the two bytes (both passed geno_bad)
VTXR_FN uint32_t pair_class(uint8_t ga, uint8_t gb) { return (ga == GENO_NONE || gb == GENO_NONE) ? PAIR_NONE_CLASS : (uint32_t)ga + (uint32_t)gb; }

// where the byte of a donor is: < n_minor * n_donors, since v < n_minor (the CSR check) and donor < n_donors (the pair check)
VTXR_FN uint64_t pair_geno_index(uint32_t v, uint32_t n_donors, uint32_t donor) { return (uint64_t)v * n_donors + donor; }

VTXR_FN PairTally pair_tally_zero() {
    return PairTally{{0ull, 0ull, 0ull, 0ull, 0ull, 0ull}, {0ull, 0ull, 0ull, 0ull, 0ull, 0ull}, {0u, 0u, 0u, 0u, 0u, 0u}};
}

// one entry into the tally of a pair whose class at the entry's variant is `cls`: every class takes an addition, five of them of zero
VTXR_FN void pair_tally_add_class(PairTally& t, uint32_t c, bool on, uint32_t alt, uint32_t ref, uint32_t seen) {      // c: a literal at every call
    t.sum_alt[c] += on ? alt : 0u;
    t.sum_ref[c] += on ? ref : 0u;
    t.n_obs[c] += on ? seen : 0u;
}
VTXR_FN void pair_tally_add(PairTally& t, uint32_t cls, uint32_t alt, uint32_t ref) {
    const uint32_t seen = (alt | ref) != 0u;                              // alt + ref > 0 without the carry
    pair_tally_add_class(t, 0, cls == 0u, alt, ref, seen);
    pair_tally_add_class(t, 1, cls == 1u, alt, ref, seen);
    pair_tally_add_class(t, 2, cls == 2u, alt, ref, seen);
    pair_tally_add_class(t, 3, cls == 3u, alt, ref, seen);
    pair_tally_add_class(t, 4, cls == 4u, alt, ref, seen);
    pair_tally_add_class(t, 5, cls == 5u, alt, ref, seen);
}

// the partial tally of another lane of the same pair
VTXR_FN void pair_tally_merge(PairTally& a, const PairTally& b) {
    for (uint32_t c = 0; c < PAIR_CLASSES; ++c) { a.sum_alt[c] += b.sum_alt[c]; a.sum_ref[c] += b.sum_ref[c]; a.n_obs[c] += b.n_obs[c]; }
}

// the element of (row r, pair p, class c) in each of the three output arrays
VTXR_FN uint64_t pair_tally_index(uint64_t r, uint32_t n_pairs, uint32_t p, uint32_t c) { return (r * n_pairs + p) * PAIR_CLASSES + c; }

}  // namespace vtxr
#endif

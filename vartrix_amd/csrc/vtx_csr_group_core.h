// vtx_csr_group_core.h — what ONE LANE does alone in the pseudobulk kernels (vtx_csr_group.hip): the label check, the window a label
// falls into, an entry's contribution to the bins of its group, and the slot of a non-empty bin in the output row.
//
// What it serves: the step after the statistics and the locus filter (vtx_csr_ops_core.h).  A consumer has a label per cell (cluster,
// donor, clone, sample) and folds variants x cells into variants x groups: per (variant, group) the seven numbers of RowStats over the
// entries of that row whose column carries that label.  The reference writes the matrix and stops (src/main.rs:381-389).
//
// The tile.  One wavefront owns one row at a time and a tile of GROUP_WINDOW groups in LDS: seven arrays side by side (four of u32, three
// of u64, 40 bytes a group), so that the 64 lanes of a sweep read 64 consecutive words of one array.  Lanes walk the row with stride 64
// and add every entry into the bins of its group (tile_add: stats_add on a zero RowStats, then one addition per non-zero number).  On
// the device the additions are LDS atomics; integer additions commute, so the result does not depend on the order of the lanes.
//
// Windows.  n_groups > GROUP_WINDOW: the wavefront repeats the row for the windows [0, W), [W, 2 W), ... in ascending order and an
// entry counts in the pass whose window holds its label (window_slot).  A pass zeroes and sweeps window_bins() bins only.  At most
// GROUP_MAX_WINDOWS passes: GROUP_MAX = W * GROUP_MAX_WINDOWS groups are accepted, no more.
//
// The output row.  The sweep takes 64 bins at a time; a lane whose bin is not empty (n_entries != 0) stores it at
//     indptr_out[r] + rank + (the number of non-empty bins on the lanes below it: step_rank of the ballot),
// and rank grows by the popcount of the ballot from step to step and from window to window: group numbers ascend inside a row.
// The count kernel needs no sums, only which groups occur: one bit per group (GroupBits, bits_set / bits_count).
//
// Compiles for the host too (tests/csrgroupcore/: the same functions, the lanes as loops, the tile as an array, against numpy).
#ifndef VTX_CSR_GROUP_CORE_H
#define VTX_CSR_GROUP_CORE_H

#include "vtx_csr_ops_core.h"

namespace vtxr {

// W = 256: a tile is 256 * 40 = 10 KiB, the four wavefronts of a block hold 40 KiB, and four blocks fill the 160 KiB of a CU's LDS
// (two are asked for; W = 512 would leave room for two and no more).  256 groups hold the cluster, donor and sample counts of
// single-cell work in one pass; more groups cost one more pass over the row per 256.
constexpr uint32_t GROUP_WINDOW = 256;
constexpr uint32_t GROUP_MAX_WINDOWS = 256;                               // passes over a row, at most
constexpr uint32_t GROUP_MAX = GROUP_WINDOW * GROUP_MAX_WINDOWS;          // the largest n_groups
constexpr uint32_t GROUP_NONE = 0xFFFFFFFFu;                              // VTX_GROUP_NONE: the column belongs to no group
constexpr uint32_t GROUP_WAVE = 64;                                       // lanes that share a row and a tile

struct GroupTile {
    uint32_t n_entries[GROUP_WINDOW], n_alt[GROUP_WINDOW], n_ref[GROUP_WINDOW], n_both[GROUP_WINDOW];
    uint64_t sum_alt[GROUP_WINDOW], sum_ref[GROUP_WINDOW], sum_unk[GROUP_WINDOW];
};
static_assert(sizeof(GroupTile) == 40 * GROUP_WINDOW, "40 bytes a group");

struct GroupBits { uint32_t word[GROUP_WINDOW / 32]; };                   // the count kernel's tile: bit b = group base + b occurs

// a label the calls refuse: neither a group nor VTX_GROUP_NONE
VTXR_FN bool label_bad(uint32_t label, uint32_t n_groups) { return label >= n_groups && label != GROUP_NONE; }

// the bins of the window that begins at `base` (base < n_groups, a multiple of GROUP_WINDOW)
VTXR_FN uint32_t window_bins(uint32_t n_groups, uint32_t base) { return n_groups - base < GROUP_WINDOW ? n_groups - base : GROUP_WINDOW; }

// does the label count in this window, and in which bin?  VTX_GROUP_NONE counts in none: base + bins <= GROUP_MAX < GROUP_NONE.
VTXR_FN bool window_slot(uint32_t label, uint32_t base, uint32_t bins, uint32_t* slot) {
    *slot = label - base;
    return label >= base && label - base < bins;
}

#ifdef __HIP_DEVICE_COMPILE__
#define VTXR_BIN_ADD32(p, v) ((void)atomicAdd((p), (v)))
#define VTXR_BIN_ADD64(p, v) ((void)atomicAdd((unsigned long long*)(p), (unsigned long long)(v)))
#define VTXR_BIN_OR32(p, v) ((void)atomicOr((p), (v)))
#else
#define VTXR_BIN_ADD32(p, v) ((void)(*(p) += (v)))
#define VTXR_BIN_ADD64(p, v) ((void)(*(p) += (v)))
#define VTXR_BIN_OR32(p, v) ((void)(*(p) |= (v)))
#endif

VTXR_FN void tile_zero(GroupTile& t, uint32_t b) {
    t.n_entries[b] = 0u; t.n_alt[b] = 0u; t.n_ref[b] = 0u; t.n_both[b] = 0u;
    t.sum_alt[b] = 0ull; t.sum_ref[b] = 0ull; t.sum_unk[b] = 0ull;
}

// one entry's (alt, ref, unk) counts into bin b: stats_add's seven numbers, the zeros among them not sent
VTXR_FN void tile_add(GroupTile& t, uint32_t b, uint32_t alt, uint32_t ref, uint32_t unk) {
    RowStats e = stats_zero();
    stats_add(e, alt, ref, unk);
    VTXR_BIN_ADD32(&t.n_entries[b], e.n_entries);
    if (e.n_alt) { VTXR_BIN_ADD32(&t.n_alt[b], e.n_alt); VTXR_BIN_ADD64(&t.sum_alt[b], e.sum_alt); }
    if (e.n_ref) { VTXR_BIN_ADD32(&t.n_ref[b], e.n_ref); VTXR_BIN_ADD64(&t.sum_ref[b], e.sum_ref); }
    if (e.n_both) VTXR_BIN_ADD32(&t.n_both[b], e.n_both);
    if (e.sum_unk) VTXR_BIN_ADD64(&t.sum_unk[b], e.sum_unk);
}

VTXR_FN RowStats tile_read(const GroupTile& t, uint32_t b) {
    return RowStats{t.n_entries[b], t.n_alt[b], t.n_ref[b], t.n_both[b], t.sum_alt[b], t.sum_ref[b], t.sum_unk[b]};
}

VTXR_FN void bits_zero(GroupBits& g, uint32_t w) { g.word[w] = 0u; }
VTXR_FN void bits_set(GroupBits& g, uint32_t b) { VTXR_BIN_OR32(&g.word[b / 32], 1u << (b % 32)); }
VTXR_FN uint32_t popcount32(uint32_t x) { return (uint32_t)__builtin_popcount(x); }
VTXR_FN uint32_t popcount64(uint64_t x) { return (uint32_t)__builtin_popcountll(x); }
// the groups of the window that occur in the row (a slot at or past window_bins() is never set: every label is < n_groups)
VTXR_FN uint32_t bits_count(const GroupBits& g) {
    uint32_t n = 0;
    for (uint32_t w = 0; w < GROUP_WINDOW / 32; ++w) n += popcount32(g.word[w]);
    return n;
}

// one step of the sweep: `ballot` has bit l set when lane l's bin is not empty.  The non-empty bins below this lane's:
VTXR_FN uint32_t step_rank(uint64_t ballot, uint32_t lane) { return popcount64(ballot & ((1ull << lane) - 1ull)); }

}  // namespace vtxr
#endif

// vtx_csr_ops_core.h — what ONE LANE does alone in the CSR summary and selection kernels (vtx_csr_ops.hip): the contribution of an
// entry to the statistics of its row, the number of lanes that share a row, the keep predicate of an entry, and the offsets of the
// selected matrix.
//
// What it serves: the first thing a consumer of the variants x cells matrices does — count per variant the cells with alt and with ref
// support (and per cell what it covers), then drop the variants too few cells inform (the locus filter of the demultiplexers).  The
// reference writes the matrix and stops (src/main.rs:381-389); here both steps run where the CSR already is.
//
// Row statistics.  G lanes (a power of two, 1 .. 64: a divisor of the 64-wide wavefront) work on one row: lane j of the group reads the
// entries indptr[r] + j, + G, + 2 G, ... and adds each one's contribution (stats_add) to seven registers; the group then folds its G
// partial results with stats_merge over the lane distances G / 2, G / 4, ... 1, and one lane stores.  Every operation is an integer
// addition, so the grouping cannot change a result: no atomics, no zeroing pass, the output is a function of the input alone.  The four
// counts are u32 (a row of the library's own matrices has at most n_minor < 2^32 entries), the three sums u64 (u32 counts add up
// past 2^32).  A row is walked by its ONE group however long it is: a caller's CSR with duplicate indices (rows longer than n_minor)
// is accepted and correct, and need not be fast.
//
// Selection.  keep_major[n_major] / keep_minor[n_minor] are byte masks (any non-zero byte keeps, NULL keeps everything; a torch.bool
// tensor is one as it is).  Three exclusive scans number what is kept:
//     major_map[r] = kept rows below r        (n_major + 1 values, the last one = n_major_out)
//     minor_map[j] = kept columns below j     (n_minor + 1 values, the last one = n_minor_out)
//     pos[k]       = kept entries below k     (nnz + 1 values, the last one = nnz_out)
// Entry k is kept when its row and its column are (keep_entry) and goes to pos[k] with the column minor_map[indices[k]]: rows keep
// their order and entries their order inside a row.  The offsets: lane r of n_major + 1 writes
//     indptr_out[major_map[r]] = pos[indptr[r]]      when row r is kept, or r == n_major (indptr[n_major] = nnz, so that one is nnz_out)
// (select_offset_lane).  The kept rows and r == n_major have the distinct slots 0 .. n_major_out, so every output offset is written
// exactly once, by one lane.
//
// Compiles for the host too (tests/csropscore/: the same functions, the lanes as loops, against numpy; CPU suite).
#ifndef VTX_CSR_OPS_CORE_H
#define VTX_CSR_OPS_CORE_H

#include "vtx_csr_core.h"

namespace vtxr {

struct RowStats {
    uint32_t n_entries, n_alt, n_ref, n_both;
    uint64_t sum_alt, sum_ref, sum_unk;
};

VTXR_FN RowStats stats_zero() { return RowStats{0u, 0u, 0u, 0u, 0ull, 0ull, 0ull}; }

// one entry's (alt, ref, unk) counts into the statistics of its row
VTXR_FN void stats_add(RowStats& s, uint32_t alt, uint32_t ref, uint32_t unk) {
    s.n_entries += 1u;
    s.n_alt += alt > 0u;
    s.n_ref += ref > 0u;
    s.n_both += (alt > 0u) & (ref > 0u);         // what consensus writes as 3
    s.sum_alt += alt; s.sum_ref += ref; s.sum_unk += unk;
}

// the partial result of another lane of the group
VTXR_FN void stats_merge(RowStats& s, const RowStats& o) {
    s.n_entries += o.n_entries; s.n_alt += o.n_alt; s.n_ref += o.n_ref; s.n_both += o.n_both;
    s.sum_alt += o.sum_alt; s.sum_ref += o.sum_ref; s.sum_unk += o.sum_unk;
}

// lane j of a group of G over the row [begin, end): what csr_row_stats_kernel accumulates in registers before the fold
VTXR_FN RowStats stats_walk(const uint32_t* alt, const uint32_t* ref, const uint32_t* unk, uint64_t begin, uint64_t end, uint32_t j, uint32_t G) {
    RowStats s = stats_zero();
    for (uint64_t k = begin + j; k < end; k += G) stats_add(s, alt[k], ref[k], unk[k]);
    return s;
}

// The group-size rule: the smallest power of two G with LANE_ENTRIES * G >= nnz / n_major (the mean row length), at most the wavefront's
// 64 — a lane then walks about LANE_ENTRIES entries of a mean row, and 64 / G rows share a wavefront.  From nnz / n_major alone.
// LANE_ENTRIES = 8 is measured (profiles/r13_csr_ops.json): at mean row lengths of 3.8, 38, 239 and 2392 the fastest
// G was 1 - 4, 8 - 16, 32 and 32 - 64; one lane per ENTRY of a mean row (G >= mean) cost 1.8 x at a mean of 38, where most of a
// wavefront's shuffles then fold zeros.
constexpr uint32_t MAX_GROUP = 64;
constexpr uint32_t LANE_ENTRIES = 8;
VTXR_FN uint32_t group_lanes(uint64_t nnz, uint64_t n_major) {
    uint32_t G = 1;
    while (G < MAX_GROUP && (uint64_t)LANE_ENTRIES * G * n_major < nnz) G *= 2;      // n_major < 2^32: the product stays below 2^41
    return G;
}

// a byte mask: NULL keeps everything, any non-zero byte keeps
VTXR_FN uint32_t mask_keeps(const uint8_t* mask, uint64_t i) { return (!mask || mask[i] != 0) ? 1u : 0u; }

// the keep predicate of the entry of row `row` with the column `index`
VTXR_FN uint32_t keep_entry(const uint8_t* keep_major, const uint8_t* keep_minor, uint32_t row, uint32_t index) {
    return mask_keeps(keep_major, row) & mask_keeps(keep_minor, index);
}

// lane r of n_major + 1: does it write an offset of the selected matrix (into slot major_map[r], the value pos[indptr[r]])?
VTXR_FN bool select_offset_lane(uint64_t r, uint64_t n_major, const uint8_t* keep_major) { return r == n_major || mask_keeps(keep_major, r); }

}  // namespace vtxr
#endif

// vtx_call_core.h — the calls of ONE (row, cell) group counted by one thread: the logic reduce_count_kernel and reduce_emit_kernel
// (vtx_kernels.hip) share, so that the two passes cannot disagree about a group.
//
// What it restates (reference src/main.rs): evaluate_scores (:1019-1030) per read, the per-UMI collapse (:1058-1082) and
// convert_to_counts (:1032-1039), the rule that consensus drops a cell without a REF or ALT call (:1120-1126) and the three value
// formulas (:1111-1164).  The arithmetic is count_calls_kernel's, umi_collapse_kernel's, keep_flags_kernel's and emit_coo_kernel's,
// token for token: those kernels stay as the path for deep groups and as the A/B reference.
//
// A group is the contiguous run of records [begin, end): vtx_submit rejects a batch that is not sorted by (locus, cell).  With UMIs a
// family is the run that starts at a record with head_umi != 0 (the group's first record always has it).
//
// Compiles for the host too (tests/callcore/: the same functions against tests/call_model.py; CPU suite).
#ifndef VTX_CALL_CORE_H
#define VTX_CALL_CORE_H

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define VTXC_HD __host__ __device__ __forceinline__
#else
#define VTXC_HD inline
#endif

namespace vtxcall {

enum { MODE_CONSENSUS = 0, MODE_ALT_FRAC = 1, MODE_COVERAGE = 2 };   // vtx_scoring_mode (include/vtx.h)
enum { CALL_REF = 0, CALL_ALT = 1, CALL_UNKNOWN = 2, CALL_NONE = 3 };

struct Counts { uint32_t r, a, k; };

// evaluate_scores: None when both scores are under min_score, else the larger score's haplotype, UNKNOWN on a tie
VTXC_HD uint32_t call_of(int32_t rs, int32_t as, int32_t min_score) {
    if ((rs < min_score) & (as < min_score)) return CALL_NONE;
    return rs > as ? (uint32_t)CALL_REF : (as > rs ? (uint32_t)CALL_ALT : (uint32_t)CALL_UNKNOWN);
}

// one UMI family's calls -> its call: ALT if alt / total >= 0.75, else REF if ref / total >= 0.75, else UNKNOWN; a family of None
// reads only has no entry.  0.75 is exact in binary and |x / t - 3 / 4| >= 1 / (4 t), so 4 x >= 3 t decides identically.
VTXC_HD uint32_t collapse_of(uint32_t r, uint32_t a, uint32_t k) {
    const uint32_t t = r + a + k;
    if (t == 0) return CALL_NONE;
    return (4u * a >= 3u * t) ? (uint32_t)CALL_ALT : ((4u * r >= 3u * t) ? (uint32_t)CALL_REF : (uint32_t)CALL_UNKNOWN);
}

VTXC_HD void add_call(Counts& c, uint32_t which) {
    c.r += which == CALL_REF;
    c.a += which == CALL_ALT;
    c.k += which == CALL_UNKNOWN;
}

// (ref, alt, unknown) of the group [begin, end): reads counted one by one, or UMI families collapsed first
VTXC_HD Counts count_group(const int32_t* ref_score, const int32_t* alt_score, const uint32_t* head_umi, uint32_t begin,
                           uint32_t end, int32_t min_score, bool use_umi) {
    Counts cell = {0, 0, 0};
    if (!use_umi) {
        for (uint32_t i = begin; i < end; ++i) add_call(cell, call_of(ref_score[i], alt_score[i], min_score));
        return cell;
    }
    Counts fam = {0, 0, 0};
    for (uint32_t i = begin; i < end; ++i) {
        if (i > begin && head_umi[i]) {
            add_call(cell, collapse_of(fam.r, fam.a, fam.k));
            fam.r = fam.a = fam.k = 0;
        }
        add_call(fam, call_of(ref_score[i], alt_score[i], min_score));
    }
    add_call(cell, collapse_of(fam.r, fam.a, fam.k));     // (an empty range leaves t == 0: nothing)
    return cell;
}

// consensus drops groups with no REF and no ALT call; alt_frac / coverage emit every group
VTXC_HD bool keep_of(Counts c, int mode) { return (mode != MODE_CONSENSUS) || (c.r > 0) || (c.a > 0); }

// the two matrix values of a kept group: emit_coo_kernel's expressions in its order (alt_frac: NaN for 0 / 0)
VTXC_HD void values_of(Counts c, int mode, double* v, double* rv) {
    const uint32_t r = c.r, a = c.a, k = c.k;
    *rv = 0.0;
    if (mode == MODE_CONSENSUS) *v = (r > 0 && a > 0) ? 3.0 : (a > 0 ? 2.0 : 1.0);
    else if (mode == MODE_ALT_FRAC) *v = (double)a / ((double)r + (double)a + (double)k);
    else { *v = (double)a; *rv = (double)r; }
}

}  // namespace vtxcall

#endif

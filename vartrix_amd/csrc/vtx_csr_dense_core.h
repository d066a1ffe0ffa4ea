// vtx_csr_dense_core.h — what ONE LANE does alone in the CSR x integer-table kernel (vtx_csr_dense.hip): the product of a count and a
// weight into the lane's wrapping 64-bit sum, the place of a weight in a table and of a sum in the output, and the lane's walk over its
// share of a row.  The lane map and the fold are vtx_csr_geno_core.h's (pass_lanes, lane_map, lane_live, sub_groups, fold_*): a column
// of the tables stands where a donor stands there.
//
// What it serves: the likelihoods that depend on the variant through MORE than a genotype class — clustering without genotypes (a free
// alt probability per (variant, cluster): api.cluster_donors), an ambient profile, an unequal mixture.  Their integer part is
//     out[r, h] = sum over the entries k of row r of  alt[k] * w_alt[indices[k], h] + ref[k] * w_ref[indices[k], h]
// with fixed-point tables; the floating point stays in a few lines of torch / numpy on top.  The reference writes the matrix and stops
// (src/main.rs:381-389).
//
// The tables.  w_alt, w_ref: int32[n_minor * n_cols], minor-major: the columns of one variant are consecutive.  Either may be absent
// (its term is then absent: a template parameter, not a test per entry).  Any int32 is a weight: nothing to check.
//
// The sum is computed modulo 2^64 and read as two's complement: the count is zero-extended, the weight sign-extended, and the products
// are added in uint64_t — defined for every input, equal to the true sum whenever that fits int64, and independent of the grouping.
//
// The walk.  Lane (sub, d) of a pass takes the entries begin + sub, + stride, + 2 stride, ... (stride = sub_groups(Dp)), DENSE_UNROLL of
// them per trip: first the trip's entries (indices, counts), then their table words, then the additions — the loads of a trip do not
// depend on one another, so DENSE_UNROLL chains entry -> table word are in flight per lane instead of one.  What is left of the row after
// the last whole trip goes one entry at a time.  Every load is inside [begin, end) of the checked CSR; only a live lane loads a table
// word, at an index < n_minor * n_cols.
//
// Compiles for the host too (tests/csrdensecore/: the same functions, the lanes as loops, the exchange as array reads, against a model
// in Python integers).
#ifndef VTX_CSR_DENSE_CORE_H
#define VTX_CSR_DENSE_CORE_H

#include "vtx_csr_geno_core.h"

namespace vtxr {

constexpr uint32_t DENSE_MAX_PASSES = 16;                                 // passes over a row, at most
constexpr uint32_t DENSE_MAX = GENO_WAVE * DENSE_MAX_PASSES;              // the largest n_cols
constexpr uint32_t DENSE_UNROLL = 4;                                      // entries a lane takes per trip of its walk

// count * weight modulo 2^64: the count zero-extended, the weight sign-extended
VTXR_FN uint64_t dense_mul(uint32_t count, int32_t w) { return (uint64_t)count * (uint64_t)(int64_t)w; }

// where column h of variant v is in a table: < n_minor * n_cols, since v < n_minor (the CSR check) and h < n_cols
VTXR_FN uint64_t dense_table_index(uint32_t v, uint32_t n_cols, uint32_t h) { return (uint64_t)v * n_cols + h; }

// the element of (row r, column h)
VTXR_FN uint64_t dense_out_index(uint64_t r, uint32_t n_cols, uint32_t h) { return r * n_cols + h; }

// the entries of one step of the whole wavefront over a row: `stride` sub-groups, DENSE_UNROLL entries each
VTXR_FN uint64_t dense_trip(uint32_t stride) { return (uint64_t)stride * DENSE_UNROLL; }

// The lane's share of the row [begin, end) under column h: the entries begin + sub, + stride, ...  ALT / REF: the table is there.
// `In`: any struct with the fields of vtx_dense_in (vtx_device.h).  A dead lane walks (its loads of the entries are the sub-group's)
// but loads no weight and returns 0.
template <bool ALT, bool REF, class In>
VTXR_FN uint64_t dense_walk(const In& in, uint64_t begin, uint64_t end, uint32_t sub, uint32_t stride, bool live, uint32_t h) {
    uint64_t acc = 0, k = begin + sub;
    const uint64_t trip = dense_trip(stride);
    for (; k + (trip - stride) < end; k += trip) {                        // the last entry of the trip is inside the row
        uint32_t v[DENSE_UNROLL], a[DENSE_UNROLL], f[DENSE_UNROLL];
        int32_t wa[DENSE_UNROLL], wf[DENSE_UNROLL];
        VTXR_UNROLL
        for (uint32_t j = 0; j < DENSE_UNROLL; ++j) {
            const uint64_t e = k + (uint64_t)j * stride;
            v[j] = in.indices[e];
            a[j] = ALT ? in.alt[e] : 0u;
            f[j] = REF ? in.ref[e] : 0u;
            wa[j] = wf[j] = 0;
        }
        if (live) {
            VTXR_UNROLL
            for (uint32_t j = 0; j < DENSE_UNROLL; ++j) {
                if (ALT) wa[j] = in.w_alt[dense_table_index(v[j], in.n_cols, h)];
                if (REF) wf[j] = in.w_ref[dense_table_index(v[j], in.n_cols, h)];
            }
        }
        VTXR_UNROLL
        for (uint32_t j = 0; j < DENSE_UNROLL; ++j) {
            if (ALT) acc += dense_mul(a[j], wa[j]);
            if (REF) acc += dense_mul(f[j], wf[j]);
        }
    }
    for (; k < end; k += stride) {
        const uint32_t v = in.indices[k], a = ALT ? in.alt[k] : 0u, f = REF ? in.ref[k] : 0u;
        if (!live) continue;
        if (ALT) acc += dense_mul(a, in.w_alt[dense_table_index(v, in.n_cols, h)]);
        if (REF) acc += dense_mul(f, in.w_ref[dense_table_index(v, in.n_cols, h)]);
    }
    return acc;
}

}  // namespace vtxr
#endif

// vtx_csr_core.h — the index arithmetic ONE LANE does alone in the CSR kernels (vtx_csr.hip): the boundary -> offsets rule, the
// validation predicates of a caller's CSR, and the row of an entry.
//
// What it serves: the triplets of a run come in the order of the reference's merge loop (src/main.rs:320-348: row ascending, cell
// ascending inside a row), so a compressed-row form needs only the offsets of the row boundaries; the transpose sorts the entries by
// column (stable), and its offsets are the boundaries of the sorted column keys — the same rule.
//
// The offsets rule.  key[0 .. n) is sorted ascending, every key in [begin, end).  There are n + 1 lanes: lane k looks at the boundary
// in front of entry k (lane n: behind the last entry) and writes k into indptr[r - begin] for every r with
//     prev < r <= cur,      prev = key[k - 1] (lane 0: begin - 1, i.e. r starts at begin),      cur = key[k] (lane n: end).
// Every r in [begin, end] lies in exactly one such interval, so every offset is written exactly once, by one lane: no atomics, no
// zeroing, and indptr[r - begin] = the number of keys below r = the offset of the first entry whose key is >= r.  Rows without
// entries — in front of the first key, between two keys (any run length), behind the last — fall into one lane's interval and all
// get that lane's k: an empty range each.  The interval is clamped to [begin, end], so a key outside the window (which the callers
// refuse beforehand) still cannot make a lane write outside the end - begin + 1 offsets.
//
// Long gaps.  A lane writes its interval itself only when it has at most GAP_LANE_ROWS rows: a window of billions of rows over a few
// entries must not become one lane's serial loop.  The rows of a longer interval are written by a second kernel with one lane per ROW
// (csr_fill_kernel): lane r finds k = the number of keys below r (lower_bound, a binary search), rebuilds the interval of boundary
// k with the same offset_rows, and stores k only when that interval is a long one.  Both kernels judge an interval with the same
// predicate (long_gap), so every offset is still written exactly once.
//
// Compiles for the host too (tests/csrcore/: the same functions, the lanes as a loop, against numpy / scipy; CPU suite).
#ifndef VTX_CSR_CORE_H
#define VTX_CSR_CORE_H

#include <stdint.h>

#ifdef __HIPCC__
#define VTXR_FN __host__ __device__ __forceinline__
#else
#define VTXR_FN static inline
#endif

namespace vtxr {

// why a caller's CSR is refused (vtx_csr_transpose; the first bit set names the message)
enum Bad : uint32_t {
    BAD_FIRST = 1u,      // indptr[0] != 0
    BAD_ORDER = 2u,      // indptr[i + 1] < indptr[i]
    BAD_LAST = 4u,       // indptr[n_major] != nnz
    BAD_INDEX = 8u,      // an index >= n_minor
    BAD_WINDOW = 16u     // vtx_device_csr: a triplet's row outside [row_begin, row_end)
};

// lane k of n + 1: the rows [*lo, *hi] (inclusive; none when *lo > *hi) whose offset is k.  prev / cur: key[k - 1] / key[k]; prev is
// not read for k == 0, cur not for k == n.
VTXR_FN void offset_rows(uint64_t k, uint64_t n, uint32_t prev, uint32_t cur, uint32_t begin, uint32_t end, uint64_t* lo, uint64_t* hi) {
    uint64_t a = k == 0 ? (uint64_t)begin : (uint64_t)prev + 1;
    uint64_t b = k == n ? (uint64_t)end : (uint64_t)cur;
    if (a < begin) a = begin;
    if (b > end) b = end;
    *lo = a; *hi = b;
}

// an interval the boundary lane leaves to the per-row kernel
constexpr uint64_t GAP_LANE_ROWS = 256;
VTXR_FN bool long_gap(uint64_t lo, uint64_t hi) { return hi >= lo && hi - lo >= GAP_LANE_ROWS; }

// the number of keys below r in the sorted key[0 .. n): the boundary whose interval holds row r
VTXR_FN uint64_t lower_bound(const uint32_t* key, uint64_t n, uint64_t r) {
    uint64_t lo = 0, hi = n;                 // invariant: key[i] < r for i < lo, key[i] >= r for i >= hi
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (key[mid] < r) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// lane i of n_major + 1 over indptr: cur = indptr[i], next = indptr[i + 1] (not read for i == n_major).  0 = fine.
VTXR_FN uint32_t indptr_bad(uint64_t i, uint64_t n_major, uint64_t nnz, uint64_t cur, uint64_t next) {
    uint32_t bad = 0;
    if (i == 0 && cur != 0) bad |= BAD_FIRST;
    if (i < n_major && next < cur) bad |= BAD_ORDER;
    if (i == n_major && cur != nnz) bad |= BAD_LAST;
    return bad;
}

VTXR_FN uint32_t index_bad(uint32_t index, uint32_t n_minor) { return index >= n_minor ? (uint32_t)BAD_INDEX : 0u; }

VTXR_FN uint32_t row_bad(uint32_t row, uint32_t begin, uint32_t end) { return (row < begin || row >= end) ? (uint32_t)BAD_WINDOW : 0u; }

// the row that holds entry p of a VALIDATED CSR (indptr[0] = 0, non-decreasing, p < indptr[n_major]): the last r with indptr[r] <= p.
// Among rows with equal offsets (empty ones) that is the last, the one whose range [indptr[r], indptr[r + 1]) is not empty.
VTXR_FN uint32_t row_of(const uint64_t* indptr, uint32_t n_major, uint64_t p) {
    uint32_t lo = 0, hi = n_major;          // invariant: indptr[lo] <= p < indptr[hi]
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (indptr[mid] <= p) lo = mid; else hi = mid;
    }
    return lo;
}

}  // namespace vtxr
#endif
